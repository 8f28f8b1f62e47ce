"""The per-knot interior-point operators in `numpy.longdouble`: what `IpSolver<M>` of csrc/ip_kernel_impl.h (`residual`, `factorize`,
`linear_solve`, the sensitivity pass) and the runtime-dimension kernel of csrc/ip_generic.hip are held to, next to the float64
restatements of oracle/lcp.py that state the device's algorithm (explicit A^-1, Schur complement, MGS-QR).

Everything is built from the blocks of an `oracle.lcp.LinTable` (float64, as the device's table is) and solved DENSE with
`gains_ref.solve_ld` (hand-written LU, first largest pivot) and plain-sum products: no LAPACK, no BLAS, no Schur complement, no QR - so
the reference shares no intermediate with the code it judges.

The system the device solves.  `factorize(reg)` + `linear_solve()` are rzlin! / linear_solve! of linearized_solver.jl:378-444 with
y1r = max(y1, reg), y2r = max(y2, reg):  D = Ry1 - diag(Ry2 y2r / y1r),  v = rrst - Ry2 rbil / y1r,  [Dx Dy1; Rx D][dx; dy1] = [rdyn; v],
dy2 = (rbil - y2r dy1) / y1r.  Putting dy2 back into the second block row gives Rx dx + Ry1 dy1 + Ry2 dy2 = rrst, and the last line is
y2r dy1 + y1r dy2 = rbil: the dense rz of `lcp.dense_rz` with y1, y2 replaced by their clamped values (`rz_reg`)."""
import numpy as np

from gains_ref import LD, mm_ld, solve_ld

EPS64 = 2.2e-16      # the float64 floor of a distance (2^-52)


def _ld(a):
    return np.asarray(a, dtype=LD)


def rlin_ld(tab, z, th, kappa, alt=None):
    """`lcp.rlin` (rlin!, linearized_solver.jl:364-373) in longdouble, as one (nz,) vector [rdyn; rrst; rbil]; `alt` (nc,) is the
    altitude term on the impact rows (RLin.alt, :64-65), None = zeros."""
    d = tab.dims
    z, th = _ld(z), _ld(th)
    dx, dy1, dy2, dth = z[d.ix] - _ld(tab.x0), z[d.iy1] - _ld(tab.y10), z[d.iy2] - _ld(tab.y20), th - _ld(tab.th0)
    rdyn = _ld(tab.rdyn0) + mm_ld(_ld(tab.Dx), dx) + mm_ld(_ld(tab.Dy1), dy1) + mm_ld(_ld(tab.rthdyn), dth)
    rrst = _ld(tab.rrst0) + mm_ld(_ld(tab.Rx), dx) + mm_ld(_ld(tab.Ry1), dy1) + _ld(tab.Ry2) * dy2 + mm_ld(_ld(tab.rthrst), dth)
    if alt is not None:
        rrst[:d.nc] += _ld(alt)
    rbil = z[d.iy1] * z[d.iy2] - LD(kappa)
    return np.concatenate([rdyn, rrst, rbil])


def rz_reg(tab, z, reg):
    """The dense (nz, nz) system of `factorize(reg)` + `linear_solve()`: `lcp.dense_rz` with y1, y2 replaced by max(y, reg)."""
    d = tab.dims
    nx, ny = d.nx, d.ny
    z = _ld(z)
    y1r, y2r = np.maximum(z[d.iy1], LD(reg)), np.maximum(z[d.iy2], LD(reg))
    M = np.zeros((d.nz, d.nz), dtype=LD)
    M[:nx, :nx] = tab.Dx
    M[:nx, nx:nx + ny] = tab.Dy1
    M[nx:nx + ny, :nx] = tab.Rx
    M[nx:nx + ny, nx:nx + ny] = tab.Ry1
    M[nx:nx + ny, nx + ny:] = np.diag(_ld(tab.Ry2))
    M[nx + ny:, nx:nx + ny] = np.diag(y2r)
    M[nx + ny:, nx + ny:] = np.diag(y1r)
    return M


def linear_solve_ld(tab, z, r, reg):
    """rz_reg^-1 r, (nz,) or (nz, k)."""
    return solve_ld(rz_reg(tab, z, reg), _ld(r))


def rth_dense(tab):
    """The (nz, nth) rtheta of the table: [rthdyn; rthrst; rthbil]."""
    return np.vstack([tab.rthdyn, tab.rthrst, tab.rthbil])


def sensitivities_ld(tab, z, reg, d=None):
    """-rz_reg^-1 rtheta restricted to what implicit_dynamics.jl:84-86 consumes: rows 1:nd (`d.nd`: gamma and b included in
    :configurationforce mode), columns q0, q1, u1.  Returns dict(dq0 (nd, nq), dq1 (nd, nq), du1 (nd, nu)), longdouble."""
    d = tab.dims if d is None else d
    nq, nu, nd = d.nq, d.nu, d.nd
    dz = -solve_ld(rz_reg(tab, z, reg), _ld(rth_dense(tab)[:, :2 * nq + nu]))[:nd]
    return dict(dq0=dz[:, :nq], dq1=dz[:, nq:2 * nq], du1=dz[:, 2 * nq:])


def dist(a, ref):
    """Relative max-norm distance of `a` to the longdouble `ref`: max|a - ref| / max|ref|, evaluated in longdouble.  Where the answer is
    exactly zero (a zero right-hand side: r0 of a synthetic knot) the distance is max|a| itself, so only an exact zero is at distance 0."""
    ref = _ld(ref)
    err, scale = np.abs(_ld(a) - ref).max(), np.abs(ref).max()
    return float(err if scale == 0 else err / scale)


def bound(d_ref):
    """The per-point bound of a device figure: min(1e-7, 100 max(d_ref, 2.2e-16)).  d_ref comes from the references alone."""
    return min(1e-7, 100.0 * max(float(d_ref), EPS64))
