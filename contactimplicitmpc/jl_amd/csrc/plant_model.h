// Plant-side residuals of the reference's models for the batched simulator step: the planar chains
// (quadruped, flamingo) and hopper_2D, centroidal_quadruped with its box and wall variants, particle, particle_2D, hopper_3D and
// the two models between walls, pushbot and walledcartpole.
// Host- and device-compilable.
//
//   residual            src/simulation/simulation.jl:133-158     (LinearizedCone; plant_residual: flat ground, surface rotation =
//                                                                 identity; plant_residual_terrain: any cimpc_terrain)
//   dynamics            src/dynamics/model.jl:11-36              (variational midpoint integrator)
//   quadruped           src/dynamics/quadruped/model.jl:75-590   flamingo  src/dynamics/flamingo/model.jl:62-503
//
// Each model's residual is one function: the ground is a template parameter (the chains, the particle) or a nullable terrain
// (hopper_3D), and the seven rows of a contact are written by plant_contact_rows for all of them.
//
// A planar-chain model is a table: bodies and contact points are chains of (signed length, angle index) segments from the hip at
// (x, z) - a segment adds r (sin θ, -cos θ).  For such a chain with absolute angles the Lagrangian derivatives the
// integrator needs are explicit sums over the bodies,
//   D2L = dL/dq' ,   D1L = dL/dq - (d/dq dL/dq') q'      (dynamics/model.jl:11-15 with C of quadruped/model.jl:479-484),
// so no code generation is involved.  The Jacobian dr/dz comes from evaluating the same code on first-order dual
// numbers (one tangent direction per lane in the kernel): exact derivatives.
#pragma once
#include <cmath>

#include "../../../include/cimpc.h"

#if defined(__HIPCC__)
#define PLANT_HD __host__ __device__ __forceinline__
#else
#define PLANT_HD inline
#endif

namespace cimpc {

struct Dual {            // value + one tangent, eps^2 = 0
    double v, d;
};
PLANT_HD Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
PLANT_HD Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
PLANT_HD Dual operator-(Dual a) { return {-a.v, -a.d}; }
PLANT_HD Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
PLANT_HD Dual operator*(double a, Dual b) { return {a * b.v, a * b.d}; }
PLANT_HD Dual operator*(Dual a, double b) { return {a.v * b, a.d * b}; }
PLANT_HD Dual operator+(Dual a, double b) { return {a.v + b, a.d}; }
PLANT_HD Dual operator-(Dual a, double b) { return {a.v - b, a.d}; }
PLANT_HD Dual operator/(Dual a, double b) { return {a.v / b, a.d / b}; }
PLANT_HD Dual psin(Dual a) { return {sin(a.v), a.d * cos(a.v)}; }
PLANT_HD Dual pcos(Dual a) { return {cos(a.v), -a.d * sin(a.v)}; }
PLANT_HD double psin(double a) { return sin(a); }
PLANT_HD double pcos(double a) { return cos(a); }
PLANT_HD double pval(double a) { return a; }
PLANT_HD double pval(Dual a) { return a.v; }
PLANT_HD Dual operator/(Dual a, Dual b) { return {a.v / b.v, (a.d * b.v - a.v * b.d) / (b.v * b.v)}; }
PLANT_HD Dual operator/(double a, Dual b) { return {a / b.v, -a * b.d / (b.v * b.v)}; }
PLANT_HD Dual operator+(double a, Dual b) { return {a + b.v, b.d}; }
PLANT_HD Dual operator-(double a, Dual b) { return {a - b.v, -b.d}; }
PLANT_HD Dual psqrt(Dual a) { const double r = sqrt(a.v); return {r, a.d / (2.0 * r)}; }
PLANT_HD Dual pexp(Dual a) { const double e = exp(a.v); return {e, a.d * e}; }
PLANT_HD Dual plog1p(Dual a) { return {log1p(a.v), a.d / (1.0 + a.v)}; }
PLANT_HD double psqrt(double a) { return sqrt(a); }
PLANT_HD double pexp(double a) { return exp(a); }
PLANT_HD double plog1p(double a) { return log1p(a); }
PLANT_HD Dual ptanh(Dual a) { const double t = tanh(a.v); return {t, a.d * (1.0 - t * t)}; }
PLANT_HD double ptanh(double a) { return tanh(a); }
template <class T> PLANT_HD T pconst(double a);
template <> PLANT_HD double pconst<double>(double a) { return a; }
template <> PLANT_HD Dual pconst<Dual>(double a) { return {a, 0.0}; }
// θ on dual numbers (dr/dθ, plant_linearize.hip): an entry of θ is a DualTh, a Dual in every operation (an expression of θ is a
// Dual) but one - as a divisor (the time step h) its quotient's tangent is (a' - (a / b) b') / b, which with b' = 0 is a' / b rounded
// as Dual / double rounds it.  Sums and products are exact in a zero tangent, so the z-columns of a (Dual, DualTh) evaluation are the
// (Dual, double) Jacobian bit for bit (tests/test_plant_linearize.py).
struct DualTh : Dual {};
PLANT_HD Dual operator/(Dual a, DualTh b) { const double q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
// The lift of a θ-expression (type TH) into the residual's type T: with θ on dual numbers it is the identity, so
// pconst<T>(expr of θ) serves (T, TH) = (double, double), (Dual, double) and (Dual, DualTh) as written.
template <class T> PLANT_HD T pconst(Dual a);
template <> PLANT_HD Dual pconst<Dual>(Dual a) { return a; }

constexpr int PLANT_MAX_Q = 18, PLANT_MAX_U = 12, PLANT_MAX_BODIES = 9, PLANT_MAX_SEG = 3;
constexpr int PLANT_NC = 4, PLANT_NB = 16, PLANT_NW = 3;     // maxima: four contacts, two (flat_2D_lc) or four (flat_3D_lc) friction directions each
// PLANT_NW is the nw of the models with the longest θ (centroidal: 2 * 18 + 12 + 3 + 2 = 53), which is all it sizes; walledcartpole
// has nw = 4 with nθ = 15.
constexpr int PLANT_KIND_CHAIN = 0, PLANT_KIND_HOPPER_2D = 1, PLANT_KIND_CENTROIDAL = 2, PLANT_KIND_PARTICLE = 3, PLANT_KIND_PARTICLE_2D = 4;
// centroidal_quadruped_box / _wall: plant_residual_centroidal_env, stepped by their own kernel instantiations (plant_kernel.hip)
constexpr int PLANT_KIND_CENTROIDAL_BOX = 5, PLANT_KIND_CENTROIDAL_WALL = 6;
constexpr int PLANT_KIND_HOPPER_3D = 7;                      // hopper_3D: plant_residual_hopper_3d, stepped by kernel instantiations of its own size
// pushbot and walledcartpole: plant_residual_walls, stepped by a kernel instantiation of their own size (flat_2D_lc only)
constexpr int PLANT_KIND_PUSHBOT = 8, PLANT_KIND_WALLEDCARTPOLE = 9;
constexpr int PLANT_WALL_NC = 8, PLANT_WALL_NB = 32;          // the wall model: four feet on the floor and the same four on the wall

struct PlantChain { int n; double r[PLANT_MAX_SEG]; int k[PLANT_MAX_SEG]; };
struct PlantModel {
    int kind = PLANT_KIND_CHAIN;      // planar chain with absolute angles | hopper_2D (constant mass matrix, prismatic leg)
    int nc = PLANT_NC;                // contacts
    int fd = 2;                       // friction directions per contact: 2 (planar) or 4 (spatial)
    int nw = 2;                       // disturbance dimension (A = eye(nw, nq))
    int nq, nu, n_bodies;
    double g, mu_world;
    double mass[PLANT_MAX_BODIES], inertia[PLANT_MAX_BODIES];
    int own[PLANT_MAX_BODIES];
    PlantChain body[PLANT_MAX_BODIES];
    PlantChain foot[PLANT_NC];
    int tq_a[PLANT_MAX_U], tq_b[PLANT_MAX_U];     // actuator i: torque between links a and b (B = -e_a + e_b)
    double joint_friction[PLANT_MAX_Q];
    PLANT_HD int nb() const { return fd * nc; }
    PLANT_HD int nz() const { return nq + 4 * nc + 2 * nb(); }
    PLANT_HD int nth() const { return 2 * nq + nu + nw + 2; }
};

// The rows of contact c in r(z), z = [q2; γ; b; ψ; s1; η; s2] with FD friction directions per contact (2 planar: m = [1 -1]; 4 spatial:
// m = [1 0 -1 0; 0 1 0 -1]), given the contact's gap ϕ and tangential velocity vt (FD / 2 entries):
//   s1 - ϕ,   η - mᵀ v_T - Eᵀψ,   s2 - (μ γ - Σ b),   γ s1 - κ,   b ∘ η - κ,   ψ s2 - κ       (simulation.jl:141-157)
template <int FD, class T, class TH = double>
PLANT_HD void plant_contact_rows(int nq, int nc, int c, const T* z, T phi, const T* vt, TH mu, double kappa, T* r) {
    const int nb = FD * nc;
    const T* gam = z + nq; const T* b = gam + nc + FD * c; const T* psi = gam + nc + nb; const T* s1 = psi + nc;
    const T* eta = s1 + nc + FD * c; const T* s2 = s1 + nc + nb;
    r[nq + c] = s1[c] - phi;
    T* re = r + nq + nc + FD * c;
    for (int k = 0; k < FD / 2; ++k) { re[k] = eta[k] - vt[k] - psi[c]; re[FD / 2 + k] = eta[FD / 2 + k] + vt[k] - psi[c]; }
    T sb = b[0];
    for (int k = 1; k < FD; ++k) sb = sb + b[k];
    r[nq + nc + nb + c] = s2[c] - (mu * gam[c] - sb);
    r[nq + 2 * nc + nb + c] = gam[c] * s1[c] - kappa;
    for (int k = 0; k < FD; ++k) r[nq + 3 * nc + nb + FD * c + k] = b[k] * eta[k] - kappa;
    r[nq + 3 * nc + 2 * nb + c] = psi[c] * s2[c] - kappa;
}

// D1L, D2L at (q, v), accumulated into d1, d2 (nq entries each, zeroed here)
template <class T>
PLANT_HD void plant_lagrangian_derivatives(const PlantModel& M, const T* q, const T* v, T* d1, T* d2) {
    T s[PLANT_MAX_Q], c[PLANT_MAX_Q];
    if (M.kind == PLANT_KIND_HOPPER_2D) {
        // hopper_2D/model.jl:41-55: M = diag(mb + ml, mb + ml, Jb + Jl, ml) (kept in mass[0..3]), C = (0, (mb + ml) g, 0, 0);
        // lagrangian = 0, so D1L = -C and D2L = M v (dynamics/model.jl:11-15)
        for (int i = 0; i < 4; ++i) { d1[i] = pconst<T>(0.0); d2[i] = M.mass[i] * v[i]; }
        d1[1] = pconst<T>(-(M.mass[1] * M.g));
        return;
    }
    for (int i = 0; i < M.nq; ++i) { d1[i] = pconst<T>(0.0); d2[i] = pconst<T>(0.0); s[i] = psin(q[i]); c[i] = pcos(q[i]); }
    for (int b = 0; b < M.n_bodies; ++b) {
        const double m = M.mass[b];
        const PlantChain& ch = M.body[b];
        T vx = v[0], vz = v[1], ax = pconst<T>(0.0), az = pconst<T>(0.0);
        for (int e = 0; e < ch.n; ++e) {
            const int k = ch.k[e]; const double r = ch.r[e];
            vx = vx + r * (c[k] * v[k]);
            vz = vz + r * (s[k] * v[k]);
            ax = ax - r * (s[k] * (v[k] * v[k]));      // derivative of the body velocity along q' in q
            az = az + r * (c[k] * (v[k] * v[k]));
        }
        d2[0] = d2[0] + m * vx;
        d2[1] = d2[1] + m * vz;
        d1[0] = d1[0] - m * ax;
        d1[1] = d1[1] - (m * az + m * M.g);
        for (int e = 0; e < ch.n; ++e) {
            const int k = ch.k[e]; const double r = ch.r[e];
            d2[k] = d2[k] + (r * m) * (c[k] * vx + s[k] * vz);
            // dL/dθ_k - d(dL/dθ'_k)/dq q': the velocity-product terms cancel, gravity and the centripetal part stay
            d1[k] = d1[k] - ((m * M.g * r) * s[k] + (r * m) * (c[k] * ax + s[k] * az));
        }
        d2[M.own[b]] = d2[M.own[b]] + M.inertia[b] * v[M.own[b]];
    }
}

// ---- centroidal_quadruped (src/dynamics/centroidal_quadruped/model.jl): q = (body position, body orientation, four foot
// positions), one rigid body + point feet.  M = blkdiag(m_b I, I_b, m_f I_12) (:67-74), C = (m_b g e_z, w x I_b w, m_f g e_z ...)
// (:76-85) with lagrangian = 0, so D1L = -C, D2L = M v; B(q)^T u = (sum u_i, sum R^T skew(r_i) u_i, -u_1 .. -u_4) with the
// Euler rotation R of euler.jl:3-11 and r_i = foot_i - body (:98-121); contacts are the feet themselves (J = selection, :129-138),
// four friction directions per contact (flat_3D_lc: m = [1 0 -1 0; 0 1 0 -1]).  mass[0] = m_b, mass[1] = m_f, inertia[0..2] = I_b.
template <class T>
PLANT_HD void plant_centroidal_derivatives(const PlantModel& M, const T* v, T* d1, T* d2) {
    const double mb = M.mass[0], mf = M.mass[1];
    const double I0 = M.inertia[0], I1 = M.inertia[1], I2 = M.inertia[2];
    for (int i = 0; i < 3; ++i) { d2[i] = mb * v[i]; d1[i] = pconst<T>(i == 2 ? -mb * M.g : 0.0); }
    const T wx = v[3], wy = v[4], wz = v[5];
    d2[3] = I0 * wx; d2[4] = I1 * wy; d2[5] = I2 * wz;
    // -(w x I w)
    d1[3] = -(wy * (I2 * wz) - wz * (I1 * wy));
    d1[4] = -(wz * (I0 * wx) - wx * (I2 * wz));
    d1[5] = -(wx * (I1 * wy) - wy * (I0 * wx));
    for (int i = 6; i < 18; ++i) { d2[i] = mf * v[i]; d1[i] = pconst<T>((i % 3) == 2 ? -mf * M.g : 0.0); }
}
// dyn += B(qm2)^T u: (sum u_i, sum R^T skew(r_i) u_i, -u_1 .. -u_4), centroidal_quadruped/model.jl:98-121 (the box and the wall
// share it, centroidal_quadruped_box/model.jl:109-131, centroidal_quadruped_wall/model.jl:102-124)
template <class T, class TH = double>
PLANT_HD void plant_centroidal_actuation(const T* qm2, const TH* u1, T* dyn) {
    const T sa = psin(qm2[3]), ca = pcos(qm2[3]), sb = psin(qm2[4]), cb = pcos(qm2[4]), sc = psin(qm2[5]), cc = pcos(qm2[5]);
    T R[3][3];
    R[0][0] = ca * cb; R[0][1] = ca * sb * sc - sa * cc; R[0][2] = ca * sb * cc + sa * sc;
    R[1][0] = sa * cb; R[1][1] = sa * sb * sc + ca * cc; R[1][2] = sa * sb * cc - ca * sc;
    R[2][0] = -sb;     R[2][1] = cb * sc;                R[2][2] = cb * cc;
    for (int f = 0; f < 4; ++f) {
        const TH ux = u1[3 * f], uy = u1[3 * f + 1], uz = u1[3 * f + 2];
        const T rx = qm2[6 + 3 * f] - qm2[0], ry = qm2[7 + 3 * f] - qm2[1], rz = qm2[8 + 3 * f] - qm2[2];
        // skew(r) u = r x u
        const T cx = ry * uz - rz * uy, cy = rz * ux - rx * uz, cz = rx * uy - ry * ux;
        dyn[0] = dyn[0] + ux; dyn[1] = dyn[1] + uy; dyn[2] = dyn[2] + uz;
        for (int k = 0; k < 3; ++k) dyn[3 + k] = dyn[3 + k] + (R[0][k] * cx + R[1][k] * cy + R[2][k] * cz);      // R^T (r x u)
        dyn[6 + 3 * f] = dyn[6 + 3 * f] - ux; dyn[7 + 3 * f] = dyn[7 + 3 * f] - uy; dyn[8 + 3 * f] = dyn[8 + 3 * f] - uz;
    }
}
// the dynamics rows before the contact forces: integrator (dynamics/model.jl:11-36) with the joint damping, B(qm2)^T u and A^T w
template <class T, class TH = double>
PLANT_HD void plant_centroidal_dynamics(const PlantModel& M, const T* q2, const TH* th, T* dyn) {
    constexpr int nq = 18, nu = 12;
    const TH* q0 = th; const TH* q1 = th + nq; const TH* u1 = th + 2 * nq; const TH* w1 = u1 + nu;
    const TH h = w1[4];
    T qm2[nq], vm1[nq], vm2[nq];
    for (int i = 0; i < nq; ++i) { vm1[i] = pconst<T>((q1[i] - q0[i]) / h); qm2[i] = (q2[i] + q1[i]) * 0.5; vm2[i] = (q2[i] - q1[i]) / h; }
    T a1[nq], b1[nq], a2[nq], b2[nq];
    plant_centroidal_derivatives(M, vm1, a1, b1);
    plant_centroidal_derivatives(M, vm2, a2, b2);
    for (int i = 0; i < nq; ++i)
        dyn[i] = (0.5 * h) * a1[i] + b1[i] + (0.5 * h) * a2[i] - b2[i] - (h * M.joint_friction[i]) * vm2[i];
    plant_centroidal_actuation(qm2, u1, dyn);
    for (int i = 0; i < 3; ++i) dyn[i] = dyn[i] + w1[i];
}

// centroidal_quadruped: the four feet on the floor, phi_i = p_z,i.  It equals plant_residual_centroidal_env on this model bit for bit
// (tests/test_centroidal_wall_box.py) and stays a function of its own with compile-time loops: through the env function the FLAT
// kernel measured 2.4 % slower, and with a compile-time contact count there the TERRAIN kernel's scratch grew.
template <class T, class TH = double>
PLANT_HD void plant_residual_centroidal(const PlantModel& M, const T* z, const TH* th, double kappa, T* r) {
    constexpr int nq = 18, nc = 4;
    const TH* q1 = th + nq; const TH mu = th[2 * nq + 12 + 3], h = th[2 * nq + 12 + 4];
    const T* q2 = z; const T* gam = z + nq; const T* b = gam + nc;
    T dyn[nq];
    plant_centroidal_dynamics(M, q2, th, dyn);
    for (int f = 0; f < nc; ++f) {
        const T* bf = b + 4 * f;
        // J^T lambda: the foot's own coordinates, lambda = [m b; gamma]
        dyn[6 + 3 * f] = dyn[6 + 3 * f] + (bf[0] - bf[2]);
        dyn[7 + 3 * f] = dyn[7 + 3 * f] + (bf[1] - bf[3]);
        dyn[8 + 3 * f] = dyn[8 + 3 * f] + gam[f];
        const T vt[2] = {(q2[6 + 3 * f] - q1[6 + 3 * f]) / h, (q2[7 + 3 * f] - q1[7 + 3 * f]) / h};
        plant_contact_rows<4>(nq, nc, f, z, q2[8 + 3 * f], vt, mu, kappa, r);
    }
    for (int i = 0; i < nq; ++i) r[i] = dyn[i];
}

// ---- centroidal_quadruped_box (src/dynamics/centroidal_quadruped_box/model.jl) and centroidal_quadruped_wall
// (src/dynamics/centroidal_quadruped_wall/model.jl): the centroidal model (same M, C, B, A; plant_centroidal_dynamics) with
// other contacts.  Both files define only the damped model (box :221-230, wall :226-235); the box's feet weigh 0.5 (:219).
//   box   nc 4: phi_i = p_z,i - e(p_x,i), e(x) = 0.2 (1 + tanh(200 (x - 0.25))) / 2 (:87-107).  The reference rotates neither J
//         nor the force on the step edge: the normal stays vertical (its behaviour, kept).
//   wall  nc 8: contacts 1-4 are the feet on the floor; 5-8 the same feet against the plane x = 0.25 (:87-99), phi = 0.25 - p_x,
//         J rows = the feet's rows again (:132-145), force [-gamma; m b] on (x; y, z) (:147-160), tangential velocity
//         m^T (v_y, v_z) (:162-173).
// mass[1] = m_f; nc = 4 (box) or 8 (wall).
template <class T>
PLANT_HD T plant_box_elevation(T x) {
    return 0.1 * (1.0 + ptanh(200.0 * (x - 0.25)));
}
template <class T, class TH = double>
PLANT_HD void plant_residual_centroidal_env(const PlantModel& M, const T* z, const TH* th, double kappa, T* r) {
    constexpr int nq = 18;
    const int nc = M.nc;
    const TH* q1 = th + nq; const TH mu = th[2 * nq + 12 + 3], h = th[2 * nq + 12 + 4];
    const T* q2 = z; const T* gam = z + nq; const T* b = gam + nc;
    T dyn[nq];
    plant_centroidal_dynamics(M, q2, th, dyn);
    for (int c = 0; c < nc; ++c) {
        const int f = c & 3;                                          // the foot of contact c
        const T* bc = b + 4 * c;
        const T t1 = bc[0] - bc[2], t2 = bc[1] - bc[3];                // m b
        const T* p2 = q2 + 6 + 3 * f; const TH* p1 = q1 + 6 + 3 * f;
        T phi, vt[2];
        if (c < 4) {                                                   // floor: force (m b; gamma) on the foot's own coordinates, velocity (v_x, v_y)
            dyn[6 + 3 * f] = dyn[6 + 3 * f] + t1;
            dyn[7 + 3 * f] = dyn[7 + 3 * f] + t2;
            dyn[8 + 3 * f] = dyn[8 + 3 * f] + gam[c];
            phi = M.kind == PLANT_KIND_CENTROIDAL_BOX ? p2[2] - plant_box_elevation(p2[0]) : p2[2];
            vt[0] = (p2[0] - p1[0]) / h; vt[1] = (p2[1] - p1[1]) / h;
        } else {                                                       // wall: force (-gamma; m b), velocity (v_y, v_z)
            dyn[6 + 3 * f] = dyn[6 + 3 * f] - gam[c];
            dyn[7 + 3 * f] = dyn[7 + 3 * f] + t1;
            dyn[8 + 3 * f] = dyn[8 + 3 * f] + t2;
            phi = 0.25 - p2[0];
            vt[0] = (p2[1] - p1[1]) / h; vt[1] = (p2[2] - p1[2]) / h;
        }
        plant_contact_rows<4>(nq, nc, c, z, phi, vt, mu, kappa, r);
    }
    for (int i = 0; i < nq; ++i) r[i] = dyn[i];
}

// ---- terrain (src/simulator/environment.jl, src/simulation/environments/*.jl) ----------------
// surf(x[, y]) and its gradient on T = double | Dual, so the dual-number Jacobian carries d(surface)/dq and d(rotation)/dq.
// Branches (piece of a PIECEWISE table, sign in the softplus) are taken on the value, like the reference's IfElse.
template <class T>
PLANT_HD void terrain_eval(const cimpc_terrain& E, T x, T y, T& s, T& gx, T& gy) {
    const double* p = E.p;
    gy = pconst<T>(0.0);
    switch (E.kind) {
    case CIMPC_TERRAIN_PIECEWISE: {
        int i = 0;
        for (int k = 1; k < E.n_pieces; ++k) if (pval(x) >= E.brk[k]) i = k;
        const double* a = E.coef[i];
        const T t = x - E.off[i];
        s = ((a[3] * t + a[2]) * t + a[1]) * t + a[0];
        gx = (3.0 * a[3] * t + 2.0 * a[2]) * t + a[1];
        return;
    }
    case CIMPC_TERRAIN_SOFTPLUS: {          // (m / t) log(1 + e^u), u = t (x - x0); gradient m e^u / (1 + e^u)
        const T u = p[1] * (x - p[2]);
        if (pval(u) > 0.0) {
            const T e = pexp(-u);
            s = (p[0] / p[1]) * (u + plog1p(e));
            gx = p[0] / (1.0 + e);
        } else {
            const T e = pexp(u);
            s = (p[0] / p[1]) * plog1p(e);
            gx = (p[0] * e) / (1.0 + e);
        }
        return;
    }
    case CIMPC_TERRAIN_SINE: {
        const T c = pcos(p[2] * x), sn = psin(p[2] * x);
        s = (p[0] * c + p[1] * sn) + p[3];
        gx = p[2] * (p[1] * c - p[0] * sn);
        return;
    }
    case CIMPC_TERRAIN_SINE_SUM_3D:
        s = p[0] * psin(p[1] * x) + p[2] * psin(p[3] * y);
        gx = (p[0] * p[1]) * pcos(p[1] * x);
        gy = (p[2] * p[3]) * pcos(p[3] * y);
        return;
    case CIMPC_TERRAIN_SINE_PRODUCT_3D: {
        const T sx = psin(p[1] * x), sy = psin(p[1] * y);
        s = p[0] * (sx * sy);
        gx = (p[0] * p[1]) * (pcos(p[1] * x) * sy);
        gy = (p[0] * p[1]) * (sx * pcos(p[1] * y));
        return;
    }
    case CIMPC_TERRAIN_BOWL_3D:
        s = p[0] * (x * x + y * y);
        gx = (2.0 * p[0]) * x;
        gy = (2.0 * p[0]) * y;
        return;
    default:
        s = pconst<T>(0.0); gx = pconst<T>(0.0);
        return;
    }
}
PLANT_HD bool terrain_is_3d(int kind) {
    return kind == CIMPC_TERRAIN_SINE_SUM_3D || kind == CIMPC_TERRAIN_SINE_PRODUCT_3D || kind == CIMPC_TERRAIN_BOWL_3D;
}

// 2-D contact frame: rotation(env, x) of environment.jl:79-92 in closed form (no atan): the angle between the world normal and
// n = (-g, 1) / sqrt(1 + g^2) is -atan(g), so R = [c -s; s c] with c = 1 / sqrt(1 + g^2), s = -g c.  The foot's world force is
// R^T [lt; γ], its tangential velocity the first entry of R v.
template <class T>
PLANT_HD void terrain_frame_2d(const cimpc_terrain& E, T px, T& surf, T& c, T& s) {
    T gx, gy;
    terrain_eval(E, px, pconst<T>(0.0), surf, gx, gy);
    c = 1.0 / psqrt(1.0 + gx * gx);
    s = -(gx * c);
}

// 3-D contact frame: R = rot(n_s, e_z) = I + [v]x + [v]x^2 / (1 + c), v = n_s x e_z = (n_y, -n_x, 0), c = n_z (environment.jl:58-77),
// written out, with the surface normal n_s = (-g_x, -g_y, 1) / |.| at (x, y).
template <class T>
PLANT_HD void terrain_frame_3d(const cimpc_terrain& E, T x, T y, T& surf, T R[3][3]) {
    T gx, gy;
    terrain_eval(E, x, y, surf, gx, gy);
    const T inv = 1.0 / psqrt(1.0 + gx * gx + gy * gy);
    const T nx = -(gx * inv), ny = -(gy * inv), nz = inv;
    const T vx = ny, vy = -nx, k = 1.0 / (1.0 + nz);
    R[0][0] = 1.0 - k * (vy * vy); R[0][1] = k * (vx * vy);       R[0][2] = vy;
    R[1][0] = k * (vx * vy);       R[1][1] = 1.0 - k * (vx * vx); R[1][2] = -vx;
    R[2][0] = -vy;                 R[2][1] = vx;                  R[2][2] = 1.0 - k * (vx * vx + vy * vy);
}
// ---- particle (src/dynamics/particle/model.jl): a point mass that is its own contact point; M = m I, C = (0, 0, m g),
// B = A = J = I, four friction directions.  mass[0] = m.  ROUGH = false is flat_3D_lc (E unused); ROUGH = true is a 3-D surface
// (particle/model.jl:58-109): force R^T [m b; γ], tangential velocity (R v)[0:2], ϕ = z - surf(x, y).  The ground is a compile-time
// choice, as for the chains: behind a run-time branch the device compiler contracts these rows differently.
template <bool ROUGH, class T, class TH = double>
PLANT_HD void plant_residual_particle(const PlantModel& M, const cimpc_terrain* E, const T* z, const TH* th, double kappa, T* r) {
    const TH* q0 = th; const TH* q1 = th + 3; const TH* u1 = th + 6; const TH* w1 = th + 9;
    const TH mu = th[12], h = th[13];
    const double m = M.mass[0];
    const T* q2 = z; const T* gam = z + 3; const T* b = z + 4;
    T surf{}, R[3][3];
    if constexpr (ROUGH) terrain_frame_3d(*E, q2[0], q2[1], surf, R);
    const T fl[3] = {b[0] - b[2], b[1] - b[3], gam[0]};
    T vm2[3];
    for (int i = 0; i < 3; ++i) vm2[i] = (q2[i] - q1[i]) / h;
    for (int i = 0; i < 3; ++i) {
        const double grav = i == 2 ? -m * M.g : 0.0;
        T lam = fl[i];
        if constexpr (ROUGH) lam = R[0][i] * fl[0] + R[1][i] * fl[1] + R[2][i] * fl[2];
        r[i] = pconst<T>(0.5 * h * grav + m * ((q1[i] - q0[i]) / h) + 0.5 * h * grav + u1[i] + w1[i]) - m * vm2[i] + lam;
    }
    T vt[2] = {vm2[0], vm2[1]}, phi = q2[2];
    if constexpr (ROUGH) {
        for (int k = 0; k < 2; ++k) vt[k] = R[k][0] * vm2[0] + R[k][1] * vm2[1] + R[k][2] * vm2[2];
        phi = q2[2] - surf;
    }
    plant_contact_rows<4>(3, 1, 0, z, phi, vt, mu, kappa, r);
}

// particle_2D (src/dynamics/particle_2D/model.jl): q = (x, z), M = m I, C = (0, m g), B = A = J = I, one contact (the particle)
// with two friction directions.  mass[0] = m.  Also its flat case: the model has no cimpc_plant_step path.
template <class T, class TH = double>
PLANT_HD void plant_residual_particle_2d(const PlantModel& M, const cimpc_terrain& E, const T* z, const TH* th, double kappa, T* r) {
    const TH* q0 = th; const TH* q1 = th + 2; const TH* u1 = th + 4; const TH* w1 = th + 6;
    const TH mu = th[8], h = th[9];
    const double m = M.mass[0];
    const T* q2 = z; const T* gam = z + 2; const T* b = z + 3;
    T surf, c, s;
    terrain_frame_2d(E, q2[0], surf, c, s);
    const T lt = b[0] - b[1];
    const T lam[2] = {c * lt + s * gam[0], c * gam[0] - s * lt};
    T vm2[2];
    for (int i = 0; i < 2; ++i) vm2[i] = (q2[i] - q1[i]) / h;
    for (int i = 0; i < 2; ++i) {
        const double grav = i == 1 ? -m * M.g : 0.0;
        r[i] = pconst<T>(0.5 * h * grav + m * ((q1[i] - q0[i]) / h) + 0.5 * h * grav + u1[i] + w1[i]) - m * vm2[i] + lam[i];
    }
    const T vt = c * vm2[0] - s * vm2[1];
    plant_contact_rows<2>(2, 1, 0, z, q2[1] - surf, &vt, mu, kappa, r);
}

// ---- hopper_3D (src/dynamics/hopper_3D/model.jl): q = (body position, modified Rodrigues parameters p, leg length l), all mass
// at the body: M = diag(mb + ml x3, Jb + Jl x3, ml) (mass[0..6]), C = (0, 0, (mb + ml) g, 0...), lagrangian = 0 (:30-48); the one
// contact is the foot k = pos - R(p) e_3 l (:33-37), four friction directions; B(qm2)^T u = (R e_3 u_3; R[:, 1:2] u_{1:2}; u_3)
// (:54-60), A = eye(3, 7).  R is the standard rotation of the parameters, R = I + (8 S^2 + 4 (1 - |p|^2) S) / (1 + |p|^2)^2 with
// S = skew(p): the convention the model's gait files satisfy (tests/test_hopper_3d.py).
template <class T>
PLANT_HD void plant_mrp_rotation(const T* p, T R[3][3]) {
    const T n = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    const T c = 1.0 / ((1.0 + n) * (1.0 + n)), f = 4.0 * (1.0 - n);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = c * (8.0 * (p[i] * p[j]));
    for (int i = 0; i < 3; ++i) R[i][i] = R[i][i] + (1.0 - c * (8.0 * n));
    R[0][1] = R[0][1] - c * (f * p[2]); R[0][2] = R[0][2] + c * (f * p[1]);
    R[1][0] = R[1][0] + c * (f * p[2]); R[1][2] = R[1][2] - c * (f * p[0]);
    R[2][0] = R[2][0] - c * (f * p[1]); R[2][1] = R[2][1] + c * (f * p[0]);
}
// a = R(p) e_3 and D[i][j] = da_i / dp_j.  The reference takes J = dk/dq from ForwardDiff (:70-73); a one-tangent dual cannot nest,
// so the derivative is written out: a = e_3 + N / d, N = 8 (p_x p_z, p_y p_z, p_z^2 - |p|^2) + 4 (1 - |p|^2) (p_y, -p_x, 0),
// d = (1 + |p|^2)^2, da_i/dp_j = (dN_i/dp_j - 4 N_i p_j / (1 + |p|^2)) / d.
template <class T>
PLANT_HD void plant_mrp_axis(const T* p, T a[3], T D[3][3]) {
    const T px = p[0], py = p[1], pz = p[2];
    const T n = px * px + py * py + pz * pz;
    const T c = 1.0 / ((1.0 + n) * (1.0 + n)), f = 4.0 * (1.0 - n), g = 4.0 / (1.0 + n);
    const T N[3] = {8.0 * (px * pz) + f * py, 8.0 * (py * pz) - f * px, -8.0 * (px * px + py * py)};
    T dN[3][3];
    dN[0][0] = 8.0 * pz - 8.0 * (px * py);  dN[0][1] = f - 8.0 * (py * py);         dN[0][2] = 8.0 * px - 8.0 * (py * pz);
    dN[1][0] = 8.0 * (px * px) - f;         dN[1][1] = 8.0 * pz + 8.0 * (px * py);  dN[1][2] = 8.0 * py + 8.0 * (px * pz);
    dN[2][0] = -16.0 * px;                  dN[2][1] = -16.0 * py;                  dN[2][2] = pconst<T>(0.0);
    for (int i = 0; i < 3; ++i) {
        a[i] = c * N[i];
        for (int j = 0; j < 3; ++j) D[i][j] = c * (dN[i][j] - (g * N[i]) * p[j]);
    }
    a[2] = a[2] + 1.0;
}
// Both grounds: E = nullptr (or a flat E) is flat_3D_lc, surface rotation = identity; otherwise surface and rotation are taken at
// the foot k[0:2] as the particle takes them at itself: force Rs^T [m b; γ], tangential velocity (Rs J (q2 - q1) / h)[0:2],
// ϕ = k_z - surf(k_x, k_y) (:50-52, :75-87).
template <class T, class TH = double>
PLANT_HD void plant_residual_hopper_3d(const PlantModel& M, const cimpc_terrain* E, const T* z, const TH* th, double kappa, T* r) {
    constexpr int nq = 7;
    const TH* q0 = th; const TH* q1 = th + 7; const TH* u1 = th + 14; const TH* w1 = th + 17;
    const TH mu = th[20], h = th[21];
    const T* q2 = z; const T* gam = z + 7; const T* b = z + 8;
    T qm2[nq], vm2[nq], dyn[nq];
    for (int i = 0; i < nq; ++i) { qm2[i] = (q2[i] + q1[i]) * 0.5; vm2[i] = (q2[i] - q1[i]) / h; }
    // 0.5 h D1L + D2L at (qm1, vm1), 0.5 h D1L - D2L at (qm2, vm2): D1L = -C, D2L = M v
    for (int i = 0; i < nq; ++i) dyn[i] = pconst<T>(M.mass[i] * ((q1[i] - q0[i]) / h)) - M.mass[i] * vm2[i];
    dyn[2] = dyn[2] - h * (M.mass[2] * M.g);
    T Rm[3][3];
    plant_mrp_rotation(qm2 + 3, Rm);
    for (int i = 0; i < 3; ++i) {
        dyn[i] = dyn[i] + Rm[i][2] * u1[2] + w1[i];
        dyn[3 + i] = dyn[3 + i] + (Rm[i][0] * u1[0] + Rm[i][1] * u1[1]);
    }
    dyn[6] = dyn[6] + u1[2];
    // the foot k = pos - a l at q2, J = [I, -l da/dp, -a], its velocity J (q2 - q1) / h
    T a[3], D[3][3], k[3], v[3];
    plant_mrp_axis(q2 + 3, a, D);
    const T l = q2[6];
    for (int i = 0; i < 3; ++i) {
        k[i] = q2[i] - a[i] * l;
        v[i] = vm2[i] - l * (D[i][0] * vm2[3] + D[i][1] * vm2[4] + D[i][2] * vm2[5]) - a[i] * vm2[6];
    }
    const T fl[3] = {b[0] - b[2], b[1] - b[3], gam[0]};
    T F[3], vt[2], phi;
    if (E && E->kind != CIMPC_TERRAIN_FLAT) {
        T surf, R[3][3];
        terrain_frame_3d(*E, k[0], k[1], surf, R);
        for (int i = 0; i < 3; ++i) F[i] = R[0][i] * fl[0] + R[1][i] * fl[1] + R[2][i] * fl[2];
        for (int i = 0; i < 2; ++i) vt[i] = R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2];
        phi = k[2] - surf;
    } else {
        for (int i = 0; i < 3; ++i) F[i] = fl[i];
        vt[0] = v[0]; vt[1] = v[1];
        phi = k[2];
    }
    // J^T F
    for (int i = 0; i < 3; ++i) dyn[i] = dyn[i] + F[i];
    for (int j = 0; j < 3; ++j) dyn[3 + j] = dyn[3 + j] - l * (D[0][j] * F[0] + D[1][j] * F[1] + D[2][j] * F[2]);
    dyn[6] = dyn[6] - (a[0] * F[0] + a[1] * F[1] + a[2] * F[2]);
    for (int i = 0; i < nq; ++i) r[i] = dyn[i];
    plant_contact_rows<4>(nq, 1, 0, z, phi, vt, mu, kappa, r);
}

// ---- pushbot (src/dynamics/pushbot/model.jl) and walledcartpole (src/dynamics/walledcartpole/model.jl): one point between two
// walls, nc = 2, flat_2D_lc (surface rotation = identity), so the generic contact_forces and velocity_stack (contact_methods.jl:27-48)
// are the force [m b; γ] and the stack (v_T, -v_T) of plant_contact_rows<2>.  A = I on all nq coordinates.
//   pushbot         q = (θ, d): a pendulum of length l with a sliding arm; the point p = (-l sinθ + d cosθ, l cosθ + d sinθ) between walls at
//                   x = -+0.5.  M = mb Jcᵀ Jc + ma Jdᵀ Jd and C from the Lagrangian (:66-85), Bᵀu = (l u_1 + u_2, u_1 + u_2 / l) (:106-109).
//                   mass = (mb, ma), inertia = (l, half the distance between the walls).
//   walledcartpole  q = (θ, x, xw1, xw2): the tip p = (x - l sinθ, l cosθ) between two walls on springs at -w + xw1 and w + xw2; M and C
//                   from the Lagrangian (:75-99, with the pole's lc in the place of l), Bᵀu = (0, u, 0, 0) (:119-121).
//                   mass = (mb, mt, mw), inertia = (l, w, lc, k).
// Contact 1 is the left wall, contact 2 the right one: with G_i the 2 x nq Jacobian of p minus wall i's own coordinate, the rows are
// r1 G_1 and r2 G_2, r1 = [0 -1; 1 0] = -r2 (pushbot :98-104, walledcartpole :111-117): tangent -+G_z, normal +-G_x.
template <class T>
PLANT_HD void plant_walls_derivatives(const PlantModel& M, const T* q, const T* v, T* d1, T* d2) {
    const T s = psin(q[0]), c = pcos(q[0]);
    if (M.kind == PLANT_KIND_PUSHBOT) {
        const double mb = M.mass[0], ma = M.mass[1], l = M.inertia[0];
        const T d = q[1];
        d2[0] = (mb * l * l + ma * (l * l)) * v[0] + ma * ((d * d) * v[0]) - (ma * l) * v[1];
        d2[1] = ma * v[1] - (ma * l) * v[0];
        d1[0] = -((2.0 * ma) * (d * (v[1] * v[0])) - (mb * M.g * l) * s - (ma * M.g) * (l * s - d * c));
        d1[1] = -((ma * M.g) * s - ma * (d * (v[0] * v[0])));
        return;
    }
    const double mb = M.mass[0], mt = M.mass[1], mw = M.mass[2], lc = M.inertia[2], k = M.inertia[3];
    d2[0] = (mt * lc * lc) * v[0] - (mt * lc) * (c * v[1]);
    d2[1] = (mt + mb) * v[1] - (mt * lc) * (c * v[0]);
    d2[2] = mw * v[2];
    d2[3] = mw * v[3];
    d1[0] = (mt * M.g * lc) * s;
    d1[1] = -((mt * lc) * ((v[0] * v[0]) * s));
    d1[2] = -((2.0 * k) * q[2]);
    d1[3] = -((2.0 * k) * q[3]);
}
template <class T, class TH = double>
PLANT_HD void plant_residual_walls(const PlantModel& M, const T* z, const TH* th, double kappa, T* r) {
    constexpr int MQ = 4, nc = 2;
    const int nq = M.nq, nu = M.nu;
    const bool push = M.kind == PLANT_KIND_PUSHBOT;
    const TH* q0 = th; const TH* q1 = th + nq; const TH* u1 = th + 2 * nq; const TH* w1 = u1 + nu;
    const TH mu = w1[M.nw], h = w1[M.nw + 1];
    const double l = M.inertia[0], wall = M.inertia[1];
    const T* q2 = z; const T* gam = z + nq; const T* b = gam + nc;
    T qm1[MQ]{}, vm1[MQ]{}, qm2[MQ]{}, vm2[MQ]{};       // pushbot fills two of the four
    for (int i = 0; i < nq; ++i) {
        qm1[i] = pconst<T>(0.5 * (q0[i] + q1[i])); vm1[i] = pconst<T>((q1[i] - q0[i]) / h);
        qm2[i] = (q2[i] + q1[i]) * 0.5; vm2[i] = (q2[i] - q1[i]) / h;
    }
    T a1[MQ], b1[MQ], a2[MQ], b2[MQ], dyn[MQ];
    plant_walls_derivatives(M, qm1, vm1, a1, b1);
    plant_walls_derivatives(M, qm2, vm2, a2, b2);
    for (int i = 0; i < nq; ++i)
        dyn[i] = (0.5 * h) * a1[i] + b1[i] + (0.5 * h) * a2[i] - b2[i] - (h * M.joint_friction[i]) * vm2[i];
    if (push) { dyn[0] = dyn[0] + (l * u1[0] + u1[1]); dyn[1] = dyn[1] + (u1[0] + u1[1] / l); }      // B is constant
    else dyn[1] = dyn[1] + u1[0];
    for (int i = 0; i < M.nw; ++i) dyn[i] = dyn[i] + w1[i];
    // the point at q2: its x and the two rows of its Jacobian on (q_0, q_1)
    const T s = psin(q2[0]), c = pcos(q2[0]);
    T px, gx[2], gz[2];
    if (push) {
        const T d = q2[1];
        px = d * c - l * s;
        gx[0] = -(l * c) - d * s; gx[1] = c;
        gz[0] = d * c - l * s;    gz[1] = s;
    } else {
        px = q2[1] - l * s;
        gx[0] = -(l * c); gx[1] = pconst<T>(1.0);
        gz[0] = -(l * s); gz[1] = pconst<T>(0.0);
    }
    for (int i = 0; i < nc; ++i) {
        const double sg = i == 0 ? 1.0 : -1.0;
        const T lt = b[2 * i] - b[2 * i + 1];
        // Jᵀ λ with tangent row -sg G_z and normal row sg G_x; the cart-pole's wall i adds -1 on its own coordinate of G_x
        const T fx = sg * gam[i], fz = -(sg * lt);
        dyn[0] = dyn[0] + (gx[0] * fx + gz[0] * fz);
        dyn[1] = dyn[1] + (gx[1] * fx + gz[1] * fz);
        T phi = sg * px + wall;
        if (!push) { dyn[2 + i] = dyn[2 + i] - fx; phi = phi - sg * q2[2 + i]; }
        const T vt = -(sg * (gz[0] * vm2[0] + gz[1] * vm2[1]));
        plant_contact_rows<2>(nq, nc, i, z, phi, &vt, mu, kappa, r);
    }
    for (int i = 0; i < nq; ++i) r[i] = dyn[i];
}

// ---- planar chains and hopper_2D: r(z, θ, κ), z = [q2; γ; b; ψ; s1; η; s2], θ = [q0; q1; u1; w1; μ; h].
// θ has a type of its own, TH: double (the default) where only dr/dz is needed (the step kernel), Dual where dr/dθ is too
// (plant_linearize.hip); every residual above takes it the same way.
// ROUGH = false is flat ground (E unused): ϕ = p_z, force [m b; γ], tangential velocity v_x.  ROUGH = true, on terrain E, has per
// contact i at foot p_i ϕ_i = p_z - surf(p_x), the world force R_i^T [m b_i; γ_i] through both Jacobian rows of the foot and the
// tangential velocity (R_i J_i (q2 - q1) / h)[1] (simulation.jl:133-158, contact_methods.jl, quadruped/model.jl:472-492,
// hopper_2D/model.jl:54-85).  Each contact's rotation is taken at its own foot.
template <bool ROUGH, class T, class TH = double>
PLANT_HD void plant_residual_chain(const PlantModel& M, const cimpc_terrain* E, const T* z, const TH* th, double kappa, T* r) {
    const int nq = M.nq, nu = M.nu, nc = M.nc;
    const bool hopper = M.kind == PLANT_KIND_HOPPER_2D;
    const TH* q0 = th; const TH* q1 = th + nq; const TH* u1 = th + 2 * nq; const TH* w1 = u1 + nu;
    const TH mu = w1[M.nw], h = w1[M.nw + 1];
    const T* q2 = z; const T* gam = z + nq; const T* b = gam + nc;
    T qm1[PLANT_MAX_Q], vm1[PLANT_MAX_Q], qm2[PLANT_MAX_Q], vm2[PLANT_MAX_Q];
    for (int i = 0; i < nq; ++i) {
        qm1[i] = pconst<T>(0.5 * (q0[i] + q1[i])); vm1[i] = pconst<T>((q1[i] - q0[i]) / h);
        qm2[i] = (q2[i] + q1[i]) * 0.5; vm2[i] = (q2[i] - q1[i]) / h;
    }
    T a1[PLANT_MAX_Q], b1[PLANT_MAX_Q], a2[PLANT_MAX_Q], b2[PLANT_MAX_Q];
    plant_lagrangian_derivatives(M, qm1, vm1, a1, b1);
    plant_lagrangian_derivatives(M, qm2, vm2, a2, b2);
    T dyn[PLANT_MAX_Q];
    for (int i = 0; i < nq; ++i)
        dyn[i] = (0.5 * h) * a1[i] + b1[i] + (0.5 * h) * a2[i] - b2[i] - (h * M.joint_friction[i]) * vm2[i];
    if (hopper) {
        // B(qm2)^T u, hopper_2D/model.jl:68-71: body torque on t; leg force along the leg axis (-sin t, cos t) and on r
        const T st = psin(qm2[2]), ct = pcos(qm2[2]);
        dyn[2] = dyn[2] + u1[0];
        dyn[0] = dyn[0] - u1[1] * st; dyn[1] = dyn[1] + u1[1] * ct; dyn[3] = dyn[3] + u1[1];
    } else {
        for (int i = 0; i < nu; ++i) { dyn[M.tq_a[i]] = dyn[M.tq_a[i]] - u1[i]; dyn[M.tq_b[i]] = dyn[M.tq_b[i]] + u1[i]; }
    }
    for (int i = 0; i < M.nw; ++i) dyn[i] = dyn[i] + w1[i];
    // contacts: position, velocity J (q2 - q1) / h and Jacobian rows (x and z) of every foot at q2; px and vz on rough ground only
    T s[PLANT_MAX_Q], c[PLANT_MAX_Q];
    for (int i = 0; i < nq; ++i) { s[i] = psin(q2[i]); c[i] = pcos(q2[i]); }
    for (int f = 0; f < nc; ++f) {
        const PlantChain& ch = M.foot[f];
        const int ne = hopper ? 0 : ch.n;
        T px{}, pz = q2[1], vx = (q2[0] - q1[0]) / h, vz{};
        if constexpr (ROUGH) { px = q2[0]; vz = (q2[1] - q1[1]) / h; }
        if (hopper) {
            // foot = (x + r sin t, z - r cos t), J = [1 0 r cos t sin t; 0 1 r sin t -cos t] at q2 (hopper_2D/model.jl:35-66)
            const T rl = q2[3];
            pz = pz - rl * c[2];
            vx = vx + rl * (c[2] * ((q2[2] - q1[2]) / h)) + s[2] * ((q2[3] - q1[3]) / h);
            if constexpr (ROUGH) {
                px = px + rl * s[2];
                vz = vz + rl * (s[2] * ((q2[2] - q1[2]) / h)) - c[2] * ((q2[3] - q1[3]) / h);
            }
        }
        for (int e = 0; e < ne; ++e) {
            const int k = ch.k[e]; const double rr = ch.r[e];
            pz = pz - rr * c[k];
            vx = vx + rr * (c[k] * ((q2[k] - q1[k]) / h));
            if constexpr (ROUGH) {
                px = px + rr * s[k];
                vz = vz + rr * (s[k] * ((q2[k] - q1[k]) / h));
            }
        }
        T lx = b[2 * f] - b[2 * f + 1], lz = gam[f], vt = vx, phi = pz;      // contact force [m b; γ]
        if constexpr (ROUGH) {
            T surf, cr, sr;
            terrain_frame_2d(*E, px, surf, cr, sr);
            const T lt = lx;
            lx = cr * lt + sr * gam[f]; lz = cr * gam[f] - sr * lt;           // R^T [lt; γ]
            vt = cr * vx - sr * vz;                                           // (R v)[1]
            phi = pz - surf;
        }
        dyn[0] = dyn[0] + lx; dyn[1] = dyn[1] + lz;                           // J^T λ: base columns
        if (hopper) {
            const T rl = q2[3];
            dyn[2] = dyn[2] + rl * (c[2] * lx + s[2] * lz);
            dyn[3] = dyn[3] + (s[2] * lx - c[2] * lz);
        }
        for (int e = 0; e < ne; ++e) {
            const int k = ch.k[e]; const double rr = ch.r[e];
            dyn[k] = dyn[k] + rr * (c[k] * lx + s[k] * lz);
        }
        plant_contact_rows<2>(nq, nc, f, z, phi, &vt, mu, kappa, r);
    }
    for (int i = 0; i < nq; ++i) r[i] = dyn[i];
}

// The flat entry: every model cimpc_plant_step has (particle_2D has none; the box and the wall call plant_residual_centroidal_env,
// pushbot and walledcartpole plant_residual_walls).
template <class T, class TH = double>
PLANT_HD void plant_residual(const PlantModel& M, const T* z, const TH* th, double kappa, T* r) {
    if (M.kind == PLANT_KIND_CENTROIDAL) { plant_residual_centroidal<T>(M, z, th, kappa, r); return; }
    if (M.kind == PLANT_KIND_PARTICLE) { plant_residual_particle<false, T>(M, nullptr, z, th, kappa, r); return; }
    if (M.kind == PLANT_KIND_HOPPER_3D) { plant_residual_hopper_3d<T>(M, nullptr, z, th, kappa, r); return; }
    plant_residual_chain<false, T>(M, nullptr, z, th, kappa, r);
}
// The terrain entry: planar chains, hopper_2D, particle_2D and (3-D kinds) particle and hopper_3D; the centroidal models are
// refused by the caller.
template <class T, class TH = double>
PLANT_HD void plant_residual_terrain(const PlantModel& M, const cimpc_terrain& E, const T* z, const TH* th, double kappa, T* r) {
    if (M.kind == PLANT_KIND_PARTICLE) { plant_residual_particle<true, T>(M, &E, z, th, kappa, r); return; }
    if (M.kind == PLANT_KIND_PARTICLE_2D) { plant_residual_particle_2d<T>(M, E, z, th, kappa, r); return; }
    if (M.kind == PLANT_KIND_HOPPER_3D) { plant_residual_hopper_3d<T>(M, &E, z, th, kappa, r); return; }
    plant_residual_chain<true, T>(M, &E, z, th, kappa, r);
}

// Which terrains a model takes (cimpc_plant_step_terrain): FLAT everywhere; planar kinds on the planar models; 3-D kinds on the
// particle and hopper_3D; centroidal_quadruped, _box and _wall flat only (their reference models never call surf or rotation: the box's step
// and the wall are inside their phi); pushbot and walledcartpole flat only as well (their walls are inside their phi, and the
// reference runs both on flat_2D_lc alone).
inline bool terrain_valid_for(const PlantModel& M, const cimpc_terrain& E) {
    const double* f[] = {E.p, E.brk + 1, E.off, &E.coef[0][0]};
    const int n[] = {4, CIMPC_TERRAIN_MAX_PIECES - 1, CIMPC_TERRAIN_MAX_PIECES, 4 * CIMPC_TERRAIN_MAX_PIECES};
    for (int a = 0; a < 4; ++a) for (int i = 0; i < n[a]; ++i) if (!std::isfinite(f[a][i])) return false;
    if (E.kind < CIMPC_TERRAIN_FLAT || E.kind > CIMPC_TERRAIN_BOWL_3D) return false;
    if (E.kind == CIMPC_TERRAIN_PIECEWISE) {
        if (E.n_pieces < 1 || E.n_pieces > CIMPC_TERRAIN_MAX_PIECES) return false;
        for (int i = 2; i < E.n_pieces; ++i) if (!(E.brk[i] > E.brk[i - 1])) return false;
    }
    if (E.kind == CIMPC_TERRAIN_SOFTPLUS && E.p[1] == 0.0) return false;
    if (E.kind == CIMPC_TERRAIN_FLAT) return true;
    if (M.kind == PLANT_KIND_CENTROIDAL || M.kind == PLANT_KIND_CENTROIDAL_BOX || M.kind == PLANT_KIND_CENTROIDAL_WALL) return false;
    if (M.kind == PLANT_KIND_PUSHBOT || M.kind == PLANT_KIND_WALLEDCARTPOLE) return false;
    return terrain_is_3d(E.kind) == (M.kind == PLANT_KIND_PARTICLE || M.kind == PLANT_KIND_HOPPER_3D);
}

// ---- the models: one table per CIMPC_PLANT_* id, from the reference's model files ----------------------------------------
inline PlantChain plant_chain(int n, double r0, int k0, double r1 = 0, int k1 = 0, double r2 = 0, int k2 = 0) {
    PlantChain c{}; c.n = n; c.r[0] = r0; c.k[0] = k0; c.r[1] = r1; c.k[1] = k1; c.r[2] = r2; c.k[2] = k2; return c;
}
inline PlantModel plant_quadruped() {          // quadruped/model.jl:516-575
    PlantModel M{};
    M.nq = 11; M.nu = 8; M.g = 9.81; M.mu_world = 1.0;
    const double m_torso = 4.713 + 4 * 0.696, m_thigh = 1.013, m_leg = 0.166;
    const double J_torso = 0.01683 + 4 * 0.696 * 0.183 * 0.183, J_thigh = 0.00552, J_leg = 0.00299;
    const double l_torso = 0.183 * 2, l_thigh = 0.2, l_leg = 0.2;
    const double d_torso = 0.5 * l_torso + 0.0127, d_thigh = 0.5 * l_thigh - 0.00323, d_leg = 0.5 * l_leg - 0.006435;
    int nb = 0;
    auto add = [&](double m, double J, int own, PlantChain c) { M.mass[nb] = m; M.inertia[nb] = J; M.own[nb] = own; M.body[nb] = c; ++nb; };
    add(m_torso, J_torso, 2, plant_chain(1, d_torso, 2));
    const int legs[4][2] = {{3, 4}, {5, 6}, {7, 8}, {9, 10}};
    for (int l = 0; l < 4; ++l) {
        const int th = legs[l][0], ca = legs[l][1];
        if (l < 2) {
            add(m_thigh, J_thigh, th, plant_chain(1, d_thigh, th));
            add(m_leg, J_leg, ca, plant_chain(2, l_thigh, th, d_leg, ca));
            M.foot[l] = plant_chain(2, l_thigh, th, l_leg, ca);
        } else {                                   // legs 3, 4 hang from the far end of the torso
            add(m_thigh, J_thigh, th, plant_chain(2, l_torso, 2, d_thigh, th));
            add(m_leg, J_leg, ca, plant_chain(3, l_torso, 2, l_thigh, th, d_leg, ca));
            M.foot[l] = plant_chain(3, l_torso, 2, l_thigh, th, l_leg, ca);
        }
    }
    M.n_bodies = nb;
    const int pairs[8][2] = {{2, 3}, {3, 4}, {2, 5}, {5, 6}, {2, 7}, {7, 8}, {2, 9}, {9, 10}};
    for (int i = 0; i < 8; ++i) { M.tq_a[i] = pairs[i][0]; M.tq_b[i] = pairs[i][1]; }
    for (int i = 0; i < 11; ++i) M.joint_friction[i] = i < 3 ? 0.0 : 0.1;
    return M;
}
inline PlantModel plant_hopper_2d() {          // hopper_2D/model.jl:95-121
    PlantModel M{};
    M.kind = PLANT_KIND_HOPPER_2D; M.nc = 1;
    M.nq = 4; M.nu = 2; M.g = 9.81; M.mu_world = 0.8; M.n_bodies = 0;
    const double mb = 3.0, ml = 0.3, Jb = 0.75, Jl = 0.075;
    M.mass[0] = mb + ml; M.mass[1] = mb + ml; M.mass[2] = Jb + Jl; M.mass[3] = ml;      // diagonal of the mass matrix
    for (int i = 0; i < 4; ++i) M.joint_friction[i] = 0.0;
    return M;
}
inline PlantModel plant_centroidal(bool damped) {          // centroidal_quadruped/model.jl:187-228
    PlantModel M{};
    M.kind = PLANT_KIND_CENTROIDAL; M.nc = 4; M.fd = 4; M.nw = 3;
    M.nq = 18; M.nu = 12; M.g = 9.81; M.mu_world = 0.3; M.n_bodies = 0;
    M.mass[0] = 13.5; M.mass[1] = 0.2;
    M.inertia[0] = 0.0178533 * 10.0; M.inertia[1] = 0.0377999 * 10.0; M.inertia[2] = 0.0456542 * 10.0;
    for (int i = 0; i < 18; ++i) M.joint_friction[i] = damped ? ((i >= 3 && i < 6) ? 30.0 : 10.0) : 0.0;      // mu_joint = 1
    return M;
}
inline PlantModel plant_centroidal_box() {         // centroidal_quadruped_box/model.jl:199-230: the damped centroidal model, m_f = 0.5
    PlantModel M = plant_centroidal(true);
    M.kind = PLANT_KIND_CENTROIDAL_BOX;
    M.mass[1] = 0.5;
    return M;
}
inline PlantModel plant_centroidal_wall() {        // centroidal_quadruped_wall/model.jl:204-235: the damped centroidal model, nc = 8
    PlantModel M = plant_centroidal(true);
    M.kind = PLANT_KIND_CENTROIDAL_WALL; M.nc = PLANT_WALL_NC;
    return M;
}
inline PlantModel plant_particle() {           // particle/model.jl:113-121
    PlantModel M{};
    M.kind = PLANT_KIND_PARTICLE; M.nc = 1; M.fd = 4; M.nw = 3;
    M.nq = 3; M.nu = 3; M.g = 9.81; M.mu_world = 1.0; M.n_bodies = 0;
    M.mass[0] = 1.0;
    for (int i = 0; i < 3; ++i) M.joint_friction[i] = 0.0;
    return M;
}
inline PlantModel plant_hopper_3d() {          // hopper_3D/model.jl:96-118
    PlantModel M{};
    M.kind = PLANT_KIND_HOPPER_3D; M.nc = 1; M.fd = 4; M.nw = 3;
    M.nq = 7; M.nu = 3; M.g = 9.81; M.mu_world = 1.5; M.n_bodies = 0;
    const double mb = 3.0, ml = 0.3, Jb = 0.75, Jl = 0.075;
    for (int i = 0; i < 3; ++i) { M.mass[i] = mb + ml; M.mass[3 + i] = Jb + Jl; }      // diagonal of the mass matrix
    M.mass[6] = ml;
    for (int i = 0; i < 7; ++i) M.joint_friction[i] = 0.0;
    return M;
}
inline PlantModel plant_particle_2d() {        // particle_2D/model.jl (particle_2D = Particle2D(2, 2, 2, 1, 1.0, 9.81, 1.0, 0.0, ...))
    PlantModel M{};
    M.kind = PLANT_KIND_PARTICLE_2D; M.nc = 1; M.fd = 2; M.nw = 2;
    M.nq = 2; M.nu = 2; M.g = 9.81; M.mu_world = 1.0; M.n_bodies = 0;
    M.mass[0] = 1.0;
    for (int i = 0; i < 2; ++i) M.joint_friction[i] = 0.0;
    return M;
}
inline PlantModel plant_pushbot() {            // pushbot/model.jl:116-136
    PlantModel M{};
    M.kind = PLANT_KIND_PUSHBOT; M.nc = 2; M.fd = 2; M.nw = 2;
    M.nq = 2; M.nu = 2; M.g = 9.81; M.mu_world = 0.5; M.n_bodies = 0;
    M.mass[0] = 1.0; M.mass[1] = 0.01;             // mb, ma
    M.inertia[0] = 1.0; M.inertia[1] = 0.5;        // l, walls at x = -+0.5
    for (int i = 0; i < 2; ++i) M.joint_friction[i] = 10.0;
    return M;
}
inline PlantModel plant_walledcartpole() {     // walledcartpole/model.jl:130-154
    PlantModel M{};
    M.kind = PLANT_KIND_WALLEDCARTPOLE; M.nc = 2; M.fd = 2; M.nw = 4;
    M.nq = 4; M.nu = 1; M.g = 9.81; M.mu_world = 0.1; M.n_bodies = 0;
    M.mass[0] = 0.978; M.mass[1] = 0.411; M.mass[2] = 0.1;                              // mb, mt, mw
    M.inertia[0] = 0.6; M.inertia[1] = 0.35; M.inertia[2] = 0.4267; M.inertia[3] = 50.0;      // l, w, lc, k
    M.joint_friction[0] = 0.0; M.joint_friction[1] = 1.0; M.joint_friction[2] = 3.0; M.joint_friction[3] = 3.0;
    return M;
}
inline PlantModel plant_flamingo() {           // flamingo/model.jl:458-495
    PlantModel M{};
    M.nq = 9; M.nu = 6; M.g = 9.81; M.mu_world = 0.9;
    const double m_torso = 12.0, m_thigh = 0.4598, m_calf = 0.306, m_foot = 0.3466;
    const double J_torso = 0.10, J_thigh = 0.01256, J_calf = 0.00952, J_foot = 0.0015;
    const double l_thigh = 0.42, l_calf = 0.45, l_foot = 0.1725;
    const double d_torso = 0.20, d_thigh = 0.21, d_calf = 0.225, d_foot = 0.0525, cb = 0.5 * (l_foot - d_foot);
    int nb = 0;
    auto add = [&](double m, double J, int own, PlantChain c) { M.mass[nb] = m; M.inertia[nb] = J; M.own[nb] = own; M.body[nb] = c; ++nb; };
    add(m_torso, J_torso, 2, plant_chain(1, -d_torso, 2));           // the torso points up from the hip
    const int legs[2][3] = {{3, 4, 7}, {5, 6, 8}};
    for (int l = 0; l < 2; ++l) {
        const int th = legs[l][0], ca = legs[l][1], ft = legs[l][2];
        add(m_thigh, J_thigh, th, plant_chain(1, d_thigh, th));
        add(m_calf, J_calf, ca, plant_chain(2, l_thigh, th, d_calf, ca));
        add(m_foot, J_foot, ft, plant_chain(3, l_thigh, th, l_calf, ca, cb, ft));
        M.foot[2 * l] = plant_chain(3, l_thigh, th, l_calf, ca, l_foot, ft);          // toe
        M.foot[2 * l + 1] = plant_chain(3, l_thigh, th, l_calf, ca, -d_foot, ft);     // heel
    }
    M.n_bodies = nb;
    const int pairs[6][2] = {{2, 3}, {3, 4}, {2, 5}, {5, 6}, {4, 7}, {6, 8}};
    for (int i = 0; i < 6; ++i) { M.tq_a[i] = pairs[i][0]; M.tq_b[i] = pairs[i][1]; }
    for (int i = 0; i < 9; ++i) M.joint_friction[i] = 0.0;
    return M;
}

// CIMPC_PLANT_* id (include/cimpc.h) -> its model; false for any other id
inline bool plant_model_by_id(int id, PlantModel* out) {
    switch (id) {
    case CIMPC_PLANT_QUADRUPED: *out = plant_quadruped(); return true;
    case CIMPC_PLANT_FLAMINGO: *out = plant_flamingo(); return true;
    case CIMPC_PLANT_HOPPER_2D: *out = plant_hopper_2d(); return true;
    case CIMPC_PLANT_CENTROIDAL: *out = plant_centroidal(true); return true;
    case CIMPC_PLANT_CENTROIDAL_UNDAMPED: *out = plant_centroidal(false); return true;
    case CIMPC_PLANT_PARTICLE: *out = plant_particle(); return true;
    case CIMPC_PLANT_PARTICLE_2D: *out = plant_particle_2d(); return true;
    case CIMPC_PLANT_CENTROIDAL_BOX: *out = plant_centroidal_box(); return true;
    case CIMPC_PLANT_CENTROIDAL_WALL: *out = plant_centroidal_wall(); return true;
    case CIMPC_PLANT_HOPPER_3D: *out = plant_hopper_3d(); return true;      // id 9 is unassigned
    case CIMPC_PLANT_PUSHBOT: *out = plant_pushbot(); return true;          // id 11 is unassigned
    case CIMPC_PLANT_WALLEDCARTPOLE: *out = plant_walledcartpole(); return true;
    default: return false;
    }
}

// The model behind a CIMPC_PLANT_* id and the ground of a call over n robots or knots: terrain null (flat ground), or 1 terrain for
// all or n, one each, every one a terrain the model can stand on.  *rough: the terrain list has to reach the device (a terrain that is
// not flat, or particle_2D, which has no flat residual and so no call without a terrain).  False: an entry point refuses the call.
inline bool plant_model_and_ground(int model, int n, int n_terrain, const cimpc_terrain* terrain, PlantModel* M, bool* rough) {
    if (!plant_model_by_id(model, M) || (model == CIMPC_PLANT_PARTICLE_2D && !terrain)) return false;
    *rough = model == CIMPC_PLANT_PARTICLE_2D;
    if (terrain) {
        if (n_terrain != 1 && n_terrain != n) return false;
        for (int i = 0; i < n_terrain; ++i) {
            if (!terrain_valid_for(*M, terrain[i])) return false;
            *rough = *rough || terrain[i].kind != CIMPC_TERRAIN_FLAT;
        }
    }
    return true;
}

}  // namespace cimpc
