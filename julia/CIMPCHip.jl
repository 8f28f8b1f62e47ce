# CIMPCHip.jl - Julia-side binding of libcimpc_hip.so (include/cimpc.h) for ContactImplicitMPC.jl.
#
# Drop-in at the reference's own seams (file:line relative to dojo-sim/ContactImplicitMPC.jl v0.2.0):
#   B4  newton_solve!(core, s, q0, q1, window, im_traj, ref_traj; warm_start)   src/controller/newton.jl:169-177
#   B3  implicit_dynamics!(im_traj, traj; window)                               src/controller/implicit_dynamics.jl:156-158
#   B1  linear_solve!(solver, x, A, b)   (opts.solver = :hip_kkt_solver / :hip_csc_solver)   src/controller/newton.jl:86,218
#   A1  LinearizedStep per knot -> cimpc_set_linearization                      src/controller/linearized_step.jl:10-31
#   glue rot_n_stride! / update_window!                                         src/controller/policy.jl:133-141
#
# DROP-IN under the reference's UNCHANGED policy (round 5): `NewtonOptions(solver = :hip_mpc_solver, ...)` - ONE changed line in
# e.g. examples/quadruped/flat.jl:45 (`solver = :ldl_solver`).  `Newton(...)` (newton.jl:86) then builds a `HipMPCSolver <:
# LinearSolver`, the linear-solver TYPE is a type parameter of `Newton{T,nq,nu,nw,nc,nb,nz,nθ,nν,NJ,NR,NI,O,LS,NV}`
# (newton.jl:17-35), and the method of the package's own `newton_solve!` defined below for `LS = HipMPCSolver` is what
# `policy(p::CIMPC, traj, t)` reaches at policy.jl:119-120 - the whole MPC step runs on the GPU with `ci_mpc_policy`, `policy`,
# `simulate!` untouched.  The handle is built at the first solve from what `newton_solve!` receives (`core`, `s`, `im_traj`,
# `ref_traj`): no global registry.
#
# Usage: `include("CIMPCHip.jl")` INSIDE `module ContactImplicitMPC` (src/ContactImplicitMPC.jl).  For the drop-in B4 method the
# include must come AFTER `include("controller/policy.jl")` (line 108: `Newton`, `newton_solve!`, `ImplicitTrajectory`, `ContactTraj`,
# `Simulation` exist then) - e.g. as line 111, before the visuals; for the B1 solvers alone anywhere after line 32 (the
# `import RoboDojo: LinearSolver, ..., linear_solve!` the binding's own import needs) is enough, and the B4 method is then simply
# not defined.  Library path in ENV["CIMPC_LIB"].  The file defines the submodule `CIMPCHip`, which imports
# the package's own `linear_solve!` / `LinearSolver` (so that newton.jl:218 dispatches to the GPU solvers) and, with its last
# line, makes the constructors `hip_mpc_solver` / `hip_kkt_solver` / `hip_csc_solver` visible to `eval(opts.solver)` in the package
# module (newton.jl:86).  Names the package defines LATER in its include order - `friction_dim` (simulator/environment.jl),
# `LinearizedStep` (controller/linearized_step.jl) - are NOT imported at the top: they are looked up in the parent module when a
# `Solver` is built (`_pkg()`), so the include position does not matter for them.
# Explicit form (a host that drives the handle itself):
#   p   = ci_mpc_policy(ref_traj, s, obj; H_mpc, N_sample, κ_mpc, mode, n_opts, ip_opts)
#   hip = CIMPCHip.Solver(s, ref_traj, obj; H_mpc, κ = κ_mpc, mode, n_opts, ip_opts)      # once
#   CIMPCHip.newton_solve!(hip, p.newton, p.q0, q1, p.window, p.traj; warm_start = t > 1)   # instead of newton.jl:169
# B1 alone (the reference's Newton loop with the GPU KKT solve):
#   CIMPCHip.CURRENT[] = hip                               # the handle whose device-resident sensitivities are solved with
#   n_opts = NewtonOptions(solver = :hip_kkt_solver, ...)  # -> Newton(...) calls eval(:hip_kkt_solver)(jac.R)
#
# There is no Julia toolchain in the build image of this repository: the file is written against the C header and the
# reference's types, every call it makes is exercised through the identical C ABI by the Python host
# (contactimplicitmpc/jl_amd/_lib.py, solver.py) in tests/.  Struct layouts below are checked against the header by
# tests/test_abi_and_host.py (field order / sizes of the C structs).
module CIMPCHip

using SparseArrays
using LinearAlgebra: SingularException
# the package's own generic function and abstract type (both imported from RoboDojo at src/ContactImplicitMPC.jl:32): methods
# added here are the ones newton.jl:218 `linear_solve!(core.solver, core.Δ.r, core.jac.R, core.res.r)` dispatches to
import ..ContactImplicitMPC: linear_solve!, LinearSolver
# the package module, for names it defines after this file may have been included (resolved at call time)
_pkg() = parentmodule(@__MODULE__)

const LIB = get(ENV, "CIMPC_LIB", "libcimpc_hip.so")

# ---- include/cimpc.h structs (field order = C order; all Cint / Cdouble: no padding surprises) -------------------------
struct Dims
    nq::Cint; nu::Cint; nw::Cint; nc::Cint; nb::Cint
    mode::Cint                  # 0 = :configuration, 1 = :configurationforce
    H_ref::Cint; H::Cint; B::Cint
end
struct IpOpts                   # <- InteriorPointOptions (policy.jl:54-61, implicit_dynamics.jl:25-32)
    r_tol::Cdouble; kappa_tol::Cdouble; undercut::Cdouble; gamma_reg::Cdouble
    kappa_reg::Cdouble; eps_min::Cdouble; ls_scale::Cdouble
    max_iter::Cint; max_ls::Cint; stall_alpha::Cdouble
    max_time::Cdouble           # per-solve budget, mpc_opts.ip_max_time (policy.jl:9,61); >= 1000 s = unlimited
end
# RoboDojo 0.1.3 owns InteriorPointOptions and its source is not part of the reference tree: the only field names the reference
# itself shows are r_tol, κ_tol, undercut, γ_reg, ϵ_min, max_ls, max_time, diff_sol, solver, verbose (simulator.jl:24-32,
# policy.jl:54-61, implicit_dynamics.jl:25-32).  Every field is therefore read through `_opt` - a name this RoboDojo version does
# not have falls back to the library's default (cimpc_default_ip_opts) instead of raising a FieldError at handle creation.
_opt(o, name::Symbol, default) = hasproperty(o, name) ? getproperty(o, name) : default
function IpOpts(o)
    d = Ref(IpOpts(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
    ccall((:cimpc_default_ip_opts, LIB), Cvoid, (Ref{IpOpts},), d)
    d = d[]
    IpOpts(_opt(o, :r_tol, d.r_tol), _opt(o, :κ_tol, d.kappa_tol), _opt(o, :undercut, d.undercut), _opt(o, :γ_reg, d.gamma_reg),
           _opt(o, :κ_reg, d.kappa_reg), _opt(o, :ϵ_min, d.eps_min), _opt(o, :ls_scale, d.ls_scale),
           _opt(o, :max_iter, d.max_iter), _opt(o, :max_ls, d.max_ls), d.stall_alpha, _opt(o, :max_time, d.max_time))
end
struct NewtonOpts               # <- NewtonOptions (newton.jl:2-11)
    r_tol::Cdouble; beta_init::Cdouble; max_time::Cdouble; kappa::Cdouble
    max_iter::Cint; kkt_backend::Cint
end
const KKT_CONDENSED, KKT_DENSE_LU, KKT_BANDED_LDL, KKT_CONDENSED_MIXED = Cint(0), Cint(1), Cint(2), Cint(3)

lasterror(h) = unsafe_string(ccall((:cimpc_last_error, LIB), Cstring, (Ptr{Cvoid},), h))
check(rc, h = C_NULL) = rc == 0 ? nothing : error("libcimpc_hip: ($rc) " * lasterror(h))

pack(v::AbstractVector{<:AbstractVector}, n = length(v)) = reduce(hcat, v[1:n])     # Vector{Vector} -> column-major matrix

# ---- handle = ImplicitTrajectory + Newton state on one GPU ----------------------------------------------------------------
mutable struct Solver
    h::Ptr{Cvoid}
    dims::Dims
    function Solver(h, dims)
        s = new(h, dims)
        finalizer(x -> (x.h == C_NULL || ccall((:cimpc_destroy, LIB), Cint, (Ptr{Cvoid},), x.h); x.h = C_NULL), s)
        return s
    end
end

"""
    Solver(s, ref_traj, obj; H_mpc, κ, mode, n_opts, ip_opts, B = 1, device = 0, kkt_backend = KKT_CONDENSED)

Replaces `ImplicitTrajectory(ref_traj, s; κ, mode, opts)` (implicit_dynamics.jl:21-90) and `Newton(s, H, h, traj, im_traj; obj,
opts)` (newton.jl:37-91): uploads one `LinearizedStep` per knot and the objective blocks.
"""
function Solver(s, ref_traj, obj; H_mpc::Int, κ::Float64, mode::Symbol = :configurationforce, n_opts, ip_opts,
                B::Int = 1, device::Int = 0, kkt_backend = KKT_CONDENSED)
    m = s.model
    nb = m.nc * _pkg().friction_dim(s.env)
    dims = Dims(m.nq, m.nu, m.nw, m.nc, nb, mode == :configuration ? 0 : 1, ref_traj.H, H_mpc, B)
    ip = Ref(IpOpts(ip_opts))
    nt = Ref(NewtonOpts(n_opts.r_tol, n_opts.β_init, n_opts.max_time, κ, n_opts.max_iter, kkt_backend))      # newton.jl:2-11
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:cimpc_create, LIB), Cint, (Ref{Dims}, Ref{IpOpts}, Ref{NewtonOpts}, Cint, Ref{Ptr{Cvoid}}),
                Ref(dims), ip, nt, device, h))
    hs = Solver(h[], dims)
    for t = 1:ref_traj.H                                             # A1
        lin = _pkg().LinearizedStep(s, ref_traj.z[t], ref_traj.θ[t], κ)
        check(ccall((:cimpc_set_linearization, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    hs.h, t, lin.z, lin.θ, lin.r, Matrix(lin.rz), Matrix(lin.rθ)), hs.h)
    end
    set_objective!(hs, obj, H_mpc)
    return hs
end

"TrackingObjective / TrackingVelocityObjective (objective.jl:3-47) -> cimpc_set_objective (column-major blocks per step)."
function set_objective!(hs::Solver, obj, H::Int)
    blk(v) = cat((Matrix(v[t]) for t = 1:H)...; dims = 3)
    Q, R = blk(obj.q), blk(obj.u)
    Cg = hs.dims.mode == 1 ? blk(obj.γ) : C_NULL
    Cb = hs.dims.mode == 1 ? blk(obj.b) : C_NULL
    hasv = hasproperty(obj, :v)
    V = hasv ? blk(obj.v) : C_NULL
    qt = hasv ? pack(obj.q_target, H) : C_NULL
    vt = hasv ? pack(obj.v_target, H) : C_NULL
    check(ccall((:cimpc_set_objective, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                hs.h, Q, R, Cg, Cb, V, qt, vt), hs.h)
end

"""
    set_linearization!(hs, s, t, z, θ, κ)

Re-linearisation of knot `t` in flight: what `update!(lin::LinearizedStep, s, z, θ)` + `update!` of `RLin / RZLin / RθLin` do
(linearized_step.jl:33-45, linearized_solver.jl:497-565).  The next solve on the handle uses the new table.
"""
function set_linearization!(hs::Solver, s, t::Int, z, θ, κ)
    lin = _pkg().LinearizedStep(s, z, θ, κ)
    check(ccall((:cimpc_set_linearization, LIB), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                hs.h, t, lin.z, lin.θ, lin.r, Matrix(lin.rz), Matrix(lin.rθ)), hs.h)
end

"RLin.alt of every knot (set_altitude!, implicit_dynamics.jl:141-154); alt: nc (one robot) or nc x B."
set_altitude!(hs::Solver, alt) =
    check(ccall((:cimpc_set_altitude, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), hs.h, Matrix{Float64}(reshape(alt, :, Int(hs.dims.B)))), hs.h)

# ---- B4: newton_solve! ---------------------------------------------------------------------------------------------------------
# Every buffer handed to the library is sized with `hs.dims.B` (the library reads / writes B rollouts whatever the caller meant):
# the single-trajectory forms below REQUIRE a handle built with B = 1, the batched form takes one column / entry per rollout.
_need_b1(hs::Solver, what) = hs.dims.B == 1 || error("CIMPCHip.$what: this form drives ONE trajectory, the handle was built with B = $(hs.dims.B) - use the batched form")
# B x (H+2) 1-based knot indices as the ABI reads them: rollout-major = a column-major (H+2) x B Cint matrix
_windows(hs::Solver, window::Vector{Int}) = (length(window) == hs.dims.H + 2 || error("window must have H + 2 entries"); reshape(Cint.(window), :, 1))
function _windows(hs::Solver, windows::AbstractVector{<:AbstractVector{<:Integer}})
    length(windows) == hs.dims.B || error("one window per rollout: got $(length(windows)), B = $(hs.dims.B)")
    all(w -> length(w) == hs.dims.H + 2, windows) || error("every window must have H + 2 entries")
    return Matrix{Cint}(reduce(hcat, windows))
end
# the six reference arrays of cimpc_set_reference for B rollouts: per field a (n, steps, B) array = B x steps x n row-major
function _refs(hs::Solver, refs::AbstractVector, H::Int)
    length(refs) == hs.dims.B || error("one reference trajectory per rollout: got $(length(refs)), B = $(hs.dims.B)")
    f(sel, n) = cat((pack(sel(r), n) for r in refs)...; dims = 3)
    return f(r -> r.q, H + 2), f(r -> r.u, H), f(r -> r.w, H), f(r -> r.γ, H), f(r -> r.b, H), f(r -> r.θ, H)
end

"""
    newton_solve!(hs, core, q0, q1, window, ref_traj; warm_start = false)

`newton_solve!(core, s, q0, q1, window, im_traj, ref_traj; warm_start)` (newton.jl:169-177) on the GPU for ONE trajectory (handle
built with B = 1): ONE C call (`cimpc_mpc_solve`: window, reference, q0, q1 in; `u[1]` and, with `full = true`, the whole
`core.traj`, `core.ν` out).  Returns nothing and never throws for a solve that merely ran out of iterations / time (the reference
returns silently too).  `alt`: RLin.alt (nc values) or `nothing` = unchanged.
"""
function newton_solve!(hs::Solver, core, q0, q1, window::Vector{Int}, ref_traj; warm_start::Bool = false, full::Bool = false, alt = nothing)
    _need_b1(hs, "newton_solve!")
    H = core.traj.H
    B = Int(hs.dims.B)
    nq, nu = length(core.traj.q[1]), length(core.traj.u[1]); nd = length(core.ν[1])
    qr, ur, wr, gr, br, θr = _refs(hs, [ref_traj], H)
    u1 = zeros(nu, B); iters = zeros(Cint, B); rn = zeros(Cdouble, B)
    q = full ? zeros(nq, H + 2, B) : C_NULL; u = full ? zeros(nu, H, B) : C_NULL; ν = full ? zeros(nd, H, B) : C_NULL
    a = alt === nothing ? C_NULL : Matrix{Float64}(reshape(alt, :, B))
    check(ccall((:cimpc_mpc_solve, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                 Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble},
                 Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                hs.h, _windows(hs, window), qr, ur, wr, gr, br, θr, a, Vector{Float64}(q0), Vector{Float64}(q1), warm_start, u1, iters, rn,
                q, u, C_NULL, C_NULL, ν), hs.h)
    core.traj.u[1] .= @view u1[:, 1]
    if full
        for t = 1:H + 2; core.traj.q[t] .= @view q[:, t, 1]; end
        for t = 1:H; core.traj.u[t] .= @view u[:, t, 1]; core.ν[t] .= @view ν[:, t, 1]; end
    end
    return nothing
end

"""
    newton_solve!(hs, q0::Matrix, q1::Matrix, windows, ref_trajs; warm_start = false) -> (u1, newton_iters, r_norm)

BATCHED B4: one `newton_solve!` for each of the `B = hs.dims.B` Monte-Carlo rollouts of a handle (the serial loop of
examples/quadruped/monte_carlo.jl:76-92, one policy per sample, as ONE call): `q0`, `q1` are nq x B (column b = rollout b),
`windows` a vector of B windows (`p.window` of every policy), `ref_trajs` a vector of B `ContactTraj` (`p.traj`).  Returns
`u1` (nu x B: column b = `p.newton.traj.u[1]` of rollout b, policy.jl:142), the Newton iterations and `|r|_1 / N` per rollout.
`alt`: nc x B or `nothing` = unchanged.  `windows = nothing, ref_trajs = nothing` re-solves on the window / reference already
resident (e.g. after `mpc_advance!`).
"""
function newton_solve!(hs::Solver, q0::Matrix{Float64}, q1::Matrix{Float64}, windows, ref_trajs; warm_start::Bool = false, alt = nothing)
    B = Int(hs.dims.B); H = Int(hs.dims.H)
    (size(q0) == (hs.dims.nq, B) && size(q1) == (hs.dims.nq, B)) || error("q0, q1 must be nq x B = $(hs.dims.nq) x $B")
    (windows === nothing) == (ref_trajs === nothing) || error("windows and ref_trajs go together")
    w = windows === nothing ? C_NULL : _windows(hs, windows)
    qr, ur, wr, gr, br, θr = ref_trajs === nothing ? ntuple(_ -> C_NULL, 6) : _refs(hs, ref_trajs, H)
    a = alt === nothing ? C_NULL : Matrix{Float64}(reshape(alt, :, B))
    u1 = zeros(Int(hs.dims.nu), B); iters = zeros(Cint, B); rn = zeros(Cdouble, B)
    check(ccall((:cimpc_mpc_solve, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                 Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble},
                 Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                hs.h, w, qr, ur, wr, gr, br, θr, a, q0, q1, warm_start, u1, iters, rn, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL), hs.h)
    return u1, iters, rn
end

"Policy glue after a solve: rot_n_stride!(p.traj, ...) + update_window! (policy.jl:136-139) on the device-resident copy."
mpc_advance!(hs::Solver, stride) = check(ccall((:cimpc_mpc_advance, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), hs.h, stride), hs.h)

# ---- B3: implicit_dynamics! ------------------------------------------------------------------------------------------------------
function implicit_dynamics!(hs::Solver, im_traj, traj; window = collect(1:traj.H + 2))
    _need_b1(hs, "implicit_dynamics!")      # d, dz, status, iters below hold ONE trajectory; the library writes hs.dims.B of them
    H = length(window) - 2; nd = length(im_traj.d[1]); nq = length(traj.q[1]); nu = length(traj.u[1])
    check(ccall((:cimpc_set_window, LIB), Cint, (Ptr{Cvoid}, Ptr{Cint}), hs.h, _windows(hs, window)), hs.h)
    d = zeros(nd, H); dz = zeros(nd, 2nq + nu, H); status = zeros(Cint, H); iters = zeros(Cint, H)
    cf = hs.dims.mode == 1
    check(ccall((:cimpc_implicit_dynamics, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
                hs.h, pack(traj.q, H + 2), pack(traj.θ, H), cf ? pack(traj.γ, H) : C_NULL, cf ? pack(traj.b, H) : C_NULL,
                d, dz, status, iters, C_NULL), hs.h)
    for (i, t) in enumerate(window[1:end-2])                     # write through the reference's views (implicit_dynamics.jl:84-86)
        im_traj.d[t] .= @view d[:, i]
        if status[i] == 1
            im_traj.δq0[t] .= @view dz[:, 1:nq, i]
            im_traj.δq1[t] .= @view dz[:, nq+1:2nq, i]
            im_traj.δu1[t] .= @view dz[:, 2nq+1:2nq+nu, i]
        else
            @warn "implicit dynamics failure (t = $t)"             # implicit_dynamics.jl:169-176: δz keeps its last value
        end
    end
    return nothing
end

# ---- B2: the per-knot callbacks handed to RoboDojo's interior_point (implicit_dynamics.jl:58-68) ---------------------------------
# z, r, Δ in the order [x; y1; y2] of linearization_var_index (index.jl:289-327); one point (vectors) or n points (nz x n).
"""
    rlin!(hs, r, t, z, θ, κ; alt = nothing)      # rlin!(r, z, θ, κ) of knot t, linearized_solver.jl:364-373
"""
function rlin!(hs::Solver, r::VecOrMat{Float64}, t::Int, z::VecOrMat{Float64}, θ::VecOrMat{Float64}, κ::Float64; alt = nothing)
    n = size(z, 2)
    check(ccall((:cimpc_ip_residual, LIB), Cint,
                (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
                hs.h, t, n, z, θ, alt === nothing ? C_NULL : Matrix{Float64}(reshape(alt, :, n)), κ, r), hs.h)
    return r
end
"""
    linear_solve!(hs, Δ, t, z, r; reg = 0.0)     # rzlin!(rz, z; reg) + linear_solve!(Δ, rz, r; reg), linearized_solver.jl:378-444
"""
function linear_solve!(hs::Solver, Δ::VecOrMat{Float64}, t::Int, z::VecOrMat{Float64}, r::VecOrMat{Float64}; reg::Float64 = 0.0)
    check(ccall((:cimpc_ip_linear_solve, LIB), Cint,
                (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
                hs.h, t, size(z, 2), z, r, reg, Δ), hs.h)
    return Δ
end

# ---- B1: LinearSolver seam ---------------------------------------------------------------------------------------------------------
# (a) on a handle: the KKT system of the handle's device-resident sensitivities - the ENTRIES of A are not read; requires B3 / a
#     Newton evaluation on the same handle before the call (include/cimpc.h).  Select with opts.solver = :hip_kkt_solver.
#     What IS read from A is the dual regularisation: core.β changes after every accepted step (newton.jl:280) and enters the
#     matrix as jac.reg_du .-= β κ once per window step (newton_jacobian.jl:185), i.e. A[N, N] = -ρ with ρ = H β κ.  A LinearSolver
#     is handed the matrix, not core.β (newton.jl:218) - so ρ is taken from the matrix of THIS call, every call.
const CURRENT = Ref{Union{Nothing,Solver}}(nothing)
struct HipKKTSolver <: LinearSolver
    hs::Solver
end
"`eval(opts.solver)(jac.R)` (newton.jl:86): the solver works on the handle registered in `CIMPCHip.CURRENT[]`."
function hip_kkt_solver(A)
    CURRENT[] === nothing && error("CIMPCHip.CURRENT[] = Solver(...) must be set before Newton(...; opts.solver = :hip_kkt_solver)")
    return HipKKTSolver(CURRENT[])
end
function linear_solve!(s::HipKKTSolver, x::Vector{Float64}, A::SparseMatrixCSC{Float64,Int}, b::Vector{Float64};
                       reg::Float64 = 0.0, fact::Bool = true)
    N = size(A, 1)
    ρ = -A[N, N]                                                   # dual regularisation of this Newton iteration
    check(ccall((:cimpc_kkt_solve_rho, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}), s.hs.h, b, ρ, x), s.hs.h)
    return nothing
end
# (b) stand-alone: solves with the SparseMatrixCSC passed in, exactly the contract of lu.jl:4-12 / ldl.jl:144-149.
#     Select with opts.solver = :hip_csc_solver.  A singular matrix raises like the reference's LU (SingularException).
struct HipCSCSolver <: LinearSolver
    device::Int
end
hip_csc_solver(A) = HipCSCSolver(0)
function linear_solve!(s::HipCSCSolver, x::Vector{Float64}, A::SparseMatrixCSC{Float64,Int}, b::Vector{Float64};
                       reg::Float64 = 0.0, fact::Bool = true)
    rc = ccall((:cimpc_linear_solve_csc, LIB), Cint,
               (Cint, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               s.device, size(A, 1), A.colptr, A.rowval, A.nzval, b, x)
    rc == -5 && throw(SingularException(0))                       # CIMPC_ERR_SINGULAR
    check(rc)
    return nothing
end

# ---- B4 DROP-IN: the package's own newton_solve!, specialised on the linear-solver type parameter ---------------------------------
# (c) opts.solver = :hip_mpc_solver.  `Newton(...)` calls `eval(opts.solver)(jac.R)` (newton.jl:86) BEFORE anything else of the MPC
#     problem is known to a solver constructor, so the solver object starts empty; its handle is created by the first
#     `newton_solve!` from the arguments of that call:
#         dims      s.model, s.env, im_traj.mode, ref_traj.H (= H_ref), core.traj.H (= H_mpc)
#         tables    im_traj.lin[t]  (the LinearizedStep of every knot, implicit_dynamics.jl:57 - no second linearization)
#         options   core.opts (NewtonOptions), im_traj.ip[1].opts (InteriorPointOptions), κ = im_traj.ip[1].κ[1]
#         objective core.obj
#     Afterwards every call uploads window, reference (p.traj, rotated by the policy on the host, policy.jl:133-139), q0, q1 and the
#     altitude `im_traj.ip[1].r.alt` (set_altitude!, policy.jl:113), re-uploads a knot whose LinearizedStep changed
#     (set_implicit_trajectory! at t = 1, update! in flight), solves, and writes core.traj / core.ν back (the Newton iterate the
#     next warm start and the policy's `p.newton.traj.u[1]` read).  The Newton iterate itself stays resident on the device
#     between calls (warm_start = true never uploads it).
mutable struct HipMPCSolver <: LinearSolver
    hs::Union{Nothing,Solver}
    stamps::Vector{UInt}            # per knot: hash of the LinearizedStep last uploaded
    device::Int
end
"`eval(opts.solver)(jac.R)` (newton.jl:86): an empty solver - its handle is built at the first `newton_solve!`."
hip_mpc_solver(A) = HipMPCSolver(nothing, UInt[], parse(Int, get(ENV, "CIMPC_DEVICE", "0")))
# The reference's own Newton loop never runs with this solver type (the method below replaces it); a direct call - somebody's
# test of the LinearSolver interface - still gets a correct solve of the matrix it passes (lu.jl:4-12 contract).
linear_solve!(s::HipMPCSolver, x::Vector{Float64}, A::SparseMatrixCSC{Float64,Int}, b::Vector{Float64}; reg::Float64 = 0.0, fact::Bool = true) =
    linear_solve!(HipCSCSolver(s.device), x, A, b; reg = reg, fact = fact)

# A LinearizedStep is a function of its point: `update!(lin, s, z, θ)` copies (z, θ) in and recomputes r, rz, rθ from them
# (linearized_step.jl:33-45), and set_implicit_trajectory! / update! are the only writers (policy.jl:100-107,122).  The stamp
# therefore hashes the POINT (nz + nθ doubles per knot) and the residual vector, not the two matrices - 60 knots: 0.1 MB per
# call instead of 1.6 MB, which at ~1 GB/s of hashing was comparable to the solve itself (VERDICT r05 weak 3).
_lin_stamp(lin) = hash(lin.r, hash(lin.z, hash(lin.θ)))

function _upload_changed_knots!(ls::HipMPCSolver, im_traj)
    for t = 1:length(im_traj.lin)
        st = _lin_stamp(im_traj.lin[t])
        st == ls.stamps[t] && continue
        lin = im_traj.lin[t]
        check(ccall((:cimpc_set_linearization, LIB), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ls.hs.h, t, lin.z, lin.θ, lin.r, Matrix(lin.rz), Matrix(lin.rθ)), ls.hs.h)
        ls.stamps[t] = st
    end
end

function _build_handle!(ls::HipMPCSolver, core, s, im_traj, ref_traj)
    m = s.model
    nb = m.nc * _pkg().friction_dim(s.env)
    mode = im_traj.mode
    κ = im_traj.ip[1].κ[1]
    dims = Dims(m.nq, m.nu, m.nw, m.nc, nb, mode == :configuration ? 0 : 1, ref_traj.H, core.traj.H, 1)
    ip = Ref(IpOpts(im_traj.ip[1].opts))
    nt = Ref(NewtonOpts(core.opts.r_tol, core.opts.β_init, core.opts.max_time, κ, core.opts.max_iter, KKT_CONDENSED))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:cimpc_create, LIB), Cint, (Ref{Dims}, Ref{IpOpts}, Ref{NewtonOpts}, Cint, Ref{Ptr{Cvoid}}),
                Ref(dims), ip, nt, ls.device, h))
    ls.hs = Solver(h[], dims)
    ls.stamps = zeros(UInt, ref_traj.H)                             # (no LinearizedStep hashes to 0: every knot is uploaded)
    _upload_changed_knots!(ls, im_traj)
    set_objective!(ls.hs, core.obj, core.traj.H)
    return ls.hs
end

import ..ContactImplicitMPC                                  # the module itself: `ContactImplicitMPC.newton_solve!` below extends ITS function
if isdefined(ContactImplicitMPC, :newton_solve!) && isdefined(ContactImplicitMPC, :Newton)
    @eval begin
        # Same signature as newton.jl:169-177 with the fourteenth type parameter of Newton (newton.jl:17: `LS`, the type of
        # `core.solver`) fixed - strictly more specific than the reference's method, so policy.jl:119-120 lands here.
        # (Qualified definition: this module has a `newton_solve!` of its own - the explicit, handle-first form above.)
        function ContactImplicitMPC.newton_solve!(
            core::ContactImplicitMPC.Newton{T,nq,nu,nw,nc,nb,nz,nθ,nν,NJ,NR,NI,O,HipMPCSolver,NV},
            s::ContactImplicitMPC.Simulation{T},
            q0::Vector{T},
            q1::Vector{T},
            window::Vector{Int},
            im_traj::ContactImplicitMPC.ImplicitTrajectory{T},
            ref_traj::ContactImplicitMPC.ContactTraj{T};
            warm_start::Bool = false) where {T,nq,nu,nw,nc,nb,nz,nθ,nν,NJ,NR,NI,O,NV}
            ls = core.solver
            ls.hs === nothing && _build_handle!(ls, core, s, im_traj, ref_traj)
            _upload_changed_knots!(ls, im_traj)
            # ONE C call per MPC step: window, reference (p.traj as the policy rotated it), RLin.alt as set_altitude! left it
            # (policy.jl:113), q0, q1 in - core.traj / core.ν out (cimpc_mpc_solve)
            newton_solve!(ls.hs, core, q0, q1, window, ref_traj; warm_start = warm_start, full = true, alt = im_traj.ip[1].r.alt)
            return nothing
        end
    end
end

# ---- B3 DROP-IN: the package's own implicit_dynamics!, for trajectories attached to a handle ----------------------------------------
# `implicit_dynamics!(im_traj::ImplicitTrajectory, traj::ContactTraj; threads, window)` (implicit_dynamics.jl:156-158) is called by the
# reference's Newton loop at newton.jl:62,191,234,260.  Unlike `Newton` (whose linear-solver type is a type parameter, see B4 above),
# `ImplicitTrajectory{T,R,RZ,Rθ,NQ}` has no user-selectable type parameter: a drop-in under the UNCHANGED call sites has to replace the
# method of the same signature.  That is done at RUN time, on request (`CIMPCHip.enable_b3_dropin!()` - method overwriting is not
# permitted while the package precompiles), and only trajectories attached to a handle take the GPU path: every other call runs the
# package's original method, reached through the world age in which it was the newest (`Base.invoke_in_world`).
#   hip = CIMPCHip.Solver(s, ref_traj, obj; H_mpc, κ, mode, n_opts, ip_opts)       # B = 1
#   CIMPCHip.enable_b3_dropin!(); CIMPCHip.attach!(p.im_traj, hip)
#   ... the reference's newton_solve! now evaluates implicit_dynamics! on the GPU (B3), its own KKT solve stays (or :hip_kkt_solver, B1)
const _B3_HANDLES = IdDict{Any,Solver}()
const _B3_WORLD = Ref{UInt}(0)
"Route `implicit_dynamics!(im_traj, traj; window)` of THIS ImplicitTrajectory through the handle (B = 1)."
attach!(im_traj, hs::Solver) = (_need_b1(hs, "attach!"); _B3_HANDLES[im_traj] = hs; im_traj)
detach!(im_traj) = (delete!(_B3_HANDLES, im_traj); im_traj)
function enable_b3_dropin!()
    _B3_WORLD[] != 0 && return nothing
    (isdefined(ContactImplicitMPC, :implicit_dynamics!) && isdefined(ContactImplicitMPC, :ImplicitTrajectory)) ||
        error("CIMPCHip.enable_b3_dropin!: include CIMPCHip.jl after controller/implicit_dynamics.jl")
    _B3_WORLD[] = Base.get_world_counter()          # the package's own method is the newest one in this world
    @eval ContactImplicitMPC function implicit_dynamics!(im_traj::ImplicitTrajectory, traj::ContactTraj;
                                                         threads = false, window = collect(1:traj.H + 2))
        hs = get(CIMPCHip._B3_HANDLES, im_traj, nothing)
        if hs === nothing      # not attached: the reference's method, unchanged
            return Base.invoke_in_world(CIMPCHip._B3_WORLD[], implicit_dynamics!, im_traj, traj; threads = threads, window = window)
        end
        CIMPCHip.implicit_dynamics!(hs, im_traj, traj; window = window)
        return nothing
    end
    return nothing
end

# ---- plant side: one simulator step for B robots (RoboDojo step! inside simulate!, simulator.jl:15-63) ---------------------------
# model symbol -> (CIMPC_PLANT_* id, nq, nu, nc, friction directions per contact, nw); mirrors include/cimpc.h and
# contactimplicitmpc/jl_amd/plant.py: MODELS (checked by tests/test_julia_binding.py)
const PLANT_MODELS = Dict{Symbol,NTuple{6,Int}}(
    :quadruped => (0, 11, 8, 4, 2, 2), :flamingo => (1, 9, 6, 4, 2, 2), :hopper_2D => (2, 4, 2, 1, 2, 2),
    :centroidal_quadruped => (3, 18, 12, 4, 4, 3), :centroidal_quadruped_undamped => (4, 18, 12, 4, 4, 3),
    :particle => (5, 3, 3, 1, 4, 3))
# the centroidal quadruped against a step and a wall (plant.py: CENTROIDAL_ENV_MODELS); plant_step reads both tables
const PLANT_ENV_MODELS = Dict{Symbol,NTuple{6,Int}}(
    :centroidal_quadruped_box => (7, 18, 12, 4, 4, 3), :centroidal_quadruped_wall => (8, 18, 12, 8, 4, 3))
# hopper_3D (plant.py: SPATIAL_MODELS); id 9 is unassigned
const PLANT_SPATIAL_MODELS = Dict{Symbol,NTuple{6,Int}}(:hopper_3D => (10, 7, 3, 1, 4, 3))
# pushbot and walledcartpole, a point between two walls (plant.py: WALLED_MODELS); flat ground only; id 11 is unassigned
const PLANT_WALLED_MODELS = Dict{Symbol,NTuple{6,Int}}(:pushbot => (12, 2, 2, 2, 2, 2), :walledcartpole => (13, 4, 1, 2, 2, 4))
"""
    plant_step(model, q0, q1, u, μ, h_sim, opts; w = nothing) -> (q2, γ, b, status, iters)

q0, q1: nq x B; u: nu x B; w: nw x B or nothing.  Sizes are checked against the model's table; unknown models are an error.
"""
function plant_step(model::Symbol, q0::Matrix{Float64}, q1::Matrix{Float64}, u::Matrix{Float64}, μ, h_sim, opts;
                    w::Union{Nothing,Matrix{Float64}} = nothing)
    haskey(PLANT_WALLED_MODELS, model) || haskey(PLANT_SPATIAL_MODELS, model) || haskey(PLANT_ENV_MODELS, model) || haskey(PLANT_MODELS, model) || error("cimpc_plant_step has no model $model (available: " *
        "$(vcat(collect(keys(PLANT_MODELS)), collect(keys(PLANT_ENV_MODELS)), collect(keys(PLANT_SPATIAL_MODELS)), collect(keys(PLANT_WALLED_MODELS)))))")
    id, nq, nu, nc, nf, nw = haskey(PLANT_WALLED_MODELS, model) ? PLANT_WALLED_MODELS[model] :
                             haskey(PLANT_SPATIAL_MODELS, model) ? PLANT_SPATIAL_MODELS[model] :
                             haskey(PLANT_ENV_MODELS, model) ? PLANT_ENV_MODELS[model] : PLANT_MODELS[model]
    B = size(q0, 2)
    (size(q0, 1) == nq && size(q1) == (nq, B) && size(u) == (nu, B)) || error("plant_step($model): q0, q1 must be $nq x B and u $nu x B")
    (w === nothing || size(w) == (nw, B)) || error("plant_step($model): w must be $nw x B")
    q2 = zeros(nq, B); γ = zeros(nc, B); b = zeros(nf * nc, B); status = zeros(Cint, B); iters = zeros(Cint, B)
    check(ccall((:cimpc_plant_step, LIB), Cint,
                (Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Ref{IpOpts},
                 Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}),
                id, B, q0, q1, u, w === nothing ? C_NULL : w, μ, h_sim, Ref(opts isa IpOpts ? opts : IpOpts(opts)), q2, γ, b, status, iters))
    return q2, γ, b, status, iters
end

# ---- open-loop rollout: T plant steps in one call (simulate!(sim, q1, v1) with an open_loop_policy, simulator.jl, policy.jl:4-34) -----
const TERRAIN_MAX_PIECES = 8                        # CIMPC_TERRAIN_MAX_PIECES
struct Terrain                                      # cimpc_terrain (field order = C order); coef is row-major pieces x 4
    kind::Cint; n_pieces::Cint
    p::NTuple{4,Cdouble}
    brk::NTuple{TERRAIN_MAX_PIECES,Cdouble}
    off::NTuple{TERRAIN_MAX_PIECES,Cdouble}
    coef::NTuple{4 * TERRAIN_MAX_PIECES,Cdouble}
end
# (CIMPC_PLANT_* id, nq, nu, nc, friction directions per contact, nw) of a plant model, from the four tables above
function _plant_dims(model::Symbol)
    haskey(PLANT_WALLED_MODELS, model) && return PLANT_WALLED_MODELS[model]
    haskey(PLANT_SPATIAL_MODELS, model) && return PLANT_SPATIAL_MODELS[model]
    haskey(PLANT_ENV_MODELS, model) && return PLANT_ENV_MODELS[model]
    haskey(PLANT_MODELS, model) && return PLANT_MODELS[model]
    error("cimpc_plant_rollout has no model $model (available: " *
          "$(vcat(collect(keys(PLANT_MODELS)), collect(keys(PLANT_ENV_MODELS)), collect(keys(PLANT_SPATIAL_MODELS)), collect(keys(PLANT_WALLED_MODELS)))))")
end
"""
    plant_rollout(model, q1, v1, u, μ, h_sim, opts; N_sample = 1, w = nothing, w_hold = 1, terrain = nothing, steps = K N_sample,
                  steps_per_launch = 0, diff_sol = false, grad_reg = nothing, grad_cols = nothing) -> (ok, q, u_applied, γ, b, status, iters)

`simulate!(sim, q1, v1)` under `open_loop_policy(u; N_sample)` for B robots in ONE call, every intermediate state on the device.
q1, v1: nq x B; u: nu x K (one schedule for every robot) or nu x B x K, nominal controls applied as u[k] / N_sample (policy.jl:26);
w: nothing, nw x K_w or nw x B x K_w, applied as it stands, each held for w_hold steps; μ: a number or B of them; terrain: nothing
(flat ground) or a vector of 1 or B `Terrain`.  Returns q: nq x B x (steps + 2) with q[:, :, 1] = q1 - h v1, γ: nc x B x steps,
b: nb x B x steps, status, iters: B x steps.  Sizes are checked against the model's table; unknown models are an error.

`diff_sol = true` (simulator.jl:23,31,60) appends the step gradients, a named tuple `(dz, z, status)`: dz nr x n_cols x B x steps with
nr = nq + nc + nb the rows [q2; γ; b] and the columns the leading `grad_cols` of θ = [q0; q1; u1; w1; μ; h] (default 2nq + nu: the nine
blocks ∂q3∂q1 ... ∂b1∂u1 of the reference's GradientTrajectory are its slices), z: nz x B x steps the converged z of every step, status
B x steps (0: the step is not differentiated and its block is zero).  `grad_reg` (default κ_tol γ_reg) is the regularization of
`cimpc_plant_rollout_grad`; every other return value is unchanged.
"""
function plant_rollout(model::Symbol, q1::Matrix{Float64}, v1::Matrix{Float64}, u::Array{Float64}, μ, h_sim, opts;
                       N_sample::Int = 1, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                       terrain::Union{Nothing,Vector{Terrain}} = nothing, steps::Int = size(u, ndims(u)) * N_sample, steps_per_launch::Int = 0,
                       diff_sol::Bool = false, grad_reg = nothing, grad_cols = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    (size(q1, 1) == nq && size(v1) == (nq, B)) || error("plant_rollout($model): q1, v1 must be $nq x B")
    us = ndims(u) == 2 ? reshape(u, nu, 1, :) : u                  # nu x n_u x K, column-major = K x n_u x nu in the library's order
    (ndims(us) == 3 && size(us, 1) == nu && size(us, 2) in (1, B) && size(us, 3) >= 1) || error("plant_rollout($model): u must be $nu x K or $nu x B x K")
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    (ws === nothing || (ndims(ws) == 3 && size(ws, 1) == nw && size(ws, 2) in (1, B) && size(ws, 3) >= 1)) || error("plant_rollout($model): w must be $nw x K_w or $nw x B x K_w")
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_rollout($model): one friction coefficient or one per robot")
    (terrain === nothing || length(terrain) in (1, B)) || error("plant_rollout($model): one terrain or one per robot")
    (steps >= 1 && N_sample >= 1 && w_hold >= 1) || error("plant_rollout($model): steps, N_sample, w_hold must be at least 1")
    ua = us ./ N_sample
    q0 = q1 .- h_sim .* v1
    q = zeros(nq, B, steps + 2); γ = zeros(nc, B, steps); b = zeros(nf * nc, B, steps)
    status = zeros(Cint, B, steps); iters = zeros(Cint, B, steps)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    K_u, n_u = size(ua, 3), size(ua, 2)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    if diff_sol
        nz = nq + 4 * nc + 2 * nf * nc; nθ = 2 * nq + nu + nw + 2; nr = nq + nc + nf * nc
        reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
        n_cols = grad_cols === nothing ? 2 * nq + nu : Int(grad_cols)
        (1 <= n_cols <= nθ && reg >= 0) || error("plant_rollout($model): grad_cols must be in 1 .. $nθ and grad_reg >= 0")
        z = zeros(nz, B, steps); dz = zeros(nr, n_cols, B, steps); grad_status = zeros(Cint, B, steps)
        check(@ccall LIB.cimpc_plant_rollout_grad(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                  q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                                  wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                                  h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                                  status::Ptr{Cint}, iters::Ptr{Cint}, reg::Cdouble, n_cols::Cint, z::Ptr{Cdouble},
                                                  dz::Ptr{Cdouble}, grad_status::Ptr{Cint})::Cint)
        rows = min.((0:steps - 1) .÷ N_sample, size(ua, 3) - 1) .+ 1
        u_applied = repeat(ua[:, :, rows], 1, B ÷ size(ua, 2), 1)
        return all(status .== 1), q, u_applied, γ, b, status, iters, (dz = dz, z = z, status = grad_status)
    end
    check(@ccall LIB.cimpc_plant_rollout(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                         q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                         wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                         h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                         status::Ptr{Cint}, iters::Ptr{Cint})::Cint)
    rows = min.((0:steps - 1) .÷ N_sample, size(ua, 3) - 1) .+ 1
    u_applied = repeat(ua[:, :, rows], 1, B ÷ size(ua, 2), 1)
    return all(status .== 1), q, u_applied, γ, b, status, iters
end

# ---- a loss backpropagated through a rollout: the tape of its step gradients on the device and the reverse chain over it ------------
"""
The step gradients of one rollout, kept on the device (`cimpc_plant_rollout_tape`).  `close(tape)` frees them; so does the finalizer.
"""
mutable struct PlantTape
    handle::Ptr{Cvoid}
    model::Symbol
    B::Int; T::Int; n_cols::Int
    grad_status::Matrix{Cint}
    function PlantTape(handle::Ptr{Cvoid}, model::Symbol, B::Int, T::Int, n_cols::Int, grad_status::Matrix{Cint})
        tape = new(handle, model, B, T, n_cols, grad_status)
        finalizer(close, tape)
        return tape
    end
end
function Base.close(tape::PlantTape)
    if tape.handle != C_NULL
        @ccall LIB.cimpc_plant_tape_destroy(tape.handle::Ptr{Cvoid})::Cint
        tape.handle = C_NULL
    end
    return nothing
end
"""
    plant_rollout_tape(model, q1, v1, u, μ, h_sim, opts; N_sample = 1, w = nothing, w_hold = 1, terrain = nothing, steps = K N_sample,
                       steps_per_launch = 0, grad_reg = nothing, grad_cols = nothing) -> (ok, q, u_applied, γ, b, status, iters, tape)

`plant_rollout` that records its step gradients on the device instead of returning them: the first seven values are those of
`plant_rollout`, `tape` a `PlantTape` for `plant_tape_vjp`.  `grad_cols` (default and least 2nq + nu) up to nθ adds the w, μ and h columns.
"""
function plant_rollout_tape(model::Symbol, q1::Matrix{Float64}, v1::Matrix{Float64}, u::Array{Float64}, μ, h_sim, opts;
                            N_sample::Int = 1, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                            terrain::Union{Nothing,Vector{Terrain}} = nothing, steps::Int = size(u, ndims(u)) * N_sample,
                            steps_per_launch::Int = 0, grad_reg = nothing, grad_cols = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    (size(q1, 1) == nq && size(v1) == (nq, B)) || error("plant_rollout_tape($model): q1, v1 must be $nq x B")
    us = ndims(u) == 2 ? reshape(u, nu, 1, :) : u
    (ndims(us) == 3 && size(us, 1) == nu && size(us, 2) in (1, B) && size(us, 3) >= 1) || error("plant_rollout_tape($model): u must be $nu x K or $nu x B x K")
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    (ws === nothing || (ndims(ws) == 3 && size(ws, 1) == nw && size(ws, 2) in (1, B) && size(ws, 3) >= 1)) || error("plant_rollout_tape($model): w must be $nw x K_w or $nw x B x K_w")
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_rollout_tape($model): one friction coefficient or one per robot")
    (terrain === nothing || length(terrain) in (1, B)) || error("plant_rollout_tape($model): one terrain or one per robot")
    (steps >= 1 && N_sample >= 1 && w_hold >= 1) || error("plant_rollout_tape($model): steps, N_sample, w_hold must be at least 1")
    ua = us ./ N_sample
    q0 = q1 .- h_sim .* v1
    q = zeros(nq, B, steps + 2); γ = zeros(nc, B, steps); b = zeros(nf * nc, B, steps)
    status = zeros(Cint, B, steps); iters = zeros(Cint, B, steps); grad_status = zeros(Cint, B, steps)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    K_u, n_u = size(ua, 3), size(ua, 2)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    nθ = 2 * nq + nu + nw + 2
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_cols = grad_cols === nothing ? 2 * nq + nu : Int(grad_cols)
    (2 * nq + nu <= n_cols <= nθ && reg >= 0) || error("plant_rollout_tape($model): grad_cols must be in $(2 * nq + nu) .. $nθ and grad_reg >= 0")
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    z = C_NULL
    check(@ccall LIB.cimpc_plant_rollout_tape(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                              q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                              wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                              h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                              status::Ptr{Cint}, iters::Ptr{Cint}, reg::Cdouble, n_cols::Cint, z::Ptr{Cdouble},
                                              grad_status::Ptr{Cint}, handle::Ref{Ptr{Cvoid}})::Cint)
    rows = min.((0:steps - 1) .÷ N_sample, size(ua, 3) - 1) .+ 1
    u_applied = repeat(ua[:, :, rows], 1, B ÷ size(ua, 2), 1)
    return all(status .== 1), q, u_applied, γ, b, status, iters, PlantTape(handle[], model, B, steps, n_cols, grad_status)
end

"""
    plant_tape_vjp(tape; gq = nothing, ggamma = nothing, gb = nothing) -> (g_q0, g_q1, g_u_step, g_w_step, g_μ, g_h, n_cut)

The reverse chain of `cimpc_plant_tape_vjp` over a tape: cotangents gq nq x B x (T + 2), ggamma nc x B x T, gb nb x B x T (nothing is
zeros, not all three) -> g_q0, g_q1 nq x B (the gradients with respect to q[:, :, 1] and q[:, :, 2]: that of q1 is their sum, that of v1
is -h g_q0), g_u_step nu x B x T per applied control, g_w_step nw x B x T, g_μ and g_h B each (`nothing` where the tape's columns stop
short of them), n_cut B: the steps of a robot whose gradient status is 0.  May be called any number of times.
"""
function plant_tape_vjp(tape::PlantTape; gq::Union{Nothing,Array{Float64,3}} = nothing, ggamma::Union{Nothing,Array{Float64,3}} = nothing,
                        gb::Union{Nothing,Array{Float64,3}} = nothing)
    tape.handle != C_NULL || error("plant_tape_vjp: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, nb = tape.B, tape.T, nf * nc
    (gq === nothing && ggamma === nothing && gb === nothing) && error("plant_tape_vjp: at least one of gq, ggamma, gb")
    (gq === nothing || size(gq) == (nq, B, T + 2)) || error("plant_tape_vjp: gq must be $nq x $B x $(T + 2)")
    (ggamma === nothing || size(ggamma) == (nc, B, T)) || error("plant_tape_vjp: ggamma must be $nc x $B x $T")
    (gb === nothing || size(gb) == (nb, B, T)) || error("plant_tape_vjp: gb must be $nb x $B x $T")
    c_mu = 2 * nq + nu + nw
    g_q0 = zeros(nq, B); g_q1 = zeros(nq, B); g_u = zeros(nu, B, T); n_cut = zeros(Cint, B)
    g_w = tape.n_cols >= c_mu ? zeros(nw, B, T) : nothing
    g_μ = tape.n_cols >= c_mu + 1 ? zeros(B) : nothing
    g_h = tape.n_cols >= c_mu + 2 ? zeros(B) : nothing
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve gq ggamma gb g_w g_μ g_h begin
        pq, pg, pb, pw, pm, ph = p(gq), p(ggamma), p(gb), p(g_w), p(g_μ), p(g_h)
        check(@ccall LIB.cimpc_plant_tape_vjp(tape.handle::Ptr{Cvoid}, pq::Ptr{Cdouble}, pg::Ptr{Cdouble}, pb::Ptr{Cdouble}, g_q0::Ptr{Cdouble},
                                              g_q1::Ptr{Cdouble}, g_u::Ptr{Cdouble}, pw::Ptr{Cdouble}, pm::Ptr{Cdouble}, ph::Ptr{Cdouble},
                                              n_cut::Ptr{Cint})::Cint)
    end
    return g_q0, g_q1, g_u, g_w, g_μ, g_h, n_cut
end

# ---- closed-loop rollouts under linear state feedback (cimpc.h: cimpc_feedback; DESIGN.md section 3, item 3c) --------------------------
# Unexecuted, like the rest of this binding (INTEGRATION.md).
"""
`cimpc_feedback`: the pointers and sizes of a feedback schedule as the library reads them.  Built by the closed-loop calls from
`K` (nu x 2nq x K_f shared, or nu x 2nq x B x K_f: a column-major block per row, `reference_gains`' layout) and `x_ref` (2nq x K_f or
2nq x B x K_f).
"""
struct Feedback
    K::Ptr{Cdouble}
    x_ref::Ptr{Cdouble}
    K_f::Cint; n_f::Cint; hold_f::Cint
    n_sample::Cdouble
end

# the inputs the closed-loop rollouts share, checked and laid out: the open-loop ones and the schedule's arrays
function _closed_loop_inputs(what, model, q1, v1, u, μ, w, terrain, steps, N_sample, w_hold, K, x_ref, hold, n_sample)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    (size(q1, 1) == nq && size(v1) == (nq, B)) || error("$what($model): q1, v1 must be $nq x B")
    us = ndims(u) == 2 ? reshape(u, nu, 1, :) : u
    (ndims(us) == 3 && size(us, 1) == nu && size(us, 2) in (1, B) && size(us, 3) >= 1) || error("$what($model): u must be $nu x K or $nu x B x K")
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    (ws === nothing || (ndims(ws) == 3 && size(ws, 1) == nw && size(ws, 2) in (1, B) && size(ws, 3) >= 1)) || error("$what($model): w must be $nw x K_w or $nw x B x K_w")
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("$what($model): one friction coefficient or one per robot")
    (terrain === nothing || length(terrain) in (1, B)) || error("$what($model): one terrain or one per robot")
    (steps >= 1 && N_sample >= 1 && w_hold >= 1 && hold >= 1) || error("$what($model): steps, N_sample, w_hold, hold must be at least 1")
    Ks = ndims(K) == 3 ? reshape(K, nu, 2 * nq, 1, :) : K
    xs = ndims(x_ref) == 2 ? reshape(x_ref, 2 * nq, 1, :) : x_ref
    (ndims(Ks) == 4 && size(Ks)[1:2] == (nu, 2 * nq) && size(Ks, 3) in (1, B) && size(Ks, 4) >= 1 && size(xs) == (2 * nq, size(Ks, 3), size(Ks, 4))) ||
        error("$what($model): K must be $nu x $(2 * nq) x K_f or $nu x $(2 * nq) x B x K_f beside x_ref $(2 * nq) x K_f or $(2 * nq) x B x K_f")
    ns = n_sample === nothing ? Float64(N_sample) : Float64(n_sample)
    (isfinite(ns) && ns > 0) || error("$what($model): n_sample must be finite and positive")
    return us ./ N_sample, ws, μs, Array(Ks ./ N_sample), Array(Float64.(xs)), ns
end

"""
    plant_rollout_feedback(model, q1, v1, u, μ, h_sim, opts, K, x_ref; hold = 1, n_sample = N_sample, N_sample = 1, w = nothing,
                           w_hold = 1, terrain = nothing, steps = K N_sample, steps_per_launch = 0)
        -> (ok, q, u_applied, γ, b, status, iters, fb_err)

`plant_rollout` under u_t = ū_t + (K[k] / N_sample) (x_ref[k] - x_t), k = min(t ÷ hold, K_f - 1), in one call: u_applied nu x B x steps is
what the device applied, fb_err 2nq x B x steps the errors x_ref - x_t.
"""
function plant_rollout_feedback(model::Symbol, q1::Matrix{Float64}, v1::Matrix{Float64}, u::Array{Float64}, μ, h_sim, opts,
                                K::Array{Float64}, x_ref::Array{Float64}; hold::Int = 1, n_sample = nothing,
                                N_sample::Int = 1, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                                terrain::Union{Nothing,Vector{Terrain}} = nothing, steps::Int = size(u, ndims(u)) * N_sample,
                                steps_per_launch::Int = 0)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    ua, ws, μs, Ks, xs, ns = _closed_loop_inputs("plant_rollout_feedback", model, q1, v1, u, μ, w, terrain, steps, N_sample, w_hold, K, x_ref, hold, n_sample)
    q0 = q1 .- h_sim .* v1
    q = zeros(nq, B, steps + 2); γ = zeros(nc, B, steps); b = zeros(nf * nc, B, steps)
    status = zeros(Cint, B, steps); iters = zeros(Cint, B, steps)
    u_applied = zeros(nu, B, steps); fb_err = zeros(2 * nq, B, steps)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    K_u, n_u = size(ua, 3), size(ua, 2)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    GC.@preserve Ks xs begin
        fb = Ref(Feedback(pointer(Ks), pointer(xs), size(Ks, 4), size(Ks, 3), hold, ns))
        check(@ccall LIB.cimpc_plant_rollout_feedback(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                      q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                                      wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                                      h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                                      status::Ptr{Cint}, iters::Ptr{Cint}, fb::Ref{Feedback}, u_applied::Ptr{Cdouble},
                                                      fb_err::Ptr{Cdouble})::Cint)
    end
    return all(status .== 1), q, u_applied, γ, b, status, iters, fb_err
end

"""
    plant_rollout_feedback_limits(model, q1, v1, u, μ, h_sim, opts, K, x_ref, u_lo, u_hi; ...) -> (ok, q, u_applied, γ, b, status, iters, fb_err)

`plant_rollout_feedback` under control limits (`cimpc_plant_rollout_feedback_limits`; DESIGN.md section 3, item 3g): u_lo, u_hi are nu x 1
(shared) or nu x B, ±Inf meaning no limit; a step applies and u_applied stores the law's control limited to [u_lo, u_hi]; fb_err is
unchanged.  The keywords are `plant_rollout_feedback`'s.  Unexecuted, like the rest of this binding.
"""
function plant_rollout_feedback_limits(model::Symbol, q1::Matrix{Float64}, v1::Matrix{Float64}, u::Array{Float64}, μ, h_sim, opts,
                                       K::Array{Float64}, x_ref::Array{Float64}, u_lo::Matrix{Float64}, u_hi::Matrix{Float64};
                                       hold::Int = 1, n_sample = nothing, N_sample::Int = 1, w::Union{Nothing,Array{Float64}} = nothing,
                                       w_hold::Int = 1, terrain::Union{Nothing,Vector{Terrain}} = nothing,
                                       steps::Int = size(u, ndims(u)) * N_sample, steps_per_launch::Int = 0)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    (size(u_lo) == size(u_hi) && size(u_lo, 1) == nu && size(u_lo, 2) in (1, B)) || error("plant_rollout_feedback_limits: u_lo, u_hi must be $nu x 1 or $nu x $B")
    ua, ws, μs, Ks, xs, ns = _closed_loop_inputs("plant_rollout_feedback_limits", model, q1, v1, u, μ, w, terrain, steps, N_sample, w_hold, K, x_ref, hold, n_sample)
    q0 = q1 .- h_sim .* v1
    q = zeros(nq, B, steps + 2); γ = zeros(nc, B, steps); b = zeros(nf * nc, B, steps)
    status = zeros(Cint, B, steps); iters = zeros(Cint, B, steps)
    u_applied = zeros(nu, B, steps); fb_err = zeros(2 * nq, B, steps)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    K_u, n_u = size(ua, 3), size(ua, 2)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs); n_lim = size(u_lo, 2)
    GC.@preserve Ks xs begin
        fb = Ref(Feedback(pointer(Ks), pointer(xs), size(Ks, 4), size(Ks, 3), hold, ns))
        check(@ccall LIB.cimpc_plant_rollout_feedback_limits(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                             q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                                             wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                                             h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                                             status::Ptr{Cint}, iters::Ptr{Cint}, fb::Ref{Feedback}, u_applied::Ptr{Cdouble},
                                                             fb_err::Ptr{Cdouble}, n_lim::Cint, u_lo::Ptr{Cdouble}, u_hi::Ptr{Cdouble})::Cint)
    end
    return all(status .== 1), q, u_applied, γ, b, status, iters, fb_err
end

"""
    plant_rollout_tape_feedback(model, q1, v1, u, μ, h_sim, opts, K, x_ref; hold = 1, n_sample = N_sample, ..., grad_reg = nothing,
                                grad_cols = nothing) -> (ok, q, u_applied, γ, b, status, iters, tape, fb_err)

`plant_rollout_feedback` that records its step gradients on the device: `tape` a `PlantTape` whose chain (`plant_tape_vjp`,
`plant_tape_vjp_feedback`) includes the feedback path.  The gradient of K row k is the sum of g_u_step[:, b, t] fb_err[:, b, t]' over
the steps and robots that read it, divided by N_sample.
"""
function plant_rollout_tape_feedback(model::Symbol, q1::Matrix{Float64}, v1::Matrix{Float64}, u::Array{Float64}, μ, h_sim, opts,
                                     K::Array{Float64}, x_ref::Array{Float64}; hold::Int = 1, n_sample = nothing,
                                     N_sample::Int = 1, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                                     terrain::Union{Nothing,Vector{Terrain}} = nothing, steps::Int = size(u, ndims(u)) * N_sample,
                                     steps_per_launch::Int = 0, grad_reg = nothing, grad_cols = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    ua, ws, μs, Ks, xs, ns = _closed_loop_inputs("plant_rollout_tape_feedback", model, q1, v1, u, μ, w, terrain, steps, N_sample, w_hold, K, x_ref, hold, n_sample)
    q0 = q1 .- h_sim .* v1
    q = zeros(nq, B, steps + 2); γ = zeros(nc, B, steps); b = zeros(nf * nc, B, steps)
    status = zeros(Cint, B, steps); iters = zeros(Cint, B, steps); grad_status = zeros(Cint, B, steps)
    u_applied = zeros(nu, B, steps); fb_err = zeros(2 * nq, B, steps)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    K_u, n_u = size(ua, 3), size(ua, 2)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    nθ = 2 * nq + nu + nw + 2
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_cols = grad_cols === nothing ? 2 * nq + nu : Int(grad_cols)
    (2 * nq + nu <= n_cols <= nθ && reg >= 0) || error("plant_rollout_tape_feedback($model): grad_cols must be in $(2 * nq + nu) .. $nθ and grad_reg >= 0")
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    z = C_NULL
    GC.@preserve Ks xs begin
        fb = Ref(Feedback(pointer(Ks), pointer(xs), size(Ks, 4), size(Ks, 3), hold, ns))
        check(@ccall LIB.cimpc_plant_rollout_tape_feedback(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                           q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                                           wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                                           h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                                           status::Ptr{Cint}, iters::Ptr{Cint}, reg::Cdouble, n_cols::Cint, z::Ptr{Cdouble},
                                                           grad_status::Ptr{Cint}, handle::Ref{Ptr{Cvoid}}, fb::Ref{Feedback},
                                                           u_applied::Ptr{Cdouble}, fb_err::Ptr{Cdouble})::Cint)
    end
    return all(status .== 1), q, u_applied, γ, b, status, iters, PlantTape(handle[], model, B, steps, n_cols, grad_status), fb_err
end

"""
    plant_rollout_tape_feedback_limits(model, q1, v1, u, μ, h_sim, opts, K, x_ref, u_lo, u_hi; ...)
        -> (ok, q, u_applied, γ, b, status, iters, tape, fb_err, clamped)

`plant_rollout_tape_feedback` under control limits, differentiated by DESIGN.md section 3, item 3i (`cimpc_plant_rollout_tape_feedback_limits`):
u_lo, u_hi are nu x 1 (shared) or nu x B, ±Inf meaning no limit.  Control i of a step is free where u_lo[i] < u_applied[i, b, t] < u_hi[i] and
clamped otherwise; clamped (B x steps) holds a word per step whose bit i - 1 is set where control i is clamped, the tape owns the same mask, and
`plant_tape_vjp`, `plant_tape_vjp_feedback` and `plant_tape_jvp` on it pass nothing through a clamped control: the limited law's derivative is the
unlimited law's where free and exactly 0.0 where clamped.  The keywords are `plant_rollout_tape_feedback`'s.  Unexecuted, like the rest of this binding.
"""
function plant_rollout_tape_feedback_limits(model::Symbol, q1::Matrix{Float64}, v1::Matrix{Float64}, u::Array{Float64}, μ, h_sim, opts,
                                            K::Array{Float64}, x_ref::Array{Float64}, u_lo::Matrix{Float64}, u_hi::Matrix{Float64};
                                            hold::Int = 1, n_sample = nothing, N_sample::Int = 1, w::Union{Nothing,Array{Float64}} = nothing,
                                            w_hold::Int = 1, terrain::Union{Nothing,Vector{Terrain}} = nothing,
                                            steps::Int = size(u, ndims(u)) * N_sample, steps_per_launch::Int = 0, grad_reg = nothing,
                                            grad_cols = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    (size(u_lo) == size(u_hi) && size(u_lo, 1) == nu && size(u_lo, 2) in (1, B)) || error("plant_rollout_tape_feedback_limits: u_lo, u_hi must be $nu x 1 or $nu x $B")
    ua, ws, μs, Ks, xs, ns = _closed_loop_inputs("plant_rollout_tape_feedback_limits", model, q1, v1, u, μ, w, terrain, steps, N_sample, w_hold, K, x_ref, hold, n_sample)
    q0 = q1 .- h_sim .* v1
    q = zeros(nq, B, steps + 2); γ = zeros(nc, B, steps); b = zeros(nf * nc, B, steps)
    status = zeros(Cint, B, steps); iters = zeros(Cint, B, steps); grad_status = zeros(Cint, B, steps); clamped = zeros(Cint, B, steps)
    u_applied = zeros(nu, B, steps); fb_err = zeros(2 * nq, B, steps)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    K_u, n_u = size(ua, 3), size(ua, 2)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs); n_lim = size(u_lo, 2)
    nθ = 2 * nq + nu + nw + 2
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_cols = grad_cols === nothing ? 2 * nq + nu : Int(grad_cols)
    (2 * nq + nu <= n_cols <= nθ && reg >= 0) || error("plant_rollout_tape_feedback_limits($model): grad_cols must be in $(2 * nq + nu) .. $nθ and grad_reg >= 0")
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    z = C_NULL
    GC.@preserve Ks xs begin
        fb = Ref(Feedback(pointer(Ks), pointer(xs), size(Ks, 4), size(Ks, 3), hold, ns))
        check(@ccall LIB.cimpc_plant_rollout_tape_feedback_limits(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                                  q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                                                  wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                                                  h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                                                  status::Ptr{Cint}, iters::Ptr{Cint}, reg::Cdouble, n_cols::Cint, z::Ptr{Cdouble},
                                                                  grad_status::Ptr{Cint}, handle::Ref{Ptr{Cvoid}}, fb::Ref{Feedback},
                                                                  u_applied::Ptr{Cdouble}, fb_err::Ptr{Cdouble}, n_lim::Cint, u_lo::Ptr{Cdouble},
                                                                  u_hi::Ptr{Cdouble}, clamped::Ptr{Cint})::Cint)
    end
    return all(status .== 1), q, u_applied, γ, b, status, iters, PlantTape(handle[], model, B, steps, n_cols, grad_status), fb_err, clamped
end

"""
    plant_rollout_grad_feedback_limits(model, q1, v1, u, μ, h_sim, opts, K, x_ref, u_lo, u_hi; ...)
        -> (ok, q, u_applied, γ, b, status, iters, (dz, z, status), fb_err)

`plant_rollout_feedback_limits` with the step gradients of every step (`cimpc_plant_rollout_grad_feedback_limits`; DESIGN.md section 3, item 3i):
dz nr x grad_cols x B x steps, z nz x B x steps and the gradient status B x steps, as `plant_rollout(...; diff_sol = true)` returns them.  The blocks
are taken with the applied, limited control in θ: they are those of the open-loop rollout on u_applied and do not see the clamp.  The keywords are
`plant_rollout_tape_feedback`'s.  Unexecuted, like the rest of this binding.
"""
function plant_rollout_grad_feedback_limits(model::Symbol, q1::Matrix{Float64}, v1::Matrix{Float64}, u::Array{Float64}, μ, h_sim, opts,
                                            K::Array{Float64}, x_ref::Array{Float64}, u_lo::Matrix{Float64}, u_hi::Matrix{Float64};
                                            hold::Int = 1, n_sample = nothing, N_sample::Int = 1, w::Union{Nothing,Array{Float64}} = nothing,
                                            w_hold::Int = 1, terrain::Union{Nothing,Vector{Terrain}} = nothing,
                                            steps::Int = size(u, ndims(u)) * N_sample, steps_per_launch::Int = 0, grad_reg = nothing,
                                            grad_cols = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    B = size(q1, 2)
    (size(u_lo) == size(u_hi) && size(u_lo, 1) == nu && size(u_lo, 2) in (1, B)) || error("plant_rollout_grad_feedback_limits: u_lo, u_hi must be $nu x 1 or $nu x $B")
    ua, ws, μs, Ks, xs, ns = _closed_loop_inputs("plant_rollout_grad_feedback_limits", model, q1, v1, u, μ, w, terrain, steps, N_sample, w_hold, K, x_ref, hold, n_sample)
    q0 = q1 .- h_sim .* v1
    q = zeros(nq, B, steps + 2); γ = zeros(nc, B, steps); b = zeros(nf * nc, B, steps)
    status = zeros(Cint, B, steps); iters = zeros(Cint, B, steps); grad_status = zeros(Cint, B, steps)
    u_applied = zeros(nu, B, steps); fb_err = zeros(2 * nq, B, steps)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    K_u, n_u = size(ua, 3), size(ua, 2)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs); n_lim = size(u_lo, 2)
    nb = nf * nc; nr = nq + nc + nb; nz = nq + 4 * nc + 2 * nb; nθ = 2 * nq + nu + nw + 2
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_cols = grad_cols === nothing ? 2 * nq + nu : Int(grad_cols)
    (1 <= n_cols <= nθ && reg >= 0) || error("plant_rollout_grad_feedback_limits($model): grad_cols must be in 1 .. $nθ and grad_reg >= 0")
    z = zeros(nz, B, steps); dz = zeros(nr, n_cols, B, steps)
    GC.@preserve Ks xs begin
        fb = Ref(Feedback(pointer(Ks), pointer(xs), size(Ks, 4), size(Ks, 3), hold, ns))
        check(@ccall LIB.cimpc_plant_rollout_grad_feedback_limits(id::Cint, B::Cint, steps::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                                  q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, ua::Ptr{Cdouble}, K_u::Cint, n_u::Cint, N_sample::Cint,
                                                                  wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint,
                                                                  h_sim::Cdouble, o::Ref{IpOpts}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                                                  status::Ptr{Cint}, iters::Ptr{Cint}, reg::Cdouble, n_cols::Cint, z::Ptr{Cdouble},
                                                                  dz::Ptr{Cdouble}, grad_status::Ptr{Cint}, fb::Ref{Feedback},
                                                                  u_applied::Ptr{Cdouble}, fb_err::Ptr{Cdouble}, n_lim::Cint, u_lo::Ptr{Cdouble},
                                                                  u_hi::Ptr{Cdouble})::Cint)
    end
    return all(status .== 1), q, u_applied, γ, b, status, iters, (dz = dz, z = z, status = grad_status), fb_err
end

"""
    plant_tape_vjp_feedback(tape; gq = nothing, ggamma = nothing, gb = nothing) -> (g_q0, g_q1, g_u_step, g_w_step, g_μ, g_h, n_cut, g_xref_step)

`plant_tape_vjp` on the tape of a closed-loop rollout, with g_xref_step 2nq x B x T, the gradient with respect to the reference state
each step read (an open-loop tape is refused by the library).  g_u_step is the gradient of the open-loop part ū.
"""
function plant_tape_vjp_feedback(tape::PlantTape; gq::Union{Nothing,Array{Float64,3}} = nothing, ggamma::Union{Nothing,Array{Float64,3}} = nothing,
                                 gb::Union{Nothing,Array{Float64,3}} = nothing)
    tape.handle != C_NULL || error("plant_tape_vjp_feedback: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, nb = tape.B, tape.T, nf * nc
    (gq === nothing && ggamma === nothing && gb === nothing) && error("plant_tape_vjp_feedback: at least one of gq, ggamma, gb")
    (gq === nothing || size(gq) == (nq, B, T + 2)) || error("plant_tape_vjp_feedback: gq must be $nq x $B x $(T + 2)")
    (ggamma === nothing || size(ggamma) == (nc, B, T)) || error("plant_tape_vjp_feedback: ggamma must be $nc x $B x $T")
    (gb === nothing || size(gb) == (nb, B, T)) || error("plant_tape_vjp_feedback: gb must be $nb x $B x $T")
    c_mu = 2 * nq + nu + nw
    g_q0 = zeros(nq, B); g_q1 = zeros(nq, B); g_u = zeros(nu, B, T); n_cut = zeros(Cint, B); g_x = zeros(2 * nq, B, T)
    g_w = tape.n_cols >= c_mu ? zeros(nw, B, T) : nothing
    g_μ = tape.n_cols >= c_mu + 1 ? zeros(B) : nothing
    g_h = tape.n_cols >= c_mu + 2 ? zeros(B) : nothing
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve gq ggamma gb g_w g_μ g_h begin
        pq, pg, pb, pw, pm, ph = p(gq), p(ggamma), p(gb), p(g_w), p(g_μ), p(g_h)
        check(@ccall LIB.cimpc_plant_tape_vjp_feedback(tape.handle::Ptr{Cvoid}, pq::Ptr{Cdouble}, pg::Ptr{Cdouble}, pb::Ptr{Cdouble},
                                                       g_q0::Ptr{Cdouble}, g_q1::Ptr{Cdouble}, g_u::Ptr{Cdouble}, pw::Ptr{Cdouble},
                                                       pm::Ptr{Cdouble}, ph::Ptr{Cdouble}, n_cut::Ptr{Cint}, g_x::Ptr{Cdouble})::Cint)
    end
    return g_q0, g_q1, g_u, g_w, g_μ, g_h, n_cut, g_x
end

# ---- forward tangents through a rollout's tape, many directions per launch ----------------------------------------------------------------
"""
    plant_tape_jvp(tape; dq0 = nothing, dq1 = nothing, du_step = nothing, dw_step = nothing, dμ = nothing, dh = nothing)
        -> (dq, dγ, db, n_cut)

The forward chain of `cimpc_plant_tape_jvp` over a tape, n_dir directions in one launch: tangents dq0, dq1 nq x B x n_dir of q[0], q[1],
du_step nu x B x T x n_dir per applied control, dw_step nw x B x T x n_dir, dμ and dh B x n_dir (nothing is zeros, not all of them; dw_step,
dμ, dh only where the tape's columns reach) to dq nq x B x (T + 2) x n_dir, dγ nc x B x T x n_dir, db nb x B x T x n_dir and n_cut (B).  For
the arguments of `plant_rollout_tape`: dq0 = (δq1 - h δv1) - δh v1, dq1 = δq1, du_step[:, b, t] = δu[k] / N_sample.  A direction's
result does not depend on what rides with it.
"""
function plant_tape_jvp(tape::PlantTape; dq0::Union{Nothing,Array{Float64,3}} = nothing, dq1::Union{Nothing,Array{Float64,3}} = nothing,
                        du_step::Union{Nothing,Array{Float64,4}} = nothing, dw_step::Union{Nothing,Array{Float64,4}} = nothing,
                        dμ::Union{Nothing,Matrix{Float64}} = nothing, dh::Union{Nothing,Matrix{Float64}} = nothing)
    tape.handle != C_NULL || error("plant_tape_jvp: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, nb = tape.B, tape.T, nf * nc
    given = [a for a in (dq0, dq1, du_step, dw_step, dμ, dh) if a !== nothing]
    isempty(given) && error("plant_tape_jvp: at least one tangent")
    n_dir = size(given[1], ndims(given[1]))
    (dq0 === nothing || size(dq0) == (nq, B, n_dir)) || error("plant_tape_jvp: dq0 must be $nq x $B x n_dir")
    (dq1 === nothing || size(dq1) == (nq, B, n_dir)) || error("plant_tape_jvp: dq1 must be $nq x $B x n_dir")
    (du_step === nothing || size(du_step) == (nu, B, T, n_dir)) || error("plant_tape_jvp: du_step must be $nu x $B x $T x n_dir")
    (dw_step === nothing || size(dw_step) == (nw, B, T, n_dir)) || error("plant_tape_jvp: dw_step must be $nw x $B x $T x n_dir")
    (dμ === nothing || size(dμ) == (B, n_dir)) || error("plant_tape_jvp: dμ must be $B x n_dir")
    (dh === nothing || size(dh) == (B, n_dir)) || error("plant_tape_jvp: dh must be $B x n_dir")
    dq = zeros(nq, B, T + 2, n_dir); dγ = zeros(nc, B, T, n_dir); db = zeros(nb, B, T, n_dir); n_cut = zeros(Cint, B)
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve dq0 dq1 du_step dw_step dμ dh begin
        p0, p1, pu, pw, pm, ph = p(dq0), p(dq1), p(du_step), p(dw_step), p(dμ), p(dh)
        check(@ccall LIB.cimpc_plant_tape_jvp(tape.handle::Ptr{Cvoid}, n_dir::Cint, p0::Ptr{Cdouble}, p1::Ptr{Cdouble}, pu::Ptr{Cdouble},
                                              pw::Ptr{Cdouble}, pm::Ptr{Cdouble}, ph::Ptr{Cdouble}, dq::Ptr{Cdouble}, dγ::Ptr{Cdouble},
                                              db::Ptr{Cdouble}, n_cut::Ptr{Cint})::Cint)
    end
    return dq, dγ, db, n_cut
end

"""
    plant_tape_jvp_feedback(tape; dq0, dq1, du_step, dw_step, dμ, dh, dxref_step = nothing) -> (dq, dγ, db, n_cut, du_applied)

`plant_tape_jvp` on the tape of a closed-loop rollout, with dxref_step 2nq x B x T x n_dir, the tangent of the reference state each step
read, and du_applied nu x B x T x n_dir, the tangent of the controls the device applied (an open-loop tape is refused by the library).
du_step is the tangent of the open-loop part ū; a tangent of the gain rows is added to it by the caller, (δK[k] / N_sample) fb_err[:, b, t].
"""
function plant_tape_jvp_feedback(tape::PlantTape; dq0::Union{Nothing,Array{Float64,3}} = nothing, dq1::Union{Nothing,Array{Float64,3}} = nothing,
                                 du_step::Union{Nothing,Array{Float64,4}} = nothing, dw_step::Union{Nothing,Array{Float64,4}} = nothing,
                                 dμ::Union{Nothing,Matrix{Float64}} = nothing, dh::Union{Nothing,Matrix{Float64}} = nothing,
                                 dxref_step::Union{Nothing,Array{Float64,4}} = nothing)
    tape.handle != C_NULL || error("plant_tape_jvp_feedback: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, nb = tape.B, tape.T, nf * nc
    given = [a for a in (dq0, dq1, du_step, dw_step, dμ, dh, dxref_step) if a !== nothing]
    isempty(given) && error("plant_tape_jvp_feedback: at least one tangent")
    n_dir = size(given[1], ndims(given[1]))
    (dq0 === nothing || size(dq0) == (nq, B, n_dir)) || error("plant_tape_jvp_feedback: dq0 must be $nq x $B x n_dir")
    (dq1 === nothing || size(dq1) == (nq, B, n_dir)) || error("plant_tape_jvp_feedback: dq1 must be $nq x $B x n_dir")
    (du_step === nothing || size(du_step) == (nu, B, T, n_dir)) || error("plant_tape_jvp_feedback: du_step must be $nu x $B x $T x n_dir")
    (dw_step === nothing || size(dw_step) == (nw, B, T, n_dir)) || error("plant_tape_jvp_feedback: dw_step must be $nw x $B x $T x n_dir")
    (dμ === nothing || size(dμ) == (B, n_dir)) || error("plant_tape_jvp_feedback: dμ must be $B x n_dir")
    (dh === nothing || size(dh) == (B, n_dir)) || error("plant_tape_jvp_feedback: dh must be $B x n_dir")
    (dxref_step === nothing || size(dxref_step) == (2 * nq, B, T, n_dir)) || error("plant_tape_jvp_feedback: dxref_step must be $(2 * nq) x $B x $T x n_dir")
    dq = zeros(nq, B, T + 2, n_dir); dγ = zeros(nc, B, T, n_dir); db = zeros(nb, B, T, n_dir); n_cut = zeros(Cint, B)
    du_applied = zeros(nu, B, T, n_dir)
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve dq0 dq1 du_step dw_step dμ dh dxref_step begin
        p0, p1, pu, pw, pm, ph, px = p(dq0), p(dq1), p(du_step), p(dw_step), p(dμ), p(dh), p(dxref_step)
        check(@ccall LIB.cimpc_plant_tape_jvp_feedback(tape.handle::Ptr{Cvoid}, n_dir::Cint, p0::Ptr{Cdouble}, p1::Ptr{Cdouble}, pu::Ptr{Cdouble},
                                                       pw::Ptr{Cdouble}, pm::Ptr{Cdouble}, ph::Ptr{Cdouble}, dq::Ptr{Cdouble}, dγ::Ptr{Cdouble},
                                                       db::Ptr{Cdouble}, n_cut::Ptr{Cint}, px::Ptr{Cdouble}, du_applied::Ptr{Cdouble})::Cint)
    end
    return dq, dγ, db, n_cut, du_applied
end

# ---- the LQ backward pass over a tape: time-varying LQR gains along the path taken ------------------------------------------------------
"""
    plant_tape_lqr(tape, Q, R; Qf = nothing, q = nothing, r = nothing, ρ = 0.0, laps = 1, keep = nothing)
        -> (K, k, P0, p0, dV, status, n_cut)

`cimpc_plant_tape_lqr`: with x_t = [q[t]; q[t+1]] (n = 2nq), u_t (m = nu) and A_t = [0 I; D1 D2], B_t = [0; Du] from the tape's blocks, the
gains of δu_t = k_t - K_t δx_t for the cost Σ ½ x'Q_t x + q_t'x + ½ u'R_t u + r_t'u with the terminal ½ x'Qf x + q_T'x, in ONE launch, a
workgroup per robot.  Q: n x n or n x n x T and R: m x m or m x m x T are shared by the robots, Qf defaults to Q (its last step's); q:
n x B x (T + 1) and r: m x B x T, both or neither; ρ >= 0 is added to the diagonal of Quu; laps > 1 walks the tape periodically (without
q, r); keep (default T) leading steps come back.  Returns K: m x n x B x keep, P0: n x n x B, status and n_cut (B), and with q, r
k: m x B x keep, p0: n x B, dV: 2 x B (nothing otherwise).  status[b] != 0: that robot's chain ended at that 1-based walk step (a
singular or non-finite step) and its outputs are zeros.
"""
function plant_tape_lqr(tape::PlantTape, Q::Array{Float64}, R::Array{Float64}; Qf::Union{Nothing,Matrix{Float64}} = nothing,
                        q::Union{Nothing,Array{Float64,3}} = nothing, r::Union{Nothing,Array{Float64,3}} = nothing, ρ::Real = 0.0,
                        laps::Integer = 1, keep::Union{Nothing,Integer} = nothing)
    tape.handle != C_NULL || error("plant_tape_lqr: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m = tape.B, tape.T, 2 * nq, nu
    n_keep = keep === nothing ? T : Int(keep)
    (size(Q) == (n, n) || size(Q) == (n, n, T)) || error("plant_tape_lqr: Q must be $n x $n or $n x $n x $T")
    (size(R) == (m, m) || size(R) == (m, m, T)) || error("plant_tape_lqr: R must be $m x $m or $m x $m x $T")
    n_Q = ndims(Q) == 2 ? 1 : T; n_R = ndims(R) == 2 ? 1 : T
    Qend = Qf === nothing ? (ndims(Q) == 2 ? Q : Q[:, :, T]) : Qf
    size(Qend) == (n, n) || error("plant_tape_lqr: Qf must be $n x $n")
    (q === nothing) == (r === nothing) || error("plant_tape_lqr: q and r go together")
    (q === nothing || (size(q) == (n, B, T + 1) && size(r) == (m, B, T))) || error("plant_tape_lqr: q must be $n x $B x $(T + 1) and r $m x $B x $T")
    lin = q !== nothing
    K = zeros(m, n, B, n_keep); P0 = zeros(n, n, B); status = zeros(Cint, B); n_cut = zeros(Cint, B)
    k = lin ? zeros(m, B, n_keep) : nothing; p0 = lin ? zeros(n, B) : nothing; dV = lin ? zeros(2, B) : nothing
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve Qend q r k p0 dV begin
        pQf, pq, pr, pk, pp, pV = p(Qend), p(q), p(r), p(k), p(p0), p(dV)
        check(@ccall LIB.cimpc_plant_tape_lqr(tape.handle::Ptr{Cvoid}, laps::Cint, n_Q::Cint, Q::Ptr{Cdouble}, pQf::Ptr{Cdouble}, n_R::Cint,
                                              R::Ptr{Cdouble}, pq::Ptr{Cdouble}, pr::Ptr{Cdouble}, ρ::Cdouble, n_keep::Cint, K::Ptr{Cdouble},
                                              pk::Ptr{Cdouble}, P0::Ptr{Cdouble}, pp::Ptr{Cdouble}, pV::Ptr{Cdouble}, status::Ptr{Cint},
                                              n_cut::Ptr{Cint})::Cint)
    end
    return K, k, P0, p0, dV, status, n_cut
end

"""
    plant_tape_lqr_box(tape, Q, R, q, r; Qf = nothing, ρ = 0.0, keep = nothing, u_lo = nothing, u_hi = nothing, u_nom = nothing)
        -> (K, k, P0, p0, dV, status, n_cut, clamped)

`cimpc_plant_tape_lqr_box`, the limited pass (DESIGN.md section 3, item 3g): `plant_tape_lqr` with linear terms, ρ a number or one per
robot (length B), and control limits u_lo <= u <= u_hi, each m x 1 (shared) or m x B, ±Inf meaning no limit, about the tape's applied
controls u_nom: m x B x T.  At every step the box-constrained QP min ½x'Gx + Qu'x, u_lo - u_nom <= x <= u_hi - u_nom is solved by projected
Newton; K's rows of the clamped controls are zero and k lies in the box.  clamped: B x keep, bit i-1 set where control i was clamped.
Without limits (all three nothing) the outputs are `plant_tape_lqr`'s bit for bit.  Unexecuted, like the rest of this binding.
"""
function plant_tape_lqr_box(tape::PlantTape, Q::Array{Float64}, R::Array{Float64}, q::Array{Float64,3}, r::Array{Float64,3};
                            Qf::Union{Nothing,Matrix{Float64}} = nothing, ρ::Union{Real,Vector{Float64}} = 0.0,
                            keep::Union{Nothing,Integer} = nothing, u_lo::Union{Nothing,Matrix{Float64}} = nothing,
                            u_hi::Union{Nothing,Matrix{Float64}} = nothing, u_nom::Union{Nothing,Array{Float64,3}} = nothing)
    tape.handle != C_NULL || error("plant_tape_lqr_box: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m = tape.B, tape.T, 2 * nq, nu
    n_keep = keep === nothing ? T : Int(keep)
    (size(Q) == (n, n) || size(Q) == (n, n, T)) || error("plant_tape_lqr_box: Q must be $n x $n or $n x $n x $T")
    (size(R) == (m, m) || size(R) == (m, m, T)) || error("plant_tape_lqr_box: R must be $m x $m or $m x $m x $T")
    n_Q = ndims(Q) == 2 ? 1 : T; n_R = ndims(R) == 2 ? 1 : T
    Qend = Qf === nothing ? (ndims(Q) == 2 ? Q : Q[:, :, T]) : Qf
    size(Qend) == (n, n) || error("plant_tape_lqr_box: Qf must be $n x $n")
    (size(q) == (n, B, T + 1) && size(r) == (m, B, T)) || error("plant_tape_lqr_box: q must be $n x $B x $(T + 1) and r $m x $B x $T")
    rho = ρ isa Real ? [Float64(ρ)] : ρ
    (length(rho) == 1 || length(rho) == B) || error("plant_tape_lqr_box: ρ must be a number or one per robot ($B)")
    limited = u_lo !== nothing || u_hi !== nothing
    if limited
        (u_lo !== nothing && u_hi !== nothing && u_nom !== nothing) || error("plant_tape_lqr_box: u_lo, u_hi and u_nom go together")
        (size(u_lo) == size(u_hi) && size(u_lo, 1) == m && size(u_lo, 2) in (1, B)) || error("plant_tape_lqr_box: u_lo, u_hi must be $m x 1 or $m x $B")
        size(u_nom) == (m, B, T) || error("plant_tape_lqr_box: u_nom must be $m x $B x $T")
    end
    n_rho = length(rho); n_lim = limited ? size(u_lo, 2) : 1
    K = zeros(m, n, B, n_keep); P0 = zeros(n, n, B); status = zeros(Cint, B); n_cut = zeros(Cint, B)
    k = zeros(m, B, n_keep); p0 = zeros(n, B); dV = zeros(2, B); clamped = zeros(Cint, B, n_keep)
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve Qend u_lo u_hi u_nom begin
        pQf, plo, phi, pun = p(Qend), p(u_lo), p(u_hi), p(u_nom)
        check(@ccall LIB.cimpc_plant_tape_lqr_box(tape.handle::Ptr{Cvoid}, 1::Cint, n_Q::Cint, Q::Ptr{Cdouble}, pQf::Ptr{Cdouble}, n_R::Cint,
                                                  R::Ptr{Cdouble}, q::Ptr{Cdouble}, r::Ptr{Cdouble}, n_rho::Cint, rho::Ptr{Cdouble},
                                                  n_keep::Cint, K::Ptr{Cdouble}, k::Ptr{Cdouble}, P0::Ptr{Cdouble}, p0::Ptr{Cdouble},
                                                  dV::Ptr{Cdouble}, status::Ptr{Cint}, n_cut::Ptr{Cint}, n_lim::Cint, plo::Ptr{Cdouble},
                                                  phi::Ptr{Cdouble}, pun::Ptr{Cdouble}, clamped::Ptr{Cint})::Cint)
    end
    return K, k, P0, p0, dV, status, n_cut, clamped
end

# ---- iLQR through contact: the tracking cost and the parallel line search (cimpc.h: cimpc_tracking_cost; DESIGN.md section 3, item 3f) ---
# Unexecuted, like the rest of this binding (INTEGRATION.md).
"""
`cimpc_tracking_cost`: the pointers and sizes of a tracking cost as the library reads them.  Built by `plant_tracking_cost` and
`plant_tape_linesearch` from a `TrackingCost`.
"""
struct TrackingCostC
    Q::Ptr{Cdouble}
    Qf::Ptr{Cdouble}
    R::Ptr{Cdouble}
    x_goal::Ptr{Cdouble}
    u_goal::Ptr{Cdouble}
    n_Q::Cint; n_R::Cint; n_x::Cint
end

"""
    TrackingCost(Q, R, Qf, x_goal, u_goal)

J = Σ_{t<T} ½ (x_t - x_goal_t)'Q_t (x_t - x_goal_t) + ½ (u_t - u_goal_t)'R_t (u_t - u_goal_t) + ½ (x_T - x_goal_T)'Qf (x_T - x_goal_T) with
x_t = [q[t]; q[t+1]] (n = 2nq), u_t (m = nu) the control step t applied.  Q: n x n or n x n x T, R: m x m or m x m x T, Qf: n x n, shared
by the robots; x_goal: n x n_x x (T + 1) and u_goal: m x n_x x T with n_x = 1 (shared) or B.
"""
struct TrackingCost
    Q::Array{Float64}
    R::Array{Float64}
    Qf::Matrix{Float64}
    x_goal::Array{Float64,3}
    u_goal::Array{Float64,3}
end

function _tracking_cost_sizes(what, c::TrackingCost, nq, nu, B, T)
    n, m = 2 * nq, nu
    (size(c.Q) == (n, n) || size(c.Q) == (n, n, T)) || error("$what: Q must be $n x $n or $n x $n x $T")
    (size(c.R) == (m, m) || size(c.R) == (m, m, T)) || error("$what: R must be $m x $m or $m x $m x $T")
    size(c.Qf) == (n, n) || error("$what: Qf must be $n x $n")
    n_x = size(c.x_goal, 2)
    (n_x in (1, B) && size(c.x_goal) == (n, n_x, T + 1) && size(c.u_goal) == (m, n_x, T)) || error("$what: x_goal must be $n x n_x x $(T + 1) and u_goal $m x n_x x $T, n_x 1 or $B")
    return ndims(c.Q) == 2 ? 1 : T, ndims(c.R) == 2 ? 1 : T, n_x
end

"""
    plant_tracking_cost(cost, q, u_applied) -> (J, lin_q, lin_r)

`cimpc_plant_tracking_cost` (host only): J (B), lin_q 2nq x B x (T + 1) and lin_r nu x B x T of trajectories q nq x B x (T + 2) with applied
controls u_applied nu x B x T, bit for bit what the line search computes on the device; lin_q, lin_r are the q, r of `plant_tape_lqr`.
"""
function plant_tracking_cost(cost::TrackingCost, q::Array{Float64,3}, u_applied::Array{Float64,3})
    nq, B = size(q, 1), size(q, 2)
    nu, T = size(u_applied, 1), size(u_applied, 3)
    (size(q, 3) == T + 2 && size(u_applied, 2) == B) || error("plant_tracking_cost: q must be nq x B x (T + 2) beside u_applied nu x B x T")
    n_Q, n_R, n_x = _tracking_cost_sizes("plant_tracking_cost", cost, nq, nu, B, T)
    J = zeros(B); lin_q = zeros(2 * nq, B, T + 1); lin_r = zeros(nu, B, T)
    GC.@preserve cost begin
        cc = Ref(TrackingCostC(pointer(cost.Q), pointer(cost.Qf), pointer(cost.R), pointer(cost.x_goal), pointer(cost.u_goal), n_Q, n_R, n_x))
        check(@ccall LIB.cimpc_plant_tracking_cost(nq::Cint, nu::Cint, B::Cint, T::Cint, cc::Ref{TrackingCostC}, q::Ptr{Cdouble},
                                                   u_applied::Ptr{Cdouble}, J::Ptr{Cdouble}, lin_q::Ptr{Cdouble}, lin_r::Ptr{Cdouble})::Cint)
    end
    return J, lin_q, lin_r
end

"""
    plant_tape_linesearch(tape, K, k, dV, q, u_applied, cost, J_nom, alphas, μ, h_sim, opts; armijo = 1e-4, w = nothing, w_hold = 1,
                          terrain = nothing, steps_per_launch = 0, grad_reg = nothing)
        -> (J, ok, choice, q, u_applied, γ, b, status, iters, lin_q, lin_r, tape)

`cimpc_plant_tape_linesearch`: the forward pass of an iLQR iteration about the trajectory q nq x B x (T + 2) the tape recorded, whose steps
applied u_applied nu x B x T.  K m x n x B x T, k m x B x T, dV 2 x B are `plant_tape_lqr`'s with q, r and keep = T, J_nom (B) the cost of the
nominal.  Candidate c of robot b applies (u_applied[:, b, t] + alphas[c] k[:, b, t]) + K_t (x_ref_t - x_t) and all length(alphas) (1 .. 64)
candidates of all robots run in ONE closed-loop rollout; a candidate is acceptable iff its steps converged, its J is finite and
J <= J_nom + armijo (α dV1 + α² dV2), and a robot's choice is its acceptable candidate of least J (0-based; -1: none).  Returns J and ok
B x n_alpha, choice (B), the chosen candidates' rows (candidate 0's where choice = -1: the caller keeps the nominal's there) with the cost's
lin_q, lin_r on them, and the open-loop `PlantTape` of that trajectory, in which a robot without a choice has the parent's blocks.
"""
function plant_tape_linesearch(tape::PlantTape, K::Array{Float64,4}, k::Array{Float64,3}, dV::Matrix{Float64}, q::Array{Float64,3},
                               u_applied::Array{Float64,3}, cost::TrackingCost, J_nom::Vector{Float64}, alphas::Vector{Float64}, μ, h_sim, opts;
                               armijo::Real = 1e-4, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                               terrain::Union{Nothing,Vector{Terrain}} = nothing, steps_per_launch::Int = 0, grad_reg = nothing)
    tape.handle != C_NULL || error("plant_tape_linesearch: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m = tape.B, tape.T, 2 * nq, nu
    (size(K) == (m, n, B, T) && size(k) == (m, B, T) && size(dV) == (2, B)) || error("plant_tape_linesearch: K must be $m x $n x $B x $T, k $m x $B x $T, dV 2 x $B")
    (size(q) == (nq, B, T + 2) && size(u_applied) == (nu, B, T) && length(J_nom) == B) || error("plant_tape_linesearch: q, u_applied or J_nom do not fit the tape")
    n_alpha = length(alphas)
    (1 <= n_alpha <= 64 && all(isfinite, alphas) && armijo >= 0) || error("plant_tape_linesearch: 1 to 64 finite alphas, armijo >= 0")
    n_Q, n_R, n_x = _tracking_cost_sizes("plant_tape_linesearch", cost, nq, nu, B, T)
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    (ws === nothing || (ndims(ws) == 3 && size(ws, 1) == nw && size(ws, 2) in (1, B))) || error("plant_tape_linesearch: w must be $nw x K_w or $nw x B x K_w")
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_tape_linesearch: one friction coefficient or one per robot")
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    J = zeros(B, n_alpha); ok = zeros(Cint, B, n_alpha); choice = zeros(Cint, B)
    cq = zeros(nq, B, T + 2); cu = zeros(nu, B, T); γ = zeros(nc, B, T); b = zeros(nf * nc, B, T)
    status = zeros(Cint, B, T); iters = zeros(Cint, B, T); grad_status = zeros(Cint, B, T)
    lin_q = zeros(n, B, T + 1); lin_r = zeros(m, B, T)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve cost begin
        cc = Ref(TrackingCostC(pointer(cost.Q), pointer(cost.Qf), pointer(cost.R), pointer(cost.x_goal), pointer(cost.u_goal), n_Q, n_R, n_x))
        check(@ccall LIB.cimpc_plant_tape_linesearch(tape.handle::Ptr{Cvoid}, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                     q::Ptr{Cdouble}, u_applied::Ptr{Cdouble}, wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint,
                                                     μs::Ptr{Cdouble}, n_mu::Cint, h_sim::Cdouble, o::Ref{IpOpts}, K::Ptr{Cdouble}, k::Ptr{Cdouble},
                                                     dV::Ptr{Cdouble}, J_nom::Ptr{Cdouble}, n_alpha::Cint, alphas::Ptr{Cdouble}, armijo::Cdouble,
                                                     cc::Ref{TrackingCostC}, reg::Cdouble, J::Ptr{Cdouble}, ok::Ptr{Cint}, choice::Ptr{Cint},
                                                     cq::Ptr{Cdouble}, cu::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble}, status::Ptr{Cint},
                                                     iters::Ptr{Cint}, lin_q::Ptr{Cdouble}, lin_r::Ptr{Cdouble}, grad_status::Ptr{Cint},
                                                     handle::Ref{Ptr{Cvoid}})::Cint)
    end
    return J, ok, choice, cq, cu, γ, b, status, iters, lin_q, lin_r, PlantTape(handle[], tape.model, B, T, tape.n_cols, grad_status)
end

"""
    plant_tape_linesearch_box(tape, K, k, dV, q, u_applied, cost, J_nom, alphas, μ, h_sim, opts, u_lo, u_hi; ...)

`plant_tape_linesearch` under control limits (`cimpc_plant_tape_linesearch_box`; DESIGN.md section 3, item 3g): u_lo, u_hi nu x 1 (shared) or
nu x B.  A candidate's open-loop row is limit(u_applied + α k) and its steps apply the limited law; everything else, the returned values
included, is `plant_tape_linesearch`'s.  Unexecuted, like the rest of this binding.
"""
function plant_tape_linesearch_box(tape::PlantTape, K::Array{Float64,4}, k::Array{Float64,3}, dV::Matrix{Float64}, q::Array{Float64,3},
                               u_applied::Array{Float64,3}, cost::TrackingCost, J_nom::Vector{Float64}, alphas::Vector{Float64}, μ, h_sim, opts,
                               u_lo::Matrix{Float64}, u_hi::Matrix{Float64};
                               armijo::Real = 1e-4, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                               terrain::Union{Nothing,Vector{Terrain}} = nothing, steps_per_launch::Int = 0, grad_reg = nothing)
    tape.handle != C_NULL || error("plant_tape_linesearch_box: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m = tape.B, tape.T, 2 * nq, nu
    (size(K) == (m, n, B, T) && size(k) == (m, B, T) && size(dV) == (2, B)) || error("plant_tape_linesearch_box: K must be $m x $n x $B x $T, k $m x $B x $T, dV 2 x $B")
    (size(q) == (nq, B, T + 2) && size(u_applied) == (nu, B, T) && length(J_nom) == B) || error("plant_tape_linesearch_box: q, u_applied or J_nom do not fit the tape")
    (size(u_lo) == size(u_hi) && size(u_lo, 1) == nu && size(u_lo, 2) in (1, B)) || error("plant_tape_linesearch_box: u_lo, u_hi must be $nu x 1 or $nu x $B")
    n_lim = size(u_lo, 2)
    n_alpha = length(alphas)
    (1 <= n_alpha <= 64 && all(isfinite, alphas) && armijo >= 0) || error("plant_tape_linesearch_box: 1 to 64 finite alphas, armijo >= 0")
    n_Q, n_R, n_x = _tracking_cost_sizes("plant_tape_linesearch_box", cost, nq, nu, B, T)
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    (ws === nothing || (ndims(ws) == 3 && size(ws, 1) == nw && size(ws, 2) in (1, B))) || error("plant_tape_linesearch_box: w must be $nw x K_w or $nw x B x K_w")
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_tape_linesearch_box: one friction coefficient or one per robot")
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    J = zeros(B, n_alpha); ok = zeros(Cint, B, n_alpha); choice = zeros(Cint, B)
    cq = zeros(nq, B, T + 2); cu = zeros(nu, B, T); γ = zeros(nc, B, T); b = zeros(nf * nc, B, T)
    status = zeros(Cint, B, T); iters = zeros(Cint, B, T); grad_status = zeros(Cint, B, T)
    lin_q = zeros(n, B, T + 1); lin_r = zeros(m, B, T)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve cost begin
        cc = Ref(TrackingCostC(pointer(cost.Q), pointer(cost.Qf), pointer(cost.R), pointer(cost.x_goal), pointer(cost.u_goal), n_Q, n_R, n_x))
        check(@ccall LIB.cimpc_plant_tape_linesearch_box(tape.handle::Ptr{Cvoid}, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                     q::Ptr{Cdouble}, u_applied::Ptr{Cdouble}, wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint,
                                                     μs::Ptr{Cdouble}, n_mu::Cint, h_sim::Cdouble, o::Ref{IpOpts}, K::Ptr{Cdouble}, k::Ptr{Cdouble},
                                                     dV::Ptr{Cdouble}, J_nom::Ptr{Cdouble}, n_alpha::Cint, alphas::Ptr{Cdouble}, armijo::Cdouble,
                                                     cc::Ref{TrackingCostC}, reg::Cdouble, J::Ptr{Cdouble}, ok::Ptr{Cint}, choice::Ptr{Cint},
                                                     cq::Ptr{Cdouble}, cu::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble}, status::Ptr{Cint},
                                                     iters::Ptr{Cint}, lin_q::Ptr{Cdouble}, lin_r::Ptr{Cdouble}, grad_status::Ptr{Cint},
                                                     handle::Ref{Ptr{Cvoid}}, n_lim::Cint, u_lo::Ptr{Cdouble}, u_hi::Ptr{Cdouble})::Cint)
    end
    return J, ok, choice, cq, cu, γ, b, status, iters, lin_q, lin_r, PlantTape(handle[], tape.model, B, T, tape.n_cols, grad_status)
end

"""
    plant_ilqr(tape, q, u_applied, γ, b, status, iters, cost, μ, h_sim, opts; alphas = [1.0, 0.5, 0.25, 0.125], max_iter = 10, rho0 = 1e-6,
               rho_factor = 10.0, rho_max = 1e6, tol = 1e-6, armijo = 1e-4, u_lo = nothing, u_hi = nothing, w = nothing, w_hold = 1,
               terrain = nothing, steps_per_launch = 0, grad_reg = nothing)
        -> (q, u_applied, γ, b, status, iters, lin_q, lin_r, J, alpha, rho, accepted, J0, K, k, dV, lq_status, n_cut, clamped, tape)

`cimpc_plant_ilqr`, the device-resident iLQR loop (DESIGN.md section 3, item 3h): from the nominal the open-loop `tape` recorded (q
nq x B x (T + 2), u_applied nu x B x T, γ, b, status, iters as `plant_rollout_tape` returned them), up to max_iter iterations of the limited
backward pass with a rho per robot, the line search over alphas and the loop's bookkeeping (csrc/plant_ilqr.h), all on the device; the host
reads one Cint per iteration.  The ladder rho0 rho_factor^j, j = 0 .. max_iter, is computed here.  u_lo, u_hi: nu x 1 or nu x B limits, or
nothing.  The tape is read, not consumed.  Returns the final nominal's rows with the cost's lin_q, lin_r, the history J, alpha (NaN where
rejected), rho, accepted (B x n_iter each), the first nominal's cost J0, the last iteration's gains K m x n x B x T, k, dV, lq_status, n_cut,
clamped (B x T), and the final nominal's `PlantTape`.  Unexecuted, like the rest of this binding: written against include/cimpc.h and
checked against its prototype by text only.
"""
function plant_ilqr(tape::PlantTape, q::Array{Float64,3}, u_applied::Array{Float64,3}, γ::Array{Float64,3}, b::Array{Float64,3},
                    status::Matrix{Cint}, iters::Matrix{Cint}, cost::TrackingCost, μ, h_sim, opts;
                    alphas::Vector{Float64} = [1.0, 0.5, 0.25, 0.125], max_iter::Int = 10, rho0::Real = 1e-6, rho_factor::Real = 10.0,
                    rho_max::Real = 1e6, tol::Real = 1e-6, armijo::Real = 1e-4, u_lo::Union{Nothing,Matrix{Float64}} = nothing,
                    u_hi::Union{Nothing,Matrix{Float64}} = nothing, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                    terrain::Union{Nothing,Vector{Terrain}} = nothing, steps_per_launch::Int = 0, grad_reg = nothing)
    tape.handle != C_NULL || error("plant_ilqr: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m = tape.B, tape.T, 2 * nq, nu
    (size(q) == (nq, B, T + 2) && size(u_applied) == (nu, B, T) && size(γ) == (nc, B, T) && size(b) == (nf * nc, B, T) && size(status) == (B, T) &&
     size(iters) == (B, T)) || error("plant_ilqr: the nominal's rows do not fit the tape")
    max_iter >= 1 || error("plant_ilqr: max_iter must be at least 1")
    n_alpha = length(alphas)
    (1 <= n_alpha <= 64 && all(isfinite, alphas) && armijo >= 0) || error("plant_ilqr: 1 to 64 finite alphas, armijo >= 0")
    ladder = [Float64(rho0) * Float64(rho_factor)^j for j in 0:max_iter]
    (all(isfinite, ladder) && all(>=(0), ladder)) || error("plant_ilqr: rho0 rho_factor^j must be finite and not negative")
    n_ladder = length(ladder)
    (u_lo === nothing) == (u_hi === nothing) || error("plant_ilqr: u_lo and u_hi go together")
    limited = u_lo !== nothing
    (!limited || (size(u_lo) == size(u_hi) && size(u_lo, 1) == nu && size(u_lo, 2) in (1, B))) || error("plant_ilqr: u_lo, u_hi must be $nu x 1 or $nu x $B")
    n_lim = limited ? size(u_lo, 2) : 1
    lo, hi = limited ? (u_lo, u_hi) : (C_NULL, C_NULL)
    n_Q, n_R, n_x = _tracking_cost_sizes("plant_ilqr", cost, nq, nu, B, T)
    J0, lin_q0, lin_r0 = plant_tracking_cost(cost, q, u_applied)
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    (ws === nothing || (ndims(ws) == 3 && size(ws, 1) == nw && size(ws, 2) in (1, B))) || error("plant_ilqr: w must be $nw x K_w or $nw x B x K_w")
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_ilqr: one friction coefficient or one per robot")
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    oq = zeros(nq, B, T + 2); ou = zeros(nu, B, T); og = zeros(nc, B, T); ob = zeros(nf * nc, B, T)
    ost = zeros(Cint, B, T); oit = zeros(Cint, B, T); grad_status = zeros(Cint, B, T)
    lin_q = zeros(n, B, T + 1); lin_r = zeros(m, B, T)
    hJ = zeros(B, max_iter); hal = zeros(B, max_iter); hrho = zeros(B, max_iter); hacc = zeros(Cint, B, max_iter)
    n_iter = Ref{Cint}(0)
    K = zeros(m, n, B, T); k = zeros(m, B, T); dV = zeros(2, B)
    lq_status = zeros(Cint, B); n_cut = zeros(Cint, B); clamped = zeros(Cint, B, T)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve cost begin
        cc = Ref(TrackingCostC(pointer(cost.Q), pointer(cost.Qf), pointer(cost.R), pointer(cost.x_goal), pointer(cost.u_goal), n_Q, n_R, n_x))
        check(@ccall LIB.cimpc_plant_ilqr(tape.handle::Ptr{Cvoid}, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                          q::Ptr{Cdouble}, u_applied::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble}, status::Ptr{Cint},
                                          iters::Ptr{Cint}, J0::Ptr{Cdouble}, lin_q0::Ptr{Cdouble}, lin_r0::Ptr{Cdouble},
                                          wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint, μs::Ptr{Cdouble}, n_mu::Cint, h_sim::Cdouble,
                                          o::Ref{IpOpts}, cc::Ref{TrackingCostC}, n_alpha::Cint, alphas::Ptr{Cdouble}, armijo::Cdouble,
                                          reg::Cdouble, n_ladder::Cint, ladder::Ptr{Cdouble}, rho_max::Cdouble, tol::Cdouble, max_iter::Cint,
                                          n_lim::Cint, lo::Ptr{Cdouble}, hi::Ptr{Cdouble},
                                          oq::Ptr{Cdouble}, ou::Ptr{Cdouble}, og::Ptr{Cdouble}, ob::Ptr{Cdouble}, ost::Ptr{Cint}, oit::Ptr{Cint},
                                          lin_q::Ptr{Cdouble}, lin_r::Ptr{Cdouble}, grad_status::Ptr{Cint}, hJ::Ptr{Cdouble}, hal::Ptr{Cdouble},
                                          hrho::Ptr{Cdouble}, hacc::Ptr{Cint}, n_iter::Ref{Cint}, K::Ptr{Cdouble}, k::Ptr{Cdouble},
                                          dV::Ptr{Cdouble}, lq_status::Ptr{Cint}, n_cut::Ptr{Cint}, clamped::Ptr{Cint},
                                          handle::Ref{Ptr{Cvoid}})::Cint)
    end
    it = 1:Int(n_iter[])
    return oq, ou, og, ob, ost, oit, lin_q, lin_r, hJ[:, it], hal[:, it], hrho[:, it], hacc[:, it] .!= 0, J0, K, k, dV, lq_status, n_cut, clamped,
           PlantTape(handle[], tape.model, B, T, tape.n_cols, grad_status)
end

# ---- the receding-horizon iLQR policy (DESIGN.md section 3, item 3j): a handle with the problem and the plan on the device -------------
"""
    PlantMpc

The handle of `cimpc_plant_mpc` with the sizes it was created with.  Unexecuted, like the rest of this binding.
"""
mutable struct PlantMpc
    handle::Ptr{Cvoid}
    model::Symbol
    B::Int
    H::Int
    L::Int
    n_iter::Int
end

"""
    plant_mpc_create(model, B, H, μ, h_sim, opts, Q, Qf, R, x_ref, u_ref, u0; n_iter = 1, alphas = [1.0, 0.5, 0.25, 0.125], rho0 = 1e-6,
                     rho_factor = 10.0, rho_max = 1e6, tol = 1e-6, armijo = 1e-4, u_lo = nothing, u_hi = nothing, terrain = nothing,
                     steps_per_launch = 0, grad_reg = nothing, grad_cols = nothing) -> PlantMpc

`cimpc_plant_mpc_create`: the problem of a receding-horizon iLQR policy goes up once.  Q n x n x n_Q, Qf n x n, R m x m x n_R (column-major
blocks, n = 2nq, m = nu, n_Q and n_R 1 or H); x_ref n x n_x x (L + 1) and u_ref m x n_x x L with n_x 1 or B; u0 m x B x H, the first plan,
inside the limits u_lo, u_hi (nu x 1 or nu x B) where there are any.  The ladder rho0 rho_factor^j, j = 0 .. n_iter, is computed here.
Unexecuted, like the rest of this binding: written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_mpc_create(model::Symbol, B::Int, H::Int, μ, h_sim, opts, Q::Array{Float64,3}, Qf::Matrix{Float64}, R::Array{Float64,3},
                          x_ref::Array{Float64,3}, u_ref::Array{Float64,3}, u0::Array{Float64,3}; n_iter::Int = 1,
                          alphas::Vector{Float64} = [1.0, 0.5, 0.25, 0.125], rho0::Real = 1e-6, rho_factor::Real = 10.0, rho_max::Real = 1e6,
                          tol::Real = 1e-6, armijo::Real = 1e-4, u_lo::Union{Nothing,Matrix{Float64}} = nothing,
                          u_hi::Union{Nothing,Matrix{Float64}} = nothing, terrain::Union{Nothing,Vector{Terrain}} = nothing,
                          steps_per_launch::Int = 0, grad_reg = nothing, grad_cols = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    n, m = 2 * nq, nu
    (B >= 1 && H >= 1 && n_iter >= 1) || error("plant_mpc_create: B, H and n_iter must be at least 1")
    n_Q, n_R, n_x, L = size(Q, 3), size(R, 3), size(x_ref, 2), size(u_ref, 3)
    (size(Q) == (n, n, n_Q) && n_Q in (1, H) && size(R) == (m, m, n_R) && n_R in (1, H) && size(Qf) == (n, n)) || error("plant_mpc_create: the weights do not fit the model")
    (L >= 1 && n_x in (1, B) && size(x_ref) == (n, n_x, L + 1) && size(u_ref) == (m, n_x, L)) || error("plant_mpc_create: x_ref must be $n x n_x x (L + 1) and u_ref $m x n_x x L")
    size(u0) == (m, B, H) || error("plant_mpc_create: u0 must be $m x $B x $H")
    n_alpha = length(alphas)
    (1 <= n_alpha <= 64 && all(isfinite, alphas) && armijo >= 0) || error("plant_mpc_create: 1 to 64 finite alphas, armijo >= 0")
    ladder = [Float64(rho0) * Float64(rho_factor)^j for j in 0:n_iter]
    (all(isfinite, ladder) && all(>=(0), ladder)) || error("plant_mpc_create: rho0 rho_factor^j must be finite and not negative")
    n_ladder = length(ladder)
    (u_lo === nothing) == (u_hi === nothing) || error("plant_mpc_create: u_lo and u_hi go together")
    limited = u_lo !== nothing
    (!limited || (size(u_lo) == size(u_hi) && size(u_lo, 1) == nu && size(u_lo, 2) in (1, B))) || error("plant_mpc_create: u_lo, u_hi must be $nu x 1 or $nu x $B")
    n_lim = limited ? size(u_lo, 2) : 1
    lo, hi = limited ? (u_lo, u_hi) : (C_NULL, C_NULL)
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_mpc_create: one friction coefficient or one per robot")
    n_mu = length(μs)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_cols = grad_cols === nothing ? 2 * nq + nu : Int(grad_cols)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    check(@ccall LIB.cimpc_plant_mpc_create(id::Cint, B::Cint, H::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                            μs::Ptr{Cdouble}, n_mu::Cint, h_sim::Cdouble, o::Ref{IpOpts}, Q::Ptr{Cdouble}, Qf::Ptr{Cdouble},
                                            R::Ptr{Cdouble}, n_Q::Cint, n_R::Cint, L::Cint, n_x::Cint, x_ref::Ptr{Cdouble}, u_ref::Ptr{Cdouble},
                                            n_alpha::Cint, alphas::Ptr{Cdouble}, armijo::Cdouble, reg::Cdouble, n_cols::Cint, n_ladder::Cint,
                                            ladder::Ptr{Cdouble}, rho_max::Cdouble, tol::Cdouble, n_iter::Cint, n_lim::Cint, lo::Ptr{Cdouble},
                                            hi::Ptr{Cdouble}, u0::Ptr{Cdouble}, handle::Ref{Ptr{Cvoid}})::Cint)
    return PlantMpc(handle[], model, B, H, L, n_iter)
end

"""
    plant_mpc_control(p, s, shift, q0, q1) -> (u, J0, J, alpha, rho, accepted, converged)

`cimpc_plant_mpc_control`: one control step of the policy from the measured q0, q1 (nq x B): the plan advanced by `shift`, the goal window
of step `s`, up to n_iter iterations on the device.  u nu x B is the control to apply; J, alpha, rho, accepted are B x n_done.  Unexecuted,
like the rest of this binding: written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_mpc_control(p::PlantMpc, s::Int, shift::Int, q0::Matrix{Float64}, q1::Matrix{Float64})
    p.handle != C_NULL || error("plant_mpc_control: the policy is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(p.model)
    (size(q0) == (nq, p.B) && size(q1) == (nq, p.B)) || error("plant_mpc_control: q0 and q1 must be $nq x $(p.B)")
    (s >= 0 && shift >= 0) || error("plant_mpc_control: s and shift must not be negative")
    B, n_iter = p.B, p.n_iter
    u = zeros(nu, B); J0 = zeros(B); converged = zeros(Cint, B)
    hJ = zeros(B, n_iter); hal = zeros(B, n_iter); hrho = zeros(B, n_iter); hacc = zeros(Cint, B, n_iter)
    n_done = Ref{Cint}(0)
    check(@ccall LIB.cimpc_plant_mpc_control(p.handle::Ptr{Cvoid}, s::Cint, shift::Cint, q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, u::Ptr{Cdouble},
                                             J0::Ptr{Cdouble}, hJ::Ptr{Cdouble}, hal::Ptr{Cdouble}, hrho::Ptr{Cdouble}, hacc::Ptr{Cint},
                                             n_done::Ref{Cint}, converged::Ptr{Cint})::Cint)
    it = 1:Int(n_done[])
    return u, J0, hJ[:, it], hal[:, it], hrho[:, it], hacc[:, it] .!= 0, converged .!= 0
end

"""
    plant_mpc_plan(p) -> (u, q, γ, b, status, iters)

`cimpc_plant_mpc_plan`: the current plan u nu x B x H and its nominal q nq x B x (H + 2), γ, b, status, iters.  Unexecuted, like the rest of
this binding: written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_mpc_plan(p::PlantMpc)
    p.handle != C_NULL || error("plant_mpc_plan: the policy is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(p.model)
    B, H = p.B, p.H
    u = zeros(nu, B, H); q = zeros(nq, B, H + 2); γ = zeros(nc, B, H); b = zeros(nf * nc, B, H)
    status = zeros(Cint, B, H); iters = zeros(Cint, B, H)
    check(@ccall LIB.cimpc_plant_mpc_plan(p.handle::Ptr{Cvoid}, u::Ptr{Cdouble}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                          status::Ptr{Cint}, iters::Ptr{Cint})::Cint)
    return u, q, γ, b, status, iters
end

"""
    plant_mpc_reset(p, u0)

`cimpc_plant_mpc_reset`: loads a new plan u0 (nu x B x H).  Unexecuted, like the rest of this binding: written against include/cimpc.h and
checked against its prototype by text only.
"""
function plant_mpc_reset(p::PlantMpc, u0::Array{Float64,3})
    p.handle != C_NULL || error("plant_mpc_reset: the policy is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(p.model)
    size(u0) == (nu, p.B, p.H) || error("plant_mpc_reset: u0 must be $nu x $(p.B) x $(p.H)")
    check(@ccall LIB.cimpc_plant_mpc_reset(p.handle::Ptr{Cvoid}, u0::Ptr{Cdouble})::Cint)
    return p
end

"""
    plant_mpc_dims(p) -> (model id, B, H, L, n_iter)

`cimpc_plant_mpc_dims`, as the library holds them.  Unexecuted, like the rest of this binding: written against include/cimpc.h and checked
against its prototype by text only.
"""
function plant_mpc_dims(p::PlantMpc)
    p.handle != C_NULL || error("plant_mpc_dims: the policy is closed")
    model = Ref{Cint}(0); B = Ref{Cint}(0); H = Ref{Cint}(0); L = Ref{Cint}(0); n_iter = Ref{Cint}(0)
    check(@ccall LIB.cimpc_plant_mpc_dims(p.handle::Ptr{Cvoid}, model::Ref{Cint}, B::Ref{Cint}, H::Ref{Cint}, L::Ref{Cint}, n_iter::Ref{Cint})::Cint)
    return Int(model[]), Int(B[]), Int(H[]), Int(L[]), Int(n_iter[])
end

"""
    plant_mpc_destroy(p)

`cimpc_plant_mpc_destroy`: frees the policy's device memory; a second call does nothing.  Unexecuted, like the rest of this binding: written
against include/cimpc.h and checked against its prototype by text only.
"""
function plant_mpc_destroy(p::PlantMpc)
    p.handle == C_NULL && return nothing
    h, p.handle = p.handle, C_NULL
    check(@ccall LIB.cimpc_plant_mpc_destroy(h::Ptr{Cvoid})::Cint)
    return nothing
end

# ---- the sampling policy (DESIGN.md section 3, item 3k): predictive sampling and the MPPI mean on a handle ---------------------------------
"""
    PlantSampler

The handle of `cimpc_plant_sampler` with the sizes it was created with.  Unexecuted, like the rest of this binding.
"""
mutable struct PlantSampler
    handle::Ptr{Cvoid}
    model::Symbol
    B::Int
    H::Int
    L::Int
    N::Int
    n_iter::Int
end

"""
    plant_sampler_create(model, B, H, μ, h_sim, opts, Q, Qf, R, x_ref, u_ref, u0, sigma; n_samples = 16, noise_hold = 1, lam = 0.0,
                         n_iter = 1, seed = 0, u_lo = nothing, u_hi = nothing, terrain = nothing, steps_per_launch = 0) -> PlantSampler

`cimpc_plant_sampler_create`: the problem of a sampling policy goes up once.  The weights, the reference, u0 and the limits as
`plant_mpc_create` takes them; sigma: nu standard deviations, finite and not negative; lam = 0 is predictive sampling, lam > 0 the MPPI
mean.  The noise is a centred Irwin-Hall deviate of order 8, not a Gaussian.  Unexecuted, like the rest of this binding: written against
include/cimpc.h and checked against its prototype by text only.
"""
function plant_sampler_create(model::Symbol, B::Int, H::Int, μ, h_sim, opts, Q::Array{Float64,3}, Qf::Matrix{Float64}, R::Array{Float64,3},
                              x_ref::Array{Float64,3}, u_ref::Array{Float64,3}, u0::Array{Float64,3}, sigma::Vector{Float64};
                              n_samples::Int = 16, noise_hold::Int = 1, lam::Real = 0.0, n_iter::Int = 1, seed::Integer = 0,
                              u_lo::Union{Nothing,Matrix{Float64}} = nothing, u_hi::Union{Nothing,Matrix{Float64}} = nothing,
                              terrain::Union{Nothing,Vector{Terrain}} = nothing, steps_per_launch::Int = 0)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    n, m = 2 * nq, nu
    (B >= 1 && H >= 1 && n_iter >= 1 && n_samples >= 1 && noise_hold >= 1) || error("plant_sampler_create: B, H, n_iter, n_samples and noise_hold must be at least 1")
    n_Q, n_R, n_x, L = size(Q, 3), size(R, 3), size(x_ref, 2), size(u_ref, 3)
    (size(Q) == (n, n, n_Q) && n_Q in (1, H) && size(R) == (m, m, n_R) && n_R in (1, H) && size(Qf) == (n, n)) || error("plant_sampler_create: the weights do not fit the model")
    (L >= 1 && n_x in (1, B) && size(x_ref) == (n, n_x, L + 1) && size(u_ref) == (m, n_x, L)) || error("plant_sampler_create: x_ref must be $n x n_x x (L + 1) and u_ref $m x n_x x L")
    size(u0) == (m, B, H) || error("plant_sampler_create: u0 must be $m x $B x $H")
    (length(sigma) == nu && all(isfinite, sigma) && all(>=(0), sigma)) || error("plant_sampler_create: sigma must be $nu finite entries that are not negative")
    lam >= 0 || error("plant_sampler_create: lam must not be negative")
    (u_lo === nothing) == (u_hi === nothing) || error("plant_sampler_create: u_lo and u_hi go together")
    limited = u_lo !== nothing
    (!limited || (size(u_lo) == size(u_hi) && size(u_lo, 1) == nu && size(u_lo, 2) in (1, B))) || error("plant_sampler_create: u_lo, u_hi must be $nu x 1 or $nu x $B")
    n_lim = limited ? size(u_lo, 2) : 1
    lo, hi = limited ? (u_lo, u_hi) : (C_NULL, C_NULL)
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_sampler_create: one friction coefficient or one per robot")
    n_mu = length(μs)
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    sd = UInt64(seed)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    check(@ccall LIB.cimpc_plant_sampler_create(id::Cint, B::Cint, H::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                μs::Ptr{Cdouble}, n_mu::Cint, h_sim::Cdouble, o::Ref{IpOpts}, Q::Ptr{Cdouble}, Qf::Ptr{Cdouble},
                                                R::Ptr{Cdouble}, n_Q::Cint, n_R::Cint, L::Cint, n_x::Cint, x_ref::Ptr{Cdouble}, u_ref::Ptr{Cdouble},
                                                n_samples::Cint, sigma::Ptr{Cdouble}, noise_hold::Cint, lam::Cdouble, n_iter::Cint, sd::Culonglong,
                                                n_lim::Cint, lo::Ptr{Cdouble}, hi::Ptr{Cdouble}, u0::Ptr{Cdouble}, handle::Ref{Ptr{Cvoid}})::Cint)
    return PlantSampler(handle[], model, B, H, L, n_samples, n_iter)
end

"""
    plant_sampler_control(p, s, shift, q0, q1) -> (u, J0, J_nom, J_best, choice, n_eligible, J, weights, converged)

`cimpc_plant_sampler_control`: one control step of the policy from the measured q0, q1 (nq x B).  u nu x B is the control to apply; J_nom,
J_best, choice (-1: the plan was kept), n_eligible are B x n_iter; J and the normalised weights B x N x n_iter.  Unexecuted, like the rest
of this binding: written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_sampler_control(p::PlantSampler, s::Int, shift::Int, q0::Matrix{Float64}, q1::Matrix{Float64})
    p.handle != C_NULL || error("plant_sampler_control: the policy is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(p.model)
    (size(q0) == (nq, p.B) && size(q1) == (nq, p.B)) || error("plant_sampler_control: q0 and q1 must be $nq x $(p.B)")
    (s >= 0 && shift >= 0) || error("plant_sampler_control: s and shift must not be negative")
    B, N, n_iter = p.B, p.N, p.n_iter
    u = zeros(nu, B); J0 = zeros(B); converged = zeros(Cint, B)
    hJn = zeros(B, n_iter); hJb = zeros(B, n_iter); hch = zeros(Cint, B, n_iter); hne = zeros(Cint, B, n_iter)
    J = zeros(B, N, n_iter); weights = zeros(B, N, n_iter)
    check(@ccall LIB.cimpc_plant_sampler_control(p.handle::Ptr{Cvoid}, s::Cint, shift::Cint, q0::Ptr{Cdouble}, q1::Ptr{Cdouble}, u::Ptr{Cdouble},
                                                 J0::Ptr{Cdouble}, hJn::Ptr{Cdouble}, hJb::Ptr{Cdouble}, hch::Ptr{Cint}, hne::Ptr{Cint},
                                                 J::Ptr{Cdouble}, weights::Ptr{Cdouble}, converged::Ptr{Cint})::Cint)
    return u, J0, hJn, hJb, Int.(hch), Int.(hne), J, weights, converged .!= 0
end

"""
    plant_sampler_plan(p) -> (u, q, γ, b, status, iters)

`cimpc_plant_sampler_plan`: the current plan u nu x B x H and its trajectory q nq x B x (H + 2), γ, b, status, iters; with lam > 0 the first
call after a control step rolls the mean out.  Unexecuted, like the rest of this binding: written against include/cimpc.h and checked
against its prototype by text only.
"""
function plant_sampler_plan(p::PlantSampler)
    p.handle != C_NULL || error("plant_sampler_plan: the policy is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(p.model)
    B, H = p.B, p.H
    u = zeros(nu, B, H); q = zeros(nq, B, H + 2); γ = zeros(nc, B, H); b = zeros(nf * nc, B, H)
    status = zeros(Cint, B, H); iters = zeros(Cint, B, H)
    check(@ccall LIB.cimpc_plant_sampler_plan(p.handle::Ptr{Cvoid}, u::Ptr{Cdouble}, q::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                              status::Ptr{Cint}, iters::Ptr{Cint})::Cint)
    return u, q, γ, b, status, iters
end

"""
    plant_sampler_raw_weights(p) -> w

`cimpc_plant_sampler_raw_weights`: the unnormalised weights B x N x n_iter of the last control step.  Unexecuted, like the rest of this
binding: written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_sampler_raw_weights(p::PlantSampler)
    p.handle != C_NULL || error("plant_sampler_raw_weights: the policy is closed")
    w = zeros(p.B, p.N, p.n_iter)
    check(@ccall LIB.cimpc_plant_sampler_raw_weights(p.handle::Ptr{Cvoid}, w::Ptr{Cdouble})::Cint)
    return w
end

"""
    plant_sampler_reset(p, u0)

`cimpc_plant_sampler_reset`: loads a new plan u0 (nu x B x H).  Unexecuted, like the rest of this binding: written against include/cimpc.h
and checked against its prototype by text only.
"""
function plant_sampler_reset(p::PlantSampler, u0::Array{Float64,3})
    p.handle != C_NULL || error("plant_sampler_reset: the policy is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(p.model)
    size(u0) == (nu, p.B, p.H) || error("plant_sampler_reset: u0 must be $nu x $(p.B) x $(p.H)")
    check(@ccall LIB.cimpc_plant_sampler_reset(p.handle::Ptr{Cvoid}, u0::Ptr{Cdouble})::Cint)
    return p
end

"""
    plant_sampler_dims(p) -> (model id, B, H, L, N, n_iter, n_rollouts)

`cimpc_plant_sampler_dims`, as the library holds them; n_rollouts counts the rollouts `plant_sampler_plan` has run.  Unexecuted, like the
rest of this binding: written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_sampler_dims(p::PlantSampler)
    p.handle != C_NULL || error("plant_sampler_dims: the policy is closed")
    model = Ref{Cint}(0); B = Ref{Cint}(0); H = Ref{Cint}(0); L = Ref{Cint}(0); N = Ref{Cint}(0); n_iter = Ref{Cint}(0); n_rollouts = Ref{Cint}(0)
    check(@ccall LIB.cimpc_plant_sampler_dims(p.handle::Ptr{Cvoid}, model::Ref{Cint}, B::Ref{Cint}, H::Ref{Cint}, L::Ref{Cint}, N::Ref{Cint},
                                              n_iter::Ref{Cint}, n_rollouts::Ref{Cint})::Cint)
    return Int(model[]), Int(B[]), Int(H[]), Int(L[]), Int(N[]), Int(n_iter[]), Int(n_rollouts[])
end

"""
    plant_sampler_destroy(p)

`cimpc_plant_sampler_destroy`: frees the policy's device memory; a second call does nothing.  Unexecuted, like the rest of this binding:
written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_sampler_destroy(p::PlantSampler)
    p.handle == C_NULL && return nothing
    h, p.handle = p.handle, C_NULL
    check(@ccall LIB.cimpc_plant_sampler_destroy(h::Ptr{Cvoid})::Cint)
    return nothing
end

"""
    plant_sample_noise(seed, draw, B, N, n_rows, nu) -> eps

`cimpc_plant_sample_noise`: the deviates of the sampling policy on the host, nu x B x N x n_rows, the device's bits; no device is needed.
Unexecuted, like the rest of this binding: written against include/cimpc.h and checked against its prototype by text only.
"""
function plant_sample_noise(seed::Integer, draw::Integer, B::Int, N::Int, n_rows::Int, nu::Int)
    (B >= 1 && N >= 1 && n_rows >= 1 && nu >= 1) || error("plant_sample_noise: B, N, n_rows and nu must be at least 1")
    eps = zeros(nu, B, N, n_rows)
    sd, dr = UInt64(seed), UInt32(draw)
    check(@ccall LIB.cimpc_plant_sample_noise(sd::Culonglong, dr::Cuint, B::Cint, N::Cint, n_rows::Cint, nu::Cint, eps::Ptr{Cdouble})::Cint)
    return eps
end

# ---- multiple shooting: the segments of a horizon rolled out abreast (DESIGN.md section 3, item 3l; csrc/plant_shooting.h) --------------
# Unexecuted, like the rest of this binding: written against include/cimpc.h and checked against its prototypes by text only.
"""
    plant_rollout_segments(model, nodes, u, μ, h_sim, opts; cost = nothing, w = nothing, w_hold = 1, terrain = nothing,
                           steps_per_launch = 0, grad_reg = nothing, grad_cols = nothing)
        -> (qs, γ, b, status, iters, defects, D, J, lin_q, lin_r, tape)

`cimpc_plant_rollout_segments`: nodes 2nq x B x M and u nu x B x T with T = M L.  Segment j of robot b is virtual robot j B + b of ONE
rollout of M B robots for L steps; qs is nq x (M B) x (L + 2), γ, b, status, iters are in (T, B) layout, defects 2nq x B x (M - 1), D (B).
With a `TrackingCost` J (B), lin_q 2nq x B x (T + 1) and lin_r nu x B x T are the cost on the segments' own rows, else `nothing`.  The
tape is an ordinary `PlantTape` of B robots and T steps.
"""
function plant_rollout_segments(model::Symbol, nodes::Array{Float64,3}, u::Array{Float64,3}, μ, h_sim, opts;
                                cost::Union{Nothing,TrackingCost} = nothing, w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1,
                                terrain::Union{Nothing,Vector{Terrain}} = nothing, steps_per_launch::Int = 0, grad_reg = nothing, grad_cols = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    n, B, M, T = 2 * nq, size(nodes, 2), size(nodes, 3), size(u, 3)
    (size(nodes, 1) == n && size(u, 1) == nu && size(u, 2) == B) || error("plant_rollout_segments: nodes must be $n x B x M and u $nu x B x T")
    (M >= 1 && T >= 1 && T % M == 0) || error("plant_rollout_segments: T must be a multiple of the number of segments")
    L = T ÷ M
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    (ws === nothing || (ndims(ws) == 3 && size(ws, 1) == nw && size(ws, 2) in (1, B))) || error("plant_rollout_segments: w must be $nw x K_w or $nw x B x K_w")
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_rollout_segments: one friction coefficient or one per robot")
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_cols = grad_cols === nothing ? n + nu : Int(grad_cols)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu = length(μs)
    qs = zeros(nq, M * B, L + 2); γ = zeros(nc, B, T); b = zeros(nf * nc, B, T)
    status = zeros(Cint, B, T); iters = zeros(Cint, B, T); grad_status = zeros(Cint, B, T)
    defects = zeros(n, B, M - 1); D = zeros(B)
    J = zeros(B); lin_q = zeros(n, B, T + 1); lin_r = zeros(nu, B, T)
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve cost begin
        cc = cost === nothing ? C_NULL : begin
            n_Q, n_R, n_x = _tracking_cost_sizes("plant_rollout_segments", cost, nq, nu, B, T)
            Ref(TrackingCostC(pointer(cost.Q), pointer(cost.Qf), pointer(cost.R), pointer(cost.x_goal), pointer(cost.u_goal), n_Q, n_R, n_x))
        end
        check(@ccall LIB.cimpc_plant_rollout_segments(id::Cint, B::Cint, T::Cint, M::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                      nodes::Ptr{Cdouble}, u::Ptr{Cdouble}, wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint,
                                                      μs::Ptr{Cdouble}, n_mu::Cint, h_sim::Cdouble, o::Ref{IpOpts}, cc::Ptr{TrackingCostC},
                                                      reg::Cdouble, n_cols::Cint, qs::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble},
                                                      status::Ptr{Cint}, iters::Ptr{Cint}, defects::Ptr{Cdouble}, D::Ptr{Cdouble}, J::Ptr{Cdouble},
                                                      lin_q::Ptr{Cdouble}, lin_r::Ptr{Cdouble}, grad_status::Ptr{Cint}, handle::Ref{Ptr{Cvoid}})::Cint)
    end
    cost === nothing && return qs, γ, b, status, iters, defects, D, nothing, nothing, nothing, PlantTape(handle[], model, B, T, n_cols, grad_status)
    return qs, γ, b, status, iters, defects, D, J, lin_q, lin_r, PlantTape(handle[], model, B, T, n_cols, grad_status)
end

"""
    plant_tape_lqr_shooting(tape, Q, R, q, r, defects, segment_len; Qf = nothing, ρ = 0.0, keep = nothing, u_lo = nothing, u_hi = nothing,
                            u_nom = nothing) -> (K, k, P0, p0, dV, status, n_cut, clamped)

`cimpc_plant_tape_lqr_shooting`: `plant_tape_lqr_box` on the tape of `plant_rollout_segments` with the defects 2nq x B x (T / segment_len - 1)
at the nodes t = j segment_len: the walk step of t = j segment_len - 1 starts from p + P d.  With all-zero defects K and k are
`plant_tape_lqr_box`'s.  Unexecuted, like the rest of this binding.
"""
function plant_tape_lqr_shooting(tape::PlantTape, Q::Array{Float64}, R::Array{Float64}, q::Array{Float64,3}, r::Array{Float64,3},
                                 defects::Array{Float64,3}, segment_len::Int; Qf::Union{Nothing,Matrix{Float64}} = nothing,
                                 ρ::Union{Real,Vector{Float64}} = 0.0, keep::Union{Nothing,Integer} = nothing,
                                 u_lo::Union{Nothing,Matrix{Float64}} = nothing, u_hi::Union{Nothing,Matrix{Float64}} = nothing,
                                 u_nom::Union{Nothing,Array{Float64,3}} = nothing)
    tape.handle != C_NULL || error("plant_tape_lqr_shooting: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m = tape.B, tape.T, 2 * nq, nu
    n_keep = keep === nothing ? T : Int(keep)
    (segment_len >= 1 && T % segment_len == 0) || error("plant_tape_lqr_shooting: T must be a multiple of segment_len")
    size(defects) == (n, B, T ÷ segment_len - 1) || error("plant_tape_lqr_shooting: defects must be $n x $B x $(T ÷ segment_len - 1)")
    (size(Q) == (n, n) || size(Q) == (n, n, T)) || error("plant_tape_lqr_shooting: Q must be $n x $n or $n x $n x $T")
    (size(R) == (m, m) || size(R) == (m, m, T)) || error("plant_tape_lqr_shooting: R must be $m x $m or $m x $m x $T")
    n_Q = ndims(Q) == 2 ? 1 : T; n_R = ndims(R) == 2 ? 1 : T
    Qend = Qf === nothing ? (ndims(Q) == 2 ? Q : Q[:, :, T]) : Qf
    size(Qend) == (n, n) || error("plant_tape_lqr_shooting: Qf must be $n x $n")
    (size(q) == (n, B, T + 1) && size(r) == (m, B, T)) || error("plant_tape_lqr_shooting: q must be $n x $B x $(T + 1) and r $m x $B x $T")
    rho = ρ isa Real ? [Float64(ρ)] : ρ
    (length(rho) == 1 || length(rho) == B) || error("plant_tape_lqr_shooting: ρ must be a number or one per robot ($B)")
    limited = u_lo !== nothing || u_hi !== nothing
    if limited
        (u_lo !== nothing && u_hi !== nothing && u_nom !== nothing) || error("plant_tape_lqr_shooting: u_lo, u_hi and u_nom go together")
        (size(u_lo) == size(u_hi) && size(u_lo, 1) == m && size(u_lo, 2) in (1, B)) || error("plant_tape_lqr_shooting: u_lo, u_hi must be $m x 1 or $m x $B")
        size(u_nom) == (m, B, T) || error("plant_tape_lqr_shooting: u_nom must be $m x $B x $T")
    end
    n_rho = length(rho); n_lim = limited ? size(u_lo, 2) : 1
    K = zeros(m, n, B, n_keep); P0 = zeros(n, n, B); status = zeros(Cint, B); n_cut = zeros(Cint, B)
    k = zeros(m, B, n_keep); p0 = zeros(n, B); dV = zeros(2, B); clamped = zeros(Cint, B, n_keep)
    d = isempty(defects) ? zeros(1) : defects      # one segment: no node, but the library asks for a pointer
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve Qend u_lo u_hi u_nom begin
        pQf, plo, phi, pun = p(Qend), p(u_lo), p(u_hi), p(u_nom)
        check(@ccall LIB.cimpc_plant_tape_lqr_shooting(tape.handle::Ptr{Cvoid}, n_Q::Cint, Q::Ptr{Cdouble}, pQf::Ptr{Cdouble}, n_R::Cint,
                                                       R::Ptr{Cdouble}, q::Ptr{Cdouble}, r::Ptr{Cdouble}, n_rho::Cint, rho::Ptr{Cdouble},
                                                       n_keep::Cint, K::Ptr{Cdouble}, k::Ptr{Cdouble}, P0::Ptr{Cdouble}, p0::Ptr{Cdouble},
                                                       dV::Ptr{Cdouble}, status::Ptr{Cint}, n_cut::Ptr{Cint}, n_lim::Cint, plo::Ptr{Cdouble},
                                                       phi::Ptr{Cdouble}, pun::Ptr{Cdouble}, clamped::Ptr{Cint}, segment_len::Cint,
                                                       d::Ptr{Cdouble})::Cint)
    end
    return K, k, P0, p0, dV, status, n_cut, clamped
end

"""
    plant_shooting_forward(tape, Q, R, lin_q, lin_r, K, k, defects, segment_len; Qf = nothing) -> (dx_nodes, du, dJ)

`cimpc_plant_shooting_forward`: the linear forward pass at α = 1 over the tape's blocks with the gains K m x n x B x T, k m x B x T of
`plant_tape_lqr_shooting` and its defects: dx at the nodes 2nq x B x (T / segment_len - 1), du m x B x T and dJ 2 x B, the quadratic model's
two terms.  Unexecuted, like the rest of this binding.
"""
function plant_shooting_forward(tape::PlantTape, Q::Array{Float64}, R::Array{Float64}, lin_q::Array{Float64,3}, lin_r::Array{Float64,3},
                                K::Array{Float64,4}, k::Array{Float64,3}, defects::Array{Float64,3}, segment_len::Int;
                                Qf::Union{Nothing,Matrix{Float64}} = nothing)
    tape.handle != C_NULL || error("plant_shooting_forward: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m = tape.B, tape.T, 2 * nq, nu
    (segment_len >= 1 && T % segment_len == 0) || error("plant_shooting_forward: T must be a multiple of segment_len")
    M = T ÷ segment_len
    (size(defects) == (n, B, M - 1) && M > 1) || error("plant_shooting_forward: defects must be $n x $B x $(M - 1), at least one node")
    (size(K) == (m, n, B, T) && size(k) == (m, B, T)) || error("plant_shooting_forward: K must be $m x $n x $B x $T and k $m x $B x $T")
    (size(lin_q) == (n, B, T + 1) && size(lin_r) == (m, B, T)) || error("plant_shooting_forward: lin_q must be $n x $B x $(T + 1) and lin_r $m x $B x $T")
    (size(Q) == (n, n) || size(Q) == (n, n, T)) || error("plant_shooting_forward: Q must be $n x $n or $n x $n x $T")
    (size(R) == (m, m) || size(R) == (m, m, T)) || error("plant_shooting_forward: R must be $m x $m or $m x $m x $T")
    n_Q = ndims(Q) == 2 ? 1 : T; n_R = ndims(R) == 2 ? 1 : T
    Qend = Qf === nothing ? (ndims(Q) == 2 ? Q : Q[:, :, T]) : Qf
    size(Qend) == (n, n) || error("plant_shooting_forward: Qf must be $n x $n")
    dx_nodes = zeros(n, B, M - 1); du = zeros(m, B, T); dJ = zeros(2, B)
    check(@ccall LIB.cimpc_plant_shooting_forward(tape.handle::Ptr{Cvoid}, n_Q::Cint, Q::Ptr{Cdouble}, Qend::Ptr{Cdouble}, n_R::Cint, R::Ptr{Cdouble},
                                                  lin_q::Ptr{Cdouble}, lin_r::Ptr{Cdouble}, K::Ptr{Cdouble}, k::Ptr{Cdouble}, segment_len::Cint,
                                                  defects::Ptr{Cdouble}, dx_nodes::Ptr{Cdouble}, du::Ptr{Cdouble}, dJ::Ptr{Cdouble})::Cint)
    return dx_nodes, du, dJ
end

"""
    plant_shooting_linesearch(tape, segments, qs_nom, u_nom, K, k, dx_nodes, dJ, phi_nom, D_nom, weight, alphas, cost, μ, h_sim, opts; armijo = 1e-4,
                              w = nothing, w_hold = 1, terrain = nothing, steps_per_launch = 0, grad_reg = nothing, u_lo = nothing, u_hi = nothing)
        -> (J, D_cand, phi, ok, choice, qs, u_applied, γ, b, status, iters, defects, D, J_chosen, lin_q, lin_r, tape)

`cimpc_plant_shooting_linesearch`: the line search of a multiple-shooting iteration, every step length of every segment of every robot in ONE
closed-loop rollout of length(alphas) M B robots for T / M steps; phi = J + weight D, acceptance on phi, the chosen candidate's segments compacted
as `plant_rollout_segments` returns a rollout, with their stitched `PlantTape`.  weight: a vector of 1 or B defect weights.  Unexecuted, like the
rest of this binding.
"""
function plant_shooting_linesearch(tape::PlantTape, segments::Int, qs_nom::Array{Float64,3}, u_nom::Array{Float64,3}, K::Array{Float64,4}, k::Array{Float64,3},
                                   dx_nodes::Array{Float64,3}, dJ::Matrix{Float64}, phi_nom::Vector{Float64}, D_nom::Vector{Float64}, weight::Vector{Float64},
                                   alphas::Vector{Float64}, cost::TrackingCost, μ, h_sim, opts; armijo::Real = 1e-4,
                                   w::Union{Nothing,Array{Float64}} = nothing, w_hold::Int = 1, terrain::Union{Nothing,Vector{Terrain}} = nothing,
                                   steps_per_launch::Int = 0, grad_reg = nothing, u_lo::Union{Nothing,Matrix{Float64}} = nothing,
                                   u_hi::Union{Nothing,Matrix{Float64}} = nothing)
    tape.handle != C_NULL || error("plant_shooting_linesearch: the tape is closed")
    id, nq, nu, nc, nf, nw = _plant_dims(tape.model)
    B, T, n, m, M = tape.B, tape.T, 2 * nq, nu, segments
    (M >= 1 && T % M == 0) || error("plant_shooting_linesearch: T must be a multiple of the number of segments")
    L = T ÷ M
    (size(qs_nom) == (nq, M * B, L + 2) && size(u_nom) == (nu, B, T)) || error("plant_shooting_linesearch: qs_nom must be $nq x $(M * B) x $(L + 2) and u_nom $nu x $B x $T")
    (size(K) == (m, n, B, T) && size(k) == (m, B, T) && size(dJ) == (2, B)) || error("plant_shooting_linesearch: K must be $m x $n x $B x $T, k $m x $B x $T, dJ 2 x $B")
    size(dx_nodes) == (n, B, M - 1) || error("plant_shooting_linesearch: dx_nodes must be $n x $B x $(M - 1)")
    (length(phi_nom) == B && length(D_nom) == B && length(weight) in (1, B)) || error("plant_shooting_linesearch: phi_nom and D_nom have B entries, weight 1 or B")
    n_alpha = length(alphas)
    (1 <= n_alpha <= 64 && all(isfinite, alphas) && armijo >= 0) || error("plant_shooting_linesearch: 1 to 64 finite alphas, armijo >= 0")
    n_Q, n_R, n_x = _tracking_cost_sizes("plant_shooting_linesearch", cost, nq, nu, B, T)
    ws = w === nothing ? nothing : ndims(w) == 2 ? reshape(w, nw, 1, :) : w
    μs = Float64.(vcat(μ))
    length(μs) in (1, B) || error("plant_shooting_linesearch: one friction coefficient or one per robot")
    (u_lo === nothing) == (u_hi === nothing) || error("plant_shooting_linesearch: u_lo and u_hi go together")
    o = Ref(opts isa IpOpts ? opts : IpOpts(opts))
    reg = grad_reg === nothing ? o[].kappa_tol * o[].gamma_reg : Float64(grad_reg)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    wp, K_w, n_w = ws === nothing ? (C_NULL, 1, 1) : (ws, size(ws, 3), size(ws, 2))
    n_mu, n_weight = length(μs), length(weight)
    n_lim = u_lo === nothing ? 1 : size(u_lo, 2)
    J = zeros(B, n_alpha); Dc = zeros(B, n_alpha); phi = zeros(B, n_alpha); ok = zeros(Cint, B, n_alpha); choice = zeros(Cint, B)
    qs = zeros(nq, M * B, L + 2); cu = zeros(nu, B, T); γ = zeros(nc, B, T); b = zeros(nf * nc, B, T)
    status = zeros(Cint, B, T); iters = zeros(Cint, B, T); grad_status = zeros(Cint, B, T)
    defects = zeros(n, B, max(M - 1, 1)); D = zeros(B); Jn = zeros(B); lin_q = zeros(n, B, T + 1); lin_r = zeros(m, B, T)
    dxp = isempty(dx_nodes) ? zeros(1) : dx_nodes      # one segment: no node, but the library asks for a pointer
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    p(a) = a === nothing ? C_NULL : pointer(a)
    GC.@preserve cost u_lo u_hi begin
        plo, phi_ = p(u_lo), p(u_hi)
        cc = Ref(TrackingCostC(pointer(cost.Q), pointer(cost.Qf), pointer(cost.R), pointer(cost.x_goal), pointer(cost.u_goal), n_Q, n_R, n_x))
        check(@ccall LIB.cimpc_plant_shooting_linesearch(tape.handle::Ptr{Cvoid}, M::Cint, steps_per_launch::Cint, n_ter::Cint, ter::Ptr{Terrain},
                                                         qs_nom::Ptr{Cdouble}, u_nom::Ptr{Cdouble}, wp::Ptr{Cdouble}, K_w::Cint, n_w::Cint, w_hold::Cint,
                                                         μs::Ptr{Cdouble}, n_mu::Cint, h_sim::Cdouble, o::Ref{IpOpts}, K::Ptr{Cdouble}, k::Ptr{Cdouble},
                                                         dxp::Ptr{Cdouble}, dJ::Ptr{Cdouble}, phi_nom::Ptr{Cdouble}, D_nom::Ptr{Cdouble}, n_weight::Cint,
                                                         weight::Ptr{Cdouble}, n_alpha::Cint, alphas::Ptr{Cdouble}, armijo::Cdouble, cc::Ref{TrackingCostC},
                                                         reg::Cdouble, J::Ptr{Cdouble}, Dc::Ptr{Cdouble}, phi::Ptr{Cdouble}, ok::Ptr{Cint}, choice::Ptr{Cint},
                                                         qs::Ptr{Cdouble}, cu::Ptr{Cdouble}, γ::Ptr{Cdouble}, b::Ptr{Cdouble}, status::Ptr{Cint},
                                                         iters::Ptr{Cint}, defects::Ptr{Cdouble}, D::Ptr{Cdouble}, Jn::Ptr{Cdouble}, lin_q::Ptr{Cdouble},
                                                         lin_r::Ptr{Cdouble}, grad_status::Ptr{Cint}, handle::Ref{Ptr{Cvoid}}, n_lim::Cint, plo::Ptr{Cdouble},
                                                         phi_::Ptr{Cdouble})::Cint)
    end
    return J, Dc, phi, ok, choice, qs, cu, γ, b, status, iters, defects[:, :, 1:M-1], D, Jn, lin_q, lin_r, PlantTape(handle[], tape.model, B, T, tape.n_cols, grad_status)
end

"""
    plant_shooting_cost(cost, qs, u, segments) -> (J, D, defects, lin_q, lin_r)

`cimpc_plant_shooting_cost` (host only): the cost and the defects of segment trajectories qs nq x (M B) x (L + 2) under the controls u
nu x B x T, bit for bit what `plant_rollout_segments` computes on the device.
"""
function plant_shooting_cost(cost::TrackingCost, qs::Array{Float64,3}, u::Array{Float64,3}, segments::Int)
    nq, nu, B, T, M = size(qs, 1), size(u, 1), size(u, 2), size(u, 3), segments
    (M >= 1 && T % M == 0 && size(qs, 2) == M * B && size(qs, 3) == T ÷ M + 2) || error("plant_shooting_cost: qs must be nq x (M B) x (T / M + 2) beside u nu x B x T")
    n_Q, n_R, n_x = _tracking_cost_sizes("plant_shooting_cost", cost, nq, nu, B, T)
    J = zeros(B); D = zeros(B); defects = zeros(2 * nq, B, M - 1); lin_q = zeros(2 * nq, B, T + 1); lin_r = zeros(nu, B, T)
    GC.@preserve cost begin
        cc = Ref(TrackingCostC(pointer(cost.Q), pointer(cost.Qf), pointer(cost.R), pointer(cost.x_goal), pointer(cost.u_goal), n_Q, n_R, n_x))
        check(@ccall LIB.cimpc_plant_shooting_cost(nq::Cint, nu::Cint, B::Cint, T::Cint, M::Cint, cc::Ref{TrackingCostC}, qs::Ptr{Cdouble},
                                                   u::Ptr{Cdouble}, J::Ptr{Cdouble}, D::Ptr{Cdouble}, defects::Ptr{Cdouble}, lin_q::Ptr{Cdouble},
                                                   lin_r::Ptr{Cdouble})::Cint)
    end
    return J, D, defects, lin_q, lin_r
end

# ---- the plant models linearized on the device: the `LinearizedStep` triple of N knots in one call (linearized_step.jl:10-31) --------
"""
    plant_linearize(model, z, θ, κ; terrain = nothing) -> (r0, rz0, rθ0)

z: nz x N and θ: nθ x N (a vector is one knot), in the model's own z = [q2; γ; b; ψ; s1; η; s2] and θ = [q0; q1; u1; w1; μ; h].
Returns r0: nz x N, rz0: nz x nz x N, rθ0: nz x nθ x N - `rz0[:, :, k]` and `rθ0[:, :, k]` are the matrices `LinearizedStep` holds
and `set_linearization!` takes.  terrain: nothing (flat ground) or a vector of 1 or N `Terrain`.  The device models carry the
reference's parameter tables.  Sizes are checked against the model's table; unknown models are an error.
"""
function plant_linearize(model::Symbol, z::VecOrMat{Float64}, θ::VecOrMat{Float64}, κ::Real;
                         terrain::Union{Nothing,Vector{Terrain}} = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    nz = nq + 4 * nc + 2 * nf * nc; nθ = 2 * nq + nu + nw + 2
    zs = reshape(z, size(z, 1), :); θs = reshape(θ, size(θ, 1), :)
    N = size(zs, 2)
    (size(zs, 1) == nz && size(θs) == (nθ, N) && N >= 1) || error("plant_linearize($model): z must be $nz x N and θ $nθ x N")
    (terrain === nothing || length(terrain) in (1, N)) || error("plant_linearize($model): one terrain or one per knot")
    r0 = zeros(nz, N); rz0 = zeros(nz, nz, N); rθ0 = zeros(nz, nθ, N)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    check(@ccall LIB.cimpc_plant_linearize(id::Cint, N::Cint, n_ter::Cint, ter::Ptr{Terrain}, zs::Ptr{Cdouble}, θs::Ptr{Cdouble},
                                           κ::Cdouble, r0::Ptr{Cdouble}, rz0::Ptr{Cdouble}, rθ0::Ptr{Cdouble})::Cint)
    return r0, rz0, rθ0
end

# ---- step gradients of N knots: the kernel of `plant_rollout(...; diff_sol = true)` alone ------------------------------------------------
"""
    plant_sensitivity(model, z, θ, reg; n_cols = 2nq + nu, terrain = nothing) -> (dz, status)

dz[:, :, k] = -R(z, θ; reg)⁻¹ ∂r/∂θ[:, 1:n_cols] at knot k, rows [q2; γ; b] (nr = nq + nc + nb), where R is ∂r/∂z with the bilinear
rows' diagonals max(y2, reg), max(y1, reg) (`cimpc_plant_sensitivity`).  z: nz x N, θ: nθ x N (a vector is one knot); status[k] = 0
marks a knot that is not differentiable (a zero or non-finite pivot or result): its block is zero.
"""
function plant_sensitivity(model::Symbol, z::VecOrMat{Float64}, θ::VecOrMat{Float64}, reg::Real;
                           n_cols::Union{Nothing,Int} = nothing, terrain::Union{Nothing,Vector{Terrain}} = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    nz = nq + 4 * nc + 2 * nf * nc; nθ = 2 * nq + nu + nw + 2; nr = nq + nc + nf * nc
    zs = reshape(z, size(z, 1), :); θs = reshape(θ, size(θ, 1), :)
    N = size(zs, 2)
    cols = n_cols === nothing ? 2 * nq + nu : n_cols
    (size(zs, 1) == nz && size(θs) == (nθ, N) && N >= 1) || error("plant_sensitivity($model): z must be $nz x N and θ $nθ x N")
    (1 <= cols <= nθ) || error("plant_sensitivity($model): n_cols must be in 1 .. $nθ")
    (terrain === nothing || length(terrain) in (1, N)) || error("plant_sensitivity($model): one terrain or one per knot")
    dz = zeros(nr, cols, N); status = zeros(Cint, N)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    check(@ccall LIB.cimpc_plant_sensitivity(id::Cint, N::Cint, n_ter::Cint, ter::Ptr{Terrain}, zs::Ptr{Cdouble}, θs::Ptr{Cdouble},
                                             reg::Cdouble, cols::Cint, dz::Ptr{Cdouble}, status::Ptr{Cint})::Cint)
    return dz, status
end

# ---- A1 on the device: the tables of knots t0 .. t0+N-1 in one call, built by one workgroup per knot -----------------------------------
_lin_dims(hs::Solver) = (d = hs.dims; (Int(d.nq + 4 * d.nc + 2 * d.nb), Int(2 * d.nq + d.nu + d.nw + 2)))      # nz, nθ of the handle

"""
    set_linearization_batch!(hs, t0, z0, θ0, r0, rz0, rθ0)

`set_linearization!` of knots `t0 .. t0+N-1` in one call: z0, r0: nz x N, θ0: nθ x N, rz0: nz x nz x N, rθ0: nz x nθ x N (what
`plant_linearize` returns).  One upload, the tables built on the device, equal bit for bit to N single calls; a knot with a
singular Dx fails the whole call and changes no table.
"""
function set_linearization_batch!(hs::Solver, t0::Int, z0::Matrix{Float64}, θ0::Matrix{Float64}, r0::Matrix{Float64},
                                  rz0::Array{Float64,3}, rθ0::Array{Float64,3})
    nz, nθ = _lin_dims(hs)
    N = size(z0, 2)
    (N >= 1 && size(z0, 1) == nz && size(θ0) == (nθ, N) && size(r0) == (nz, N) && size(rz0) == (nz, nz, N) && size(rθ0) == (nz, nθ, N)) ||
        error("set_linearization_batch!: z0, r0 must be $nz x N, θ0 $nθ x N, rz0 $nz x $nz x N, rθ0 $nz x $nθ x N")
    (1 <= t0 && t0 + N - 1 <= hs.dims.H_ref) || error("set_linearization_batch!: knots $t0 .. $(t0 + N - 1) are not in 1 .. $(hs.dims.H_ref)")
    check(ccall((:cimpc_set_linearization_batch, LIB), Cint,
                (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                hs.h, t0, N, z0, θ0, r0, rz0, rθ0), hs.h)
end

"""
    linearize_knots!(hs, model, z, θ, κ; t0 = 1, terrain = nothing)

Knots `t0 .. t0+N-1` linearized at κ and their tables built, all on the handle's device: `plant_linearize(model, z, θ, κ; terrain)`
followed by `set_linearization!` of every knot, bit for bit, with only z (nz x N), θ (nθ x N) and the terrains crossing to the
device - the in-flight `update!` of `RLin / RZLin / RθLin` for N knots.  The model's dimensions must be the handle's.
"""
function linearize_knots!(hs::Solver, model::Symbol, z::Matrix{Float64}, θ::Matrix{Float64}, κ::Real; t0::Int = 1,
                          terrain::Union{Nothing,Vector{Terrain}} = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    d = hs.dims
    (nq, nu, nw, nc, nf * nc) == (d.nq, d.nu, d.nw, d.nc, d.nb) || error("linearize_knots!: $model does not have the handle's dimensions")
    nz, nθ = _lin_dims(hs)
    N = size(z, 2)
    (N >= 1 && size(z, 1) == nz && size(θ) == (nθ, N)) || error("linearize_knots!($model): z must be $nz x N and θ $nθ x N")
    (1 <= t0 && t0 + N - 1 <= d.H_ref) || error("linearize_knots!: knots $t0 .. $(t0 + N - 1) are not in 1 .. $(d.H_ref)")
    (terrain === nothing || length(terrain) in (1, N)) || error("linearize_knots!($model): one terrain or one per knot")
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    check(@ccall LIB.cimpc_linearize_knots(hs.h::Ptr{Cvoid}, id::Cint, t0::Cint, N::Cint, n_ter::Cint, ter::Ptr{Terrain}, z::Ptr{Cdouble},
                                           θ::Ptr{Cdouble}, κ::Cdouble)::Cint, hs.h)
end

"One knot's packed table (csrc/lin_table.h) as the kernels read it - for tests and diagnostics."
function get_table(hs::Solver, t::Int)
    n = Ref{Cint}(0); nkkt = Ref{Cint}(0)
    check(ccall((:cimpc_query_sizes, LIB), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), hs.h, n, nkkt), hs.h)
    table = zeros(Int(n[]))
    check(ccall((:cimpc_get_table, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), hs.h, t, table), hs.h)
    return table
end

# ---- time-varying LQR feedback gains along the reference (src/controller/gains.jl:1-51) on the device ---------------------------------
"""
    tvlqr(A, B, Q, R) -> (K, P1)

`tvlqr` of gains.jl:1-15 with the reference's arguments: vectors of T-1 matrices A (n x n), B (n x m), R (m x m) and of T matrices Q.
K is the reference's vector of T-1 gains (m x n).  The cost-to-go matrices stay on the device: of the reference's `P` only `P[1]`
comes back.  A singular `R + B'PB` is an error naming the step, like the reference's `\\`.
"""
function tvlqr(A::AbstractVector, B::AbstractVector, Q::AbstractVector, R::AbstractVector)
    T = length(Q)
    (T >= 2 && length(A) == T - 1 && length(B) == T - 1 && length(R) == T - 1) || error("tvlqr: T = length(Q) >= 2 and T - 1 matrices A, B, R")
    n, m = size(B[1])
    dense(v, r, c) = (M = zeros(r, c, length(v)); for (i, x) in enumerate(v); M[:, :, i] .= x; end; M)
    Ac = dense(A, n, n); Bc = dense(B, n, m); Qc = dense(Q, n, n); Rc = dense(R, m, m)
    K = zeros(m, n, T - 1); P1 = zeros(n, n)
    check(ccall((:cimpc_tvlqr, LIB), Cint,
                (Cint, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                1, n, m, T, T - 1, Ac, Bc, T, Qc, T - 1, Rc, T - 1, K, P1))
    return [K[:, :, t] for t = 1:T - 1], P1
end

"""
    reference_gains(model, traj, obj; N = 10, κ = 2e-4, U_scaling = 100, V_scaling = 100) -> K[1:H]

`reference_gains(s, traj, obj; ...)` of gains.jl:17-51 with the device plant model `model` (a key of the plant tables) in the place
of the simulation: traj.z, traj.θ are linearized on the device, dz/dθ, the N-fold Riccati chain and nothing but the H gains
(nu x 2nq each) come back.  `obj` is the TrackingVelocityObjective: obj.q[1], obj.v[1], obj.u[1] are used.  κ is accepted and does
not enter (the derivatives do not depend on it).  The planar models at their shipped gaits are singular here, as in the reference.
"""
function reference_gains(model::Symbol, traj, obj; N::Int = 10, κ = 2e-4, U_scaling = 100, V_scaling = 100,
                         terrain::Union{Nothing,Vector{Terrain}} = nothing)
    id, nq, nu, nc, nf, nw = _plant_dims(model)
    nz = nq + 4 * nc + 2 * nf * nc; nθ = 2 * nq + nu + nw + 2
    H = traj.H
    z = pack(traj.z, H); θ = pack(traj.θ, H)
    (size(z) == (nz, H) && size(θ) == (nθ, H)) || error("reference_gains($model): traj.z must be $nz x H and traj.θ $nθ x H")
    (terrain === nothing || length(terrain) in (1, H)) || error("reference_gains($model): one terrain or one per knot")
    Qq = Matrix{Float64}(obj.q[1]); Qv = Matrix{Float64}(obj.v[1]); Ru = Matrix{Float64}(obj.u[1])
    K = zeros(nu, 2 * nq, H)
    n_ter, ter = terrain === nothing ? (0, C_NULL) : (length(terrain), terrain)
    Us = Float64(U_scaling); Vs = Float64(V_scaling); P1 = C_NULL
    check(@ccall LIB.cimpc_reference_gains(id::Cint, H::Cint, N::Cint, n_ter::Cint, ter::Ptr{Terrain}, z::Ptr{Cdouble}, θ::Ptr{Cdouble},
                                           Qq::Ptr{Cdouble}, Qv::Ptr{Cdouble}, Ru::Ptr{Cdouble}, Us::Cdouble, Vs::Cdouble,
                                           K::Ptr{Cdouble}, P1::Ptr{Cdouble})::Cint)
    return [K[:, :, t] for t = 1:H]
end

"The same from a linearization made elsewhere: rz0 nz x nz x H, rθ0 nz x nθ x H (what `plant_linearize` returns)."
function reference_gains_lin(nq::Int, nu::Int, rz0::Array{Float64,3}, rθ0::Array{Float64,3}, obj; N::Int = 10, U_scaling = 100, V_scaling = 100)
    nz, nθ, H = size(rθ0)
    size(rz0) == (nz, nz, H) || error("reference_gains_lin: rz0 must be $nz x $nz x $H")
    Qq = Matrix{Float64}(obj.q[1]); Qv = Matrix{Float64}(obj.v[1]); Ru = Matrix{Float64}(obj.u[1])
    K = zeros(nu, 2 * nq, H)
    check(ccall((:cimpc_reference_gains_lin, LIB), Cint,
                (Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble,
                 Ptr{Cdouble}, Ptr{Cdouble}),
                nq, nu, nz, nθ, H, N, rz0, rθ0, Qq, Qv, Ru, U_scaling, V_scaling, K, C_NULL))
    return [K[:, :, t] for t = 1:H]
end

# The gains in the policy: the feedback line of examples/centroidal_quadruped/continuous_policy_v3.jl:74-85 placed in the discrete
# policy() - a placement of this build, the reference's policy() never applies its gains (include/cimpc.h).
"""
    set_gains!(hs, K)

K: the vector `reference_gains` returns - H_ref matrices nu x 2nq, one per reference knot; `nothing` switches the feedback off.
"""
function set_gains!(hs::Solver, K::Union{Nothing,AbstractVector{<:AbstractMatrix}})
    K === nothing && return check(ccall((:cimpc_set_gains, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), hs.h, C_NULL), hs.h)
    d = hs.dims
    (length(K) == d.H_ref && all(size(k) == (d.nu, 2 * d.nq) for k in K)) ||
        error("set_gains!: K must be $(d.H_ref) matrices $(d.nu) x $(2 * d.nq)")
    Kc = Array{Float64,3}(cat(K...; dims = 3))          # nu x 2nq x H_ref, column-major: the library's H_ref x (nu x 2nq)
    check(ccall((:cimpc_set_gains, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), hs.h, Kc), hs.h)
end
"After a Newton solve and before `mpc_advance!`: keeps u1, K[window[1]] and [q_ref[1]; q_ref[2]] of every rollout."
gain_latch!(hs::Solver) = check(ccall((:cimpc_gain_latch, LIB), Cint, (Ptr{Cvoid},), hs.h), hs.h)
"u (nu x B) = (u1 + K ([q_ref[1]; q_ref[2]] - [q0; q_cur])) / n_sample with q0 = q_cur - n_sample (q_cur - q_prev); q_prev, q_cur: nq x B."
function gain_feedback!(hs::Solver, u::Matrix{Float64}, q_prev::Matrix{Float64}, q_cur::Matrix{Float64}, n_sample::Real)
    check(ccall((:cimpc_gain_feedback, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
                hs.h, q_prev, q_cur, n_sample, u), hs.h)
    return u
end

end # module

# executed in the INCLUDING module (ContactImplicitMPC): `eval(opts.solver)` of newton.jl:86 looks the constructor up there
using .CIMPCHip: hip_mpc_solver, hip_kkt_solver, hip_csc_solver
