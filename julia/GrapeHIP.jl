# GrapeHIP.jl -- thin `ccall` glue between GRAPE.jl and libgrape_hip.so (include/grape_hip.h, ABI v7).
#
# NOT EXECUTED in this repository's CI: the build image has no Julia toolchain.  It is written
# against the C ABI and the reference's own interfaces and shows exactly what a GRAPE.jl maintainer
# would add.  Drop-in point: the closure `fg!(F, G, pulsevals)` of GRAPE.optimize
# (/root/reference/src/optimize.jl:105-111), which run_optimizer calls at
# ext/GRAPELBFGSBExt.jl:99 (`f = fg!(f, obj.g, x)`) and ext/GRAPEOptimExt.jl:31.
module GrapeHIP

using LinearAlgebra
import QuantumControl
import QuantumControl.QuantumPropagators
using QuantumControl.QuantumPropagators.Controls: discretize_on_midpoints, evaluate, get_controls
using QuantumControl.QuantumPropagators.Amplitudes: ShapedAmplitude
using QuantumControl.Functionals: J_T_sm, J_T_ss, J_T_re

const libgrape = get(ENV, "GRAPE_HIP_LIB", "libgrape_hip.so")
const ABI_VERSION = 7

# mirror of `grape_problem` (include/grape_hip.h); field order and types must match the C struct
# (tests/test_abi.py compares the field lists)
struct GrapeProblem
    abi_version::Int32
    N::Int32
    L::Int32
    K::Int32
    K_total::Int32
    N_T::Int32
    functional::Int32        # 0 = J_T_sm, 1 = J_T_ss, 2 = J_T_re
    gradient_method::Int32   # 0 = :gradgen, 1 = :taylor
    hc_per_traj::Int32
    device::Int32
    tlist::Ptr{Float64}
    H0::Ptr{ComplexF64}      # K matrices, column-major (Julia's own layout: no copy)
    Hc::Ptr{ComplexF64}
    shape::Ptr{Float64}
    psi0::Ptr{ComplexF64}
    target::Ptr{ComplexF64}
    weights::Ptr{Float64}
    chi_min_norm::Float64
    taylor_max_order::Int32
    taylor_tolerance::Float64
    Dpen::Ptr{ComplexF64}    # state running cost g_b = <Psi|D|Psi> (C_NULL = off)
    dpen_per_traj::Int32
    lambda_b::Float64
    prop_method::Int32       # 0 = ExpProp (materialised Pade propagators), 1 = matrix-free series (Cheby/Newton role)
    prop_tolerance::Float64  # <= 0: 1e-17
    ndev::Int32              # > 1: the trajectories are dealt to several GPUs behind this one handle
    devices::Ptr{Int32}      # C_NULL: device, device+1, ...
    taylor_no_check::Int32   # ABI v6: 1 = taylor_grad_check_convergence = false (optimize.jl:917-918)
end

mutable struct Handle
    ptr::Ptr{Cvoid}
    keepalive::Vector{Any}   # arrays whose pointers were handed over during grape_create
    K::Int
    N::Int
    functional::Int          # -1: user-supplied J_T / chi (split-phase calls + grape_backward_chi)
    no_target::Vector{Int}   # trajectories without a target_state: tau_vals[k] = NaN on the host (optimize.jl:753)
    L::Int                   # optimised controls (length(wrk.controls))
    N_T::Int
    fixed::Vector{Float64}   # pulse values of the pseudo-controls ([P*N_T], control-major; empty: none), see problem_arrays
    x_full::Vector{Float64}  # [(L+P)*N_T] staging: wrk.pulsevals followed by `fixed`
    G_full::Vector{Float64}  # [(L+P)*N_T] staging of the gradient (the first L*N_T entries are the caller's)
end

last_error(ptr) = unsafe_string(ccall((:grape_last_error, libgrape), Cstring, (Ptr{Cvoid},), ptr))

function check(h::Handle, rc::Integer)
    # becomes result.message = "Exception: ..." via src/optimize.jl:125-135 (or is rethrown with rethrow_exceptions)
    rc == 0 || error(last_error(h.ptr))
end


# ---- the static problem out of the reference's own types -----------------------------------------------------------

"""
    drift, control_ops, amplitudes = split_generator(generator)

`QuantumPropagators.Generators.Generator` keeps `ops` (drift terms first, then one operator per amplitude) and
`amplitudes` (`hamiltonian(H0, (H1, ϵ1), ...)`, docs/src/tutorial.md:55-73).
"""
function split_generator(gen)
    ops, amps = gen.ops, gen.amplitudes
    nd = length(ops) - length(amps)
    n = size(ops[1], 1)
    drift = zeros(ComplexF64, n, n)
    for op in ops[1:nd]
        drift .+= Matrix{ComplexF64}(op)
    end
    return drift, [Matrix{ComplexF64}(op) for op in ops[nd+1:end]], collect(amps)
end

control_of(a) = a
control_of(a::ShapedAmplitude) = a.control

"""
    H0, Hc, hc_per_traj, shape, fixed = problem_arrays(wrk)

Drift `H0[k]` of every trajectory, the operator `Hc[k][l]` = ∂H_k/∂ϵ_l multiplying control `l` of `wrk.controls`
(src/workspace.jl:152-157; a control that enters a generator through several amplitudes gets the sum of their
operators), and the static shapes `S_l(t_n)` of `ShapedAmplitude`s discretised on the midpoints of the time grid
(docs/src/tutorial.md:75-107) -- `nothing` if no amplitude is shaped.  Control amplitudes that depend non-linearly on
their control are not expressible in `grape_problem` (INTEGRATION.md: host-side chain rule).

A time-dependent amplitude that is NOT a control (`get_controls(a) == ()`: the reference re-evaluates the generator on
every interval, `evaluate(a, tlist, n)`, src/optimize.jl:732, 881, 937-945) becomes a PSEUDO-CONTROL: an extra operator
slot `L + j` in every `Hc[k]` and a row of fixed pulse values in `fixed` ([N_T, P]); `make_fg!` appends those values to
every pulse vector and drops the pseudo-controls' rows of the gradient.  (`grape_problem.H0` is one constant matrix per
trajectory; the library limits L + P to 8.)
"""
function problem_arrays(wrk)
    tlist, controls = wrk.result.tlist, wrk.controls
    K, L, N_T = length(wrk.trajectories), length(controls), length(tlist) - 1
    # pass 1: the amplitudes without a control, by identity, in order of first appearance
    fixed_amps = Any[]
    for traj in wrk.trajectories
        for a in split_generator(traj.generator)[3]
            isempty(get_controls(a)) && !any(b -> b === a, fixed_amps) && push!(fixed_amps, a)
        end
    end
    P = length(fixed_amps)
    fixed = Float64[real(evaluate(a, tlist, n)) for n = 1:N_T, a in fixed_amps]   # [N_T, P]
    H0 = Matrix{ComplexF64}[]
    Hc = Vector{Matrix{ComplexF64}}[]
    shape = ones(Float64, N_T, L + P)
    shaped = false
    for traj in wrk.trajectories
        drift, ops, amps = split_generator(traj.generator)
        n = size(drift, 1)
        per_l = [zeros(ComplexF64, n, n) for _ = 1:(L + P)]
        for (op, a) in zip(ops, amps)
            j = findfirst(b -> b === a, fixed_amps)
            if !isnothing(j)
                per_l[L + j] .+= op
                continue
            end
            l = findfirst(c -> c === control_of(a), controls)
            isnothing(l) && error("GrapeHIP: amplitude of type $(typeof(a)) is neither a (shaped) control of the problem nor control-free")
            per_l[l] .+= op
            if a isa ShapedAmplitude
                shape[:, l] .= discretize_on_midpoints(a.shape, tlist)
                shaped = true
            end
        end
        push!(H0, drift)
        push!(Hc, per_l)
    end
    hc_per_traj = any(Hc[k] != Hc[1] for k = 2:K)
    return H0, Hc, hc_per_traj, (shaped ? shape : nothing), fixed
end

"""J_T_sm / J_T_ss / J_T_re have a device-side χ (fast path); any other functional goes through `grape_backward_chi`."""
function functional_code(J_T)
    J_T === J_T_sm && return 0
    J_T === J_T_ss && return 1
    J_T === J_T_re && return 2
    return -1
end


"""
    Handle(wrk; device = 0, devices = nothing, prop_method = 0, D = nothing)

Uploads the static problem of a `GrapeWrk` (replaces the buffer set-up of src/workspace.jl:147-362).  Options are
taken from `wrk.kwargs` exactly where the reference reads them: `gradient_method` (workspace.jl:150), `chi_min_norm`
(optimize.jl:846), `taylor_grad_max_order` / `taylor_grad_tolerance` / `taylor_grad_check_convergence` (optimize.jl:915-918),
`lambda_b` (:833).
`D` (one matrix or one per trajectory) selects the state running cost of the family `g_b(Ψ) = ⟨Ψ|D|Ψ⟩`, `ξ = −DΨ`
(test/test_state_running_cost.jl:32-40).  `devices = [0, 1, ...]` spreads the trajectories over several GPUs behind this
one handle -- the analogue of `use_threads` (optimize.jl:720, 876).
"""
function Handle(wrk; device = 0, devices = nothing, prop_method = 0, D = nothing)
    tlist = Vector{Float64}(wrk.result.tlist)
    kw = wrk.kwargs
    H0, Hc, hc_per_traj, shape, fixed = problem_arrays(wrk)
    K, N, L, N_T = length(H0), size(H0[1], 1), length(wrk.controls), length(tlist) - 1
    P = size(fixed, 2)                                                      # pseudo-controls behind the L optimised ones
    H0f = reduce(hcat, vec.(H0))                                            # [N*N, K]: K column-major matrices
    Hcf = hc_per_traj ? reduce(hcat, [reduce(hcat, vec.(Hc[k])) for k = 1:K]) : reduce(hcat, vec.(Hc[1]))
    p0 = reduce(hcat, [Vector{ComplexF64}(t.initial_state) for t in wrk.trajectories])
    # trajectories without a target_state (optimize.jl:753: tau_k = NaN for THOSE k only, legal with a user J_T): no target
    # array at all when no trajectory has one; otherwise zeros in the gaps and tau_vals[k] = NaN set on the host (make_fg!)
    no_target = findall(t -> isnothing(t.target_state), wrk.trajectories)
    tg = length(no_target) == K ? nothing :
         reduce(hcat, [isnothing(t.target_state) ? zeros(ComplexF64, N) : Vector{ComplexF64}(t.target_state) for t in wrk.trajectories])
    weights = Float64[hasproperty(t, :weight) ? t.weight : 1.0 for t in wrk.trajectories]
    shp = isnothing(shape) ? nothing : Matrix{Float64}(shape)               # [N_T, L] column-major == [l][n]
    Df = isnothing(D) ? nothing : (D isa AbstractMatrix ? Matrix{ComplexF64}(D) : reduce(hcat, vec.(Matrix{ComplexF64}.(D))))
    devs = isnothing(devices) ? nothing : Vector{Int32}(devices)
    functional = functional_code(kw[:J_T])
    keep = Any[H0f, Hcf, p0, tg, tlist, weights, shp, Df, devs]
    prob = Ref(GrapeProblem(
        ABI_VERSION, N, L + P, K, 0, N_T, max(functional, 0),
        get(kw, :gradient_method, :gradgen) == :taylor ? 1 : 0, hc_per_traj ? 1 : 0, device,
        pointer(tlist), pointer(H0f), pointer(Hcf), isnothing(shp) ? C_NULL : pointer(shp), pointer(p0), isnothing(tg) ? C_NULL : pointer(tg),
        pointer(weights), get(kw, :chi_min_norm, 0.0), get(kw, :taylor_grad_max_order, 0),
        get(kw, :taylor_grad_tolerance, 0.0), isnothing(Df) ? C_NULL : pointer(Df),
        (D isa AbstractMatrix || isnothing(D)) ? 0 : 1, isnothing(D) ? 0.0 : get(kw, :lambda_b, 1.0), prop_method, 0.0,
        isnothing(devs) ? 0 : length(devs), isnothing(devs) ? C_NULL : pointer(devs),
        get(kw, :taylor_grad_check_convergence, true) ? 0 : 1))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve keep ccall((:grape_create, libgrape), Cint, (Ref{Ptr{Cvoid}}, Ref{GrapeProblem}), out, prob)
    rc == 0 || error(last_error(C_NULL))
    h = Handle(out[], keep, K, N, functional, no_target, L, N_T, vec(fixed), zeros(Float64, (L + P) * N_T), zeros(Float64, (L + P) * N_T))
    h.x_full[(L * N_T + 1):end] .= h.fixed
    finalizer(x -> ccall((:grape_destroy, libgrape), Cvoid, (Ptr{Cvoid},), x.ptr), h)
    # caller-supplied chi (functional == -1) or xi (a g_b that is not given as the operator D): the backward sweep runs
    # when that data arrives -- the forward call must not run a (unit-target) backward sweep in the same launch
    if functional < 0 || (!isnothing(get(kw, :g_b, nothing)) && isnothing(D))
        ccall((:grape_set_fused_sweeps, libgrape), Cint, (Ptr{Cvoid}, Cint), h.ptr, 0)
    end
    return h
end


"""
    fg! = make_fg!(h, wrk)

Replacement for the closure at src/optimize.jl:105-111.  Keeps the side effects callers rely on (SURVEY.md 8b):
`wrk.pulsevals`, the call counters, `wrk.result.tau_vals`, `wrk.J_parts[1:3]`, `wrk.grad_J_Tb`, `wrk.grad_J_a` and the
final states that `update_result!` reads (src/optimize.jl:187-189).
"""
function make_fg!(h::Handle, wrk)
    K, N = h.K, h.N
    kw = wrk.kwargs
    tlist = wrk.result.tlist
    psiT = Matrix{ComplexF64}(undef, N, K)
    chiT = Matrix{ComplexF64}(undef, N, K)
    sums = zeros(Float64, 8)
    J_T, chi = kw[:J_T], kw[:chi]
    J_a, grad_J_a = get(kw, :J_a, nothing), get(kw, :grad_J_a, nothing)
    λₐ, λ_b = get(kw, :lambda_a, 1.0), get(kw, :lambda_b, 1.0)
    has_gb = !isnothing(get(kw, :g_b, nothing))
    # g_b / xi as callbacks (src/optimize.jl:727-750, 856-866, 897-908) when no operator D was handed to create_handle:
    # evaluated here on the stored forward states, the array xi_k(t_n) goes to grape_backward_xi (ABI v5)
    g_b, xi = get(kw, :g_b, nothing), get(kw, :xi, nothing)
    xi_route = has_gb && isnothing(h.keep[8])                              # (keep[8]: the operator D handed to Handle(...))
    # (the reference derives a missing xi by automatic differentiation, src/workspace.jl:313-316; this glue has no AD
    # hook: say so HERE, at construction, not as a MethodError on `nothing` inside fg!)
    xi_route && isnothing(xi) && error("GrapeHIP.make_fg!: a running cost g_b given as a callback needs xi " *
                                       "(xi(state, trajectory, tlist, n) = -∂g_b/∂⟨Ψ|); pass xi = ... or hand the operator D to Handle(...)")
    N_T = length(tlist) - 1
    fw = xi_route ? Array{ComplexF64}(undef, N, N_T + 1, K) : nothing      # Ψ_k(t_n): [K][N_T+1][N] on the C side
    xi_arr = xi_route ? zeros(ComplexF64, N, N_T + 1, K) : nothing
    states() = [view(psiT, :, k) for k = 1:K]
    function J_b_and_xi!(want_xi)
        check(h, ccall((:grape_get_storage, libgrape), Cint, (Ptr{Cvoid}, Cint, Ptr{ComplexF64}), h.ptr, 0, fw))
        J_b = 0.0
        for k = 1:K
            traj = wrk.trajectories[k]
            J_b += g_b(view(fw, :, 1, k), traj, tlist, 1) * (tlist[2] - tlist[1]) / 2          # :728-730
            for n = 2:(N_T + 1)                                                                 # :739-749
                dt = n <= N_T ? (tlist[n + 1] - tlist[n - 1]) / 2 : (tlist[end] - tlist[end - 1]) / 2
                J_b += g_b(view(fw, :, n, k), traj, tlist, n) * dt
                want_xi && (xi_arr[:, n, k] .= xi(view(fw, :, n, k), traj, tlist, n))
            end
        end
        return J_b
    end

    return function fg!(F, G, pulsevals)
        (pulsevals !== wrk.pulsevals) && (wrk.pulsevals .= pulsevals)      # src/optimize.jl:706-713
        if isnothing(G)
            wrk.result.f_calls += 1; wrk.fg_count[2] += 1                  # :715-716
        else
            wrk.result.fg_calls += 1; wrk.fg_count[1] += 1                 # :838-839
        end
        tau = wrk.result.tau_vals
        # pseudo-controls (problem_arrays): the library sees L + P controls -- the fixed pulse values ride behind the caller's,
        # and the gradient lands in a staging vector whose first L*N_T entries are the caller's rows
        pseudo = !isempty(h.fixed)
        pseudo && copyto!(h.x_full, 1, wrk.pulsevals, 1, h.L * h.N_T)
        x = pseudo ? h.x_full : wrk.pulsevals
        Gbuf = pseudo ? h.G_full : wrk.grad_J_Tb
        if h.functional >= 0 && xi_route
            # built-in J_T with a g_b given as callbacks: split-phase calls, xi on the host
            check(h, GC.@preserve x tau h ccall((:grape_forward, libgrape), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}), h.ptr, pointer(x), pointer(tau)))
            check(h, ccall((:grape_get_final_states, libgrape), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}), h.ptr, psiT))
            check(h, ccall((:grape_get_sums, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, sums))
            Ψ = states()
            wrk.J_parts[1] = wrk.J_T_takes_tau ? J_T(Ψ, wrk.trajectories; tau = tau) : J_T(Ψ, wrk.trajectories)
            wrk.J_parts[3] = λ_b * J_b_and_xi!(!isnothing(G))
            if !isnothing(G)
                f_total = Float64[sums[1], sums[2]]                        # Σ_k w_k τ_k of this (unsharded) handle
                check(h, GC.@preserve f_total xi_arr wrk h ccall((:grape_backward_xi, libgrape), Cint,
                    (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Cdouble, Ptr{Float64}),
                    h.ptr, pointer(f_total), C_NULL, pointer(xi_arr), λ_b, pointer(Gbuf)))
            end
        elseif h.functional >= 0
            # built-in functional: one call, χ is formed on the device
            J = Ref{Float64}(0.0)
            Gp = isnothing(G) ? Ptr{Float64}(C_NULL) : pointer(Gbuf)
            rc = GC.@preserve x tau psiT wrk h ccall((:grape_eval, libgrape), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}),
                h.ptr, pointer(x), J, Gp, pointer(tau), pointer(psiT))
            check(h, rc)
            J_b = 0.0
            if has_gb                                                      # J_parts[3] = λ_b Σ_k J_b,k, :764-766
                check(h, ccall((:grape_get_sums, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, sums))
                J_b = λ_b * sums[5]
                wrk.J_parts[3] = J_b
            end
            wrk.J_parts[1] = J[] - J_b                                     # :757-760
        else
            # user-supplied J_T / chi (optimize.jl:757-760, 845-855): forward on the device, J_T and χ(T) on the host,
            # backward sweep and gradient on the device from the χ the user's function returns
            check(h, GC.@preserve x tau h ccall((:grape_forward, libgrape), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}), h.ptr, pointer(x), pointer(tau)))
            check(h, ccall((:grape_get_final_states, libgrape), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}), h.ptr, psiT))
            Ψ = states()
            wrk.J_parts[1] = wrk.J_T_takes_tau ? J_T(Ψ, wrk.trajectories; tau = tau) : J_T(Ψ, wrk.trajectories)
            if has_gb
                check(h, ccall((:grape_get_sums, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, sums))
                wrk.J_parts[3] = λ_b * sums[5]
            end
            xi_route && (wrk.J_parts[3] = λ_b * J_b_and_xi!(!isnothing(G)))
            if !isnothing(G)
                χ = wrk.chi_takes_tau ? chi(Ψ, wrk.trajectories; tau = tau) : chi(Ψ, wrk.trajectories)
                for k = 1:K
                    chiT[:, k] .= χ[k]
                end
                if xi_route
                    check(h, GC.@preserve chiT xi_arr wrk h ccall((:grape_backward_xi, libgrape), Cint,
                        (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Cdouble, Ptr{Float64}),
                        h.ptr, C_NULL, pointer(chiT), pointer(xi_arr), λ_b, pointer(Gbuf)))
                else
                    check(h, GC.@preserve chiT wrk h ccall((:grape_backward_chi, libgrape), Cint,
                        (Ptr{Cvoid}, Ptr{ComplexF64}, Ptr{Float64}), h.ptr, pointer(chiT), pointer(Gbuf)))
                end
            end
        end
        for k in h.no_target                                               # :753 -- only the trajectories without a target
            tau[k] = NaN
        end
        (pseudo && !isnothing(G)) && copyto!(wrk.grad_J_Tb, 1, h.G_full, 1, h.L * h.N_T)
        if !isnothing(J_a)
            wrk.J_parts[2] = λₐ * J_a(wrk.pulsevals, tlist)                # :761-763
        end
        for k = 1:K
            copyto!(wrk.fw_propagators[k].state, view(psiT, :, k))         # read by update_result! :187-189
        end
        if !isnothing(G)
            copyto!(G, wrk.grad_J_Tb)                                      # :1002-1003
            if !isnothing(grad_J_a)                                        # :1004-1011
                wrk.grad_J_a = grad_J_a(wrk.pulsevals, tlist)
                axpy!(λₐ, wrk.grad_J_a, G)
            end
        end
        return sum(wrk.J_parts)
    end
end


"""
    time_gradient!(dJdt, h)

`dJdt[n] = ∂J/∂Δt_n` (`length(dJdt) == N_T`) of the last evaluation with a gradient (grape_get_time_gradient, ABI v7), at
fixed per-interval pulse and shape values.  Shapes and pulses sampled on interval midpoints move with `Δt_n`: that chain
rule is the caller's, and so is the explicit weight term of a `g_b` handed over as data (grape_backward_xi).  Grid-point
form: `∂J/∂t_j = dJdt[j] - dJdt[j+1]`; duration of a scaled grid: `dJ/dT = sum(Δt .* dJdt) / T`.
"""
function time_gradient!(dJdt::Vector{Float64}, h::Handle)
    length(dJdt) == h.N_T || throw(DimensionMismatch("dJdt must have N_T = $(h.N_T) entries"))
    check(h, GC.@preserve dJdt ccall((:grape_get_time_gradient, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, dJdt))
    return dJdt
end

"""
    set_tlist!(h, tlist)

A new time grid for the handle (grape_set_tlist, ABI v7): same `N_T`, strictly increasing and finite; the next `fg!` call
evaluates on it.  The pulses stay per interval: resampling them (and `wrk.tlist`) is the caller's.
"""
function set_tlist!(h::Handle, tlist::AbstractVector{Float64})
    length(tlist) == h.N_T + 1 || throw(DimensionMismatch("tlist must have N_T + 1 = $(h.N_T + 1) points"))
    t = collect(Float64, tlist)
    check(h, GC.@preserve t ccall((:grape_set_tlist, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, t))
    return h
end

"""
    eval_batch!(h, J, G, tau, pulsevals)

`P = size(pulsevals, 2)` pulse vectors through the problem of `h` in ONE call (grape_eval_batch): column `p` of the
`L*N_T × P` matrix `pulsevals` is one `wrk.pulsevals`; `J[p]`, `G[:, p]` (`G === nothing`: functional only) and
`tau[:, p]` (`K × P`, or `nothing`) are what `fg!` on that column returns.  For the multi-start loop of INTEGRATION.md 3c:
P optimiser states, one call per round.  Small systems (N ≤ 16) run all sets side by side on the GPU (`batch_info(h).route
== 1`); everything else takes one ordinary evaluation per set inside the library.  The outputs of `h`'s getters
(`time_gradient!`, stored states) are not defined after a batch call.
"""
function eval_batch!(h::Handle, J::Vector{Float64}, G::Union{Nothing,Matrix{Float64}}, tau::Union{Nothing,Matrix{ComplexF64}},
                     pulsevals::Matrix{Float64})
    P = size(pulsevals, 2)
    # (pseudo-controls -- time-dependent drift terms carried as fixed controls, see problem_arrays -- would have to be
    # appended to every column: not offered here)
    isempty(h.fixed) || error("GrapeHIP.eval_batch!: handles with pseudo-controls evaluate one pulse vector at a time (fg!)")
    size(pulsevals, 1) == h.L * h.N_T || throw(DimensionMismatch("pulsevals must be L*N_T = $(h.L * h.N_T) × P"))
    length(J) == P || throw(DimensionMismatch("J must have one entry per pulse vector ($P)"))
    isnothing(G) || size(G) == size(pulsevals) || throw(DimensionMismatch("G must have the size of pulsevals"))
    isnothing(tau) || size(tau, 2) == P || throw(DimensionMismatch("tau must be K × $P"))
    Gp = isnothing(G) ? Ptr{Float64}(C_NULL) : pointer(G)
    tp = isnothing(tau) ? Ptr{ComplexF64}(C_NULL) : pointer(tau)
    check(h, GC.@preserve J G tau pulsevals ccall((:grape_eval_batch, libgrape), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{ComplexF64}), h.ptr, P, pulsevals, J, Gp, tp))
    return J
end

"""
    batch_info(h)

What the last `eval_batch!` did (grape_get_batch_info): `route` (1: batched kernels, 0: one ordinary evaluation per set),
`sets_per_group`, `groups`, `bytes` of batch storage held by the handle.
"""
function batch_info(h::Handle)
    out = zeros(Float64, 4)
    GC.@preserve out ccall((:grape_get_batch_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), h.ptr, out, 4)
    return (route = Int(out[1]), sets_per_group = Int(out[2]), groups = Int(out[3]), bytes = Int(out[4]))
end

"""
    hvp!(HV, h, V)

Exact Hessian-vector products of `J` at the pulses of the last evaluation of `h` (grape_hvp): `HV[:, j] = (∂²J/∂ϵ²) V[:, j]` for
the columns of the `L*N_T × nv` matrix `V` (vectors: one direction), all directions in one call.  What a Newton-CG or
trust-region solver passes as its Hessian operator (`Optim.TwiceDifferentiableHV`, `hv!(Hv, x, v)`: call `fg!` at `x` first).
Valid after `fg!` (with or without gradient) or `grape_forward` on the current time grid, for the built-in functionals on one
device, `N ≤ 64`; everything else is refused with a message (include/grape_hip.h).
"""
function hvp!(HV::VecOrMat{Float64}, h::Handle, V::VecOrMat{Float64})
    isempty(h.fixed) || error("GrapeHIP.hvp!: handles with pseudo-controls are not supported (the directions have no entries for them)")
    size(V, 1) == h.L * h.N_T || throw(DimensionMismatch("V must be L*N_T = $(h.L * h.N_T) × nv"))
    size(HV) == size(V) || throw(DimensionMismatch("HV must have the size of V"))
    nv = size(V, 2)
    nv >= 1 || throw(DimensionMismatch("V must hold at least one direction"))
    check(h, GC.@preserve HV V ccall((:grape_hvp, libgrape), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), h.ptr, nv, V, HV))
    return HV
end

"""
    hvp_info(h)

What the last `hvp!` did (grape_get_hvp_info): series `terms` and (sub-)`steps` summed over the workgroups of both sweeps,
directions per launch group, `bytes` of storage held by the handle, milliseconds of the call.
"""
function hvp_info(h::Handle)
    out = zeros(Float64, 5)
    GC.@preserve out ccall((:grape_get_hvp_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), h.ptr, out, 5)
    return (terms = Int(out[1]), steps = Int(out[2]), dirs_per_group = Int(out[3]), bytes = Int(out[4]), ms = out[5])
end

"""
    hessian!(H, h)

The exact Hessian of `J` at the pulses of the last evaluation of `h` as a matrix (grape_hessian): `H` is `L*N_T × L*N_T`, indexed
as the gradient, both triangles filled and bitwise symmetric; column `q` is what `hvp!` returns for the unit direction `e_q`.
What Newton-Raphson / RFO with a regularised Hessian or `Optim.NewtonTrustRegion` (`h!(H, x)`: call `fg!` at `x` first) take.
Valid where `hvp!` is valid, for `L ≤ 4` and `L*N_T ≤ 8192`; everything else is refused with a message (include/grape_hip.h).
"""
function hessian!(H::Matrix{Float64}, h::Handle)
    isempty(h.fixed) || error("GrapeHIP.hessian!: handles with pseudo-controls are not supported (the matrix has no entries for them)")
    size(H) == (h.L * h.N_T, h.L * h.N_T) || throw(DimensionMismatch("H must be L*N_T × L*N_T = $(h.L * h.N_T) × $(h.L * h.N_T)"))
    check(h, GC.@preserve H ccall((:grape_hessian, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, H))
    return H
end

"""
    hessian_info(h)

What the last `hessian!` did (grape_get_hessian_info): series `terms` and (sub-)`steps` summed over all workgroups, trajectories
per pass, `bytes` of storage held by the handle, milliseconds of the call, and the series terms of the forward seeds, the
backward seeds and the fan.
"""
function hessian_info(h::Handle)
    out = zeros(Float64, 8)
    GC.@preserve out ccall((:grape_get_hessian_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), h.ptr, out, 8)
    return (terms = Int(out[1]), steps = Int(out[2]), traj_per_pass = Int(out[3]), bytes = Int(out[4]), ms = out[5],
            terms_forward_seeds = Int(out[6]), terms_backward_seeds = Int(out[7]), terms_fan = Int(out[8]))
end

"""
    expect!(out, h, ops)

Expectation values of operator observables on the stored forward states of the last evaluation of `h`, computed on the device
(grape_expect): what the reference hands to `cb(propagator, observables)` after every `prop_step!` of its forward sweep
(src/optimize.jl:733-737), without moving the states to the host.  `ops` is `N × N × M` (one set of operators for all
trajectories) or `N × N × M × K` (Julia's column-major layout is the ABI's: no copy), `1 ≤ M ≤ 16`, not necessarily Hermitian;
`out` is `M × (N_T+1) × K` with `out[m, n, k] = ⟨Ψ_k(t_{n-1})|O_m|Ψ_k(t_{n-1})⟩` (`tr(O_m ρ_k)` on an open-system handle, `N = d`);
`out[:, 1, k]` belongs to the initial state.  Valid after `fg!` (with or without gradient) or `grape_forward` on the current
time grid; everything else is refused with a message (include/grape_hip.h).
"""
function expect!(out::Array{ComplexF64,3}, h::Handle, ops::Array{ComplexF64})
    ndims(ops) in (3, 4) || throw(DimensionMismatch("ops must be N × N × M or N × N × M × K"))
    size(ops, 1) == h.N && size(ops, 2) == h.N || throw(DimensionMismatch("ops must hold N × N = $(h.N) × $(h.N) matrices"))
    ndims(ops) == 3 || size(ops, 4) == h.K || throw(DimensionMismatch("ops per trajectory need K = $(h.K) sets"))
    M = size(ops, 3)
    size(out) == (M, h.N_T + 1, h.K) || throw(DimensionMismatch("out must be M × (N_T+1) × K = $M × $(h.N_T + 1) × $(h.K)"))
    check(h, GC.@preserve out ops ccall((:grape_expect, libgrape), Cint, (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Cint, Ptr{ComplexF64}),
                                        h.ptr, M, ops, ndims(ops) == 4 ? 1 : 0, out))
    return out
end

"""
    expect_info(h)

What the last `expect!` did (grape_get_expect_info): its `M`, `bytes` the feature holds on the device, milliseconds of the call
(host wall time, copies included), `mfma_flop` of the matrix instructions (0 on an open-system handle).
"""
function expect_info(h::Handle)
    out = zeros(Float64, 4)
    GC.@preserve out ccall((:grape_get_expect_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), h.ptr, out, 4)
    return (M = Int(out[1]), bytes = Int(out[2]), ms = out[3], mfma_flop = out[4])
end

"""
    hvp_forward!(h, V; dtau=nothing, dsums=nothing, dpsiT=nothing)

First half of a split Hessian-vector product (grape_hvp_forward): the tangent forward sweep of the columns of the `L*N_T × nv`
matrix `V` at the pulses of the last evaluation.  All directions stay on the device for `hvp_backward!` / `hvp_backward_chi!`.
Filled where given: `dtau` (`K × nv` complex, `τ′ₖ = ⟨tgtₖ|Ψ′ₖ(T)⟩`), `dsums` (`nv` complex, `Σₖ wₖ τ′ₖ` over THIS handle's
trajectories: what a sharded caller all-reduces) and `dpsiT` (`N × K × nv` complex, `Ψ′ₖ(T)`: what a caller's `χ′` is formed
from).  This is the route for trajectory shards (`K < K_total`) and for a functional of the caller's, which `hvp!` refuses.
"""
function hvp_forward!(h::Handle, V::VecOrMat{Float64}; dtau::Union{Nothing,VecOrMat{ComplexF64}}=nothing,
                      dsums::Union{Nothing,Vector{ComplexF64}}=nothing, dpsiT::Union{Nothing,Array{ComplexF64}}=nothing)
    isempty(h.fixed) || error("GrapeHIP.hvp_forward!: handles with pseudo-controls are not supported (the directions have no entries for them)")
    size(V, 1) == h.L * h.N_T || throw(DimensionMismatch("V must be L*N_T = $(h.L * h.N_T) × nv"))
    nv = size(V, 2)
    nv >= 1 || throw(DimensionMismatch("V must hold at least one direction"))
    isnothing(dtau) || length(dtau) == h.K * nv || throw(DimensionMismatch("dtau must be K × nv"))
    isnothing(dsums) || length(dsums) == nv || throw(DimensionMismatch("dsums must hold nv sums"))
    isnothing(dpsiT) || length(dpsiT) == h.N * h.K * nv || throw(DimensionMismatch("dpsiT must be N × K × nv"))
    ptr(a) = isnothing(a) ? Ptr{ComplexF64}(C_NULL) : pointer(a)
    check(h, GC.@preserve V dtau dsums dpsiT ccall((:grape_hvp_forward, libgrape), Cint,
          (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}), h.ptr, nv, V, ptr(dtau), ptr(dsums), ptr(dpsiT)))
    return nothing
end

"""
    hvp_backward!(HV, h, f_total, df_total)

Second half for the built-in functional (grape_hvp_backward): `f_total` the all-reduced `Σₖ wₖ τₖ` of the evaluation (as for
`grape_backward`), `df_total` (`nv` complex) the all-reduced `dsums` of `hvp_forward!`.  `HV` (`L*N_T × nv`) is the sum over
this handle's trajectories: all-reduce it like the gradient when `K < K_total`.
"""
function hvp_backward!(HV::VecOrMat{Float64}, h::Handle, f_total::Number, df_total::Vector{ComplexF64})
    size(HV, 1) == h.L * h.N_T || throw(DimensionMismatch("HV must be L*N_T = $(h.L * h.N_T) × nv"))
    nv = size(HV, 2)
    length(df_total) == nv || throw(DimensionMismatch("df_total must hold nv = $nv sums"))
    f = ComplexF64[f_total]
    check(h, GC.@preserve HV f df_total ccall((:grape_hvp_backward, libgrape), Cint,
          (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}), h.ptr, nv, f, df_total, HV))
    return HV
end

"""
    hvp_backward_chi!(HV, h, chi, dchi)

Second half for a functional of the caller's (grape_hvp_backward_chi): `chi` (`N × K`) as for `grape_backward_chi`, not
normalised, and `dchi` (`N × K × nv`) its derivative along each direction of the last `hvp_forward!` -- from AD of `χ` along
`Ψ′ₖ(T)`, as `χ` itself usually comes from AD of `J_T`.  The only route on handles without targets.
"""
function hvp_backward_chi!(HV::VecOrMat{Float64}, h::Handle, chi::Matrix{ComplexF64}, dchi::Array{ComplexF64})
    size(HV, 1) == h.L * h.N_T || throw(DimensionMismatch("HV must be L*N_T = $(h.L * h.N_T) × nv"))
    nv = size(HV, 2)
    size(chi) == (h.N, h.K) || throw(DimensionMismatch("chi must be N × K"))
    length(dchi) == h.N * h.K * nv || throw(DimensionMismatch("dchi must be N × K × nv"))
    check(h, GC.@preserve HV chi dchi ccall((:grape_hvp_backward_chi, libgrape), Cint,
          (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}), h.ptr, nv, chi, dchi, HV))
    return HV
end


# ---- open quantum systems (include/grape_hip.h: grape_create_open; INTEGRATION.md 3d) ---------------------------------------

# mirror of `grape_lindblad`
struct GrapeLindblad
    J::Int32                 # collapse operators, 0 <= J <= 8
    cops_per_traj::Int32     # 0: cops is [J] matrices shared by all trajectories; 1: [K][J]
    cops::Ptr{ComplexF64}    # column-major, rates folded in; C_NULL iff J == 0
end

"""
    h = create_open(H0, Hc, cops, tlist, rho0, target; functional = 0, weights = nothing, shape = nothing, K_total = 0, device = 0)

A handle whose states are `d × d` density matrices propagated in matrix form under the Lindblad generator
`𝓛(ρ) = −i(H_eff ρ − ρ H_eff†) + Σ_j A_j ρ A_j†`, `H_eff = H − (i/2) Σ_j A_j†A_j`.  `H0`: vector of `K` matrices; `Hc`: vector of `L`
matrices (shared) or vector of `K` such vectors; `cops`: vector of `J` matrices `A_j = √γ_j a_j` (shared), vector of `K` such
vectors, or empty; `rho0`, `target`: vectors of `K` matrices (`target = nothing`: only `grape_forward` +
`grape_get_final_states` + `grape_backward_chi`).  The returned `Handle` works with `make_fg!`-style calls of `grape_eval`;
states come back as `d*d` column-major blocks, i.e. `reshape(·, d, d)`.
"""
function create_open(H0, Hc, cops, tlist, rho0, target; functional = 0, weights = nothing, shape = nothing, K_total = 0, device = 0)
    K, N = length(H0), size(H0[1], 1)
    hc_per_traj = !(Hc[1] isa AbstractMatrix)
    L = hc_per_traj ? length(Hc[1]) : length(Hc)
    cops_per_traj = !isempty(cops) && !(cops[1] isa AbstractMatrix)
    J = isempty(cops) ? 0 : (cops_per_traj ? length(cops[1]) : length(cops))
    t = Vector{Float64}(tlist)
    N_T = length(t) - 1
    cat(ms) = reduce(hcat, [vec(Matrix{ComplexF64}(m)) for m in ms])
    H0f = cat(H0)
    Hcf = hc_per_traj ? reduce(hcat, [cat(Hc[k]) for k = 1:K]) : cat(Hc)
    Af = J == 0 ? nothing : (cops_per_traj ? reduce(hcat, [cat(cops[k]) for k = 1:K]) : cat(cops))
    r0 = cat(rho0)
    tg = isnothing(target) ? nothing : cat(target)
    w = isnothing(weights) ? nothing : Vector{Float64}(weights)
    shp = isnothing(shape) ? nothing : Matrix{Float64}(shape)               # [N_T, L] column-major == [l][n]
    keep = Any[H0f, Hcf, Af, r0, tg, t, w, shp]
    prob = Ref(GrapeProblem(
        ABI_VERSION, N, L, K, K_total, N_T, functional, 0, hc_per_traj ? 1 : 0, device,
        pointer(t), pointer(H0f), pointer(Hcf), isnothing(shp) ? C_NULL : pointer(shp), pointer(r0), isnothing(tg) ? C_NULL : pointer(tg),
        isnothing(w) ? C_NULL : pointer(w), 0.0, 0, 0.0, C_NULL, 0, 0.0, 0, 0.0, 0, C_NULL, 0))
    diss = Ref(GrapeLindblad(J, cops_per_traj ? 1 : 0, isnothing(Af) ? C_NULL : pointer(Af)))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve keep ccall((:grape_create_open, libgrape), Cint, (Ref{Ptr{Cvoid}}, Ref{GrapeProblem}, Ref{GrapeLindblad}), out, prob, diss)
    rc == 0 || error(last_error(C_NULL))
    h = Handle(out[], keep, K, N * N, functional, isnothing(target) ? collect(1:K) : Int[], L, N_T, Float64[], zeros(Float64, L * N_T), zeros(Float64, L * N_T))
    finalizer(x -> ccall((:grape_destroy, libgrape), Cvoid, (Ptr{Cvoid},), x.ptr), h)
    return h
end

"""
    open_time_gradient!(dJdt, h)

`dJdt[n] = ∂J/∂Δt_n` (`length(dJdt) == N_T`) for a handle made by `create_open` (grape_open_time_gradient): the call of the
duration loop of INTEGRATION.md 3b on an open system, where the optimal duration is an interior optimum.  A function of its
own, not a method of `time_gradient!`: `Handle` does not record which constructor made it, and the library refuses
`grape_get_time_gradient` on such a handle (and this call on a closed one) with a message.  Valid after `fg!` with a gradient,
`grape_backward` or `grape_backward_chi` (then with the caller's `χ_k(T)`) on the current grid; fixed per-interval pulse and
shape values, grid-point form and `dJ/dT` as for `time_gradient!`.
"""
function open_time_gradient!(dJdt::Vector{Float64}, h::Handle)
    length(dJdt) == h.N_T || throw(DimensionMismatch("dJdt must have N_T = $(h.N_T) entries"))
    check(h, GC.@preserve dJdt ccall((:grape_open_time_gradient, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, dJdt))
    return dJdt
end

"""
    open_hvp!(HV, h, V)

Exact Hessian-vector products `HV[:, j] = (∂²J/∂ε²) V[:, j]` for a handle made by `create_open` (grape_open_hvp), at the pulses
of the last evaluation: `V`, `HV` are `L*N_T × nv` (or vectors of length `L*N_T`), control-major like the pulse vector.  All
directions run side by side on the GPU.  A function of its own, as `open_time_gradient!` is: the library refuses `grape_hvp`
on such a handle (and this call on a closed one) with a message.  Valid after `fg!` (with or without gradient) or
`grape_forward` on the current time grid, for the built-in functionals with `K == K_total`.
"""
function open_hvp!(HV::VecOrMat{Float64}, h::Handle, V::VecOrMat{Float64})
    isempty(h.fixed) || error("GrapeHIP.open_hvp!: handles with pseudo-controls are not supported (the directions have no entries for them)")
    size(V, 1) == h.L * h.N_T || throw(DimensionMismatch("V must be L*N_T = $(h.L * h.N_T) × nv"))
    size(HV) == size(V) || throw(DimensionMismatch("HV must have the size of V"))
    nv = size(V, 2)
    nv >= 1 || throw(DimensionMismatch("V must hold at least one direction"))
    check(h, GC.@preserve HV V ccall((:grape_open_hvp, libgrape), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}), h.ptr, nv, V, HV))
    return HV
end

"""
    open_hvp_info(h)

What the last `open_hvp!` did (grape_get_open_hvp_info): series `terms` and (sub-)`steps` summed over the workgroups of both
sweeps, directions per launch group, `bytes` of storage held by the handle, milliseconds of the call, and the terms of the
tangent forward / the backward sweeps.
"""
function open_hvp_info(h::Handle)
    out = zeros(Float64, 7)
    GC.@preserve out ccall((:grape_get_open_hvp_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), h.ptr, out, 7)
    return (terms = Int(out[1]), steps = Int(out[2]), dirs_per_group = Int(out[3]), bytes = Int(out[4]), ms = out[5],
            terms_forward = Int(out[6]), terms_backward = Int(out[7]))
end

"""
    open_hessian!(H, h)

The exact Hessian of `J` at the pulses of the last evaluation of a handle made by `create_open`, as a matrix
(grape_open_hessian): `H` is `L*N_T × L*N_T`, indexed like the gradient, both triangles, bitwise symmetric.  Column `q` is what
`open_hvp!` gives for the unit direction `e_q`, to rounding.  Valid whenever `open_hvp!` is, for `L ≤ 4` and `L*N_T ≤ 8192`.
"""
function open_hessian!(H::Matrix{Float64}, h::Handle)
    isempty(h.fixed) || error("GrapeHIP.open_hessian!: handles with pseudo-controls are not supported (the matrix has no entries for them)")
    size(H) == (h.L * h.N_T, h.L * h.N_T) || throw(DimensionMismatch("H must be L*N_T × L*N_T = $(h.L * h.N_T) × $(h.L * h.N_T)"))
    check(h, GC.@preserve H ccall((:grape_open_hessian, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, H))
    return H
end

"""
    open_hessian_info(h)

What the last `open_hessian!` did (grape_get_open_hessian_info): series `terms` and (sub-)`steps` summed over all workgroups,
trajectories per pass, `bytes` of storage held by the handle, milliseconds of the call, and terms and steps of the forward
seeds, the backward seeds and the fan, and the columns per workgroup of the fan.
"""
function open_hessian_info(h::Handle)
    out = zeros(Float64, 12)
    GC.@preserve out ccall((:grape_get_open_hessian_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), h.ptr, out, 12)
    return (terms = Int(out[1]), steps = Int(out[2]), traj_per_pass = Int(out[3]), bytes = Int(out[4]), ms = out[5],
            terms_forward_seeds = Int(out[6]), terms_backward_seeds = Int(out[7]), terms_fan = Int(out[8]),
            steps_forward_seeds = Int(out[9]), steps_backward_seeds = Int(out[10]), steps_fan = Int(out[11]), fan_columns = Int(out[12]))
end

"""
    open_hvp_forward!(h, V; dtau=nothing, dsums=nothing, drhoT=nothing)

First half of a split Hessian-vector product on a handle made by `create_open` (grape_open_hvp_forward): the tangent forward
sweep of the columns of the `L*N_T × nv` matrix `V` at the pulses of the last forward half.  All directions stay on the device
for `open_hvp_backward!` / `open_hvp_backward_chi!`.  Filled where given: `dtau` (`K × nv` complex, `τ′ₖ = ⟨⟨σₖ|ρ′ₖ(T)⟩⟩`),
`dsums` (`nv` complex, `Σₖ wₖ τ′ₖ` over THIS handle's trajectories: what a sharded caller all-reduces) and `drhoT`
(`N × N × K × nv` complex, `ρ′ₖ(T)`: what a caller's `χ′` is formed from).  This is the route for trajectory shards
(`K < K_total`) and for a functional of the caller's, which `open_hvp!` refuses.
"""
function open_hvp_forward!(h::Handle, V::VecOrMat{Float64}; dtau::Union{Nothing,VecOrMat{ComplexF64}}=nothing,
                           dsums::Union{Nothing,Vector{ComplexF64}}=nothing, drhoT::Union{Nothing,Array{ComplexF64}}=nothing)
    isempty(h.fixed) || error("GrapeHIP.open_hvp_forward!: handles with pseudo-controls are not supported (the directions have no entries for them)")
    size(V, 1) == h.L * h.N_T || throw(DimensionMismatch("V must be L*N_T = $(h.L * h.N_T) × nv"))
    nv = size(V, 2)
    nv >= 1 || throw(DimensionMismatch("V must hold at least one direction"))
    isnothing(dtau) || length(dtau) == h.K * nv || throw(DimensionMismatch("dtau must be K × nv"))
    isnothing(dsums) || length(dsums) == nv || throw(DimensionMismatch("dsums must hold nv sums"))
    isnothing(drhoT) || length(drhoT) == h.N * h.N * h.K * nv || throw(DimensionMismatch("drhoT must be N × N × K × nv"))
    ptr(a) = isnothing(a) ? Ptr{ComplexF64}(C_NULL) : pointer(a)
    check(h, GC.@preserve V dtau dsums drhoT ccall((:grape_open_hvp_forward, libgrape), Cint,
          (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{ComplexF64}), h.ptr, nv, V, ptr(dtau), ptr(dsums), ptr(drhoT)))
    return nothing
end

"""
    open_hvp_backward!(HV, h, f_total, df_total)

Second half for the built-in functional (grape_open_hvp_backward): `f_total` the all-reduced `Σₖ wₖ τₖ` of the evaluation (as
for `grape_backward`), `df_total` (`nv` complex) the all-reduced `dsums` of `open_hvp_forward!`.  `HV` (`L*N_T × nv`) is the sum
over this handle's trajectories: all-reduce it like the gradient when `K < K_total`.
"""
function open_hvp_backward!(HV::VecOrMat{Float64}, h::Handle, f_total::Number, df_total::Vector{ComplexF64})
    size(HV, 1) == h.L * h.N_T || throw(DimensionMismatch("HV must be L*N_T = $(h.L * h.N_T) × nv"))
    nv = size(HV, 2)
    length(df_total) == nv || throw(DimensionMismatch("df_total must hold nv = $nv sums"))
    f = ComplexF64[f_total]
    check(h, GC.@preserve HV f df_total ccall((:grape_open_hvp_backward, libgrape), Cint,
          (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}), h.ptr, nv, f, df_total, HV))
    return HV
end

"""
    open_hvp_backward_chi!(HV, h, chi, dchi)

Second half for a functional of the caller's (grape_open_hvp_backward_chi): `chi` (`N × N × K`) as for `grape_backward_chi` on
an open handle, not normalised, and `dchi` (`N × N × K × nv`) its derivative along each direction of the last
`open_hvp_forward!` -- from AD of `χ` along `ρ′ₖ(T)`, as `χ` itself usually comes from AD of `J_T`.  The only route on handles
without targets.
"""
function open_hvp_backward_chi!(HV::VecOrMat{Float64}, h::Handle, chi::Array{ComplexF64,3}, dchi::Array{ComplexF64})
    size(HV, 1) == h.L * h.N_T || throw(DimensionMismatch("HV must be L*N_T = $(h.L * h.N_T) × nv"))
    nv = size(HV, 2)
    size(chi) == (h.N, h.N, h.K) || throw(DimensionMismatch("chi must be N × N × K"))
    length(dchi) == h.N * h.N * h.K * nv || throw(DimensionMismatch("dchi must be N × N × K × nv"))
    check(h, GC.@preserve HV chi dchi ccall((:grape_open_hvp_backward_chi, libgrape), Cint,
          (Ptr{Cvoid}, Cint, Ptr{ComplexF64}, Ptr{ComplexF64}, Ptr{Float64}), h.ptr, nv, chi, dchi, HV))
    return HV
end

"""
    open_eval_batch!(h, J, G, tau, pulsevals)

`P = size(pulsevals, 2)` pulse vectors through the problem of a handle made by `create_open`, side by side on the GPU
(grape_open_eval_batch): arguments as `eval_batch!`.  Column `p` is what `fg!` on that column returns, to rounding, and does not
depend on the other columns, bit for bit.  Unlike `eval_batch!` on such a handle (one ordinary evaluation per set), the call
owns its buffers: the handle's last ordinary evaluation stays defined (`open_time_gradient!`, `open_hvp!`, stored states).
Multi-start, populations, line-search trial points, amplitude scans: up to `256 ÷ (K*L)` evaluations for the time of one.
"""
function open_eval_batch!(h::Handle, J::Vector{Float64}, G::Union{Nothing,Matrix{Float64}}, tau::Union{Nothing,Matrix{ComplexF64}},
                          pulsevals::Matrix{Float64})
    P = size(pulsevals, 2)
    # (pseudo-controls would have to be appended to every column: not offered here, as in eval_batch!)
    isempty(h.fixed) || error("GrapeHIP.open_eval_batch!: handles with pseudo-controls evaluate one pulse vector at a time (fg!)")
    size(pulsevals, 1) == h.L * h.N_T || throw(DimensionMismatch("pulsevals must be L*N_T = $(h.L * h.N_T) × P"))
    length(J) == P || throw(DimensionMismatch("J must have one entry per pulse vector ($P)"))
    isnothing(G) || size(G) == size(pulsevals) || throw(DimensionMismatch("G must have the size of pulsevals"))
    isnothing(tau) || size(tau, 2) == P || throw(DimensionMismatch("tau must be K × $P"))
    Gp = isnothing(G) ? Ptr{Float64}(C_NULL) : pointer(G)
    tp = isnothing(tau) ? Ptr{ComplexF64}(C_NULL) : pointer(tau)
    check(h, GC.@preserve J G tau pulsevals ccall((:grape_open_eval_batch, libgrape), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{ComplexF64}), h.ptr, P, pulsevals, J, Gp, tp))
    return J
end

"""
    open_batch_info(h)

What the last `open_eval_batch!` did (grape_get_open_batch_info): `sets_per_group`, `groups`, `bytes` of batch storage held by
the handle, milliseconds of the call, series terms of the forward and of the backward sweeps and (sub-)`steps`, summed over all
workgroups of the call.
"""
function open_batch_info(h::Handle)
    out = zeros(Float64, 7)
    GC.@preserve out ccall((:grape_get_open_batch_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), h.ptr, out, 7)
    return (sets_per_group = Int(out[1]), groups = Int(out[2]), bytes = Int(out[3]), ms = out[4], terms_forward = Int(out[5]),
            terms_backward = Int(out[6]), steps = Int(out[7]))
end

"""
    open_set_running_cost!(h, D, lambda_b)

Install the state running cost `g_b(ρ) = Re tr(D ρ)` with weight `lambda_b` on a handle made by `create_open`
(grape_open_set_running_cost), or remove it (`D === nothing` or `lambda_b == 0`).  `D`: one `d × d` matrix shared by all
trajectories or a vector of `K` of them (a projector on leakage levels penalises their population during the pulse).  While
the cost is set `fg!` returns `J_T + λ_b J_b` and its gradient, and `grape_get_sums[5]` holds `Σ_k J_b,k`; the next call has to
be a forward evaluation.  `open_time_gradient!`, `open_hvp!` and `open_eval_batch!` refuse while the cost is in effect.
"""
function open_set_running_cost!(h::Handle, D::Union{Nothing,AbstractMatrix,AbstractVector{<:AbstractMatrix}}, lambda_b::Real)
    if isnothing(D)
        check(h, ccall((:grape_open_set_running_cost, libgrape), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Cint, Cdouble), h.ptr, C_NULL, 0, 0.0))
        return h
    end
    per_traj = D isa AbstractVector
    per_traj && length(D) != h.K && throw(DimensionMismatch("D must hold one matrix per trajectory ($(h.K))"))
    Df = per_traj ? ComplexF64.(reduce(hcat, vec.(D))) : ComplexF64.(vec(D))
    length(Df) == h.N * (per_traj ? h.K : 1) || throw(DimensionMismatch("every D must be d × d with d^2 = $(h.N)"))
    check(h, GC.@preserve Df ccall((:grape_open_set_running_cost, libgrape), Cint, (Ptr{Cvoid}, Ptr{ComplexF64}, Cint, Cdouble),
        h.ptr, Df, per_traj ? 1 : 0, Float64(lambda_b)))
    return h
end

"""
    open_backward_xi!(G, h, xi, lambda_b; f_total = nothing, chi = nothing)

The backward half with the inhomogeneity of an arbitrary state running cost on a handle made by `create_open`
(grape_open_backward_xi): `xi` is `d^2 × (N_T+1) × K` (column `[:, n+1, k]` is `vec(ξ_k(t_n))`, defined by
`dg_b = -2 Re⟨⟨ξ|dρ⟩⟩` and evaluated by the caller on the stored states; `n = 0` is not read), `chi` is `nothing` (the
handle's functional with `f_total = Σ_k w_k τ_k`) or `d^2 × K`, the caller's `χ_k(T)`.  `G` receives the gradient of
`J_T + λ_b J_b`; `J_b` itself stays the caller's.  A function of its own: the library refuses `grape_backward_xi` on such a
handle (and this call on a closed one) with a message.
"""
function open_backward_xi!(G::Vector{Float64}, h::Handle, xi::Array{ComplexF64,3}, lambda_b::Real;
                           f_total::Union{Nothing,Complex} = nothing, chi::Union{Nothing,Matrix{ComplexF64}} = nothing)
    size(xi) == (h.N, h.N_T + 1, h.K) || throw(DimensionMismatch("xi must be d^2 × (N_T+1) × K = $(h.N) × $(h.N_T + 1) × $(h.K)"))
    length(G) == h.L * h.N_T || throw(DimensionMismatch("G must have L*N_T = $(h.L * h.N_T) entries"))
    isnothing(chi) || size(chi) == (h.N, h.K) || throw(DimensionMismatch("chi must be d^2 × K"))
    isnothing(chi) && isnothing(f_total) && error("GrapeHIP.open_backward_xi!: either f_total or chi")
    f = isnothing(f_total) ? Float64[0.0, 0.0] : Float64[real(f_total), imag(f_total)]
    cp = isnothing(chi) ? Ptr{ComplexF64}(C_NULL) : pointer(chi)
    check(h, GC.@preserve G xi f chi ccall((:grape_open_backward_xi, libgrape), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ptr{ComplexF64}, Cdouble, Ptr{Float64}),
        h.ptr, f, cp, xi, Float64(lambda_b), G))
    return G
end

end # module
