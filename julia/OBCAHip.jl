# OBCAHip.jl -- thin Julia shim (Julia >= 1.6) over libobca_hip.so.
#
# Drop-in replacements, with the reference's positional signatures and return tuples, for
#   ParkingSignedDist(x0,xF,N,Ts,L,ego,XYbounds,nOb,vOb,A,b,rx,ry,ryaw,fixTime,xWS,uWS)   (AutonomousParking/ParkingSignedDist.jl:29)
#   DualMultWS(N,nOb,vOb,A,b,rx,ry,ryaw)                                                   (AutonomousParking/DualMultWS.jl:29)
#   ParkingDist(...)                                                                       (AutonomousParking/ParkingDist.jl:29)
#   QuadcopterSignedDist(x0,xF,N,Ts,R,ob1,ob2,ob3,ob4,ob5,xWS,uWS,timeWS)                  (QuadcopterNavigation/QuadcopterSignedDist.jl:25)
#   QuadcopterDist(...)                                                                    (QuadcopterNavigation/QuadcopterDist.jl:25)
#   ParkingConstraints(x0,xF,N,Ts,L,ego,XYbounds,nOb,vOb,A,b,x,u,l,n,timeScale,fixTime,sd) (AutonomousParking/ParkingConstraints.jl:29)
#   constrSatisfaction(x,u,timeScale,x0,xF,Ts,lambda,ob1,ob2,ob3,ob4,ob5,R)                (QuadcopterNavigation/constrSatisfaction.jl:25)
# plus batched variants and multi-GPU contexts.  Julia arrays are column-major, which is exactly the "stage-contiguous" layout of the C ABI
# (include/obca_hip.h), so every array is passed with zero copies.
#
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; the
# same C entry points are exercised through ctypes by tests/test_gpu_parity.py.
module OBCAHip

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
# One hardware queue per stream: the HIP runtime's default of four serialises streams that share one (the worker lanes of the host-pointer entry points, several contexts
# in flight).  Read by the runtime at its first call in the process; a value the caller has set stays.  (INTEGRATION.md, profiles/r06_hw_queues.txt)
function __init__()
    haskey(ENV, "GPU_MAX_HW_QUEUES") || (ENV["GPU_MAX_HW_QUEUES"] = "16")
end

mutable struct Context
    h::Ptr{Cvoid}
end

function Context(device::Integer=0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:obca_create, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint), r, device)
    rc == 0 || error("obca_create failed: " * unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    c = Context(r[])
    finalizer(x -> ccall((:obca_destroy, LIB), Cint, (Ptr{Cvoid},), x.h), c)
    return c
end

"Context over several GPUs of the node (all visible ones by default): the batched calls shard their batch over them (obca_create_multi)."
function MultiContext(devices::Vector{<:Integer}=Int[])
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:obca_create_multi, LIB), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cint}, Cint), r, isempty(devices) ? C_NULL : Cint.(devices), length(devices))
    rc == 0 || error("obca_create_multi failed: " * unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), C_NULL)))
    c = Context(r[])
    finalizer(x -> ccall((:obca_destroy, LIB), Cint, (Ptr{Cvoid},), x.h), c)
    return c
end
device_count(c::Context) = Int(ccall((:obca_device_count, LIB), Cint, (Ptr{Cvoid},), c.h))
"make every later call of this module use context `c` (e.g. `use!(MultiContext())` for all GPUs of the node)"
use!(c::Context) = (_ctx[] = c)

const _ctx = Ref{Union{Nothing,Context}}(nothing)
ctx() = (_ctx[] === nothing && (_ctx[] = Context(0)); _ctx[])
lasterr(c) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), c.h))

f64(a) = convert(Array{Float64}, a)

"""
Interior-point options: the record `obca_opts` of include/obca_hip.h, field for field.  `ipopt_opts()` = the reference's IPOPT configuration as far as the kernels carry it
(ParkingSignedDist.jl:41-43 incl. recalc_y = "yes", IPOPT's default second-order correction max_soc = 4 and least-squares initial multipliers): the default of the drop-ins
`ParkingSignedDist` / `ParkingDist`.  `default_opts()` = the library's throughput defaults (the three switches off: the same solved set, a quarter fewer GPU seconds, 1-18 % of the
instances of a batch end in another local solution -- include/obca_hip.h has the numbers): the default of the batched calls (`opts=nothing`).
"""
mutable struct Opts
    tol::Cdouble; max_iter::Cint
    mu_init::Cdouble; kappa_eps::Cdouble; kappa_mu::Cdouble; theta_mu::Cdouble; tau_min::Cdouble; bound_push::Cdouble; bound_frac::Cdouble
    dw_min::Cdouble; dw0::Cdouble; dw_max::Cdouble; kw_inc0::Cdouble; kw_inc::Cdouble; kw_dec::Cdouble; dc_bar::Cdouble; kappa_c::Cdouble
    gamma_theta::Cdouble; gamma_phi::Cdouble; delta::Cdouble; s_theta::Cdouble; s_phi::Cdouble; eta_phi::Cdouble; gamma_alpha::Cdouble; s_max::Cdouble; kappa_sigma::Cdouble
    constr_viol_tol::Cdouble; dual_inf_tol::Cdouble; compl_inf_tol::Cdouble; rho_term::Cdouble
    max_soc::Cint; recalc_y::Cint; lsq_init::Cint; obj_scaling::Cint; restoration::Cint
    Opts() = new()
end
function default_opts()
    o = Opts()
    ccall((:obca_default_opts, LIB), Cint, (Ref{Opts},), o) == 0 || error("obca_default_opts failed")
    return o
end
function ipopt_opts()
    o = Opts()
    ccall((:obca_reference_opts, LIB), Cint, (Ref{Opts},), o) == 0 || error("obca_reference_opts failed")
    return o
end
optsptr(o) = o === nothing ? C_NULL : pointer_from_objref(o)
"the reference's IPOPT configuration of the quadcopter call as far as the kernel carries it (max_soc = 4, least-squares initial multipliers, gradient-based objective scaling; recalc_y = \"no\" as QuadcopterSignedDist.jl:29 sets it): default of the quadcopter drop-ins"
function quadcopter_ipopt_opts()
    o = Opts()
    ccall((:obca_quadcopter_reference_opts, LIB), Cint, (Ref{Opts},), o) == 0 || error("obca_quadcopter_reference_opts failed")
    return o
end

"""
    ParkingSignedDist_batch(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS)

Batched form: x0, xF are 4xB; rx, ry, ryaw (N+1)xB; xWS 4x(N+1)xB (already transposed to the x layout); uWS 2xNxB; Ts a vector of
length B; the obstacle set (nOb, vOb, A (Mx2), b) is shared by the batch.  Returns (xp 4x(N+1)xB, up 2xNxB, timeScale (N+1)xB,
exitflag B, time, lp Mx(N+1)xB, np 4nObx(N+1)xB).
"""
function ParkingSignedDist_batch(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS; opts=nothing)
    B = size(x0, 2); M = sum(vOb)
    nObs = fill(Cint(nOb), B); vflat = repeat(Cint.(vec(vOb)), B)
    At = repeat(vec(permutedims(f64(A))), B)         # row k of A as (A[k,1], A[k,2]), per instance
    bt = repeat(vec(f64(b)), B)
    xp = zeros(4, N + 1, B); up = zeros(2, N, B); ts = zeros(N + 1, B); ef = zeros(Cint, B)
    lp = zeros(M, N + 1, B); np = zeros(4nOb, N + 1, B); info = zeros(8, B)
    t0 = time()
    rc = GC.@preserve opts ccall((:obca_parking_signed_dist_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}),
               ctx().h, B, N, f64(vec(Ts)), L, f64(vec(ego)), f64(vec(XYbounds)), fixTime, f64(x0), f64(xF), nObs, vflat, At, bt,
               f64(rx), f64(ry), f64(ryaw), f64(xWS), f64(uWS), C_NULL, C_NULL,   # lWS = nWS = NULL: DualMultWS runs on the GPU
               optsptr(opts), xp, up, ts, ef, lp, np, C_NULL, info)
    rc == 0 || error("obca_parking_signed_dist_batch failed: " * lasterr(ctx()))
    return xp, up, ts, ef, time() - t0, lp, np
end

"Drop-in for ParkingSignedDist.jl:29 (one instance): same arguments, same 7-tuple."
function ParkingSignedDist(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS; opts=ipopt_opts())      # default: the reference's IPOPT configuration; `default_opts()` = the library's throughput defaults
    xp, up, ts, ef, t, lp, np = ParkingSignedDist_batch(reshape(f64(vec(x0)), 4, 1), reshape(f64(vec(xF)), 4, 1), N, [Float64(Ts)], L, ego,
        XYbounds, nOb, vOb, A, b, reshape(f64(rx)[1:N+1], N + 1, 1), reshape(f64(ry)[1:N+1], N + 1, 1), reshape(f64(ryaw)[1:N+1], N + 1, 1),
        fixTime, reshape(permutedims(f64(xWS)[1:N+1, :]), 4, N + 1, 1), reshape(permutedims(f64(uWS)[1:N, :]), 2, N, 1); opts=opts)
    timeScalep = fixTime == 1 ? ones(1, N + 1) : ts[:, 1]          # ParkingSignedDist.jl:304-308
    return xp[:, :, 1], up[:, :, 1], timeScalep, Int(ef[1]), t, lp[:, :, 1], np[:, :, 1]
end

"Drop-in for ParkingDist.jl:29 (collision-free sibling; entry point obca_parking_dist_batch has the same arguments minus the slack output)."
function ParkingDist(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, rx, ry, ryaw, fixTime, xWS, uWS; opts=ipopt_opts())      # (ParkingDist.jl:41 sets recalc_y = "yes" too)
    M = sum(vOb)
    xp = zeros(4, N + 1); up = zeros(2, N); ts = zeros(N + 1); ef = zeros(Cint, 1); lp = zeros(M, N + 1); np = zeros(4nOb, N + 1)
    t0 = time()
    rc = GC.@preserve opts ccall((:obca_parking_dist_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx().h, 1, N, [Float64(Ts)], L, f64(vec(ego)), f64(vec(XYbounds)), fixTime, f64(vec(x0)), f64(vec(xF)), Cint[nOb], Cint.(vec(vOb)),
               vec(permutedims(f64(A))), f64(vec(b)), f64(rx)[1:N+1], f64(ry)[1:N+1], f64(ryaw)[1:N+1], vec(permutedims(f64(xWS)[1:N+1, :])),
               vec(permutedims(f64(uWS)[1:N, :])), C_NULL, C_NULL, optsptr(opts), xp, up, ts, ef, lp, np, C_NULL)
    rc == 0 || error("obca_parking_dist_batch failed: " * lasterr(ctx()))
    timeScalep = fixTime == 1 ? ones(1, N + 1) : ts
    return xp, up, timeScalep, Int(ef[1]), time() - t0, lp, np          # ParkingDist.jl:313
end

"""
    ParkingConstraints_batch(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd; sl=nothing, tol=5e-5)

Batched a-posteriori check on the GPU (obca_parking_constraints_batch): x0, xF 4xB; Ts a vector of length B; x 4x(N+1)xB; u 2xNxB; l Mx(N+1)xB; n 4nObx(N+1)xB;
timeScale (N+1)xB (it may vary over the stages); sl nObx(N+1)xB or nothing (zeros); the obstacle set is shared by the batch.  Returns (ok B, ref_ok B, viol 14xB):
ok = every class of the full checker except the penetration <= tol, ref_ok = the reference's own test (ParkingConstraints.jl:29-149, quirks included) at 5e-5,
viol = u_bounds, x_bounds, ts_bounds, ts_chain, dual_pos, start, end, dyn, steer_rate, norm, rot, sep, penetration, ref_worst.
"""
function ParkingConstraints_batch(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd; sl=nothing, tol=5e-5)
    B = size(x0, 2)
    nObs = fill(Cint(nOb), B); vflat = repeat(Cint.(vec(vOb)), B)
    At = repeat(vec(permutedims(f64(A))), B); bt = repeat(vec(f64(b)), B)
    ok = zeros(Cint, B); rok = zeros(Cint, B); viol = zeros(14, B)
    rc = ccall((:obca_parking_constraints_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Cdouble, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
               ctx().h, B, N, f64(vec(Ts)), L, f64(vec(ego)), f64(vec(XYbounds)), fixTime, f64(x0), f64(xF), nObs, vflat, At, bt, sd == 1 ? 0 : 1,
               f64(x), f64(u), f64(timeScale), f64(l), f64(n), sl === nothing ? C_NULL : f64(sl), tol, ok, rok, viol)
    rc == 0 || error("obca_parking_constraints_batch failed: " * lasterr(ctx()))
    return ok, rok, viol
end

"Drop-in for ParkingConstraints.jl:29 (one instance): same arguments (x 4x(N+1), u 2xN, l Mx(N+1), n 4nObx(N+1), timeScale of length N+1), returns 1 or 0 like :141-148."
function ParkingConstraints(x0, xF, N, Ts, L, ego, XYbounds, nOb, vOb, A, b, x, u, l, n, timeScale, fixTime, sd)
    M = sum(vOb)
    ts = length(timeScale) == 1 ? fill(Float64(timeScale[1]), N + 1) : f64(vec(timeScale))[1:N+1]
    ok, rok, viol = ParkingConstraints_batch(reshape(f64(vec(x0)), 4, 1), reshape(f64(vec(xF)), 4, 1), N, [Float64(Ts)], L, ego, XYbounds, nOb, vOb, A, b,
        reshape(f64(x)[:, 1:N+1], 4, N + 1, 1), reshape(f64(u)[:, 1:N], 2, N, 1), reshape(f64(l)[:, 1:N+1], M, N + 1, 1), reshape(f64(n)[:, 1:N+1], 4nOb, N + 1, 1),
        reshape(ts, N + 1, 1), fixTime, sd)
    return Int(rok[1])
end

"Drop-in for DualMultWS.jl:29; `ego` defaults to the global the reference reads (DualMultWS.jl:39-45). Returns (lp (N+1)xM, np (N+1)x4nOb)."
function DualMultWS(N, nOb, vOb, A, b, rx, ry, ryaw; ego=Main.ego)
    M = sum(vOb)
    lw = zeros(M, N + 1); nw = zeros(4nOb, N + 1)
    rc = ccall((:obca_dualmult_ws_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx().h, 1, N, f64(vec(ego)), Cint[nOb], Cint.(vec(vOb)), vec(permutedims(f64(A))), f64(vec(b)), f64(rx)[1:N+1], f64(ry)[1:N+1],
               f64(ryaw)[1:N+1], lw, nw, C_NULL)
    rc == 0 || error("obca_dualmult_ws_batch failed: " * lasterr(ctx()))
    return permutedims(lw), permutedims(nw)                        # DualMultWS.jl:81-84 returns the transposes
end


"""
    QuadcopterSignedDist_batch(x0, xF, N, Ts, R, ob, xWS, timeWS; dual_ws=true, dist=false)

Batched form: x0, xF 12xB; Ts, timeWS vectors of length B; ob 6x5xB (ob1..ob5 of every instance back to back, each
[xmax,ymax,zmax,-xmin,-ymin,-zmin]); xWS 12x(N+1)xB.  Returns (xp 12x(N+1)xB, up 4xNxB, timeScale (N+1)xB, exitflag B, time, lp 30x(N+1)xB,
status codes B).  dist=true solves the QuadcopterDist formulation (obca_quadcopter_dist_batch).  opts=nothing: the library's throughput defaults
(obca_quadcopter_default_opts); `quadcopter_ipopt_opts()`: with IPOPT's second-order correction and least-squares initial multipliers.
"""
function QuadcopterSignedDist_batch(x0, xF, N, Ts, R, ob, xWS, timeWS; dual_ws::Bool=true, dist::Bool=false, opts=nothing)
    B = size(x0, 2)
    xp = zeros(12, N + 1, B); up = zeros(4, N, B); ts = zeros(N + 1, B); ef = zeros(Cint, B); lp = zeros(30, N + 1, B); info = zeros(8, B)
    t0 = time()
    if dist
        rc = GC.@preserve opts ccall((:obca_quadcopter_dist_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                    Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                   ctx().h, B, N, f64(vec(Ts)), Float64(R), f64(x0), f64(xF), f64(ob), f64(xWS), C_NULL, f64(vec(timeWS)), dual_ws ? 1 : 0, optsptr(opts),
                   xp, up, ts, ef, lp, info)
    else
        rc = GC.@preserve opts ccall((:obca_quadcopter_signed_dist_batch, LIB), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                    Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                   ctx().h, B, N, f64(vec(Ts)), Float64(R), f64(x0), f64(xF), f64(ob), f64(xWS), C_NULL, f64(vec(timeWS)), dual_ws ? 1 : 0, optsptr(opts),
                   xp, up, ts, ef, lp, C_NULL, info)
    end
    rc == 0 || error("obca_quadcopter_(signed_)dist_batch failed: " * lasterr(ctx()))
    return xp, up, ts, ef, time() - t0, lp, info[1, :]
end

"""
    constrSatisfaction_batch(x, u, timeScale, x0, xF, Ts, lambda, ob, R; tol=1e-3)

Batched constrSatisfaction on the GPU (obca_quadcopter_constr_satisfaction_batch): x 12x(N+1)xB; u 4xNxB; timeScale (N+1)xB; x0, xF 12xB; Ts a vector of length B;
lambda 30x(N+1)xB; ob 6x5xB.  Returns (ok B, viol 9xB): viol = start, end, u_bounds, x_bounds, dyn, ts_chain, dual_pos, norm, sep (constrSatisfaction.jl:25-204).
"""
function constrSatisfaction_batch(x, u, timeScale, x0, xF, Ts, lambda, ob, R; tol=1e-3)
    B = size(x, 3); N = size(x, 2) - 1
    ok = zeros(Cint, B); viol = zeros(9, B)
    rc = ccall((:obca_quadcopter_constr_satisfaction_batch, LIB), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Cdouble, Ptr{Cint}, Ptr{Cdouble}),
               ctx().h, B, N, f64(vec(Ts)), Float64(R), f64(x0), f64(xF), f64(ob), f64(x), f64(u), f64(timeScale), f64(lambda), tol, ok, viol)
    rc == 0 || error("obca_quadcopter_constr_satisfaction_batch failed: " * lasterr(ctx()))
    return ok, viol
end

"Drop-in for constrSatisfaction.jl:25 (call sites mainQuadcopter.jl:147,154): same arguments (x 12x(N+1), u 4xN, lambda 30x(N+1)), returns true / false."
function constrSatisfaction(x, u, timeScale, x0, xF, Ts, lambda, ob1, ob2, ob3, ob4, ob5, R)
    N = size(x, 2) - 1
    ob = reshape(f64(vcat(map(vec, (ob1, ob2, ob3, ob4, ob5))...)), 6, 5, 1)
    ts = length(timeScale) == 1 ? fill(Float64(timeScale[1]), N + 1) : f64(vec(timeScale))[1:N+1]
    ok, viol = constrSatisfaction_batch(reshape(f64(x), 12, N + 1, 1), reshape(f64(u), 4, N, 1), reshape(ts, N + 1, 1), reshape(f64(vec(x0)), 12, 1), reshape(f64(vec(xF)), 12, 1),
        [Float64(Ts)], reshape(f64(lambda), 30, N + 1, 1), ob, R)
    return ok[1] == 1
end

_quad_status(c) = c == 0 ? "Optimal" : (c == 1 ? "UserLimit" : "Error")

# xWS is 12 x (N+1) in the reference (mainQuadcopter.jl:136 builds [rx'; ry'; rz'; zeros...], QuadcopterSignedDist.jl:201 does setvalue(x, xWS)
# without a transpose): column-major, that is already the stage-contiguous layout of the C ABI.
function _quad_one(x0, xF, N, Ts, R, obs, xWS, timeWS, dual_ws, dist, opts)
    ob = reshape(f64(vcat(map(vec, obs)...)), 6, 5, 1)               # [xmax,ymax,zmax,-xmin,-ymin,-zmin] per box (:162-166)
    xp, up, ts, ef, t, lp, st = QuadcopterSignedDist_batch(reshape(f64(vec(x0)), 12, 1), reshape(f64(vec(xF)), 12, 1), N, [Float64(Ts)], R, ob,
        reshape(f64(xWS)[:, 1:N+1], 12, N + 1, 1), [Float64(timeWS)]; dual_ws=dual_ws, dist=dist, opts=opts)
    return xp[:, :, 1], up[:, :, 1], ts[:, 1], Int(ef[1]), t, lp[:, :, 1], _quad_status(st[1])
end

"Drop-in for QuadcopterSignedDist.jl:25 (one instance): same arguments, same 7-tuple (xp, up, timeScalep, exitflag, time, lp, status), :298."
QuadcopterSignedDist(x0, xF, N, Ts, R, ob1, ob2, ob3, ob4, ob5, xWS, uWS, timeWS; dual_ws::Bool=true, opts=quadcopter_ipopt_opts()) =
    _quad_one(x0, xF, N, Ts, R, (ob1, ob2, ob3, ob4, ob5), xWS, timeWS, dual_ws, false, opts)

"Drop-in for QuadcopterDist.jl:25 (call site mainQuadcopter.jl:145): the collision-free sibling, same arguments and 7-tuple (:282)."
QuadcopterDist(x0, xF, N, Ts, R, ob1, ob2, ob3, ob4, ob5, xWS, uWS, timeWS; dual_ws::Bool=true, opts=quadcopter_ipopt_opts()) =
    _quad_one(x0, xF, N, Ts, R, (ob1, ob2, ob3, ob4, ob5), xWS, timeWS, dual_ws, true, opts)

# ---------------------------------------------------------------- device-resident quadcopter batch: upload once, solve / shift / solve ... (receding horizon)
"options for a solve that starts from `shift_warm_start!`: the quadcopter defaults (reference=true: `quadcopter_ipopt_opts()`) with mu_init = bound_push = bound_frac = 1e-4"
function quad_warm_restart_opts(; reference::Bool=false)
    o = Opts()
    sym_ok = reference ? ccall((:obca_quadcopter_reference_opts, LIB), Cint, (Ref{Opts},), o) : ccall((:obca_quadcopter_default_opts, LIB), Cint, (Ref{Opts},), o)
    sym_ok == 0 || error("obca_quadcopter_*_opts failed")
    o.mu_init = 1e-4; o.bound_push = 1e-4; o.bound_frac = 1e-4
    return o
end

"""
    QuadBatch(B, N)

B quadcopter instances of horizon N resident on the GPU (obca_quad_batch_* of include/obca_hip.h): `upload!`, `solve!`, `sync!`, `shift_warm_start!`, `download`, `validate`,
`destroy!`.  The iterate stays on the device between solves: a receding-horizon loop moves 12 numbers per instance up (the measured state) and whatever it downloads.
"""
mutable struct QuadBatch
    h::Ptr{Cvoid}
    B::Int
    N::Int
    c::Context
end
function QuadBatch(B::Integer, N::Integer; context::Context=ctx())
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:obca_quad_batch_create, LIB), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}), context.h, B, N, r)
    rc == 0 || error("obca_quad_batch_create failed: " * lasterr(context))
    b = QuadBatch(r[], B, N, context)
    finalizer(destroy!, b)
    return b
end
function destroy!(b::QuadBatch)
    b.h == C_NULL || ccall((:obca_quad_batch_destroy, LIB), Cint, (Ptr{Cvoid},), b.h)
    b.h = C_NULL
    return nothing
end
_qcheck(b::QuadBatch, rc, what) = rc == 0 || error(what * " failed: " * lasterr(b.c))

"x0, xF 12xB; Ts, timeWS vectors of length B; ob 6x5xB; xWS 12x(N+1)xB (the layouts of `QuadcopterSignedDist_batch`)"
function upload!(b::QuadBatch, x0, xF, Ts, R, ob, xWS, timeWS; dual_ws::Bool=true, dist::Bool=false)
    size(xWS) == (12, b.N + 1, b.B) || error("xWS must be 12 x (N+1) x B")
    _qcheck(b, ccall((:obca_quad_batch_upload, LIB), Cint,
                     (Ptr{Cvoid}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint),
                     b.h, f64(vec(Ts)), Float64(R), f64(x0), f64(xF), f64(ob), f64(xWS), f64(vec(timeWS)), dual_ws ? 1 : 0, dist ? 1 : 0), "obca_quad_batch_upload")
    return b
end
"queue a solve on the context's stream (asynchronous; `sync!` waits).  opts=nothing: the throughput defaults; after `shift_warm_start!`: `quad_warm_restart_opts()`"
function solve!(b::QuadBatch; opts=nothing)
    _qcheck(b, GC.@preserve(opts, ccall((:obca_quad_batch_solve, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), b.h, optsptr(opts))), "obca_quad_batch_solve")
    return b
end
sync!(b::QuadBatch) = (_qcheck(b, ccall((:obca_quad_batch_sync, LIB), Cint, (Ptr{Cvoid},), b.h), "obca_quad_batch_sync"); b)
"""
    shift_warm_start!(b, shift; x0_new=nothing, xF_new=nothing)

Receding-horizon restart on the device (obca_quad_batch_shift_warm_start): the next `solve!` starts from the last solution advanced by `shift` stages, from `x0_new` (12xB, the
measured state; nothing: stage `shift` of the solution) towards `xF_new` (12xB, a moving goal; nothing: unchanged).  A failed instance keeps its uploaded warm start.
"""
function shift_warm_start!(b::QuadBatch, shift::Integer; x0_new=nothing, xF_new=nothing)
    a0 = x0_new === nothing ? C_NULL : f64(x0_new); aF = xF_new === nothing ? C_NULL : f64(xF_new)
    (x0_new === nothing || length(a0) == 12 * b.B) && (xF_new === nothing || length(aF) == 12 * b.B) || error("x0_new / xF_new must be 12 x B")
    _qcheck(b, ccall((:obca_quad_batch_shift_warm_start, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}), b.h, shift, a0, aF), "obca_quad_batch_shift_warm_start")
    return b
end
"(xp 12x(N+1)xB, up 4xNxB, timeScale (N+1)xB, exitflag B, lp 30x(N+1)xB, slack 5x(N+1)xB, info 8xB) of the last solve; synchronises"
function download(b::QuadBatch)
    B, N = b.B, b.N
    xp = zeros(12, N + 1, B); up = zeros(4, N, B); ts = zeros(N + 1, B); ef = zeros(Cint, B); lp = zeros(30, N + 1, B); sl = zeros(5, N + 1, B); info = zeros(8, B)
    _qcheck(b, ccall((:obca_quad_batch_download, LIB), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                     b.h, xp, up, ts, ef, lp, sl, info), "obca_quad_batch_download")
    return xp, up, ts, ef, lp, sl, info
end
"constrSatisfaction on the last solution, on the device: (ok B, viol 9xB); refused between `shift_warm_start!` and the next `solve!`"
function validate(b::QuadBatch; tol=1e-3)
    ok = zeros(Cint, b.B); viol = zeros(9, b.B)
    _qcheck(b, ccall((:obca_quad_batch_validate, LIB), Cint, (Ptr{Cvoid}, Cdouble, Ptr{Cint}, Ptr{Cdouble}), b.h, tol, ok, viol), "obca_quad_batch_validate")
    return ok, viol
end

"""
    batch_shift_warm_start!(h, shift; x0_new=nothing)

The parking restart (obca_batch_shift_warm_start) for a caller that holds an `obca_batch` handle `h` (a `Ptr{Cvoid}` from `obca_batch_create`): the uploaded warm start becomes
the last solution advanced by `shift` stages -- x, u, lambda, mu and the tracking reference --, x0 becomes `x0_new` (4xB) or stage `shift` of the solution.
"""
function batch_shift_warm_start!(h::Ptr{Cvoid}, shift::Integer; x0_new=nothing)
    rc = ccall((:obca_batch_shift_warm_start, LIB), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), h, shift, x0_new === nothing ? C_NULL : f64(x0_new))
    rc == 0 || error("obca_batch_shift_warm_start failed: " * lasterr(ctx()))
    return nothing
end

# ---- clearance between the nodes (include/obca_clearance.h; the entry points live in the same library)
const CLR = LIB
const CLR_OUT = 24      # OBCA_CLR_OUT

"the records (24 x B, see include/obca_clearance.h) as a named tuple: min, min_nodes, sample, stage, substep, obstacle, below, samples, per_obstacle (nOb x B), finite"
function _clearance(rec::Matrix{Float64}, S::Integer, nOb::Integer)
    q = Int.(rec[3, :])
    return (min=rec[1, :], min_nodes=rec[2, :], sample=q, stage=[v >= 0 ? div(v, S) : -1 for v in q], substep=[v >= 0 ? rem(v, S) : -1 for v in q], obstacle=Int.(rec[4, :]),
            below=Int.(rec[5, :]), samples=Int.(rec[6, :]), per_obstacle=rec[9:8+nOb, :], finite=rec[7, :] .== 0)
end

"""
    clearance(h, B; substeps=8, need=0.05, nOb=16)

Clearance of the last solution of the resident parking batch `h` (an obca_batch handle of B instances) BETWEEN its nodes: every interval is sampled `substeps` times with the
discretisation's own partial step, the car's distance to every obstacle is computed anew (0 = touches or overlaps).  `context`: the context `h` was created on.
"""
function clearance(h::Ptr{Cvoid}, B::Integer; substeps::Integer=8, need=0.05, nOb::Integer=16, context::Context=ctx())
    rec = zeros(CLR_OUT, B)
    rc = ccall((:obca_batch_clearance, CLR), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ptr{Cdouble}), h, substeps, need, rec)
    rc == 0 || error("obca_batch_clearance failed: " * lasterr(context))
    return _clearance(rec, substeps, nOb)
end
function clearance_ms(h::Ptr{Cvoid})
    ms = Ref{Cfloat}(0)
    ccall((:obca_batch_clearance_ms, CLR), Cint, (Ptr{Cvoid}, Ref{Cfloat}), h, ms) == 0 || error("obca_batch_clearance_ms failed")
    return Float64(ms[])
end

"the same for the last solution of a QuadBatch: the straight segment of every interval, clearance = distance of the point to a box - R"
function clearance(b::QuadBatch; substeps::Integer=8, need=0.0)
    rec = zeros(CLR_OUT, b.B)
    _qcheck(b, ccall((:obca_quad_batch_clearance, CLR), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ptr{Cdouble}), b.h, substeps, need, rec), "obca_quad_batch_clearance")
    return _clearance(rec, substeps, 5)
end
function clearance_ms(b::QuadBatch)
    ms = Ref{Cfloat}(0)
    _qcheck(b, ccall((:obca_quad_batch_clearance_ms, CLR), Cint, (Ptr{Cvoid}, Ref{Cfloat}), b.h, ms), "obca_quad_batch_clearance_ms")
    return Float64(ms[])
end

"""
    ParkingClearance_batch(N, Ts, L, ego, nOb, vOb, A, b, x, u; timeScale=nothing, substeps=8, need=0.05)

Clearance between the nodes of B arbitrary parking trajectories: x 4 x (N+1) x B, u 2 x N x B, timeScale (N+1) x B or nothing (= 1), Ts B; nOb (B, Cint), vOb, A (rows as
2 x M columns), b packed per instance as for ParkingConstraints_batch.
"""
function ParkingClearance_batch(N::Integer, Ts, L, ego, nOb, vOb, A, b, x, u; timeScale=nothing, substeps::Integer=8, need=0.05, context::Context=ctx())
    xs = f64(x); B = size(xs, 3)
    ts = timeScale === nothing ? C_NULL : f64(timeScale)
    rec = zeros(CLR_OUT, B)
    rc = ccall((:obca_parking_clearance_batch, CLR), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{Cdouble}),
               context.h, B, N, f64(Ts), L, f64(ego), convert(Array{Cint}, nOb), convert(Array{Cint}, vOb), f64(A), f64(b), xs, f64(u), ts, substeps, need, rec)
    rc == 0 || error("obca_parking_clearance_batch failed: " * lasterr(context))
    return _clearance(rec, substeps, Int(maximum(nOb)))
end

"the same for B quadcopter trajectories: x 12 x (N+1) x B, timeScale (N+1) x B, ob 6 x 5 x B ([hi; -lo] per box), Ts B"
function QuadcopterClearance_batch(x, timeScale, Ts, ob, R; substeps::Integer=8, need=0.0, context::Context=ctx())
    xs = f64(x); B = size(xs, 3); N = size(xs, 2) - 1
    rec = zeros(CLR_OUT, B)
    rc = ccall((:obca_quadcopter_clearance_batch, CLR), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{Cdouble}),
               context.h, B, N, f64(Ts), R, f64(ob), xs, f64(timeScale), substeps, need, rec)
    rc == 0 || error("obca_quadcopter_clearance_batch failed: " * lasterr(context))
    return _clearance(rec, substeps, 5)
end

# ---- solved parking batches on a finer horizon (include/obca_refine.h; the entry points live in the same library)
const RFN = LIB
const REFINE_MAXFACTOR = 32      # OBCA_REFINE_MAXFACTOR

"""
    refine(dst, src, factor; select=nothing, duals=false) -> status

Instance `select[j]` (0-based indices into the solved resident parking batch `src`; nothing: 0 .. n-1 with n = `count`) becomes instance j of the resident batch `dst`, whose
horizon is factor times src's: the same NLP with Ts / factor, the tracking reference interpolated, started from the solution -- its nodes, between them the poses
clearance(substeps=factor) sampled, u held, t = 1.  duals=false: dst's next solve runs DualMultWS; duals=true: stage q starts from the multipliers of stage div(q, factor).
`dst` and `src` are obca_batch handles of one context.  Returns the status per instance: 0 refined from the solution, 1 from the start iterate, -1 zero start.
"""
function refine(dst::Ptr{Cvoid}, src::Ptr{Cvoid}, factor::Integer; select=nothing, count::Integer=0, duals::Bool=false, context::Context=ctx())
    sel = select === nothing ? C_NULL : convert(Array{Cint}, select)
    n = select === nothing ? count : length(select)
    status = zeros(Cint, max(n, 1))
    rc = ccall((:obca_batch_refine_into, RFN), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Ptr{Cint}, Cint, Ptr{Cint}), dst, src, factor, duals ? 1 : 0, sel, n, status)
    rc == 0 || error("obca_batch_refine_into failed: " * lasterr(context))
    return Int.(status[1:n])
end
function refine_ms(dst::Ptr{Cvoid})
    ms = Ref{Cfloat}(0)
    ccall((:obca_batch_refine_ms, RFN), Cint, (Ptr{Cvoid}, Ref{Cfloat}), dst, ms) == 0 || error("obca_batch_refine_ms failed")
    return Float64(ms[])
end

"""
    ParkingRefine_batch(N, factor, Ts, L, x, u; timeScale=nothing) -> (Ts_f, x_f, u_f)

The primal part of `refine` for B arbitrary parking trajectories: x 4 x (N+1) x B, u 2 x N x B, timeScale (N+1) x B or nothing (= 1), Ts B.  Returns Ts / factor (B),
x_f 4 x (factor N + 1) x B and u_f 2 x factor N x B; an instance with a non-finite number among its inputs comes back as NaN.
"""
function ParkingRefine_batch(N::Integer, factor::Integer, Ts, L, x, u; timeScale=nothing, context::Context=ctx())
    xs = f64(x); B = size(xs, 3); Nf = N * factor
    ts = timeScale === nothing ? C_NULL : f64(timeScale)
    Tsf = zeros(B); xf = zeros(4, Nf + 1, B); uf = zeros(2, Nf, B)
    rc = ccall((:obca_parking_refine_batch, RFN), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               context.h, B, N, factor, f64(Ts), L, xs, f64(u), ts, Tsf, xf, uf)
    rc == 0 || error("obca_parking_refine_batch failed: " * lasterr(context))
    return Tsf, xf, uf
end

# ---- solved quadcopter batches on a finer horizon (include/obca_quad_subdivide.h; the entry points live in the same library)
const QSD = LIB
const QUAD_SUBDIVIDE_MAXFACTOR = 32      # OBCA_QUAD_SUBDIVIDE_MAXFACTOR

"""
    refine(dst::QuadBatch, src::QuadBatch, factor; select=nothing, margin=0.0) -> status

Instance `select[j]` (0-based indices into the solved resident batch `src`; nothing: all of them) becomes instance j of the resident batch `dst`, whose horizon is factor times
src's: the same NLP with Ts / factor and the radius R + margin, warm-started from the solution -- its nodes, between them the points clearance(substeps=factor) sampled and the
other nine states interpolated, timeWS = the solution's t, closed-form duals.  `validate` and `clearance` of `dst` use R + margin: clearance against the true radius is
`clearance(dst; need=-margin)`.  Returns the status per instance: 0 refined from the solution, 1 interpolated from the uploaded warm start, -1 zero warm start.
"""
function refine(dst::QuadBatch, src::QuadBatch, factor::Integer; select=nothing, margin=0.0)
    sel = select === nothing ? C_NULL : convert(Array{Cint}, select)
    n = select === nothing ? src.B : length(select)
    status = zeros(Cint, max(n, 1))
    _qcheck(dst, ccall((:obca_quad_batch_subdivide_into, QSD), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cdouble, Ptr{Cint}, Cint, Ptr{Cint}), dst.h, src.h, factor, margin, sel, n, status),
            "obca_quad_batch_subdivide_into")
    dst.B = n
    return Int.(status[1:n])
end
function refine_ms(dst::QuadBatch)
    ms = Ref{Cfloat}(0)
    _qcheck(dst, ccall((:obca_quad_batch_subdivide_ms, QSD), Cint, (Ptr{Cvoid}, Ref{Cfloat}), dst.h, ms), "obca_quad_batch_subdivide_ms")
    return Float64(ms[])
end

"""
    QuadcopterRefine_batch(factor, Ts, x; timeScale=nothing) -> (Ts_f, x_f)

The trajectory part of `refine` for B arbitrary quadcopter trajectories: x 12 x (N+1) x B, timeScale (N+1) x B or nothing (= 1), Ts B.  Returns Ts / factor (B) and
x_f 12 x (factor N + 1) x B; an instance with a non-finite number among its inputs comes back as NaN.
"""
function QuadcopterRefine_batch(factor::Integer, Ts, x; timeScale=nothing, context::Context=ctx())
    xs = f64(x); B = size(xs, 3); N = size(xs, 2) - 1
    ts = timeScale === nothing ? C_NULL : f64(timeScale)
    Tsf = zeros(B); xf = zeros(12, N * factor + 1, B)
    rc = ccall((:obca_quadcopter_subdivide_batch, QSD), Cint,
               (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               context.h, B, N, factor, f64(Ts), xs, ts, Tsf, xf)
    rc == 0 || error("obca_quadcopter_subdivide_batch failed: " * lasterr(context))
    return Tsf, xf
end

end # module
