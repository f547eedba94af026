# OBCARollout.jl -- the rollout of solved batches and of arbitrary trajectories on the continuous vehicle models (include/obca_rollout.h) for Julia (>= 1.6): the ccalls
# on libobca_hip.so, beside OBCAHip.jl (whose Batch / QuadBatch handles they take).  The inputs of a trajectory are held over every interval and the kinematic bicycle /
# the quadcopter's rigid body is integrated with classical RK4; what comes back per instance is how far the vehicle ends up from the nodes the NLP promised, and the
# clearance of the states it passes through.
#
#   using .OBCAHip, .OBCARollout
#   # bt: an obca_quad_batch handle that has been uploaded and solved (B instances, horizon N); ctx: the handle of the context it was created on
#   r = OBCARollout.quad_rollout(ctx, bt, B; substeps=8, restart=false)       # r.out[:, i]: the 40 doubles of instance i (include/obca_rollout.h)
#   X = OBCARollout.quad_rollout_states(ctx, bt, B, N)                        # X[:, k + 1, i]: the state instance i reaches after k intervals
#   # receding horizon: X[:, shift + 1, :] is the x0_new of obca_quad_batch_shift_warm_start(bt, shift, x0_new, C_NULL)
#
# Julia arrays are column-major: out is 40 x B, X is nx x (N+1) x B, x is nx x (N+1) x B, u is nu x N x B -- the dense arrays of the C calls with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_rollout_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_rollout.py.
module OBCARollout

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const ROL = LIB
const OUT = 40          # OBCA_ROLL_OUT
const MAXSUB = 32       # OBCA_ROLL_MAXSUB

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, what, ctx)
    rc == 0 || error("$what failed ($rc): " * lasterr(ctx))
end

"the last solution of a solved parking batch on the kinematic bicycle: (out = 40 x B,)"
function rollout(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; substeps::Integer=8, restart::Bool=false, need::Real=0.05)
    out = zeros(OUT, B)
    check(ccall((:obca_batch_rollout, ROL), Cint, (Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}), bt, substeps, restart ? 1 : 0, need, out), "obca_batch_rollout", ctx)
    return (out=out,)
end

"HIP-event duration of the last rollout kernel on the parking batch [ms]"
function rollout_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_batch_rollout_ms, ROL), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_batch_rollout_ms", ctx)
    return Float64(a[])
end

"the node states of the last rollout on the parking batch: 4 x (N+1) x B"
function rollout_states(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    X = zeros(4, N + 1, B)
    check(ccall((:obca_batch_rollout_states, ROL), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, X), "obca_batch_rollout_states", ctx)
    return X
end

"any parking trajectories: x 4 x (N+1) x B, u 2 x N x B, timeScale (N+1) x B or nothing (= 1); obstacles as OBCAHip packs them; (out = 40 x B, X = 4 x (N+1) x B)"
function parking_rollout(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, L::Real, ego::Vector{Float64}, nOb::Vector{Cint}, vOb::Vector{Cint}, A::Vector{Float64}, b::Vector{Float64},
                         x::Array{Float64,3}, u::Array{Float64,3}, timeScale::Union{Nothing,Matrix{Float64}}=nothing; substeps::Integer=8, restart::Bool=false, need::Real=0.05)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); X = zeros(4, N + 1, B)
    rc = ccall((:obca_parking_rollout_batch, ROL), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, L, ego, nOb, vOb, A, b, x, u, timeScale === nothing ? C_NULL : timeScale, substeps, restart ? 1 : 0, need, out, X)
    check(rc, "obca_parking_rollout_batch", ctx)
    return (out=out, X=X)
end

"the last solution of a solved quadcopter batch on the rigid body: (out = 40 x B,)"
function quad_rollout(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; substeps::Integer=8, restart::Bool=false, need::Real=0.0)
    out = zeros(OUT, B)
    check(ccall((:obca_quad_batch_rollout, ROL), Cint, (Ptr{Cvoid}, Cint, Cint, Cdouble, Ptr{Cdouble}), bt, substeps, restart ? 1 : 0, need, out), "obca_quad_batch_rollout", ctx)
    return (out=out,)
end

function quad_rollout_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_quad_batch_rollout_ms, ROL), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_quad_batch_rollout_ms", ctx)
    return Float64(a[])
end

"the node states of the last rollout on the quadcopter batch: 12 x (N+1) x B"
function quad_rollout_states(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    X = zeros(12, N + 1, B)
    check(ccall((:obca_quad_batch_rollout_states, ROL), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, X), "obca_quad_batch_rollout_states", ctx)
    return X
end

"any quadcopter trajectories: x 12 x (N+1) x B, u 4 x N x B, timeScale (N+1) x B, ob 6 x 5 x B as [hi; -lo]; (out = 40 x B, X = 12 x (N+1) x B)"
function quadcopter_rollout(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, R::Real, ob::Array{Float64,3}, x::Array{Float64,3}, u::Array{Float64,3}, timeScale::Matrix{Float64};
                            substeps::Integer=8, restart::Bool=false, need::Real=0.0)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); X = zeros(12, N + 1, B)
    rc = ccall((:obca_quadcopter_rollout_batch, ROL), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, R, ob, x, u, timeScale, substeps, restart ? 1 : 0, need, out, X)
    check(rc, "obca_quadcopter_rollout_batch", ctx)
    return (out=out, X=X)
end

end # module
