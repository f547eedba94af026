# OBCATrack.jl -- solved batches and arbitrary trajectories TRACKED on the continuous vehicle models by a time-varying LQR (include/obca_track.h) for Julia (>= 1.6): the
# ccalls on libobca_hip.so, beside OBCAHip.jl (whose Batch / QuadBatch handles they take) and OBCARollout.jl (the open loop).  The gains come from the derivative of the
# map the plant applies over an interval (RK4, the input held) and a backward Riccati recursion; the closed loop u = u_k + K_k (X_k - x_k), evaluated at the nodes and
# held, is rolled on the kinematic bicycle / the quadcopter's rigid body.
#
#   using .OBCAHip, .OBCATrack
#   # bt: an obca_quad_batch handle that has been uploaded and solved (B instances, horizon N); ctx: the handle of the context it was created on
#   r = OBCATrack.quad_track(ctx, bt, B; substeps=8)                  # r.out[:, i]: the 48 doubles of instance i (include/obca_track.h)
#   X = OBCATrack.quad_track_states(ctx, bt, B, N)                    # X[:, k + 1, i]: the state instance i reaches after k intervals under the feedback
#   K = OBCATrack.quad_track_gains(ctx, bt, B, N)                     # K[:, :, k + 1, i]' is K_k (4 x 12): the C array is row-major
#
# Julia arrays are column-major: out is 48 x B, X is nx x (N+1) x B, K is nx x nu x N x B, dx0 is nx x B -- the dense arrays of the C calls with no copy.
# The default weights are those of obca_amd/validate.py (TRACK_*): untuned.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_track_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_track.py.
module OBCATrack

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const TRK = LIB
const OUT = 48          # OBCA_TRK_OUT
const Q_PARKING = [10.0, 10.0, 10.0, 1.0]
const R_PARKING = [1.0, 1.0]
const Q_QUAD = [10.0, 10.0, 10.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.1, 0.1, 0.1]
const R_QUAD = [0.1, 0.1, 0.1, 0.1]

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, what, ctx)
    rc == 0 || error("$what failed ($rc): " * lasterr(ctx))
end

"the last solution of a solved parking batch tracked on the kinematic bicycle; dx0: 4 x B or nothing: (out = 48 x B,)"
function track(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; substeps::Integer=8, feedback::Bool=true, clamp::Bool=true, Q::Vector{Float64}=Q_PARKING, R::Vector{Float64}=R_PARKING,
               Qf::Vector{Float64}=10.0 .* Q, dx0::Union{Nothing,Matrix{Float64}}=nothing, need::Real=0.05)
    out = zeros(OUT, B)
    rc = ccall((:obca_batch_track, TRK), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
               bt, substeps, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf, dx0 === nothing ? C_NULL : dx0, need, out)
    check(rc, "obca_batch_track", ctx)
    return (out=out,)
end

"HIP-event duration of the last track kernel on the parking batch [ms]"
function track_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_batch_track_ms, TRK), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_batch_track_ms", ctx)
    return Float64(a[])
end

"the node states of the last track call on the parking batch: 4 x (N+1) x B"
function track_states(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    X = zeros(4, N + 1, B)
    check(ccall((:obca_batch_track_states, TRK), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, X), "obca_batch_track_states", ctx)
    return X
end

"its gains: 4 x 2 x N x B (K[:, a, k + 1, i] is row a of K_k)"
function track_gains(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    K = zeros(4, 2, N, B)
    check(ccall((:obca_batch_track_gains, TRK), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, K), "obca_batch_track_gains", ctx)
    return K
end

"any parking trajectories: the arguments of OBCARollout.parking_rollout; (out = 48 x B, X = 4 x (N+1) x B, K = 4 x 2 x N x B)"
function parking_track(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, L::Real, ego::Vector{Float64}, nOb::Vector{Cint}, vOb::Vector{Cint}, A::Vector{Float64}, b::Vector{Float64},
                       x::Array{Float64,3}, u::Array{Float64,3}, timeScale::Union{Nothing,Matrix{Float64}}=nothing; substeps::Integer=8, feedback::Bool=true, clamp::Bool=true,
                       Q::Vector{Float64}=Q_PARKING, R::Vector{Float64}=R_PARKING, Qf::Vector{Float64}=10.0 .* Q, dx0::Union{Nothing,Matrix{Float64}}=nothing, need::Real=0.05)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); X = zeros(4, N + 1, B); K = zeros(4, 2, N, B)
    rc = ccall((:obca_parking_track_batch, TRK), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, L, ego, nOb, vOb, A, b, x, u, timeScale === nothing ? C_NULL : timeScale, substeps, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf,
               dx0 === nothing ? C_NULL : dx0, need, out, X, K)
    check(rc, "obca_parking_track_batch", ctx)
    return (out=out, X=X, K=K)
end

"the last solution of a solved quadcopter batch tracked on the rigid body; dx0: 12 x B or nothing: (out = 48 x B,)"
function quad_track(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; substeps::Integer=8, feedback::Bool=true, clamp::Bool=true, Q::Vector{Float64}=Q_QUAD, R::Vector{Float64}=R_QUAD,
                    Qf::Vector{Float64}=10.0 .* Q, dx0::Union{Nothing,Matrix{Float64}}=nothing, need::Real=0.0)
    out = zeros(OUT, B)
    rc = ccall((:obca_quad_batch_track, TRK), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
               bt, substeps, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf, dx0 === nothing ? C_NULL : dx0, need, out)
    check(rc, "obca_quad_batch_track", ctx)
    return (out=out,)
end

function quad_track_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_quad_batch_track_ms, TRK), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_quad_batch_track_ms", ctx)
    return Float64(a[])
end

"the node states of the last track call on the quadcopter batch: 12 x (N+1) x B"
function quad_track_states(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    X = zeros(12, N + 1, B)
    check(ccall((:obca_quad_batch_track_states, TRK), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, X), "obca_quad_batch_track_states", ctx)
    return X
end

"its gains: 12 x 4 x N x B"
function quad_track_gains(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    K = zeros(12, 4, N, B)
    check(ccall((:obca_quad_batch_track_gains, TRK), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, K), "obca_quad_batch_track_gains", ctx)
    return K
end

"any quadcopter trajectories: the arguments of OBCARollout.quadcopter_rollout; (out = 48 x B, X = 12 x (N+1) x B, K = 12 x 4 x N x B)"
function quadcopter_track(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, Rv::Real, ob::Array{Float64,3}, x::Array{Float64,3}, u::Array{Float64,3}, timeScale::Matrix{Float64};
                          substeps::Integer=8, feedback::Bool=true, clamp::Bool=true, Q::Vector{Float64}=Q_QUAD, R::Vector{Float64}=R_QUAD, Qf::Vector{Float64}=10.0 .* Q,
                          dx0::Union{Nothing,Matrix{Float64}}=nothing, need::Real=0.0)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); X = zeros(12, N + 1, B); K = zeros(12, 4, N, B)
    rc = ccall((:obca_quadcopter_track_batch, TRK), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, Rv, ob, x, u, timeScale, substeps, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf, dx0 === nothing ? C_NULL : dx0, need, out, X, K)
    check(rc, "obca_quadcopter_track_batch", ctx)
    return (out=out, X=X, K=K)
end

end # module
