# OBCAEnsemble.jl -- ensembles of disturbed closed-loop rollouts about solved batches and arbitrary trajectories (include/obca_ensemble.h) for Julia (>= 1.6): the ccalls on
# libobca_hip.so, beside OBCAHip.jl (whose Batch / QuadBatch handles they take) and OBCATrack.jl (one closed loop per call).  The gains of OBCATrack are computed once per
# instance; up to 64 members per instance -- start offsets dx0 and constant input biases dub -- are rolled in one launch, one member per lane of the instance's wavefront,
# and every sample a member passes is measured against the obstacles.
#
#   using .OBCAHip, .OBCAEnsemble
#   # bt: an obca_quad_batch handle that has been uploaded and solved (B instances, horizon N); ctx: the handle of the context it was created on
#   dx0 = OBCAEnsemble.offsets(12, M, B, sigma)                              # 12 x M x B normal rows, member 1 exactly zero: the nominal closed loop
#   r = OBCAEnsemble.quad_ensemble(ctx, bt, B; members=M, dx0=dx0)           # r.out[:, i]: the 32 doubles of instance i (include/obca_ensemble.h)
#   mem = OBCAEnsemble.quad_ensemble_members(ctx, bt, B, M)                  # mem[:, m, i]: the 16 doubles of member m of instance i
#   fin = OBCAEnsemble.quad_ensemble_final(ctx, bt, B, M)                    # fin[:, m, i]: its final state X_N
#
# Julia arrays are column-major: out is 32 x B, mem is 16 x M x B, fin is nx x M x B, dx0 is nx x M x B, dub is nu x M x B -- the dense arrays of the C calls with no copy.
# The default weights are those of obca_amd/validate.py (TRACK_*): untuned.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_ensemble_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_ensemble.py.
module OBCAEnsemble

using Random

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const ENS = LIB
const OUT = 32          # OBCA_ENS_OUT
const MEM = 16          # OBCA_ENS_MEM
const MMAX = 64         # OBCA_ENS_MMAX
const Q_PARKING = [10.0, 10.0, 10.0, 1.0]
const R_PARKING = [1.0, 1.0]
const Q_QUAD = [10.0, 10.0, 10.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.1, 0.1, 0.1]
const R_QUAD = [0.1, 0.1, 0.1, 0.1]
const Rows = Union{Nothing,Array{Float64,3}}

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, what, ctx)
    rc == 0 || error("$what failed ($rc): " * lasterr(ctx))
end

ptr(a) = a === nothing ? C_NULL : a

"n x M x B rows drawn from N(0, diag(sigma^2)), member 1 exactly zero (there is no random number generator on the device)"
function offsets(n::Integer, M::Integer, B::Integer, sigma::Vector{Float64}; seed::Integer=0)
    d = randn(MersenneTwister(seed), n, M, B) .* sigma
    d[:, 1, :] .= 0.0
    return d
end

"`members` closed loops about the last solution of a solved parking batch; dx0: 4 x M x B or nothing, dub: 2 x M x B or nothing: (out = 32 x B,)"
function ensemble(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; members::Integer=64, substeps::Integer=8, feedback::Bool=true, clamp::Bool=true, Q::Vector{Float64}=Q_PARKING,
                  R::Vector{Float64}=R_PARKING, Qf::Vector{Float64}=10.0 .* Q, dx0::Rows=nothing, dub::Rows=nothing, need::Real=0.05)
    out = zeros(OUT, B)
    rc = ccall((:obca_batch_ensemble, ENS), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
               bt, substeps, members, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf, ptr(dx0), ptr(dub), need, out)
    check(rc, "obca_batch_ensemble", ctx)
    return (out=out,)
end

"HIP-event duration of the last ensemble kernel on the parking batch [ms]"
function ensemble_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_batch_ensemble_ms, ENS), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_batch_ensemble_ms", ctx)
    return Float64(a[])
end

"the member records of the last ensemble call on the parking batch: 16 x M x B"
function ensemble_members(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, M::Integer)
    mem = zeros(MEM, M, B)
    check(ccall((:obca_batch_ensemble_members, ENS), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, mem), "obca_batch_ensemble_members", ctx)
    return mem
end

"their final states: 4 x M x B"
function ensemble_final(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, M::Integer)
    fin = zeros(4, M, B)
    check(ccall((:obca_batch_ensemble_final, ENS), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, fin), "obca_batch_ensemble_final", ctx)
    return fin
end

"any parking trajectories: the arguments of OBCATrack.parking_track up to timeScale; (out = 32 x B, mem = 16 x M x B, fin = 4 x M x B)"
function parking_ensemble(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, L::Real, ego::Vector{Float64}, nOb::Vector{Cint}, vOb::Vector{Cint}, A::Vector{Float64}, b::Vector{Float64},
                          x::Array{Float64,3}, u::Array{Float64,3}, timeScale::Union{Nothing,Matrix{Float64}}=nothing; members::Integer=64, substeps::Integer=8, feedback::Bool=true,
                          clamp::Bool=true, Q::Vector{Float64}=Q_PARKING, R::Vector{Float64}=R_PARKING, Qf::Vector{Float64}=10.0 .* Q, dx0::Rows=nothing, dub::Rows=nothing,
                          need::Real=0.05)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); mem = zeros(MEM, members, B); fin = zeros(4, members, B)
    rc = ccall((:obca_parking_ensemble_batch, ENS), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, L, ego, nOb, vOb, A, b, x, u, ptr(timeScale), substeps, members, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf, ptr(dx0), ptr(dub), need, out, mem, fin)
    check(rc, "obca_parking_ensemble_batch", ctx)
    return (out=out, mem=mem, fin=fin)
end

"`members` closed loops about the last solution of a solved quadcopter batch; dx0: 12 x M x B or nothing, dub: 4 x M x B or nothing: (out = 32 x B,)"
function quad_ensemble(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; members::Integer=64, substeps::Integer=8, feedback::Bool=true, clamp::Bool=true, Q::Vector{Float64}=Q_QUAD,
                       R::Vector{Float64}=R_QUAD, Qf::Vector{Float64}=10.0 .* Q, dx0::Rows=nothing, dub::Rows=nothing, need::Real=0.0)
    out = zeros(OUT, B)
    rc = ccall((:obca_quad_batch_ensemble, ENS), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}),
               bt, substeps, members, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf, ptr(dx0), ptr(dub), need, out)
    check(rc, "obca_quad_batch_ensemble", ctx)
    return (out=out,)
end

function quad_ensemble_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_quad_batch_ensemble_ms, ENS), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_quad_batch_ensemble_ms", ctx)
    return Float64(a[])
end

"the member records of the last ensemble call on the quadcopter batch: 16 x M x B"
function quad_ensemble_members(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, M::Integer)
    mem = zeros(MEM, M, B)
    check(ccall((:obca_quad_batch_ensemble_members, ENS), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, mem), "obca_quad_batch_ensemble_members", ctx)
    return mem
end

"their final states: 12 x M x B"
function quad_ensemble_final(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, M::Integer)
    fin = zeros(12, M, B)
    check(ccall((:obca_quad_batch_ensemble_final, ENS), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, fin), "obca_quad_batch_ensemble_final", ctx)
    return fin
end

"any quadcopter trajectories: the arguments of OBCATrack.quadcopter_track up to timeScale; (out = 32 x B, mem = 16 x M x B, fin = 12 x M x B)"
function quadcopter_ensemble(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, Rv::Real, ob::Array{Float64,3}, x::Array{Float64,3}, u::Array{Float64,3}, timeScale::Matrix{Float64};
                             members::Integer=64, substeps::Integer=8, feedback::Bool=true, clamp::Bool=true, Q::Vector{Float64}=Q_QUAD, R::Vector{Float64}=R_QUAD,
                             Qf::Vector{Float64}=10.0 .* Q, dx0::Rows=nothing, dub::Rows=nothing, need::Real=0.0)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); mem = zeros(MEM, members, B); fin = zeros(12, members, B)
    rc = ccall((:obca_quadcopter_ensemble_batch, ENS), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, Rv, ob, x, u, timeScale, substeps, members, feedback ? 1 : 0, clamp ? 1 : 0, Q, R, Qf, ptr(dx0), ptr(dub), need, out, mem, fin)
    check(rc, "obca_quadcopter_ensemble_batch", ctx)
    return (out=out, mem=mem, fin=fin)
end

end # module
