# OBCACertify.jl -- the clearance of solved batches and arbitrary trajectories CERTIFIED along the whole path (include/obca_certify.h) for Julia (>= 1.6): the ccalls on
# libobca_hip.so, beside OBCAHip.jl (whose Batch / QuadBatch handles they take; its `clearance` samples a fixed number of poses per interval and says nothing about what
# lies between them).  Every (interval, obstacle) pair is walked by conservative advancement: a pose with clearance c clears the stretch of the path on which no point of
# the vehicle moves farther than c, and the next sample is taken at the end of that stretch.
#
#   using .OBCAHip, .OBCACertify
#   # bt: an obca_batch handle that has been uploaded and solved (B instances, horizon N); ctx: the handle of the context it was created on
#   r = OBCACertify.certify(ctx, bt, B; need=0.05, slack=0.01)               # r.out[:, i]: the 16 doubles of instance i (include/obca_certify.h)
#   r.certified[i]                                                           # clearance >= need - slack everywhere on the path of instance i
#   iv = OBCACertify.certify_intervals(ctx, bt, B, N)                        # iv[:, k, i] = [lb_k, seen_k] of interval k - 1 (column N + 1: node N)
#
# Julia arrays are column-major: out is 16 x B, iv is 2 x (N + 1) x B -- the dense arrays of the C calls with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_certify_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_certify.py.
module OBCACertify

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const CERT = LIB
const OUT = 16          # OBCA_CERT_OUT
const TICKS = 4096      # OBCA_CERT_TICKS

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, what, ctx)
    rc == 0 || error("$what failed ($rc): " * lasterr(ctx))
end

ptr(a) = a === nothing ? C_NULL : a

"the records (16 x B) with their named fields: lb, seen, where (interval, tick, obstacle; 0-based as the library counts), violated, undecided, samples, certified, finite"
record(out::Matrix{Float64}) = (out=out, lb=out[1, :], seen=out[2, :], interval=Int.(out[3, :]), tick=Int.(out[4, :]), obstacle=Int.(out[5, :]), violated=Int.(out[6, :]),
                                first_violation=Int.(out[7:9, :]), undecided=Int.(out[10, :]), samples=Int.(out[11, :]), samples_max=Int.(out[12, :]), lipschitz=out[13, :],
                                certified=out[14, :] .!= 0, finite=out[15, :] .== 0)

"the certificate of the last solution of a solved parking batch"
function certify(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; need::Real=0.05, slack::Real=0.01, max_steps::Integer=TICKS)
    out = zeros(OUT, B)
    rc = ccall((:obca_batch_certify, CERT), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cint, Ptr{Cdouble}), bt, need, slack, max_steps, out)
    check(rc, "obca_batch_certify", ctx)
    return record(out)
end

"HIP-event duration of the last certify kernel on the parking batch [ms]"
function certify_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_batch_certify_ms, CERT), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_batch_certify_ms", ctx)
    return Float64(a[])
end

"[lb_k, seen_k] of the last certify call on the parking batch: 2 x (N + 1) x B"
function certify_intervals(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    iv = zeros(2, N + 1, B)
    check(ccall((:obca_batch_certify_intervals, CERT), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, iv), "obca_batch_certify_intervals", ctx)
    return iv
end

"any parking trajectories: x 4 x (N+1) x B, u 2 x N x B, timeScale (N+1) x B or nothing (= 1), obstacles packed as for OBCAHip.ParkingClearance_batch; the record and iv = 2 x (N+1) x B"
function parking_certify(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, L::Real, ego::Vector{Float64}, nOb::Vector{Cint}, vOb::Vector{Cint}, A::Vector{Float64}, b::Vector{Float64},
                         x::Array{Float64,3}, u::Array{Float64,3}, timeScale::Union{Nothing,Matrix{Float64}}=nothing; need::Real=0.05, slack::Real=0.01, max_steps::Integer=TICKS)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); iv = zeros(2, N + 1, B)
    rc = ccall((:obca_parking_certify_batch, CERT), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Cdouble, Cdouble, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, L, ego, nOb, vOb, A, b, x, u, ptr(timeScale), need, slack, max_steps, out, iv)
    check(rc, "obca_parking_certify_batch", ctx)
    return merge(record(out), (intervals=iv,))
end

"the certificate of the last solution of a solved quadcopter batch"
function quad_certify(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; need::Real=0.0, slack::Real=0.01, max_steps::Integer=TICKS)
    out = zeros(OUT, B)
    rc = ccall((:obca_quad_batch_certify, CERT), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cint, Ptr{Cdouble}), bt, need, slack, max_steps, out)
    check(rc, "obca_quad_batch_certify", ctx)
    return record(out)
end

function quad_certify_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_quad_batch_certify_ms, CERT), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_quad_batch_certify_ms", ctx)
    return Float64(a[])
end

"[lb_k, seen_k] of the last certify call on the quadcopter batch: 2 x (N + 1) x B"
function quad_certify_intervals(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    iv = zeros(2, N + 1, B)
    check(ccall((:obca_quad_batch_certify_intervals, CERT), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, iv), "obca_quad_batch_certify_intervals", ctx)
    return iv
end

"any quadcopter trajectories: x 12 x (N+1) x B, timeScale (N+1) x B, ob 6 x 5 x B ([hi; -lo] per box), Rv the vehicle's radius; the record and iv = 2 x (N+1) x B"
function quadcopter_certify(ctx::Ptr{Cvoid}, Ts::Vector{Float64}, Rv::Real, ob::Array{Float64,3}, x::Array{Float64,3}, timeScale::Matrix{Float64};
                            need::Real=0.0, slack::Real=0.01, max_steps::Integer=TICKS)
    B = size(x, 3); N = size(x, 2) - 1
    out = zeros(OUT, B); iv = zeros(2, N + 1, B)
    rc = ccall((:obca_quadcopter_certify_batch, CERT), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cdouble, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, Rv, ob, x, timeScale, need, slack, max_steps, out, iv)
    check(rc, "obca_quadcopter_certify_batch", ctx)
    return merge(record(out), (intervals=iv,))
end

end # module
