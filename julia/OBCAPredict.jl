# OBCAPredict.jl -- the clearance of a held plan against obstacles that move (include/obca_predict.h) for Julia (>= 1.6): the ccalls on libobca_hip.so, beside OBCAHip.jl
# (whose Batch / QuadBatch handles they take) and OBCASceneEdit.jl (whose motion, pivot and inflation the rates are, per second).  A predict call measures every sample of
# the last solution against the obstacles where they will be when the vehicle gets there; nothing is written to the batch.
#
#   using .OBCAHip, .OBCAPredict
#   # bt: an obca_batch handle that has been uploaded and solved (B instances, nOb obstacles in all); ctx: the handle of the context it was created on
#   rec = OBCAPredict.predict_clearance(ctx, bt, B, rates; substeps=8, need=0.05)   # rates: 6 x nOb, (vx, vy, w, cx, cy, g) per obstacle in upload order; rec: 32 x B
#   resolve = findall(isfinite, rec[26, :])                                         # t_first is finite: the plan stops being clear at that time
#   prof = OBCAPredict.predict_profile(ctx, bt, B, N, 8)                            # after a call with keep_profile=true: (N S + 1) x B
#
# Julia arrays are column-major: rates is 6 x nOb (4 x 5 x B for the quadcopter), the records 32 x B, the profile (N S + 1) x B -- the dense arrays of the C calls with no
# copy.  The host-pointer calls take the arrays of the clearance calls of OBCAHip.jl, in their layout.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_predict_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_predict.py.
module OBCAPredict

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const PRD = LIB
const PRD_OUT = 32
const Rows = Union{Nothing,Array{Float64}}

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, what, ctx)
    rc == 0 || error("$what failed ($rc): " * lasterr(ctx))
end

ptr(a) = a === nothing ? C_NULL : a

"the last solution of a parking batch against obstacles moving at `rates` (6 x nOb): records 32 x B"
function predict_clearance(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, rates::Array{Float64}; substeps::Integer=8, need::Real=0.05, keep_profile::Bool=false)
    out = zeros(PRD_OUT, B)
    rc = ccall((:obca_batch_predict_clearance, PRD), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cint, Ptr{Cdouble}), bt, rates, substeps, need, keep_profile ? 1 : 0, out)
    check(rc, "obca_batch_predict_clearance", ctx)
    return out
end

"HIP-event duration of the last predict kernel on the parking batch [ms]"
function predict_clearance_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_batch_predict_clearance_ms, PRD), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_batch_predict_clearance_ms", ctx)
    return Float64(a[])
end

"the profile the last call with keep_profile=true left on the device: (N S + 1) x B"
function predict_profile(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer, substeps::Integer)
    out = zeros(N * substeps + 1, B)
    check(ccall((:obca_batch_predict_profile, PRD), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), bt, out, length(out)), "obca_batch_predict_profile", ctx)
    return out
end

"any parking trajectories: the arrays of OBCAHip's parking clearance call, then rates 6 x nOb; profile: (N S + 1) x B or nothing"
function parking_predict_batch(ctx::Ptr{Cvoid}, B::Integer, N::Integer, Ts::Array{Float64}, L::Real, ego::Array{Float64}, nOb::Array{Cint}, vOb::Array{Cint}, A::Array{Float64},
                               b::Array{Float64}, x::Array{Float64}, u::Array{Float64}, timeScale::Rows, rates::Array{Float64}; substeps::Integer=8, need::Real=0.05, profile::Rows=nothing)
    out = zeros(PRD_OUT, B)
    rc = ccall((:obca_parking_predict_batch, PRD), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble,
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, L, ego, nOb, vOb, A, b, x, u, ptr(timeScale), substeps, need, out, rates, ptr(profile))
    check(rc, "obca_parking_predict_batch", ctx)
    return out
end

"the same for the quadcopter's boxes; rates 4 x 5 x B, (vx, vy, vz, g) per box"
function quad_predict_clearance(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, rates::Array{Float64}; substeps::Integer=8, need::Real=0.0, keep_profile::Bool=false)
    out = zeros(PRD_OUT, B)
    rc = ccall((:obca_quad_batch_predict_clearance, PRD), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cint, Ptr{Cdouble}), bt, rates, substeps, need, keep_profile ? 1 : 0, out)
    check(rc, "obca_quad_batch_predict_clearance", ctx)
    return out
end

function quad_predict_clearance_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_quad_batch_predict_clearance_ms, PRD), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_quad_batch_predict_clearance_ms", ctx)
    return Float64(a[])
end

function quad_predict_profile(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer, substeps::Integer)
    out = zeros(N * substeps + 1, B)
    check(ccall((:obca_quad_batch_predict_profile, PRD), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), bt, out, length(out)), "obca_quad_batch_predict_profile", ctx)
    return out
end

"any quadcopter trajectories: x 12 x (N + 1) x B, timeScale (N + 1) x B, ob 6 x 5 x B, rates 4 x 5 x B; profile: (N S + 1) x B or nothing"
function quadcopter_predict_batch(ctx::Ptr{Cvoid}, B::Integer, N::Integer, Ts::Array{Float64}, R::Real, ob::Array{Float64}, x::Array{Float64}, timeScale::Array{Float64},
                                  rates::Array{Float64}; substeps::Integer=8, need::Real=0.0, profile::Rows=nothing)
    out = zeros(PRD_OUT, B)
    rc = ccall((:obca_quadcopter_predict_batch, PRD), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
               ctx, B, N, Ts, R, ob, x, timeScale, substeps, need, out, rates, ptr(profile))
    check(rc, "obca_quadcopter_predict_batch", ctx)
    return out
end

end # module
