# OBCAQuadPlanResident.jl -- the resident route of the quadcopter's grid planner (include/obca_quad_plan_resident.h) for Julia (>= 1.6): the ccalls on libobca_hip.so,
# beside OBCAHip.jl (whose QuadBatch handle they take) and OBCAPlan3D.jl (the host-pointer planner, a library of its own).  An uploaded quadcopter batch is planned on the
# GPU from what it holds -- x0, xF and the five boxes of every instance -- and the resampled path is written into the instance's warm start; only the selection goes up and
# two Cints per instance come back.
#
#   using .OBCAHip, .OBCAQuadPlanResident
#   # bt: an obca_quad_batch handle that obca_quad_batch_upload has filled (B instances, horizon N); ctx: the handle of the context it was created on
#   r = OBCAQuadPlanResident.plan_warm_start!(ctx, bt, B; timeWS=1.0)      # upload -> plan -> solve: obca_quad_batch_solve starts from the planned paths
#   r.counts[i] >= 2                                                       # instance i has a path and a new warm start; below 2 it keeps the uploaded one
#   again = findall(e -> e == 0, exitflag) .- 1                            # replan only the instances whose solve failed (0-based indices)
#   OBCAQuadPlanResident.plan_warm_start!(ctx, bt, B; select=again)
#   s = OBCAQuadPlanResident.warm_start(ctx, bt, B, N)                     # s.xWS[:, :, i]: the 12 x (N+1) start instance i will solve from
#
# Julia arrays are column-major: paths is 3 x cap x B, xWS 12 x (N+1) x B -- the dense arrays of the C call with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_quad_plan_resident_cpu.py checks every
# ccall against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_quad_plan_resident.py.
module OBCAQuadPlanResident

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const QPR = LIB
const WS_CAP = 1024      # OBCA_PLAN3D_WS_CAP
const SKIPPED = -4       # OBCA_QUAD_PLAN_SKIPPED
const ROOM = [10.0, 10.0, 5.0]

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

"plans the instances `select` (0-based, distinct; nothing: all B) of the uploaded batch `bt` on the GPU and writes their warm starts into it: (counts, sweeps), B Cints each"
function plan_warm_start!(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; clear::Real=0.4, room::Vector{Float64}=ROOM, res::Real=0.25, cap::Integer=WS_CAP,
                          select::Union{Nothing,AbstractVector{<:Integer}}=nothing, timeWS::Union{Nothing,Real}=nothing)
    2 <= cap <= WS_CAP || error("need 2 <= cap <= $WS_CAP")
    length(room) == 3 || error("room has three entries")
    counts = zeros(Cint, B); sweeps = zeros(Cint, B)
    sel = select === nothing ? Cint[] : convert(Vector{Cint}, select)
    tws = timeWS === nothing ? Cdouble[] : Cdouble[timeWS]
    rc = ccall((:obca_quad_batch_grid_plan_warm_start, QPR), Cint,
               (Ptr{Cvoid}, Cdouble, Ptr{Cdouble}, Cdouble, Cint, Ptr{Cint}, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}),
               bt, clear, room, res, cap, select === nothing ? C_NULL : sel, length(sel), timeWS === nothing ? C_NULL : tws, counts, sweeps)
    rc == 0 || error("obca_quad_batch_grid_plan_warm_start failed ($rc): " * lasterr(ctx))
    return (counts=counts, sweeps=sweeps)
end

"HIP-event duration of the kernel of the last plan_warm_start! on the batch [ms]"
function plan_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    rc = ccall((:obca_quad_batch_grid_plan_ms, QPR), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a)
    rc == 0 || error("obca_quad_batch_grid_plan_ms failed ($rc): " * lasterr(ctx))
    return Float64(a[])
end

"the way-points of the last plan_warm_start!: 3 x cap x B (start point, grid nodes, goal point; zeros behind an instance's count)"
function plan_paths(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer)
    cap = ccall((:obca_quad_batch_grid_plan_download, QPR), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), bt, C_NULL, 0)      # no array: the last call's cap
    cap >= 2 || error("obca_quad_batch_grid_plan_download failed ($cap): " * lasterr(ctx))
    paths = zeros(3, cap, B)
    rc = ccall((:obca_quad_batch_grid_plan_download, QPR), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), bt, paths, cap)
    rc == 0 || error("obca_quad_batch_grid_plan_download failed ($rc): " * lasterr(ctx))
    return paths
end

"the start the next solve of the batch begins from, read from the device: xWS 12 x (N+1) x B, timeWS B"
function warm_start(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, N::Integer)
    xWS = zeros(12, N + 1, B); timeWS = zeros(B)
    rc = ccall((:obca_quad_batch_start_download, QPR), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), bt, xWS, timeWS)
    rc == 0 || error("obca_quad_batch_start_download failed ($rc): " * lasterr(ctx))
    return (xWS=xWS, timeWS=timeWS)
end

end # module
