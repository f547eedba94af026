# OBCAPlanResident.jl -- the resident route of the parking planner (include/obca_plan_resident.h) for Julia (>= 1.6): the ccalls on libobca_hip.so, beside OBCAHip.jl,
# OBCAPlanDevice.jl (whose `configure` sets the slots this call uses too) and OBCAPathWS.jl.  An uploaded batch is planned on the GPU from what it holds -- x0, xF, its
# own obstacle rows, the uploaded ego, L and XYbounds -- and the warm start is written into it; only the per-instance ints come back.
#
#   using .OBCAHip, .OBCAPlanResident
#   # bt: an obca_batch handle that obca_batch_upload has filled (B instances); ctx: the handle of the context it was created on
#   r = OBCAPlanResident.plan_warm_start!(ctx, bt, B)                 # upload -> plan -> solve: obca_batch_solve starts from the planned paths
#   r.counts[i] >= 2 && r.status[i] == 0                              # instance i has a path and a warm start; a negative status keeps the uploaded start
#   p = OBCAPlanResident.plan_paths(ctx, bt, B)                       # p.paths[:, 1:r.counts[i], i]: the poses of instance i, for plots
#
# Julia arrays are column-major: paths is 3 x cap x B, dirs cap x B, inst 10 x B -- the dense arrays of the C call with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_plan_resident_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_plan_resident.py.
module OBCAPlanResident

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const PLR = LIB
const MAXCAP = 1024      # OBCA_PATH_WS_MAXNODES

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

"plans the B instances of the uploaded batch `bt` on the GPU and writes their warm starts into it: (counts, status, expansions, rounds), B Cints each"
function plan_warm_start!(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; opts::Union{Nothing,Vector{Float64}}=nothing, bucket_width::Real=0.0, cap::Integer=1024,
                          use_xF::Bool=true, v_nom::Real=0.5, smooth::Bool=false)
    2 <= cap <= MAXCAP || error("need 2 <= cap <= $MAXCAP")
    counts = zeros(Cint, B); status = zeros(Cint, B); nexp = zeros(Cint, B); rounds = zeros(Cint, B)
    rc = ccall((:obca_batch_plan_warm_start, PLR), Cint,
               (Ptr{Cvoid}, Ptr{Cdouble}, Cint, Cdouble, Cint, Cint, Cdouble, Cdouble, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
               bt, opts === nothing ? C_NULL : opts, opts === nothing ? 0 : length(opts), bucket_width, cap, use_xF ? 1 : 0, v_nom, smooth ? 0.3 : 0.0,
               counts, status, nexp, rounds)
    rc == 0 || error("obca_batch_plan_warm_start failed ($rc): " * lasterr(ctx))
    return (counts=counts, status=status, expansions=nexp, rounds=rounds)
end

"HIP-event durations of the three kernels of the last plan_warm_start! on the batch [ms]: (pack, search, ws)"
function plan_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0); b = Ref{Cfloat}(0); c = Ref{Cfloat}(0)
    rc = ccall((:obca_batch_plan_ms, PLR), Cint, (Ptr{Cvoid}, Ref{Cfloat}, Ref{Cfloat}, Ref{Cfloat}), bt, a, b, c)
    rc == 0 || error("obca_batch_plan_ms failed ($rc): " * lasterr(ctx))
    return (pack=Float64(a[]), search=Float64(b[]), ws=Float64(c[]))
end

"what the last plan_warm_start! (with this `cap`) planned: paths 3 x cap x B, dirs cap x B, inst 10 x B (start and goal with sin, cos of their headings)"
function plan_paths(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; cap::Integer=1024)
    paths = zeros(3, cap, B); dirs = zeros(Cint, cap, B); inst = zeros(10, B)
    rc = ccall((:obca_batch_plan_download, PLR), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cint}, Cint, Ptr{Cdouble}), bt, paths, dirs, cap, inst)
    rc == 0 || error("obca_batch_plan_download failed ($rc): " * lasterr(ctx))
    return (paths=paths, dirs=dirs, inst=inst)
end

end # module
