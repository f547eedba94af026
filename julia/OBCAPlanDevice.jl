# OBCAPlanDevice.jl -- the parking planner on the GPU (include/obca_plan_device.h) for Julia (>= 1.6): the ccalls on libobca_hip.so, beside OBCAHip.jl.
#
#   using .OBCAHip, .OBCAPlanDevice
#   r = OBCAPlanDevice.hybrid_astar_batch(OBCAHip.ctx().h, starts, goals, vOb, A, b, ego, L, XYbounds)      # starts, goals: 3 x B
#   r.paths[:, 1:r.counts[i], i]                                                                              # the poses of instance i
#
# Julia arrays are column-major: paths is 3 x cap x B, dirs cap x B -- the dense arrays of the C call with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_hybrid_cpu.py checks every ccall against
# the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_hybrid.py.
module OBCAPlanDevice

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const HYB = LIB
const STATUS = Dict(0 => "no path", -1 => "more nodes than cap", -2 => "the start or goal pose collides", -3 => "a sizing limit of the slot was hit")

lasterr(h::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), h))

"slots of the context's planner: searches in flight, nodes and bucket chunks per search (0 = the default)"
function configure(h::Ptr{Cvoid}; slots::Integer=0, max_nodes::Integer=0, max_chunks::Integer=0)
    rc = ccall((:obca_hybrid_configure, HYB), Cint, (Ptr{Cvoid}, Cint, Cint, Cint), h, slots, max_nodes, max_chunks)
    rc == 0 || error("obca_hybrid_configure failed ($rc): " * lasterr(h))
    return nothing
end

"B Hybrid A* searches in one obstacle field on the GPU; opts: the option array of include/obca_plan.h (or nothing), bucket_width <= 0: the library's default"
function hybrid_astar_batch(h::Ptr{Cvoid}, starts::Matrix{Float64}, goals::Matrix{Float64}, vOb::Vector{Cint}, A::Matrix{Float64}, b::Vector{Float64},
                            ego::Vector{Float64}, L::Real, XYbounds::Vector{Float64}; opts::Union{Nothing,Vector{Float64}}=nothing, bucket_width::Real=0.0, cap::Integer=1024)
    B = size(starts, 2)
    At = Matrix{Float64}(transpose(A))      # the ABI's rows: M x 2 row-major
    paths = zeros(3, cap, B); dirs = zeros(Cint, cap, B); counts = zeros(Cint, B); nexp = zeros(Cint, B); rounds = zeros(Cint, B)
    rc = ccall((:obca_hybrid_astar_batch, HYB), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble,
                Ptr{Cdouble}, Ptr{Cint}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
               h, B, starts, goals, length(vOb), vOb, At, b, ego, L, XYbounds, opts === nothing ? C_NULL : opts, opts === nothing ? 0 : length(opts), bucket_width,
               paths, dirs, cap, counts, nexp, rounds)
    rc == 0 || error("obca_hybrid_astar_batch failed ($rc): " * lasterr(h))
    return (paths=paths, dirs=dirs, counts=counts, expansions=nexp, rounds=rounds)
end

"duration of the last search kernel of the context [ms]"
function hybrid_ms(h::Ptr{Cvoid})
    ms = Ref{Cfloat}(0)
    rc = ccall((:obca_hybrid_ms, HYB), Cint, (Ptr{Cvoid}, Ref{Cfloat}), h, ms)
    rc == 0 || error("obca_hybrid_ms failed ($rc): " * lasterr(h))
    return ms[]
end

end # module
