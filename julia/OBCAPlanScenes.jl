# OBCAPlanScenes.jl -- the parking planner on the GPU in per-instance obstacle fields (include/obca_plan_scenes.h) for Julia (>= 1.6): the ccalls on libobca_hip.so,
# beside OBCAHip.jl and OBCAPlanDevice.jl (whose `configure` sets the slots this call uses too).
#
#   using .OBCAHip, .OBCAPlanScenes
#   r = OBCAPlanScenes.scene_astar_batch(OBCAHip.ctx().h, starts, goals, vObs, As, bs, ego, L, XYbounds)      # starts, goals: 3 x B; vObs, As, bs: one entry per instance
#   r.paths[:, 1:r.counts[i], i]                                                                                # the poses of instance i, planned in ITS field
#
# Julia arrays are column-major: paths is 3 x cap x B, dirs cap x B -- the dense arrays of the C call with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_scenes_cpu.py checks every ccall against
# the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_scenes.py.
module OBCAPlanScenes

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const SCN = LIB
const STATUS = Dict(0 => "no path", -1 => "more nodes than cap", -2 => "the start or goal pose collides with the instance's own field", -3 => "a sizing limit of the slot was hit")

lasterr(h::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), h))

"B Hybrid A* searches on the GPU, search i in the obstacle field (vObs[i], As[i] (rows x 2), bs[i]) of its own instance; an instance may have no obstacle at all"
function scene_astar_batch(h::Ptr{Cvoid}, starts::Matrix{Float64}, goals::Matrix{Float64}, vObs::Vector{Vector{Cint}}, As::Vector{Matrix{Float64}}, bs::Vector{Vector{Float64}},
                           ego::Vector{Float64}, L::Real, XYbounds::Vector{Float64}; opts::Union{Nothing,Vector{Float64}}=nothing, bucket_width::Real=0.0, cap::Integer=1024)
    B = size(starts, 2)
    nOb = Cint[length(v) for v in vObs]
    vOb = isempty(vObs) ? Cint[] : reduce(vcat, vObs; init=Cint[])
    At = reduce(hcat, [Matrix{Float64}(transpose(A)) for A in As]; init=zeros(2, 0))      # the ABI's rows: M x 2 row-major, instance after instance
    b = reduce(vcat, bs; init=Float64[])
    paths = zeros(3, cap, B); dirs = zeros(Cint, cap, B); counts = zeros(Cint, B); nexp = zeros(Cint, B); rounds = zeros(Cint, B)
    rc = ccall((:obca_scene_astar_batch, SCN), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble,
                Ptr{Cdouble}, Ptr{Cint}, Cint, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}),
               h, B, starts, goals, nOb, vOb, At, b, ego, L, XYbounds, opts === nothing ? C_NULL : opts, opts === nothing ? 0 : length(opts), bucket_width,
               paths, dirs, cap, counts, nexp, rounds)
    rc == 0 || error("obca_scene_astar_batch failed ($rc): " * lasterr(h))
    return (paths=paths, dirs=dirs, counts=counts, expansions=nexp, rounds=rounds)
end

"duration of the last per-instance search kernel of the context [ms]"
function scene_astar_ms(h::Ptr{Cvoid})
    ms = Ref{Cfloat}(0)
    rc = ccall((:obca_scene_astar_ms, SCN), Cint, (Ptr{Cvoid}, Ref{Cfloat}), h, ms)
    rc == 0 || error("obca_scene_astar_ms failed ($rc): " * lasterr(h))
    return ms[]
end

end # module
