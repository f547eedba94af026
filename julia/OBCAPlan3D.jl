# OBCAPlan3D.jl -- thin wrapper of libobca_plan3d.so (include/obca_plan3d.h): the quadcopter's 3-D grid planner on the GPU, a batch of searches per call.
# Stands where mainQuadcopter.jl:124-128 calls a_star_3D.jl, for many start / goal pairs at once.  A module of its own: OBCAHip.jl (the drop-in of the solves) does not
# need it.  Arrays are Julia's column-major ones: starts / goals 3 x B, x0 / xF 12 x B, boxes 6 x nBox x B (or 6 x nBox, shared), xWS 12 x (N+1) x B -- what
# OBCAHip.QuadcopterSignedDistBatch takes.
#
#   using OBCAPlan3D
#   xWS, ok = OBCAPlan3D.warm_start_batch(x0, xF, N)            # boxes = the five of mainQuadcopter.jl:36-54, clear = 0.4, room = (10, 10, 5), res = 0.25
#   paths = OBCAPlan3D.paths_batch(starts, goals)               # Vector of 3 x K way-point matrices, `nothing` where there is no path
module OBCAPlan3D

const PLAN3D = get(ENV, "OBCA_PLAN3D_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_plan3d.so"))
const QUAD_OB = Float64[2.5 7.5 7.5 7.5 7.5; 10 10 4 5 5; 5 5 5 2 5; -2 -7 -7 -7 -7; 0 -5 0 -4 -4; -0.6 0 0 0 -3]      # 6 x 5: [xmax,ymax,zmax,-xmin,-ymin,-zmin] per box
const QUAD_ROOM = Float64[10, 10, 5]

mutable struct Planner
    h::Ptr{Cvoid}
end

function Planner(device::Integer=0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:obca_plan3d_create, PLAN3D), Cint, (Cint, Ref{Ptr{Cvoid}}), device, r)
    rc == 0 || error("obca_plan3d_create failed: " * unsafe_string(ccall((:obca_plan3d_last_error, PLAN3D), Cstring, (Ptr{Cvoid},), C_NULL)))
    p = Planner(r[])
    finalizer(x -> ccall((:obca_plan3d_destroy, PLAN3D), Cint, (Ptr{Cvoid},), x.h), p)
    return p
end

const _planner = Ref{Union{Nothing,Planner}}(nothing)
planner() = (_planner[] === nothing && (_planner[] = Planner()); _planner[])
lasterr(p::Planner) = unsafe_string(ccall((:obca_plan3d_last_error, PLAN3D), Cstring, (Ptr{Cvoid},), p.h))
f64(a) = convert(Array{Float64}, a)
boxes_for(boxes, B) = ndims(boxes) == 3 ? f64(boxes) : repeat(reshape(f64(boxes), 6, :, 1), 1, 1, B)

"way-points of B searches: a Vector of 3 x K matrices (start point, grid nodes, goal point) or `nothing` (no path, or an end point is blocked)"
function paths_batch(starts, goals; boxes=QUAD_OB, clear=0.4, room=QUAD_ROOM, res=0.25, cap=256, p::Planner=planner())
    s = f64(starts)[1:3, :]; g = f64(goals)[1:3, :]; B = size(s, 2)
    bx = boxes_for(boxes, B); paths = zeros(3, cap, B); counts = zeros(Cint, B); sweeps = zeros(Cint, B)
    rc = ccall((:obca_plan3d_paths_batch, PLAN3D), Cint,
               (Ptr{Cvoid}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cint, Ptr{Cint}, Ptr{Cint}),
               p.h, B, s, g, size(bx, 2), bx, clear, f64(room), res, paths, cap, counts, sweeps)
    rc == 0 || error("obca_plan3d_paths_batch failed: " * lasterr(p))
    any(counts .== -1) && error("a path has more than cap = $cap way-points")
    return [counts[i] >= 2 ? paths[:, 1:counts[i], i] : nothing for i in 1:B]
end

"warm starts of B quadcopter solves: (xWS 12 x (N+1) x B, ok::Vector{Bool}); an instance without a path has ok false and a zero warm start"
function warm_start_batch(x0, xF, N::Integer; boxes=QUAD_OB, clear=0.4, room=QUAD_ROOM, res=0.25, p::Planner=planner())
    a = f64(x0); b = f64(xF); B = size(a, 2)
    size(a, 1) == 12 && size(b, 1) == 12 || error("x0 and xF are 12 x B")
    bx = boxes_for(boxes, B); xWS = zeros(12, N + 1, B); counts = zeros(Cint, B)
    rc = ccall((:obca_plan3d_warm_start_batch, PLAN3D), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}, Ptr{Cint}),
               p.h, B, N, a, b, size(bx, 2), bx, clear, f64(room), res, xWS, counts)
    rc == 0 || error("obca_plan3d_warm_start_batch failed: " * lasterr(p))
    return xWS, counts .>= 2
end

"duration of the last call's kernel on the device [ms]"
function kernel_ms(p::Planner=planner())
    ms = Ref{Cfloat}(0)
    ccall((:obca_plan3d_kernel_ms, PLAN3D), Cint, (Ptr{Cvoid}, Ref{Cfloat}), p.h, ms) == 0 || error("obca_plan3d_kernel_ms failed")
    return Float64(ms[])
end

end
