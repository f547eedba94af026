# OBCASceneEdit.jl -- a changing scene on the device (include/obca_scene_edit.h) for Julia (>= 1.6): the ccalls on libobca_hip.so, beside OBCAHip.jl (whose Batch /
# QuadBatch handles they take) and OBCAAdvance.jl (the closed loop they join).  A move call edits the obstacle words of the problem records of an uploaded batch in place,
# one wavefront per instance: the solved state, the start iterate, the last solution and the plant state stay, so the next solve restarts warm in the moved scene.
#
#   using .OBCAHip, .OBCAAdvance, .OBCASceneEdit
#   # bt: an obca_batch handle that has been uploaded and solved (B instances, nOb obstacles and M rows in all); ctx: the handle of the context it was created on
#   OBCAAdvance.advance(ctx, bt, B, 2)
#   st = OBCASceneEdit.move_obstacles(ctx, bt, B; motion=motion)              # motion: 3 x nOb, (dx, dy, dtheta) per obstacle in upload order; st[i] = 1: left as it was
#   # ... solve bt with the warm-restart options ...
#   A, b = OBCASceneEdit.obstacles(ctx, bt, M)                                # 2 x M and M: the unit-length rows as the device holds them
#
# Julia arrays are column-major: motion is 3 x nOb, pivot 2 x nOb, A 2 x M, the boxes 6 x 5 x B -- the dense arrays of the C calls with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_scene_edit_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_scene_edit.py.
module OBCASceneEdit

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const SED = LIB
const Rows = Union{Nothing,Array{Float64}}

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, what, ctx)
    rc == 0 || error("$what failed ($rc): " * lasterr(ctx))
end

ptr(a) = a === nothing ? C_NULL : a

"move and inflate the obstacles of an uploaded parking batch; motion 3 x nOb, pivot 2 x nOb, inflate nOb, or nothing: status (B), 1 = non-finite, left as it was"
function move_obstacles(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; motion::Rows=nothing, pivot::Rows=nothing, inflate::Rows=nothing)
    st = zeros(Cint, B)
    rc = ccall((:obca_batch_move_obstacles, SED), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}), bt, ptr(motion), ptr(pivot), ptr(inflate), st)
    check(rc, "obca_batch_move_obstacles", ctx)
    return st
end

"HIP-event duration of the last move kernel on the parking batch [ms]"
function move_obstacles_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_batch_move_obstacles_ms, SED), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_batch_move_obstacles_ms", ctx)
    return Float64(a[])
end

"the unit-length rows of the records as the device holds them: (A = 2 x M, b = M), M the rows of the batch in all"
function obstacles(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, M::Integer)
    A = zeros(2, M); b = zeros(M)
    check(ccall((:obca_batch_obstacles_download, SED), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), bt, A, b), "obca_batch_obstacles_download", ctx)
    return A, b
end

"the same for the quadcopter's boxes; motion 3 x 5 x B, inflate 5 x B, or nothing"
function quad_move_obstacles(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer; motion::Rows=nothing, inflate::Rows=nothing)
    st = zeros(Cint, B)
    rc = ccall((:obca_quad_batch_move_obstacles, SED), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}), bt, ptr(motion), ptr(inflate), st)
    check(rc, "obca_quad_batch_move_obstacles", ctx)
    return st
end

function quad_move_obstacles_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_quad_batch_move_obstacles_ms, SED), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_quad_batch_move_obstacles_ms", ctx)
    return Float64(a[])
end

"the boxes as the device holds them: 6 x 5 x B, [ub(3), -lb(3)] per box"
function quad_obstacles(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer)
    ob = zeros(6, 5, B)
    check(ccall((:obca_quad_batch_obstacles_download, SED), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, ob), "obca_quad_batch_obstacles_download", ctx)
    return ob
end

end # module
