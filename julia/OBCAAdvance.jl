# OBCAAdvance.jl -- one step of the closed receding-horizon loop on the device (include/obca_advance.h) for Julia (>= 1.6): the ccalls on libobca_hip.so, beside
# OBCAHip.jl (whose Batch / QuadBatch handles they take) and OBCARollout.jl (the open loop over the whole horizon).  An advance call drives the continuous model from the
# record's X0 over the first `shift` intervals of the last solution, adds the kick, and restarts the next solve from that state as the shift calls restart it -- one
# launch, the state never leaves the device.  The re-solve is the feedback of this loop; OBCATrack.jl is the tool between two re-solves.
#
#   using .OBCAHip, .OBCAAdvance
#   # bt: an obca_quad_batch handle that has been uploaded and solved (B instances, horizon N); ctx: the handle of the context it was created on
#   OBCAAdvance.quad_advance_log(ctx, bt, 40)                                 # room for 40 nodes per instance
#   for step in 1:20
#       # ... solve bt ...
#       r = OBCAAdvance.quad_advance(ctx, bt, B, 2; kick=kick)                # r.out[:, i]: the 40 doubles of instance i (include/obca_advance.h)
#   end
#   X = OBCAAdvance.quad_advance_log_states(ctx, bt, B)                       # X[:, k, i]: node k of the driven path of instance i
#
# Julia arrays are column-major: out is 40 x B, kick and the plant state are nx x B, the log is nx x nodes x B -- the dense arrays of the C calls with no copy.
# NOTE: Julia is not installed in the build environment of this repository, so this file has not been executed there; tests/test_advance_cpu.py checks every ccall
# against the header, parameter by parameter, and the same entry points are exercised through ctypes by tests/test_gpu_advance.py.
module OBCAAdvance

const LIB = get(ENV, "OBCA_HIP_LIBRARY", joinpath(@__DIR__, "..", "obca_amd", "csrc", "libobca_hip.so"))
const ADV = LIB
const OUT = 40          # OBCA_ADV_OUT
const Rows = Union{Nothing,Matrix{Float64}}

lasterr(ctx::Ptr{Cvoid}) = unsafe_string(ccall((:obca_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))

function check(rc, what, ctx)
    rc == 0 || error("$what failed ($rc): " * lasterr(ctx))
end

ptr(a) = a === nothing ? C_NULL : a

"one closed-loop step of a solved parking batch; kick: 4 x B or nothing: (out = 40 x B,)"
function advance(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, shift::Integer; substeps::Integer=8, kick::Rows=nothing, need::Real=0.05)
    out = zeros(OUT, B)
    rc = ccall((:obca_batch_advance, ADV), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}), bt, shift, substeps, ptr(kick), need, out)
    check(rc, "obca_batch_advance", ctx)
    return (out=out,)
end

"HIP-event duration of the last advance kernel on the parking batch [ms]"
function advance_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_batch_advance_ms, ADV), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_batch_advance_ms", ctx)
    return Float64(a[])
end

"the plant state the last advance left on the device: 4 x B"
function advance_state(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer)
    X = zeros(4, B)
    check(ccall((:obca_batch_advance_state, ADV), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, X), "obca_batch_advance_state", ctx)
    return X
end

"allocate (capacity > 0) or free (0) the log of driven node states"
function advance_log(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, capacity::Integer)
    check(ccall((:obca_batch_advance_log, ADV), Cint, (Ptr{Cvoid}, Cint), bt, capacity), "obca_batch_advance_log", ctx)
end

"the log: 4 x nodes x B"
function advance_log_states(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer)
    n = Ref{Cint}(0)
    check(ccall((:obca_batch_advance_log_states, ADV), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cint}), bt, C_NULL, n), "obca_batch_advance_log_states", ctx)
    X = zeros(4, Int(n[]), B)
    n[] > 0 && check(ccall((:obca_batch_advance_log_states, ADV), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cint}), bt, X, n), "obca_batch_advance_log_states", ctx)
    return X
end

"one closed-loop step of a solved quadcopter batch; kick, xF_new: 12 x B or nothing: (out = 40 x B,)"
function quad_advance(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer, shift::Integer; substeps::Integer=8, kick::Rows=nothing, xF_new::Rows=nothing, need::Real=0.0)
    out = zeros(OUT, B)
    rc = ccall((:obca_quad_batch_advance, ADV), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Ptr{Cdouble}), bt, shift, substeps, ptr(kick), ptr(xF_new), need, out)
    check(rc, "obca_quad_batch_advance", ctx)
    return (out=out,)
end

function quad_advance_ms(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid})
    a = Ref{Cfloat}(0)
    check(ccall((:obca_quad_batch_advance_ms, ADV), Cint, (Ptr{Cvoid}, Ref{Cfloat}), bt, a), "obca_quad_batch_advance_ms", ctx)
    return Float64(a[])
end

"the plant state the last advance left on the device: 12 x B"
function quad_advance_state(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer)
    X = zeros(12, B)
    check(ccall((:obca_quad_batch_advance_state, ADV), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), bt, X), "obca_quad_batch_advance_state", ctx)
    return X
end

function quad_advance_log(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, capacity::Integer)
    check(ccall((:obca_quad_batch_advance_log, ADV), Cint, (Ptr{Cvoid}, Cint), bt, capacity), "obca_quad_batch_advance_log", ctx)
end

"the log: 12 x nodes x B"
function quad_advance_log_states(ctx::Ptr{Cvoid}, bt::Ptr{Cvoid}, B::Integer)
    n = Ref{Cint}(0)
    check(ccall((:obca_quad_batch_advance_log_states, ADV), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cint}), bt, C_NULL, n), "obca_quad_batch_advance_log_states", ctx)
    X = zeros(12, Int(n[]), B)
    n[] > 0 && check(ccall((:obca_quad_batch_advance_log_states, ADV), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cint}), bt, X, n), "obca_quad_batch_advance_log_states", ctx)
    return X
end

end # module
