# OBCAPathWS.jl -- parking warm starts from planner paths on the GPU (include/obca_path_ws.h; the entry points live in the library of the solves, OBCAHip.LIB).
# Stands between a Hybrid A* planner and OBCAHip.ParkingSignedDist_batch: the nodes of B paths go in, Ts / xWS / uWS come out in the orientation the solve takes
# (rx, ry, ryaw = rows 1-3 of xWS).  Arrays are Julia's column-major ones: paths 3 x cap x B (x, y, yaw per node), dirs cap x B (+1 / -1 per node, Cint), counts B (Cint),
# xF 4 x B, xWS 4 x (N+1) x B, uWS 2 x N x B (steering, acceleration).
#
#   include("OBCAHip.jl"); include("OBCAPathWS.jl")
#   Ts, xWS, uWS, status = OBCAPathWS.path_warm_start(paths, dirs, counts, N; xF=xF, v_nom=0.5)      # status 0: written; -1 no path, -2 too many nodes, -3 non-finite, -4 zero length
#   OBCAPathWS.set_path_warm_start!(h, B, paths, dirs, counts)                                         # h: an obca_batch handle that obca_batch_upload has filled
module OBCAPathWS

import ..OBCAHip

const PATHWS = OBCAHip.LIB
const L_WHEELBASE = 2.7
const MAXNODES = 1024      # OBCA_PATH_WS_MAXNODES

f64(a) = convert(Array{Float64}, a)
i32(a) = convert(Array{Cint}, a)

function _dense(paths, dirs, counts)
    p = f64(paths); d = i32(dirs); c = i32(vec(counts)); B = length(c)
    size(p, 1) == 3 && size(p, 3) == B && size(d) == (size(p, 2), B) || error("paths must be 3 x cap x B, dirs cap x B, counts B")
    return p, d, c, B, size(p, 2)
end

"warm starts of B paths: (Ts B, xWS 4 x (N+1) x B, uWS 2 x N x B, status B); smooth: the speed profile goes through the velocity smoother at 0.3 m/s^2"
function path_warm_start(paths, dirs, counts, N::Integer; xF=nothing, v_nom=0.5, L=L_WHEELBASE, smooth::Bool=false, context::OBCAHip.Context=OBCAHip.ctx())
    p, d, c, B, cap = _dense(paths, dirs, counts)
    g = xF === nothing ? C_NULL : f64(xF)
    xF === nothing || size(g) == (4, B) || error("xF must be 4 x B")
    Ts = zeros(B); xWS = zeros(4, N + 1, B); uWS = zeros(2, N, B); status = zeros(Cint, B)
    rc = ccall((:obca_parking_path_warm_start_batch, PATHWS), Cint,
               (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Cint, Ptr{Cdouble}, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cint}),
               context.h, B, N, p, d, c, cap, g, v_nom, L, smooth ? 0.3 : 0.0, Ts, xWS, uWS, status)
    rc == 0 || error("obca_parking_path_warm_start_batch failed: " * OBCAHip.lasterr(context))
    return Ts, xWS, uWS, status
end

"the same into the resident batch `h` (B instances): Ts, reference and start iterate are rewritten on the device; returns the status per instance.\n`context` must be the context `h` was created on: the library leaves the message of a failed call there, and this function reads it from there."
function set_path_warm_start!(h::Ptr{Cvoid}, B::Integer, paths, dirs, counts; v_nom=0.5, smooth::Bool=false, use_xF::Bool=true, context::OBCAHip.Context=OBCAHip.ctx())
    p, d, c, nB, cap = _dense(paths, dirs, counts)
    nB == B || error("counts must have one entry per instance of the batch")
    status = zeros(Cint, B)
    rc = ccall((:obca_batch_set_path_warm_start, PATHWS), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cint}, Ptr{Cint}, Cint, Cint, Cdouble, Cdouble, Ptr{Cint}),
               h, p, d, c, cap, use_xF ? 1 : 0, v_nom, smooth ? 0.3 : 0.0, status)
    rc == 0 || error("obca_batch_set_path_warm_start failed: " * OBCAHip.lasterr(context))
    return status
end

"duration of the last set_path_warm_start! kernel on the batch `h` [ms]"
function path_ws_ms(h::Ptr{Cvoid})
    ms = Ref{Cfloat}(0)
    ccall((:obca_batch_path_ws_ms, PATHWS), Cint, (Ptr{Cvoid}, Ref{Cfloat}), h, ms) == 0 || error("obca_batch_path_ws_ms failed")
    return Float64(ms[])
end

end
