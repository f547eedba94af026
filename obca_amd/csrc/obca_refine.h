// obca_refine.h -- a solved parking instance on a finer horizon, on the device: the same NLP with N' = r N stages of length Ts / r, started from the solution.  Both NLPs hold the
// obstacle separation at the nodes only; the clearance kernel finds what is lost between them, and the remedy for a constraint held at the nodes is a finer grid.  One
// wavefront (64 lanes) per DESTINATION instance; obca_amd/validate.py (refine_parking) is the numpy statement.  Write q = k r + s, 0 <= s < r; q = r N is the last node (k = N, s = 0).
//   header   : every word of the problem header bit for bit, except PH_TS = Ts / r (one fp64 division)
//   rx,ry,ryaw: ref'[q] = ref[k] + (s / r)(ref[k+1] - ref[k]) in the stored values, the product kept from contracting into the sum (rf_keep: the solver's SEAM); ref[k] itself at s = 0
//   x        : s = 0: node k of the source, bit for bit; else val::park_step(Ts, L, x_k, u_k, (double)s / (double)r * t1) with the SOURCE's Ts and t1 = the solution's t (1 with
//              fixTime; the host-pointer call: timeScale[k]) -- exactly the expression the clearance kernel evaluates for sample (k, s) at substeps = r: the refined NLP constrains
//              the very poses clearance(substeps = r) sampled
//   u        : u'[q] = u_k, a zero-order hold;  t' = 1, as every start of this project has it (ParkingSignedDist.jl:214)
//   lam, mu  : duals = 0: zeros (the destination's next solve runs DualMultWS);  duals = 1: stage q takes lam and mu of stage q / r as stored (the last node: N)
//   the rest : every other word of the row (sl, the slacks, all other multipliers, up to the row's stride) is cleared, as the upload's scatter does
// Status of a slot.  0: refined from the solution.  1: the source's last solve ended with exit flag 0 (info[7]), or x, u, t (with duals also lam, mu) of its iterate hold a
// non-finite number: refined the same way from the source's START iterate (with duals: its multipliers -- the uploaded ones, or zeros).  -1: the start iterate is not finite
// either: x' = u' = 0, t' = 1, zero multipliers -- what an upload without a warm start leaves.
// Every destination word has exactly one writer (word i of a range belongs to the lane that is dealt item i); source and destination are different buffers.  `rev` deals the
// items to the lanes backwards: the host build's test asks for the same bits.  Transcendentals are libm's / the device library's sin, cos, tan, inside val::park_step.
// The same text compiles for the host (-DOBCA_EMU) for tests/emu/refine_emu.cpp.  Nothing here is used by the solve kernels.
#pragma once
#include "obca_validate.h"

namespace obca {
namespace rfn {

static_assert(OB_NT == 64, "one wavefront per instance: wred_max reduces over 64 lanes");

#define RF_MAXFACTOR 32      // largest factor (= OBCA_REFINE_MAXFACTOR of include/obca_refine.h)

OBCA_FN double rf_keep(double x) { SEAM(x); return x; }      // a product that must not fuse with the sum it enters
// item of lane `lane` in round rd of `rounds`: ascending, or (rev) dealt backwards -- lanes and rounds
OBCA_FN int rf_item(int rd, int rounds, int lane, int rev) { return rev ? (rounds - 1 - rd) * OB_NT + (OB_NT - 1 - lane) : rd * OB_NT + lane; }
#define RF_DEAL(it, n, lane, rev) for (int rounds_ = ((n) + OB_NT - 1) / OB_NT, rd_ = 0, it; rd_ < rounds_; rd_++) if ((it = rfn::rf_item(rd_, rounds_, lane, rev)) < (n))

// the refusals of the entry points, one text for the library and the host build: n instances of horizon N by `factor`
static inline const char *refine_check_args(int n, int N, int factor, int duals) {
    if (n < 1) return "need n >= 1";
    if (factor < 1 || factor > RF_MAXFACTOR) return "need 1 <= factor <= 32";
    if (N < 1 || N > OB_NMAX || factor * N > OB_NMAX) return "need N >= 1 and factor * N <= OBCA_NMAX";
    if (duals != 0 && duals != 1) return "need duals 0 or 1";
    return nullptr;
}

// 1 if one of the `cnt` doubles at v is NaN or +-inf (wave-uniform)
OBCA_FN double rf_bad(const double *v, int cnt) {
    double b[OBCA_NL];
    PAR(lane) {
        double a = 0.0;
        for (int i = lane; i < cnt; i += OB_NT) a = val::vmax(a, val::vbad(v[i]));
        b[LI(lane)] = a;
    }
    return wred_max(b);
}

// The primal part.  x: 4 x (N + 1), u: 2 x N stage-contiguous; ts: timeScale per stage (N + 1) or nullptr (then t1 for every stage); xf: 4 x (r N + 1), uf: 2 x r N.
// The lane that is dealt node q writes x'[q] and u'[q].  Needs N >= 1, r >= 1.
OBCA_FN void refine_primal(int N, int r, double Ts, double L, const double *x, const double *u, const double *ts, double t1, int rev, double *xf, double *uf) {
    const int Nf = N * r;
    PAR(lane) {
        RF_DEAL(q, Nf + 1, lane, rev) {
            const int k = q / r, s = q - k * r;      // (q = Nf: k = N, s = 0)
            double xk[4];
#pragma unroll
            for (int i = 0; i < 4; i++) xk[i] = x[4 * k + i];
            if (s) {
                const double uk[2] = {u[2 * k], u[2 * k + 1]};
                double F[4];
                val::park_step(Ts, L, xk, uk, (double)s / (double)r * (ts ? ts[k] : t1), F);
#pragma unroll
                for (int i = 0; i < 4; i++) xk[i] = F[i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) xf[4 * q + i] = xk[i];
            if (q < Nf) { uf[2 * q] = u[2 * k]; uf[2 * q + 1] = u[2 * k + 1]; }
        }
    }
}

// One instance of the host-pointer call: Ts' = Ts / r and the primal part.  A non-finite number among Ts, x, u, timeScale marks the instance: its outputs are NaN.  Returns 0 / 1.
OBCA_FN int refine_host_instance(int N, int r, double Ts, double L, const double *x, const double *u, const double *ts, int rev, double *Tsf, double *xf, double *uf) {
    const int Nf = N * r;
    const double bad = val::vmax(val::vmax(val::vbad(Ts), rf_bad(x, 4 * (N + 1))), val::vmax(rf_bad(u, 2 * N), ts ? rf_bad(ts, N + 1) : 0.0));
    if (bad != 0.0) {
        const double nan_ = __builtin_nan("");
        PAR(lane) {
            RF_DEAL(i, 4 * (Nf + 1), lane, rev) xf[i] = nan_;
            RF_DEAL(i, 2 * Nf, lane, rev) uf[i] = nan_;
            if (lane == 0) *Tsf = nan_;
        }
        return 1;
    }
    refine_primal(N, r, Ts, L, x, u, ts, 1.0, rev, xf, uf);
    PAR(lane) { if (lane == 0) *Tsf = Ts / (double)r; }
    return 0;
}

// The resident call.  ps: the source's problem record (header | rx | ry | ryaw at horizon N), zs: its last iterate, z0s: its start iterate, info: the 8 doubles of its last
// solve; pd: the destination's problem record (horizon r N), zd: its start-iterate row of zlen doubles.  Returns the slot's status.  Needs N >= 1, r >= 1, r N <= OB_NMAX.
OBCA_FN int refine_record(int N, int r, int duals, const double *ps, const double *zs, const double *z0s, const double *info, int rev, double *pd, double *zd, int zlen) {
    const int nOb = (int)ps[PH_NOB], M = (int)ps[PH_M], Nf = N * r, N1 = N + 1, Nf1 = Nf + 1;
    Lay ls, ld; make_layout(N, nOb, M, ls); make_layout(Nf, nOb, M, ld);
    const int nprim = 4 * N1 + 2 * N + 1, ndual = (M + 4 * nOb) * N1;      // x, u, t and lam, mu are contiguous in the layout
    int st = 0;
    if (info[7] == 0.0 || rf_bad(zs + ls.x, nprim) != 0.0 || (duals && rf_bad(zs + ls.lam, ndual) != 0.0)) st = 1;
    if (st && (rf_bad(z0s + ls.x, nprim) != 0.0 || (duals && rf_bad(z0s + ls.lam, ndual) != 0.0))) st = -1;
    const double *src = st ? z0s : zs;
    const double Ts = ps[PH_TS], t1 = ps[PH_FIX] != 0.0 ? 1.0 : src[ls.t];
    PAR(lane) {
        RF_DEAL(i, OB_HDR, lane, rev) pd[i] = i == PH_TS ? Ts / (double)r : ps[i];
        RF_DEAL(it, 3 * Nf1, lane, rev) {
            const int a = it / Nf1, q = it - a * Nf1, k = q / r, s = q - k * r;
            const double *ref = ps + OB_HDR + a * N1;
            pd[OB_HDR + it] = s ? ref[k] + rf_keep((double)s / (double)r * (ref[k + 1] - ref[k])) : ref[k];
        }
    }
    if (st >= 0) refine_primal(N, r, Ts, ps[PH_L], src + ls.x, src + ls.u, nullptr, t1, rev, zd + ld.x, zd + ld.u);
    PAR(lane) {
        if (st < 0) { RF_DEAL(i, ld.t, lane, rev) zd[i] = 0.0; }
        if (lane == 0) zd[ld.t] = 1.0;
        const bool carry = duals && st >= 0;
        RF_DEAL(i, M * Nf1, lane, rev) { const int q = i / M, c = i - q * M; zd[ld.lam + i] = carry ? src[ls.lam + (q / r) * M + c] : 0.0; }
        RF_DEAL(i, 4 * nOb * Nf1, lane, rev) { const int q = i / (4 * nOb), c = i - q * 4 * nOb; zd[ld.mu + i] = carry ? src[ls.mu + (q / r) * 4 * nOb + c] : 0.0; }
        RF_DEAL(i, zlen - ld.sl, lane, rev) zd[ld.sl + i] = 0.0;
    }
    return st;
}

}  // namespace rfn
}  // namespace obca
