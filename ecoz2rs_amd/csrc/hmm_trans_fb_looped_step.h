// hmm_trans_fb_looped_step.h -- the frames of the looped forward-backward under class-to-class prices (DESIGN.md 4.8.13 and
// 4.8.14, "The looped body"), written once for its two kernels (hmm_posterior_trans_looped.hip: the class posteriors;
// hmm_trans_estep_looped.hip: the E-step of the matrix): the whole forward frame, and of a backward frame the two parts that
// both passes share -- bh_t from what the previous frame left, and u_t with its chain and the post of R_t.  What lies between
// them (the posterior's class sum, the E-step's S_t and its products) is the kernels' own.
// The arithmetic is the resident bodies' (hmm_posterior_trans.hip), operation for operation, through hmm_lane.h's chains and
// sums, so every ah, c, bh, S and R has the resident bits; only who runs it when differs:
//   forward, t >= 1   pass A over the wave's slots: ah_{t-1} = x_{t-1} / c_{t-1} by the state's own lane (stored to ahs there),
//                     chain_col_mass, the class's state-0 lane posts S[k], acc is carried.  Barrier: m[k] needs S of every
//                     class.  Pass B: the walk over the K sources from source 0, x = (acc + m pi_j) b, slot_sum to
//                     parts[parity][slot].  Barrier, then slots_sum over all `slots` partials from slot 0 (a wave never adds
//                     up its own partials first).  Two barriers a frame, as the resident body has.
//   backward          one pass and one barrier a frame: at the head of a slot's turn of frame t the lane walks r[f] along
//                     w[f][.] over R_{t+1}, which the previous frame posted, and bh_t = acc + r; at the end of the turn
//                     chain_row_pi over u_t posts R_t and acc is carried.  R is double-buffered: other waves post R_t while
//                     this one still reads R_{t+1}.
// What outlives a turn lives in one LDS array sv of sumN doubles, indexed by the composite state and touched by that state's
// own lane alone (hmm_posterior_looped.hip's argument: a register file as long as the wave's turns, no fence and no barrier
// of its own).  It holds x_{t-1} into pass A, acc across the barrier, x_t out of pass B; backward, acc across the barrier.
// pi is read in place (it cannot be mandatory in LDS at 4096 states): chain_row_pi takes the class's row of the parameter block.
// Device code only.  Internal.
#pragma once
#include "hmm_lane.h"

namespace e2hmm {

namespace {

// the lane of slot sl and the slot's chain route (wave-uniform).  A lane without a state: N = 0, j = 0, a_at = 0, ld = 0,
// class 0 in the walks (its reads stay in bounds), its values are kept at +0.0.
struct FbLane {
    SegLaneDev L;
    bool act, head;  // the lane has a state; it posts and writes for its class
    int c, k, ld;    // composite index, class, leading dimension of the class's A (N | 1)
    int maxN;
    bool single;
};

__device__ __forceinline__ FbLane fb_lane(const SegPlanDev& pl, int sl, int lane)
{
    FbLane q;
    q.L = pl.lanes[sl * 64 + lane];
    q.act = q.L.cls >= 0;
    q.head = q.act && q.L.j == 0;
    q.c = q.act ? q.L.comp : 0;
    q.k = q.act ? q.L.cls : 0;
    q.ld = q.act ? (q.L.N | 1) : 0;
    q.maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl]);
    q.single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl + 1]) != 0;
    return q;
}

// what the frames read: the parameter block's parts (A in LDS or in place), w followed by wT (in LDS or in place), and the
// LDS arrays of the header
struct FbTables {
    const double* pig;  // [sumN]
    const double* A;
    const double* Bg;   // [sumN][M]
    const double* wm;   // w (K x K) | wT (K x K)
    double* parts;      // [2][slots]
    double* Xb;         // [2][K]
    double* sv;         // [sumN]
};

// One forward frame of the whole workgroup: -> c_t, the same bits in every lane.  o: the frame's symbol (< M, checked by the
// caller before any arithmetic or barrier of the frame).  cprev: c_{t-1}.  aprev: the row of ahs of frame t - 1 (t >= 1).
// call: the parity of parts, alternating per frame as in block_sum.
__device__ __forceinline__ double fb_forward_frame(const SegPlanDev& pl, const FbTables& tb, long long t, int o, double cprev,
                                                   double* aprev, int call, int wib, int lane, int nw)
{
    const int K = pl.K, M = pl.M, slots = pl.slots;
    double* pt = tb.parts + (size_t)(call & 1) * slots;
    if (t == 0) {
        for (int sl = wib; sl < slots; sl += nw) {
            const FbLane q = fb_lane(pl, sl, lane);
            const double bq = q.act ? tb.Bg[(size_t)q.c * M + o] : 0.0;
            const double pij = q.act ? tb.pig[q.c] : 0.0;
            double x = pij * bq;
            if (!q.act) x = 0.0;
            if (q.act) tb.sv[q.c] = x;
            const double v = slot_sum(x);
            if (lane == 0) pt[sl] = v;
        }
    } else {
        // S of step t lives in Xb[t & 1]: a wave writes that half again at t + 2, past the barriers of t + 1
        double* St = tb.Xb + (size_t)(t & 1) * K;
        // pass A: the in-class chain over ah_{t-1}, and on the way the class's mass S = CS(ah_{t-1})
        for (int sl = wib; sl < slots; sl += nw) {
            const FbLane q = fb_lane(pl, sl, lane);
            const double ah = q.act ? tb.sv[q.c] / cprev : 0.0;  // ah_{t-1} of this state
            if (q.act) aprev[q.c] = ah;
            const ChainPair cf = chain_col_mass(ah, tb.A + q.L.a_at + q.L.j, q.ld, q.L.N, q.L.seg, q.maxN, q.single);
            if (q.head) St[q.k] = cf.sum;
            if (q.act) tb.sv[q.c] = cf.acc;
        }
        __syncthreads();
        // pass B: the mass that enters class k, sources in class order; the emission is requested first, the walk hides it
        for (int sl = wib; sl < slots; sl += nw) {
            const FbLane q = fb_lane(pl, sl, lane);
            const double bq = q.act ? tb.Bg[(size_t)q.c * M + o] : 0.0;
            const double pij = q.act ? tb.pig[q.c] : 0.0;
            const double* wTrow = tb.wm + (size_t)K * K + (size_t)q.k * K;  // w[f][k] at wTrow[f]
            double m = St[0] * wTrow[0];
            for (int f = 1; f < K; ++f) m = m + St[f] * wTrow[f];
            const double acc = q.act ? tb.sv[q.c] : 0.0;
            double x = (acc + m * pij) * bq;
            if (!q.act) x = 0.0;
            if (q.act) tb.sv[q.c] = x;
            const double v = slot_sum(x);
            if (lane == 0) pt[sl] = v;
        }
    }
    __syncthreads();
    return slots_sum(pt, slots);
}

// bh_t of the lane at the head of its slot's turn: 1 at the last frame, else acc (carried in sv) + r[f], the walk along
// w[f][.] over Rn = R_{t+1}
__device__ __forceinline__ double fb_bh(const FbLane& q, bool last, const FbTables& tb, const double* Rn, int K)
{
    if (last) return q.act ? 1.0 : 0.0;
    const double* wrow = tb.wm + (size_t)q.k * K;  // w[f][k'] at wrow[k']
    double r = wrow[0] * Rn[0];
    for (int kk = 1; kk < K; ++kk) r = r + wrow[kk] * Rn[kk];
    const double acc = q.act ? tb.sv[q.c] : 0.0;
    return q.act ? acc + r : 0.0;
}

// the end of the turn of frame t >= 1: u_t, the in-class chain, and on the way what leaves through the class's pi; the
// state-0 lane posts R_t[k] to Rt, acc waits in sv for the turn of frame t - 1
__device__ __forceinline__ void fb_post_R(const FbLane& q, const FbTables& tb, double bq, double bh, double ct, double* Rt)
{
    const double u = q.act ? (bq * bh) / ct : 0.0;
    const ChainPair cr = chain_row_pi(u, tb.A + q.L.a_at + (size_t)q.L.j * q.ld, tb.pig + (q.c - q.L.j), q.L.N, q.L.seg, q.maxN,
                                      q.single);
    if (q.head) Rt[q.k] = cr.sum;
    if (q.act) tb.sv[q.c] = cr.acc;
}

}  // namespace

}  // namespace e2hmm
