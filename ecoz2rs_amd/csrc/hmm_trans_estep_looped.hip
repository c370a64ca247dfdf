// hmm_trans_estep_looped.hip -- the looped body of `hmm transitions --em` (gfx950; DESIGN.md 4.8.14, "The looped body"): the
// expected bigram counts of hmm_trans_estep.hip for classes that take any number of wave-slots.  The contract is the resident
// body's, operation for operation: forward, scaling, status and backward are the looped posteriors' frames
// (hmm_trans_fb_looped_step.h; hmm_posterior_trans_looped.hip), and what that kernel throws away is kept:
//   xi_t[f][k] = S_t[f] * (w[f][k] * R_t[k])     t = 1 .. T - 1
//   k_hmm_trans_estep_looped   one workgroup per stream, min(slots, 16) waves; wave w serves the slots w, w + nw, .. in turn,
//                              and lane l of slot sl is the state pl.lanes[sl * 64 + l] for the whole stream.
// How the points that decide the bits are met:
//   S_t[f]     chain_sum over ah_{t-1}, loaded from the forward table by the lane that stored it: the bits the forward pass
//              used (chain_col_mass and chain_sum add the states in the same order), as the resident kernel argues.  It is
//              formed in the slot's turn of frame t and waits in a second carried array sS (sumN doubles, the state's own lane
//              only) for R_t.
//   products   R_t is whole only behind the barrier of frame t, so lane (f, i) forms S_t[f] * (w[f][k] * R_t[k]) for its
//              targets k = i, i + N_f, .. at the head of the slot's next turn (frame t - 1), where it walks R_t anyway; a
//              trailing pass behind the last barrier covers t = 1.  w[f][k] * R_t[k] is the very term the walk adds into r[f].
//              They go through an_add into the C table; the counts are integer limbs, so their order is free, and a zero
//              product issues no atomic.
//   C          2 K^2 int64 in LDS (flushed once a stream, a zero word adds nothing) or the global table directly (c_lds, the
//              host's choice).  A stream of status != 0 adds nothing to C; word 2 K^2 counts the status-0 streams, word
//              2 K^2 + 1 the others.
//   LDS        mandatory: the partials of both parities (2 slots), S / R of two steps (2 K), sv and sS (2 sumN).  Behind them,
//              in trans_estep_layout's order: the C table, A, then w with wT.  pi stays in the parameter block.
// Nothing transcendental runs here; the unit is compiled with -ffp-contract=off.
#include "hmm_limbs.h"
#include "hmm_trans_fb_looped_step.h"

namespace e2hmm {

namespace {

// the counts of the step into frame t of class f = q.k: this lane's share of the K targets, from S_t (carried) and Rt = R_t
__device__ __forceinline__ void estep_products(const FbLane& q, const FbTables& tb, const double* sS, const double* Rt, int K,
                                               bool c_lds, i64* Cs, i64* acc)
{
    if (!q.act) return;
    const double S = sS[q.c];
    const double* wrow = tb.wm + (size_t)q.k * K;
    i64* crow_l = Cs + (size_t)q.k * K * 2;
    i64* crow_g = acc + (size_t)q.k * K * 2;
    for (int kk = q.L.j; kk < K; kk += q.L.N) an_add(c_lds, crow_l + 2 * kk, crow_g + 2 * kk, S * (wrow[kk] * Rt[kk]));
}

}  // namespace

// grid: the streams of the launch, block: 64 x min(slots, 16).  Dynamic LDS: 2 x slots partials | 2 x K class masses | sv |
// sS (sumN doubles each) | the C table, 2 K^2 int64 (c_lds) | A of every class (A_LDS) | w and wT (W_LDS).  pl.params, wg and
// acc: k_hmm_trans_estep's.
template <bool A_LDS, bool W_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_trans_estep_looped(SegPlanDev pl, const u16* __restrict__ sym,
                                                                               const i64* __restrict__ offs, i64 a0,
                                                                               const double* __restrict__ wg, double* ahs, double* cs,
                                                                               bool c_lds, i64* acc, double* __restrict__ mant,
                                                                               i64* __restrict__ exp2, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K, slots = pl.slots;
    const int cells = 2 * K * K;
    FbTables tb;
    tb.parts = (double*)smem;                      // [2][slots]
    tb.Xb = tb.parts + 2 * (size_t)slots;          // [2][K]
    tb.sv = tb.Xb + 2 * (size_t)K;                 // [sumN]
    double* sS = tb.sv + sumN;                     // [sumN]
    i64* Cs = (i64*)(sS + sumN);                   // [K][K][2]
    double* As = (double*)(Cs + (c_lds ? cells : 0));
    double* ws = As + (A_LDS ? pl.a_words : 0);
    tb.pig = pl.params;
    const double* Ag = tb.pig + sumN;
    tb.Bg = Ag + pl.a_words;
    if (c_lds)
        for (int x = threadIdx.x; x < cells; x += blockDim.x) Cs[x] = 0;
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
    if (W_LDS)
        for (int x = threadIdx.x; x < cells; x += blockDim.x) ws[x] = wg[x];
    __syncthreads();
    tb.A = A_LDS ? As : Ag;
    tb.wm = W_LDS ? (const double*)ws : wg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    double* arow = ahs + (size_t)(base - a0) * sumN;     // ah_t of the state c at arow[t * sumN + c]
    double* crow = cs + (size_t)(base - a0) * nw + wib;  // c_t of this wave at crow[t * nw]
    int st = 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward (4.8.13's): x_t and c_t of every frame; the first event in frame order decides the status ------------
    double cprev = 1.0;  // c_{t-1}
    for (i64 t0 = 0; t0 < T && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane (every wave holds the same ones)
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        for (int q = 0; q < n; ++q) {
            const int o = __builtin_amdgcn_readlane(mysym, q);
            if (o >= M) {  // symbol outside the alphabet (workgroup-uniform: no wave reaches a further barrier)
                st = 2;
                break;
            }
            const i64 t = t0 + q;
            const double ct = fb_forward_frame(pl, tb, t, o, cprev, arow + (size_t)(t > 0 ? t - 1 : 0) * sumN, calls++, wib, lane, nw);
            if (!(ct > 0.0)) {  // (the same bits in every lane: workgroup-uniform)
                st = 1;
                break;
            }
            if (lane == 0) crow[(size_t)t * nw] = ct;
            scale_step(ct, p, E);
            cprev = ct;
        }
    }
    if (threadIdx.x == 0) {
        mant[s] = st == 0 ? p : 0.0;
        exp2[s] = st == 0 ? E : 0;
        status[s] = st;
        atomicAdd((u64*)&acc[cells + (st == 0 ? 0 : 1)], (u64)1);
    }
    if (st != 0) return;  // (workgroup-uniform) the stream adds nothing to C: no limb has been formed yet
    // (the last forward walk lies before that frame's second barrier: Xb is free for the backward pass.  ah_{T-1} is never
    // formed: the step into frame t reads ah_{t-1} only)

    // ---- backward (4.8.13's): frames T - 1 .. 1; the counts of the step into frame t + 1 at the head of the turn of t ------
    int steps = 0;
    for (i64 t0 = T > 1 ? ((T - 1) / 64) * 64 : -1; t0 >= 0; t0 -= 64) {
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        double cv = lane == 0 ? crow[(size_t)(t0 + n - 1) * nw] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const i64 t = t0 + q;
            if (t == 0) break;
            const double cq = cv;
            if (q > 0) cv = lane == 0 ? crow[(size_t)(t - 1) * nw] : 0.0;  // the previous frame's c, a frame ahead
            const int o = __builtin_amdgcn_readlane(mysym, q);
            const double ct = bcast(cq, 0);
            // R of this frame goes to Xb[steps & 1]; R_{t+1} lies in the other half, which is written again a frame on, past
            // the barrier that every wave reaches only after its walks and its products of this frame
            double* Rt = tb.Xb + (size_t)(steps & 1) * K;
            const double* Rn = tb.Xb + (size_t)((steps & 1) ^ 1) * K;
            ++steps;
            for (int sl = wib; sl < slots; sl += nw) {
                const FbLane L = fb_lane(pl, sl, lane);
                const double bq = L.act ? tb.Bg[(size_t)L.c * M + o] : 0.0;  // requested before the turn's walk and chains run
                const double a = L.act ? arow[(size_t)(t - 1) * sumN + L.c] : 0.0;  // ah_{t-1}: the lane's own store
                const double bh = fb_bh(L, t == T - 1, tb, Rn, K);
                if (t < T - 1) estep_products(L, tb, sS, Rn, K, c_lds, Cs, acc);  // the step into frame t + 1
                // S_t of this lane's class: the class sum of ah_{t-1} in state order
                const double S = chain_sum(a, L.L.N, L.L.seg, L.maxN, L.single);
                if (L.act) sS[L.c] = S;
                fb_post_R(L, tb, bq, bh, ct, Rt);
            }
            __syncthreads();
        }
    }
    if (T > 1) {  // the step into frame 1: R_1 lies in the half the last frame wrote
        const double* R1 = tb.Xb + (size_t)((steps - 1) & 1) * K;
        for (int sl = wib; sl < slots; sl += nw) estep_products(fb_lane(pl, sl, lane), tb, sS, R1, K, c_lds, Cs, acc);
    }
    if (c_lds) {  // the stream's table into the global one: a zero word adds nothing
        __syncthreads();
        for (int x = threadIdx.x; x < cells; x += blockDim.x) {
            const i64 v = Cs[x];
            if (v) atomicAdd((u64*)&acc[x], (u64)v);
        }
    }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------
size_t trans_estep_looped_lds_bytes(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds)
{
    return ((size_t)2 * pl.slots + (size_t)2 * pl.K + (size_t)2 * pl.sumN + (c_lds ? (size_t)2 * pl.K * pl.K : 0) +
            (a_lds ? (size_t)pl.a_words : 0) + (w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);
}

void trans_estep_looped_layout(const SegPlanDev& pl, bool c_forced, bool* c_lds, bool* a_lds, bool* w_lds)
{
    if (!c_forced) *c_lds = trans_estep_looped_lds_bytes(pl, true, false, false) <= SEG_LDS_BYTES;
    *a_lds = trans_estep_looped_lds_bytes(pl, *c_lds, true, false) <= SEG_LDS_BYTES;
    *w_lds = trans_estep_looped_lds_bytes(pl, *c_lds, *a_lds, true) <= SEG_LDS_BYTES;
}

int launch_trans_estep_looped(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds, const unsigned short* sym, const i64* offs,
                              int S, i64 a0, const double* w, double* ahs, double* cs, i64* acc, double* mant, i64* exp2, int* status,
                              hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1) return 1;
    const size_t lds = trans_estep_looped_lds_bytes(pl, c_lds, a_lds, w_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_TEST_LOOPED_LAUNCH(A_LDS, W_LDS)                                                                                      \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_trans_estep_looped<A_LDS, W_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_trans_estep_looped<A_LDS, W_LDS>), grid, block, lds, st, pl, sym, offs, a0, w, ahs, cs, c_lds,  \
                           acc, mant, exp2, status);                                                                             \
    } while (0)
    if (a_lds) {
        if (w_lds) E2_TEST_LOOPED_LAUNCH(true, true);
        else E2_TEST_LOOPED_LAUNCH(true, false);
    } else {
        if (w_lds) E2_TEST_LOOPED_LAUNCH(false, true);
        else E2_TEST_LOOPED_LAUNCH(false, false);
    }
#undef E2_TEST_LOOPED_LAUNCH
    return 0;
}

}  // namespace e2hmm
