// hmm_posterior_trans_looped.hip -- the looped body of `hmm segment --class-transitions --grammar-posteriors` (gfx950;
// DESIGN.md 4.8.13, "The looped body"): the scaled forward-backward of hmm_posterior_trans.hip for classes that take any
// number of wave-slots.  The contract is the resident body's, operation for operation: the same chains in state order, the
// same walks over the K classes from class 0, the same global sum, the same post, log_prob and status bits.
//   k_hmm_loop_posteriors_trans_looped   one workgroup per stream, min(slots, 16) waves; wave w serves the slots w, w + nw,
//                                        w + 2 nw, .. in turn, and lane l of slot sl is the state pl.lanes[sl * 64 + l] for
//                                        the whole stream.
// The frames are hmm_trans_fb_looped_step.h's (two passes around a barrier forward, one pass backward, the carried array sv).
// What this kernel adds between the backward frame's two parts: the class sum of ah_t * bh_t, written by the class's state-0
// lane.  ah_t comes from the forward table, loaded by the lane that stored it; ah_{T-1} alone is still x_{T-1} in sv when the
// backward pass begins and is formed there.
//   scratch   ah_t to ahs[(frame - a0) * sumN + composite index] by its state's lane; c_t to cs[(frame - a0) * nw + wave] by
//             each wave's lane 0 (nw copies a frame, not one per slot): the backward pass loads only what the same lane stored.
//   status    workgroup-uniform as in the resident body: the symbol check of a frame comes before its arithmetic and before
//             its barriers, c_t has the same bits in every lane, !(c_t > 0) gives 1; then the whole workgroup zero-fills the
//             stream's post rows and skips the backward pass.
//   LDS       mandatory: the partials of both parities (2 slots), S / R of two steps (2 K), sv (sumN).  A, and then w with wT,
//             go behind them where they fit: four instantiations.  pi stays in the parameter block.
// Nothing transcendental runs here; the unit is compiled with -ffp-contract=off.
#include "hmm_trans_fb_looped_step.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x min(slots, 16).  Dynamic LDS: 2 x slots partials | 2 x K class masses | sv,
// sumN doubles | A of every class (A_LDS) | w and wT (W_LDS).  pl.params and wg: k_hmm_loop_posteriors_trans's.
template <bool A_LDS, bool W_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_loop_posteriors_trans_looped(SegPlanDev pl, const u16* __restrict__ sym,
                                                                                         const i64* __restrict__ offs, i64 a0,
                                                                                         const double* __restrict__ wg, double* ahs,
                                                                                         double* cs, double* __restrict__ post,
                                                                                         double* __restrict__ mant,
                                                                                         i64* __restrict__ exp2, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K, slots = pl.slots;
    FbTables tb;
    tb.parts = (double*)smem;                      // [2][slots]
    tb.Xb = tb.parts + 2 * (size_t)slots;          // [2][K]
    tb.sv = tb.Xb + 2 * (size_t)K;                 // [sumN]
    double* As = tb.sv + sumN;
    double* ws = As + (A_LDS ? pl.a_words : 0);
    tb.pig = pl.params;
    const double* Ag = tb.pig + sumN;
    tb.Bg = Ag + pl.a_words;
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
    if (W_LDS)
        for (int x = threadIdx.x; x < 2 * K * K; x += blockDim.x) ws[x] = wg[x];
    if (A_LDS || W_LDS) __syncthreads();
    tb.A = A_LDS ? As : Ag;
    tb.wm = W_LDS ? (const double*)ws : wg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    double* arow = ahs + (size_t)(base - a0) * sumN;     // ah_t of the state c at arow[t * sumN + c]
    double* crow = cs + (size_t)(base - a0) * nw + wib;  // c_t of this wave at crow[t * nw]
    double* prow = post + (size_t)base * K;
    int st = 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward: x_t and c_t of every frame; the first event in frame order decides the status ----------------------
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
    }
    if (st != 0) {  // (workgroup-uniform) every row of the stream is 0.0
        for (i64 x = threadIdx.x; x < T * K; x += blockDim.x) prow[x] = 0.0;
        return;
    }
    // (the last forward walk lies before that frame's second barrier: Xb is free for the backward pass)

    // ---- backward: bh_t from acc and R_{t+1}, the posterior of frame t, then u_t and R_t ------------------------------------
    int steps = 0;
    for (i64 t0 = T > 0 ? ((T - 1) / 64) * 64 : -1; t0 >= 0; t0 -= 64) {
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        double cv = lane == 0 ? crow[(size_t)(t0 + n - 1) * nw] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double cq = cv;
            if (q > 0) cv = lane == 0 ? crow[(size_t)(t0 + q - 1) * nw] : 0.0;  // the previous frame's c, a frame ahead
            const int o = __builtin_amdgcn_readlane(mysym, q);
            const i64 t = t0 + q;
            const double ct = bcast(cq, 0);
            // R of this frame goes to Xb[steps & 1]; R_{t+1} lies in the other half, which is written again a frame on, past
            // the barrier that every wave reaches only after its walks of this frame
            double* Rt = tb.Xb + (size_t)(steps & 1) * K;
            const double* Rn = tb.Xb + (size_t)((steps & 1) ^ 1) * K;
            ++steps;
            for (int sl = wib; sl < slots; sl += nw) {
                const FbLane L = fb_lane(pl, sl, lane);
                const double bq = L.act ? tb.Bg[(size_t)L.c * M + o] : 0.0;  // requested before the turn's walk and chains run
                double a;
                if (t == T - 1) a = L.act ? tb.sv[L.c] / cprev : 0.0;  // ah_{T-1} is still x_{T-1} in sv
                else a = L.act ? arow[(size_t)t * sumN + L.c] : 0.0;
                const double bh = fb_bh(L, t == T - 1, tb, Rn, K);
                const double sum = chain_sum(a * bh, L.L.N, L.L.seg, L.maxN, L.single);
                if (L.head) prow[(size_t)t * K + L.k] = sum;
                if (t == 0) continue;  // (workgroup-uniform)
                fb_post_R(L, tb, bq, bh, ct, Rt);
            }
            if (t == 0) break;
            __syncthreads();
        }
    }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------
// mandatory: the partial sums of both parities, the class masses of two steps and sv; A, then w with wT, behind them
size_t posteriors_trans_looped_lds_bytes(const SegPlanDev& pl, bool a_lds, bool w_lds)
{
    return ((size_t)2 * pl.slots + (size_t)2 * pl.K + (size_t)pl.sumN + (a_lds ? (size_t)pl.a_words : 0) +
            (w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);
}

void posteriors_trans_looped_layout(const SegPlanDev& pl, bool* a_lds, bool* w_lds)
{
    *a_lds = posteriors_trans_looped_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;
    *w_lds = posteriors_trans_looped_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;
}

int launch_loop_posteriors_trans_looped(const SegPlanDev& pl, const unsigned short* sym, const i64* offs, int S, i64 a0, const double* w,
                                        double* ahs, double* cs, double* post, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || posteriors_trans_looped_lds_bytes(pl, false, false) > SEG_LDS_BYTES) return 1;
    bool a_lds, w_lds;
    posteriors_trans_looped_layout(pl, &a_lds, &w_lds);
    const size_t lds = posteriors_trans_looped_lds_bytes(pl, a_lds, w_lds);
    const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_POSTT_LOOPED_LAUNCH(A_LDS, W_LDS)                                                                                     \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_loop_posteriors_trans_looped<A_LDS, W_LDS>,                                   \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEG_LDS_BYTES) != hipSuccess)                   \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_loop_posteriors_trans_looped<A_LDS, W_LDS>), grid, block, lds, st, pl, sym, offs, a0, w, ahs,  \
                           cs, post, mant, exp2, status);                                                                        \
    } while (0)
    if (a_lds) {
        if (w_lds) E2_POSTT_LOOPED_LAUNCH(true, true);
        else E2_POSTT_LOOPED_LAUNCH(true, false);
    } else {
        if (w_lds) E2_POSTT_LOOPED_LAUNCH(false, true);
        else E2_POSTT_LOOPED_LAUNCH(false, false);
    }
#undef E2_POSTT_LOOPED_LAUNCH
    return 0;
}

}  // namespace e2hmm
