// hmm_posterior_looped.hip -- the looped body of `hmm segment --posteriors` (gfx950): the scaled
// forward-backward of hmm_posterior.hip for classes that take any number of wave-slots.  The contract is the resident body's,
// operation for operation: the same chains in state order, the same global sum GS, the same post, log_prob and status bits.
//   k_hmm_loop_posteriors_looped   one workgroup per stream, min(slots, 16) waves; wave w serves the slots w, w + nw,
//                                  w + 2 nw, .. in turn, and lane l of slot sl is the state pl.lanes[sl * 64 + l] for the
//                                  whole stream.
// How the points that decide the bits are met:
//   GS            every served slot posts its own butterfly sum to parts[parity][slot] (a wave that owns the slots 0, 16 and 32
//                 posts three partials, never their sum); behind the one barrier of the step every wave adds all `slots`
//                 partials in slot order from slot 0.  The parity alternates per call as in block_sum: a slot's entry is
//                 written again two calls later, past a barrier that every wave reaches only after its reads.
//   carried state one LDS array sv of sumN doubles, indexed by the composite state and touched by the state's own lane only, so
//                 it needs no fence and no barrier of its own: it is a register file that is as long as the wave's turns.  The
//                 lane takes its value into a register and the in-class chains run through ds_bpermute_b32 / v_readlane_b32
//                 exactly as in the resident body.  (The alternative, k_hmm_segment's double-buffered per-state array that the
//                 chains read in place, takes two arrays and an ordering fence between a wave's writes and its other lanes'
//                 reads, and would give the chains another instruction sequence than the one the resident body is tested with.)
//                 Forward, sv holds x_t from the step's chains until c_t is known; ah_t = x_t / c_t is formed by the same
//                 lane at the head of its next turn (step t + 1, or the backward pass's first step), where it is stored to ahs
//                 and feeds the chain.  Backward, sv holds u_t across the barrier of R_t; bh_{t-1} = (A u_t) + sw R_t is
//                 formed at the head of the slot's turn of step t - 1 and lives in a register from there to u_{t-1}.
//   scratch       ah_t to ahs[(frame - a0) * sumN + composite index] by its state's lane; c_t to cs[(frame - a0) * nw + wave]
//                 by each wave's lane 0 (nw copies a frame): the backward pass loads only what the same lane stored.
//   emissions     B[j][o_t] is requested at the head of a slot's turn, ahead of the turn's chains, which hide it; a frame
//                 ahead would take a register pair per served slot.  No bit depends on it.
//   status        workgroup-uniform as in the resident body: the symbol check of a frame comes before its arithmetic and before
//                 its barrier, c_t has the same bits in every lane, !(c_t > 0) gives 1; then the whole workgroup zero-fills the
//                 stream's post rows and skips the backward pass.
//   A             in LDS behind the mandatory arrays when it fits (A_LDS), else read in place: two instantiations.
// One barrier per frame and pass.  Nothing transcendental runs here; the unit is compiled with -ffp-contract=off.
#include "hmm_lane.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x min(slots, 16).  Dynamic LDS: 2 x slots partials | sv, sumN doubles | A of
// every class (A_LDS).  pl.params as k_hmm_loop_posteriors takes them: pi (sumN) | e = sw * pi (sumN) | A (a_words; class k from
// lanes[].a_at, leading dimension N_k | 1) | B (sumN rows of M).
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_loop_posteriors_looped(SegPlanDev pl, const u16* __restrict__ sym,
                                                                                   const i64* __restrict__ offs, i64 a0, double sw,
                                                                                   double* ahs, double* cs, double* __restrict__ post,
                                                                                   double* __restrict__ mant, i64* __restrict__ exp2,
                                                                                   int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K, slots = pl.slots;
    double* parts = (double*)smem;         // [2][slots]
    double* sv = parts + 2 * (size_t)slots;  // [sumN]
    double* As = sv + sumN;
    const double* pig = pl.params;
    const double* eg = pig + sumN;
    const double* Ag = eg + sumN;
    const double* Bg = Ag + pl.a_words;
    if (A_LDS) {
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
        __syncthreads();
    }
    const double* A = A_LDS ? As : Ag;
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
            double* pt = parts + (size_t)(calls++ & 1) * slots;
            for (int sl = wib; sl < slots; sl += nw) {
                // a lane without a state: N = 0, j = 0, a_at = 0, ld = 0 (its reads stay in bounds), its values are kept at +0.0
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                const bool act = L.cls >= 0;
                const int c = act ? L.comp : 0, N = L.N, ld = act ? (N | 1) : 0;
                const double bq = act ? Bg[(size_t)c * M + o] : 0.0;  // requested before the turn's chain runs
                double x;
                if (t == 0) {
                    x = act ? pig[c] * bq : 0.0;
                } else {
                    const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl]);
                    const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl + 1]) != 0;
                    const double ej = act ? eg[c] : 0.0;
                    const double ah = act ? sv[c] / cprev : 0.0;  // ah_{t-1} of this state
                    if (act) arow[(size_t)(t - 1) * sumN + c] = ah;
                    const double acc = chain_col(ah, A + L.a_at + L.j, ld, N, L.seg, maxN, single);
                    x = act ? (acc + ej) * bq : 0.0;
                }
                if (act) sv[c] = x;
                const double v = slot_sum(x);
                if (lane == 0) pt[sl] = v;
            }
            __syncthreads();
            const double ct = slots_sum(pt, slots);
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

    // ---- backward: bh_t from u_{t+1} and R_{t+1}, the posterior of frame t, then u_t ---------------------------------------
    double R = 0.0;
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
            const double r = sw * R;
            double* pt = parts + (size_t)(calls++ & 1) * slots;
            for (int sl = wib; sl < slots; sl += nw) {
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                const bool act = L.cls >= 0;
                const int c = act ? L.comp : 0, N = L.N, ld = act ? (N | 1) : 0;
                const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl]);
                const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl + 1]) != 0;
                const double bq = act ? Bg[(size_t)c * M + o] : 0.0;  // requested before the turn's chains run
                double a, bh;
                if (t == T - 1) {  // ah_{T-1} is still x_{T-1} in sv
                    a = act ? sv[c] / cprev : 0.0;
                    bh = act ? 1.0 : 0.0;
                } else {
                    a = act ? arow[(size_t)t * sumN + c] : 0.0;
                    const double u1 = act ? sv[c] : 0.0;  // u_{t+1} of this state
                    const double acc = chain_row(u1, A + L.a_at + (size_t)L.j * ld, N, L.seg, maxN, single);
                    bh = act ? acc + r : 0.0;
                }
                const double sum = chain_sum(a * bh, N, L.seg, maxN, single);
                if (act && L.j == 0) prow[(size_t)t * K + L.cls] = sum;
                if (t == 0) continue;  // (workgroup-uniform)
                const double u = act ? (bq * bh) / ct : 0.0;
                if (act) sv[c] = u;
                const double pij = act ? pig[c] : 0.0;
                const double v = slot_sum(pij * u);
                if (lane == 0) pt[sl] = v;
            }
            if (t == 0) break;
            __syncthreads();
            R = slots_sum(pt, slots);
        }
    }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------
// mandatory: the partial sums of both parities and sv; A behind them where it fits
size_t posteriors_looped_lds_bytes(const SegPlanDev& pl, bool a_lds)
{
    return (size_t)2 * pl.slots * sizeof(double) + (size_t)pl.sumN * sizeof(double) + (a_lds ? (size_t)pl.a_words * 8 : 0);
}

int launch_loop_posteriors_looped(const SegPlanDev& pl, const unsigned short* sym, const i64* offs, int S, i64 a0, double sw, double* ahs,
                                  double* cs, double* post, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || posteriors_looped_lds_bytes(pl, false) > SEG_LDS_BYTES) return 1;
    const bool a_lds = posteriors_looped_lds_bytes(pl, true) <= SEG_LDS_BYTES;
    const size_t lds = posteriors_looped_lds_bytes(pl, a_lds);
    const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_POST_LOOPED_LAUNCH(A_LDS)                                                                                             \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_loop_posteriors_looped<A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_loop_posteriors_looped<A_LDS>), grid, block, lds, st, pl, sym, offs, a0, sw, ahs, cs, post, mant, \
                           exp2, status);                                                                                        \
    } while (0)
    if (a_lds) E2_POST_LOOPED_LAUNCH(true);
    else E2_POST_LOOPED_LAUNCH(false);
#undef E2_POST_LOOPED_LAUNCH
    return 0;
}

}  // namespace e2hmm
