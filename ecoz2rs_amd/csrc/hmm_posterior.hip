// hmm_posterior.hip -- HIP kernel (gfx950) of `hmm segment --posteriors`: the smoothed class posterior
// P(class at frame t | whole stream) under the class loop of hmm_segment.hip -- the K class models side by side; at every
// frame the whole mass may leave its class and enter any class through that class's pi at the price sw = exp(ln_switch) --
// by a scaled forward-backward in the linear domain, bit-exact against the restatement.
//   k_hmm_loop_posteriors   one workgroup per stream, a wave per slot of k_hmm_segment's packing (resident only: at most 16
//                           slots).  Lane (k, j) is state j of class k.  The in-class sums are hmm_lane.h's chains in state
//                           order (the values of the other states through ds_bpermute_b32, or v_readlane where the slot holds
//                           one class); the forward pass reads a column of A, the backward pass a row.  The coupling between
//                           the classes is one sum per step over all states: a butterfly over the wave's 64 lanes, lane 0
//                           posting to a double-buffered LDS slot, one barrier, every wave adding the partials in slot order.
// Nothing transcendental runs here: sw and e = sw * pi come from the host.  Every operation is one IEEE double operation in
// the contract's order (the unit is compiled with -ffp-contract=off).  All terms are >= 0 and idle lanes carry +0.0.
// Scratch: ah_t to ahs[(frame - a0) * sumN + composite index] by its state's lane, c_t to cs[(frame - a0) * waves + wave] by
// each wave's lane 0; the backward pass loads only what the same lane stored, so no visibility between waves is needed.
#include "hmm_lane.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x slots.  Dynamic LDS: 2 x SEG_MAX_WAVES partials | A of every class (A_LDS).
// pl.params: pi (sumN) | e = sw * pi (sumN) | A (a_words; class k from lanes[].a_at, leading dimension ld = N_k | 1: odd,
// so that the rows the backward pass reads and the columns the forward pass reads both spread over the LDS banks) | B
// (sumN rows of M).
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_loop_posteriors(SegPlanDev pl, const u16* __restrict__ sym,
                                                                            const i64* __restrict__ offs, i64 a0, double sw,
                                                                            double* ahs, double* cs, double* __restrict__ post,
                                                                            double* __restrict__ mant, i64* __restrict__ exp2,
                                                                            int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* parts = (double*)smem;  // [2][SEG_MAX_WAVES]
    double* As = parts + 2 * SEG_MAX_WAVES;
    const int M = pl.M, sumN = pl.sumN, K = pl.K;
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
    // a lane without a state: N = 0, j = 0, a_at = 0, ld = 0 (its reads stay in bounds), its values are kept at +0.0
    const SegLaneDev L = pl.lanes[wib * 64 + lane];
    const bool act = L.cls >= 0;
    const int c = act ? L.comp : 0, N = L.N, seg = L.seg, ld = act ? (N | 1) : 0;
    const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib]);
    const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib + 1]) != 0;
    const double pij = act ? pig[c] : 0.0;
    const double ej = act ? eg[c] : 0.0;
    const double* Brow = Bg + (size_t)c * M;
    const double* Acol = A + L.a_at + L.j;                // A[i][j] at Acol[i * ld]
    const double* Arow = A + L.a_at + (size_t)L.j * ld;   // A[j][i] at Arow[i]
    double* arow = ahs + (size_t)(base - a0) * sumN + c;  // ah_t of this state at arow[t * sumN]
    double* crow = cs + (size_t)(base - a0) * nw + wib;   // c_t of this wave at crow[t * nw]
    double* prow = post + (size_t)base * K;
    int st = 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward: ah_t and c_t of every frame; the first event in frame order decides the status --------------------
    double ah = 0.0;
    for (i64 t0 = 0; t0 < T && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane (every wave holds the same ones)
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        int o = __builtin_amdgcn_readlane(mysym, 0);
        double b = (act && o < M) ? Brow[o] : 0.0;
        for (int q = 0; q < n; ++q) {
            const double bq = b;
            const int oq = o;
            if (q + 1 < n) {  // next step's emission is requested before this step's chain runs
                o = __builtin_amdgcn_readlane(mysym, q + 1);
                b = (act && o < M) ? Brow[o] : 0.0;
            }
            if (oq >= M) {  // symbol outside the alphabet (workgroup-uniform: no wave reaches a further barrier)
                st = 2;
                break;
            }
            const i64 t = t0 + q;
            double x;
            if (t == 0) {
                x = pij * bq;
            } else {
                const double acc = chain_col(ah, Acol, ld, N, seg, maxN, single);
                x = (acc + ej) * bq;
            }
            if (!act) x = 0.0;
            const double ct = block_sum(x, parts + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
            if (!(ct > 0.0)) {  // (the same bits in every lane: workgroup-uniform)
                st = 1;
                break;
            }
            ah = x / ct;
            if (act) arow[(size_t)t * sumN] = ah;
            if (lane == 0) crow[(size_t)t * nw] = ct;
            scale_step(ct, p, E);
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

    // ---- backward: bh_t from bh_{t+1}, and the posterior of every frame -----------------------------------------------
    double bh = act ? 1.0 : 0.0;
    for (i64 t0 = T > 0 ? ((T - 1) / 64) * 64 : -1; t0 >= 0; t0 -= 64) {
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        // what frame t = t0 + q needs: B[j][o_t], c_t (bh_{t-1} from bh_t) and ah_t (the posterior of t)
        int o = __builtin_amdgcn_readlane(mysym, n - 1);
        double b = act ? Brow[o] : 0.0;
        double a = act ? arow[(size_t)(t0 + n - 1) * sumN] : 0.0;
        double cv = lane == 0 ? crow[(size_t)(t0 + n - 1) * nw] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double bq = b, aq = a, cq = cv;
            if (q > 0) {  // the previous frame's loads are requested before this frame's chains run
                o = __builtin_amdgcn_readlane(mysym, q - 1);
                b = act ? Brow[o] : 0.0;
                a = act ? arow[(size_t)(t0 + q - 1) * sumN] : 0.0;
                cv = lane == 0 ? crow[(size_t)(t0 + q - 1) * nw] : 0.0;
            }
            const i64 t = t0 + q;
            const double g = aq * bh;
            const double sum = chain_sum(g, N, seg, maxN, single);
            if (act && L.j == 0) prow[(size_t)t * K + L.cls] = sum;
            if (t == 0) break;
            const double ct = bcast(cq, 0);
            const double u = act ? (bq * bh) / ct : 0.0;
            const double R = block_sum(pij * u, parts + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
            const double r = sw * R;
            const double acc = chain_row(u, Arow, N, seg, maxN, single);
            bh = act ? acc + r : 0.0;
        }
    }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------
size_t posteriors_lds_bytes(const SegPlanDev& pl, bool a_lds)
{
    return (size_t)2 * SEG_MAX_WAVES * sizeof(double) + (a_lds ? (size_t)pl.a_words * 8 : 0);
}

bool posteriors_a_in_lds(const SegPlanDev& pl) { return posteriors_lds_bytes(pl, true) <= SEG_LDS_BYTES; }

int launch_loop_posteriors(const SegPlanDev& pl, const unsigned short* sym, const i64* offs, int S, i64 a0, double sw, double* ahs,
                           double* cs, double* post, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || pl.slots > SEG_MAX_WAVES) return 1;
    const bool a_lds = posteriors_a_in_lds(pl);
    const size_t lds = posteriors_lds_bytes(pl, a_lds);
    const dim3 grid((unsigned)S), block((unsigned)(64 * pl.slots));
#define E2_POST_LAUNCH(A_LDS)                                                                                                    \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_loop_posteriors<A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,          \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_loop_posteriors<A_LDS>), grid, block, lds, st, pl, sym, offs, a0, sw, ahs, cs, post, mant, exp2, \
                           status);                                                                                              \
    } while (0)
    if (a_lds) E2_POST_LAUNCH(true);
    else E2_POST_LAUNCH(false);
#undef E2_POST_LAUNCH
    return 0;
}

}  // namespace e2hmm
