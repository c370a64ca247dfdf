// hmm_posterior_trans.hip -- HIP kernel (gfx950) of `hmm segment --class-transitions --grammar-posteriors` (DESIGN.md
// 4.8.13): the smoothed class posterior P(class at frame t | whole stream) under the class loop when leaving class f for
// class k costs w[f][k] = exp(lt[f][k]) -- the sum-product counterpart of hmm_segment_trans.hip's max-sum, and
// hmm_posterior.hip's scaled forward-backward with the one price sw replaced by a K x K matrix -- bit-exact against the
// restatement.
//   k_hmm_loop_posteriors_trans  one workgroup per stream, a wave per slot of k_hmm_segment's packing (resident only: at most
//                                16 slots).  Lane (k, j) is state j of class k.  The in-class chains are hmm_lane.h's.
//                                Forward: the chain reads ah_{t-1} of every state of its class anyway, so the class mass
//                                S[k] rides on it, one add a state; the class's state-0 lane posts S[k] to a double-buffered
//                                LDS array of 2 x K doubles, one barrier, then every lane of class k walks the K sources along
//                                wT[k][.] (m[k]); the global sum c_t costs the step's second barrier.  Backward: the chain
//                                reads u of every state of its class, and with pi in LDS R[f] = sum_j pi_f[j] u[f][j] rides on
//                                it; post, one barrier, every lane of class f walks w[f][.] (r[f]); bh = acc + r.
// Nothing transcendental runs here: w comes from the host, and so does its transpose wT, so that both walks read consecutive
// words.  Every operation is one IEEE double operation in the contract's order (the unit is compiled with
// -ffp-contract=off).  All terms are >= 0 and idle lanes carry +0.0.
// Scratch, as in hmm_posterior.hip: ah_t to ahs[(frame - a0) * sumN + composite index] by its state's lane, c_t to
// cs[(frame - a0) * waves + wave] by each wave's lane 0; the backward pass loads only what the same lane stored.
#include "hmm_lane.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x slots.  Dynamic LDS: 2 x SEG_MAX_WAVES partials | the class masses of two
// consecutive steps, 2 x K doubles (S forward, R backward) | pi (sumN) | A of every class (A_LDS) | w and wT (W_LDS).
// pl.params: pi (sumN) | A (a_words; class k from lanes[].a_at, leading dimension ld = N_k | 1, as in hmm_posterior.hip) |
// B (sumN rows of M).  wg: w (K x K, w[f * K + k]) followed by wT (wT[k * K + f] = w[f * K + k]).
template <bool A_LDS, bool W_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_loop_posteriors_trans(SegPlanDev pl, const u16* __restrict__ sym,
                                                                                  const i64* __restrict__ offs, i64 a0,
                                                                                  const double* __restrict__ wg, double* ahs,
                                                                                  double* cs, double* __restrict__ post,
                                                                                  double* __restrict__ mant, i64* __restrict__ exp2,
                                                                                  int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K;
    double* parts = (double*)smem;            // [2][SEG_MAX_WAVES]
    double* Xb = parts + 2 * SEG_MAX_WAVES;   // [2][K]
    double* pis = Xb + 2 * K;                 // [sumN]
    double* As = pis + sumN;
    double* ws = As + (A_LDS ? pl.a_words : 0);
    const double* pig = pl.params;
    const double* Ag = pig + sumN;
    const double* Bg = Ag + pl.a_words;
    for (int x = threadIdx.x; x < sumN; x += blockDim.x) pis[x] = pig[x];
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
    if (W_LDS)
        for (int x = threadIdx.x; x < 2 * K * K; x += blockDim.x) ws[x] = wg[x];
    __syncthreads();
    const double* A = A_LDS ? As : Ag;
    const double* wm = W_LDS ? (const double*)ws : wg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    // a lane without a state: N = 0, j = 0, a_at = 0, ld = 0, class 0 in the walks (its reads stay in bounds), its values
    // are kept at +0.0
    const SegLaneDev L = pl.lanes[wib * 64 + lane];
    const bool act = L.cls >= 0;
    const bool head = act && L.j == 0;  // the lane that posts for its class
    const int c = act ? L.comp : 0, N = L.N, seg = L.seg, ld = act ? (N | 1) : 0, k = act ? L.cls : 0;
    const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib]);
    const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib + 1]) != 0;
    const double pij = act ? pig[c] : 0.0;
    const double* Brow = Bg + (size_t)c * M;
    const double* Acol = A + L.a_at + L.j;                // A[i][j] at Acol[i * ld]
    const double* Arow = A + L.a_at + (size_t)L.j * ld;   // A[j][i] at Arow[i]
    const double* pik = pis + (c - L.j);                  // pi of this lane's class: pik[j]
    const double* wrow = wm + (size_t)k * K;              // w[k][k'] at wrow[k']: the backward walk of class f = k
    const double* wTrow = wm + (size_t)K * K + (size_t)k * K;  // w[f][k] at wTrow[f]: the forward walk
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
                // the in-class chain, and on the way the class's mass S = CS(ah_{t-1})
                const ChainPair cf = chain_col_mass(ah, Acol, ld, N, seg, maxN, single);
                const double acc = cf.acc, S = cf.sum;
                // S of step t lives in Xb[t & 1]: a wave writes that half again at t + 2, past the barriers of t + 1
                double* St = Xb + (size_t)(t & 1) * K;
                if (head) St[k] = S;
                __syncthreads();
                // the mass that enters class k: sources in class order
                double m = St[0] * wTrow[0];
                for (int f = 1; f < K; ++f) m = m + St[f] * wTrow[f];
                x = (acc + m * pij) * bq;
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
    // (the last forward walk lies before that step's block_sum barrier: Xb is free for the backward pass)

    // ---- backward: bh_t from bh_{t+1}, and the posterior of every frame -----------------------------------------------
    double bh = act ? 1.0 : 0.0;
    int steps = 0;
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
            if (head) prow[(size_t)t * K + k] = sum;
            if (t == 0) break;
            const double ct = bcast(cq, 0);
            const double u = act ? (bq * bh) / ct : 0.0;
            // the in-class chain, and on the way what leaves through the class's pi: R = sum_j pi[j] u[j]
            const ChainPair cr = chain_row_pi(u, Arow, pik, N, seg, maxN, single);
            const double acc = cr.acc, R = cr.sum;
            // R of this step lives in Xb[steps & 1]: a wave writes that half again two steps on, past the barrier of the
            // step between, which every wave reaches only after its walk of this step
            double* Rt = Xb + (size_t)(steps++ & 1) * K;
            if (head) Rt[k] = R;
            __syncthreads();
            double r = wrow[0] * Rt[0];
            for (int kk = 1; kk < K; ++kk) r = r + wrow[kk] * Rt[kk];
            bh = act ? acc + r : 0.0;
        }
    }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------
namespace {
size_t post_trans_lds_bytes(const SegPlanDev& pl, bool a_lds, bool w_lds)
{
    return ((size_t)2 * SEG_MAX_WAVES + (size_t)2 * pl.K + (size_t)pl.sumN + (a_lds ? (size_t)pl.a_words : 0) +
            (w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);
}
}  // namespace

void posteriors_trans_layout(const SegPlanDev& pl, bool* a_lds, bool* w_lds)
{
    *a_lds = post_trans_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;
    *w_lds = post_trans_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;
}

int launch_loop_posteriors_trans(const SegPlanDev& pl, const unsigned short* sym, const i64* offs, int S, i64 a0, const double* w,
                                 double* ahs, double* cs, double* post, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || pl.slots > SEG_MAX_WAVES) return 1;
    bool a_lds, w_lds;
    posteriors_trans_layout(pl, &a_lds, &w_lds);
    const size_t lds = post_trans_lds_bytes(pl, a_lds, w_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * pl.slots));
#define E2_POSTT_LAUNCH(A_LDS, W_LDS)                                                                                            \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_loop_posteriors_trans<A_LDS, W_LDS>,                                          \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEG_LDS_BYTES) != hipSuccess)                   \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_loop_posteriors_trans<A_LDS, W_LDS>), grid, block, lds, st, pl, sym, offs, a0, w, ahs, cs,    \
                           post, mant, exp2, status);                                                                            \
    } while (0)
    if (a_lds) {
        if (w_lds) E2_POSTT_LAUNCH(true, true);
        else E2_POSTT_LAUNCH(true, false);
    } else {
        if (w_lds) E2_POSTT_LAUNCH(false, true);
        else E2_POSTT_LAUNCH(false, false);
    }
#undef E2_POSTT_LAUNCH
    return 0;
}

}  // namespace e2hmm
