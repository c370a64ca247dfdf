// hmm_trans_estep.hip -- HIP kernel (gfx950) of `hmm transitions --em`: the expected bigram counts of the
// classes under the class loop and the K x K prices w[f][k] = exp(lt[f][k]) -- the E-step of Baum-Welch for the grammar --
// bit-exact against the restatement.  Forward, scaling, status and backward are hmm_posterior_trans.hip's steps (4.8.13: the
// same chains of hmm_lane.h, the same barriers, the same scratch); what that kernel throws away is kept here:
//   xi_t[f][k] = S_t[f] * (w[f][k] * R_t[k])     t = 1 .. T - 1
// with S_t[f] = CS_f(ah_{t-1}), the mass the forward step of frame t posted, and R_t[k] the entry sum the backward step of
// frame t posts.  Each xi becomes two int32 limbs (hmm_limbs.h) added to the int64 pair of cell C[f][k]: all sums are
// integers, so neither the split over workgroups nor the order of the streams nor the route of an atomic changes a bit.
//   k_hmm_trans_estep   one workgroup per stream, a wave per slot of k_hmm_segment's packing (resident only: at most 16
//                       slots).  Lane (f, i) is state i of class f.  This pass forms no posterior, so the place of 4.8.13's
//                       chain over ah_t * bh_t is taken by one class sum over ah_{t-1}, loaded from the forward table by the
//                       lane that stored it: S_t[f] in the bits the forward pass used (chain_col_mass and chain_sum add the
//                       states in the same order), and nothing more is stored per frame than 4.8.13 stores.  After the
//                       barrier that publishes R_t every lane of class f holds S_t[f], and lane (f, i) takes the targets
//                       k = i, i + N_f, ...: ceil(K / N_f) limb conversions a lane a frame.  w[f][k] * R_t[k] is the very
//                       term the walk adds into r[f]; a forbidden succession (w = 0) gives zero limbs and issues no atomic.
// The C table: 2 K^2 int64 in LDS (ds_add_u64; flushed once a stream, a zero word adds nothing) or the global table directly
// (c_lds, the host's choice).  A stream of status != 0 adds nothing to C; word 2 K^2 counts the status-0 streams, word
// 2 K^2 + 1 the others.  Nothing transcendental runs here; the unit is compiled with -ffp-contract=off.
#include "hmm_limbs.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x slots.  Dynamic LDS: 2 x SEG_MAX_WAVES partials | the class masses of two
// consecutive steps, 2 x K doubles | pi (sumN) | the C table, 2 K^2 int64 (c_lds) | A of every class (A_LDS) | w and wT
// (W_LDS).  pl.params and wg: k_hmm_loop_posteriors_trans's.  acc: 2 K^2 + 2 words, added to.
template <bool A_LDS, bool W_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_trans_estep(SegPlanDev pl, const u16* __restrict__ sym,
                                                                        const i64* __restrict__ offs, i64 a0,
                                                                        const double* __restrict__ wg, double* ahs, double* cs,
                                                                        bool c_lds, i64* acc, double* __restrict__ mant,
                                                                        i64* __restrict__ exp2, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K;
    const int cells = 2 * K * K;
    double* parts = (double*)smem;            // [2][SEG_MAX_WAVES]
    double* Xb = parts + 2 * SEG_MAX_WAVES;   // [2][K]
    double* pis = Xb + 2 * K;                 // [sumN]
    i64* Cs = (i64*)(pis + sumN);             // [K][K][2]
    double* As = (double*)(Cs + (c_lds ? cells : 0));
    double* ws = As + (A_LDS ? pl.a_words : 0);
    const double* pig = pl.params;
    const double* Ag = pig + sumN;
    const double* Bg = Ag + pl.a_words;
    for (int x = threadIdx.x; x < sumN; x += blockDim.x) pis[x] = pig[x];
    if (c_lds)
        for (int x = threadIdx.x; x < cells; x += blockDim.x) Cs[x] = 0;
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
    if (W_LDS)
        for (int x = threadIdx.x; x < cells; x += blockDim.x) ws[x] = wg[x];
    __syncthreads();
    const double* A = A_LDS ? As : Ag;
    const double* wm = W_LDS ? (const double*)ws : wg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    // a lane without a state: N = 0, j = 0, a_at = 0, ld = 0, class 0 in the walk (its reads stay in bounds), its values
    // are kept at +0.0 and it takes no target
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
    int st = 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward (4.8.13's): ah_t and c_t of every frame; the first event in frame order decides the status ----------
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
                const double acc_f = cf.acc, S = cf.sum;
                // S of step t lives in Xb[t & 1]: a wave writes that half again at t + 2, past the barriers of t + 1
                double* St = Xb + (size_t)(t & 1) * K;
                if (head) St[k] = S;
                __syncthreads();
                // the mass that enters class k: sources in class order
                double m = St[0] * wTrow[0];
                for (int f = 1; f < K; ++f) m = m + St[f] * wTrow[f];
                x = (acc_f + m * pij) * bq;
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
        atomicAdd((u64*)&acc[cells + (st == 0 ? 0 : 1)], (u64)1);
    }
    if (st != 0) return;  // (workgroup-uniform) the stream adds nothing to C: no limb has been formed yet
    // (the last forward walk lies before that step's block_sum barrier: Xb is free for the backward pass)

    // ---- backward (4.8.13's): bh_{t-1} from bh_t, and the counts of the step into frame t -----------------------------
    double bh = act ? 1.0 : 0.0;
    int steps = 0;
    for (i64 t0 = T > 1 ? ((T - 1) / 64) * 64 : -1; t0 >= 0; t0 -= 64) {
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        // what the step into frame t = t0 + q >= 1 needs: B[j][o_t], c_t and ah_{t-1} (the lane's own stores)
        int o = __builtin_amdgcn_readlane(mysym, n - 1);
        double b = act ? Brow[o] : 0.0;
        double a = (act && t0 + n - 1 >= 1) ? arow[(size_t)(t0 + n - 2) * sumN] : 0.0;
        double cv = lane == 0 ? crow[(size_t)(t0 + n - 1) * nw] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double bq = b, aq = a, cq = cv;
            const i64 t = t0 + q;
            if (t == 0) break;
            if (q > 0) {  // the previous frame's loads are requested before this frame's chains run
                o = __builtin_amdgcn_readlane(mysym, q - 1);
                b = act ? Brow[o] : 0.0;
                a = (act && t >= 2) ? arow[(size_t)(t - 2) * sumN] : 0.0;
                cv = lane == 0 ? crow[(size_t)(t - 1) * nw] : 0.0;
            }
            // S_t of this lane's class: the class sum of ah_{t-1} in state order
            const double S = chain_sum(aq, N, seg, maxN, single);
            const double ct = bcast(cq, 0);
            const double u = act ? (bq * bh) / ct : 0.0;
            // the in-class chain, and on the way what leaves through the class's pi: R = sum_j pi[j] u[j]
            const ChainPair cr = chain_row_pi(u, Arow, pik, N, seg, maxN, single);
            const double acc_b = cr.acc, R = cr.sum;
            // R of this step lives in Xb[steps & 1]: a wave writes that half again two steps on, past the barrier of the
            // step between, which every wave reaches only after its walk and its products of this step
            double* Rt = Xb + (size_t)(steps++ & 1) * K;
            if (head) Rt[k] = R;
            __syncthreads();
            double r = wrow[0] * Rt[0];
            for (int kk = 1; kk < K; ++kk) r = r + wrow[kk] * Rt[kk];
            bh = act ? acc_b + r : 0.0;
            // the counts of class f = k: this lane's share of the K targets
            if (act) {
                i64* crow_l = Cs + (size_t)k * K * 2;
                i64* crow_g = acc + (size_t)k * K * 2;
                for (int kk = L.j; kk < K; kk += N) an_add(c_lds, crow_l + 2 * kk, crow_g + 2 * kk, S * (wrow[kk] * Rt[kk]));
            }
        }
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
size_t trans_estep_lds_bytes(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds)
{
    return ((size_t)2 * SEG_MAX_WAVES + (size_t)2 * pl.K + (size_t)pl.sumN + (c_lds ? (size_t)2 * pl.K * pl.K : 0) +
            (a_lds ? (size_t)pl.a_words : 0) + (w_lds ? (size_t)2 * pl.K * pl.K : 0)) * sizeof(double);
}

void trans_estep_layout(const SegPlanDev& pl, bool c_forced, bool* c_lds, bool* a_lds, bool* w_lds)
{
    if (!c_forced) *c_lds = trans_estep_lds_bytes(pl, true, false, false) <= SEG_LDS_BYTES;
    *a_lds = trans_estep_lds_bytes(pl, *c_lds, true, false) <= SEG_LDS_BYTES;
    *w_lds = trans_estep_lds_bytes(pl, *c_lds, *a_lds, true) <= SEG_LDS_BYTES;
}

int launch_trans_estep(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds, const unsigned short* sym, const i64* offs, int S,
                       i64 a0, const double* w, double* ahs, double* cs, i64* acc, double* mant, i64* exp2, int* status,
                       hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || pl.slots > SEG_MAX_WAVES) return 1;
    const size_t lds = trans_estep_lds_bytes(pl, c_lds, a_lds, w_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * pl.slots));
#define E2_TEST_LAUNCH(A_LDS, W_LDS)                                                                                             \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_trans_estep<A_LDS, W_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,        \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_trans_estep<A_LDS, W_LDS>), grid, block, lds, st, pl, sym, offs, a0, w, ahs, cs, c_lds, acc,  \
                           mant, exp2, status);                                                                                  \
    } while (0)
    if (a_lds) {
        if (w_lds) E2_TEST_LAUNCH(true, true);
        else E2_TEST_LAUNCH(true, false);
    } else {
        if (w_lds) E2_TEST_LAUNCH(false, true);
        else E2_TEST_LAUNCH(false, false);
    }
#undef E2_TEST_LAUNCH
    return 0;
}

}  // namespace e2hmm
