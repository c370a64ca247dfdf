// hmm_loop_estep.hip -- HIP kernel (gfx950) of `hmm learn --loop`: the expected state-level counts of every
// class model under the class loop and the K x K prices w[f][k] = exp(lt[f][k]) -- the E-step of Baum-Welch for pi, A and B of
// all classes at once, and on request for the grammar too -- bit-exact against the restatement.  Forward, scaling, status and
// backward are hmm_posterior_trans.hip's steps (4.8.13: the same chains of hmm_lane.h, the same barriers, the same scratch
// discipline); the counts of lane (k, j), state j of class k, are
//   g = ah_t[k][j] * bh_t[k][j]                          -> BN[j][o_t], BD[j], and PI[j] at t = 0          every frame
//   (ah_{t-1}[k][i] * A_k[i][j]) * u_t[k][j]             -> AN[i][j]                                       t = 1 .. T - 1
//   (m_t[k] * pi_k[j]) * u_t[k][j]                       -> PI[j]: the entries through pi                  t = 1 .. T - 1
// with u_t = (B_k[j][o_t] * bh_t) / c_t, and with GRAM 4.8.14's xi_t[f][k] = S_t[f] * (w[f][k] * R_t[k]) into the K x K table.
// Each becomes two int32 limbs (hmm_limbs.h) added to int64 cells: all sums are integers, so neither the split over
// workgroups nor the order of the streams nor the route of an atomic changes a bit.
//   k_hmm_loop_estep   one workgroup per stream, a wave per slot of k_hmm_segment's packing (resident only: at most 16 slots).
//                      m_t[k], the mass that entered class k at frame t, is stored by the forward pass, once a class (8 K bytes a
//                      frame beside ah and c); the lanes of class k load it at one address and form m * pi from the operands the
//                      forward step used, hence its bits.  BD and PI stay in registers over the stream (a lane is one composite
//                      state) and are flushed once; BN goes by global atomics; AN goes to an LDS table over all classes
//                      (ds_add_u64, flushed once a stream) or to the classes' blocks directly (an_lds), the C table likewise
//                      (c_lds): the host's choices.  A zero limb adds nothing and issues no atomic.
// A stream of status != 0 adds nothing but its mark: `used` of every class counts the status-0 streams, `skipped` the others
// (every class is in the loop).  AD is k_hmm_embed_rowsum's, the M-step k_hmm_reestimate_embedded (hmm_embed.hip), unchanged.
// Nothing transcendental runs here; the unit is compiled with -ffp-contract=off.
#include "hmm_limbs.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x slots.  Dynamic LDS: 2 x SEG_MAX_WAVES partials | the class masses of two
// consecutive steps, 2 x K doubles | pi (sumN) | the AN table, 2 a_words int64 (an_lds) | the C table, 2 K^2 int64 (GRAM and
// c_lds) | A of every class (A_LDS) | w and wT (W_LDS).  pl.params and wg: k_hmm_loop_posteriors_trans's.  classes: N, a_at
// (leading dimension N | 1) and acc_at of every class.  acc: the classes' blocks, added to; acc_t (GRAM): 2 K^2 + 2 words,
// added to.  ahs / cs: 4.8.13's tables; ms: K doubles a frame, indexed as they are.
template <bool A_LDS, bool W_LDS, bool GRAM>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_loop_estep(SegPlanDev pl, const EmbedClassDev* __restrict__ classes,
                                                                       const u16* __restrict__ sym, const i64* __restrict__ offs,
                                                                       i64 a0, const double* __restrict__ wg, double* ahs, double* cs,
                                                                       double* ms, bool an_lds, bool c_lds, i64* acc, i64* acc_t,
                                                                       double* __restrict__ mant, i64* __restrict__ exp2,
                                                                       int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K;
    const int cells = 2 * K * K;
    double* parts = (double*)smem;            // [2][SEG_MAX_WAVES]
    double* Xb = parts + 2 * SEG_MAX_WAVES;   // [2][K]
    double* pis = Xb + 2 * K;                 // [sumN]
    i64* ANs = (i64*)(pis + sumN);            // [a_words][hi, lo]
    i64* Cs = ANs + (an_lds ? 2 * pl.a_words : 0);  // [K][K][2]
    double* As = (double*)(Cs + ((GRAM && c_lds) ? cells : 0));
    double* ws = As + (A_LDS ? pl.a_words : 0);
    const double* pig = pl.params;
    const double* Ag = pig + sumN;
    const double* Bg = Ag + pl.a_words;
    for (int x = threadIdx.x; x < sumN; x += blockDim.x) pis[x] = pig[x];
    if (an_lds)
        for (int x = threadIdx.x; x < 2 * pl.a_words; x += blockDim.x) ANs[x] = 0;
    if (GRAM && c_lds)
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
    // are kept at +0.0 and it adds no count
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
    double* mrow = ms + (size_t)(base - a0) * K + k;      // m_t of this lane's class at mrow[t * K]
    int st = 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward (4.8.13's): ah_t, c_t and m_t of every frame; the first event in frame order decides the status -------
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
                if (head) mrow[(size_t)t * K] = m;
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
        if (GRAM) atomicAdd((u64*)&acc_t[cells + (st == 0 ? 0 : 1)], (u64)1);
    }
    // the stream's mark in every class's block: every class is in the loop
    for (int x = threadIdx.x; x < K; x += blockDim.x) {
        const EmbedClassDev cx = classes[x];
        atomicAdd((u64*)&acc[cx.acc_at + 2 * ((i64)cx.N * (3 + cx.N + M)) + (st == 0 ? 0 : 1)], (u64)1);
    }
    if (st != 0 || T < 1) return;  // (workgroup-uniform) the stream adds nothing else: no limb has been formed yet
    // (the last forward walk lies before that step's block_sum barrier: Xb is free for the backward pass; the m_t a lane
    // loads below were stored by a lane of its own wave)

    // the class's accumulators: PI[N] | AN[N][N] | AD[N] | BN[N][M] | BD[N] | used, skipped -- [hi, lo] pairs
    i64* PI = acc + classes[k].acc_at;
    i64* AN = PI + 2 * N;
    i64* BN = AN + 2 * (i64)N * N + 2 * N;
    i64* BD = BN + 2 * (i64)N * M;
    i64* BNrow = BN + 2 * (i64)L.j * M;
    i64* ANl = ANs + 2 * (L.a_at + L.j);  // AN[i][j] of the LDS table at ANl[2 i ld]
    i64* ANg = AN + 2 * L.j;              // ... of the class's block at ANg[2 i N]

    // ---- backward (4.8.13's): bh_{t-1} from bh_t, the counts of frame t and of the step into it ---------------------------
    double bh = act ? 1.0 : 0.0;
    double a_cur = ah;  // ah_{T-1}; every earlier one was stored by this very lane
    i64 bd[2] = {0, 0}, pic[2] = {0, 0};
    int steps = 0;
    for (i64 t0 = T > 1 ? ((T - 1) / 64) * 64 : -1; t0 >= 0; t0 -= 64) {
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        // what the step into frame t = t0 + q >= 1 needs: B[j][o_t], c_t, m_t and ah_{t-1} (the lane's own wave's stores)
        int o = __builtin_amdgcn_readlane(mysym, n - 1);
        double b = act ? Brow[o] : 0.0;
        double a = (act && t0 + n - 1 >= 1) ? arow[(size_t)(t0 + n - 2) * sumN] : 0.0;
        double mv = (act && t0 + n - 1 >= 1) ? mrow[(size_t)(t0 + n - 1) * K] : 0.0;
        double cv = lane == 0 ? crow[(size_t)(t0 + n - 1) * nw] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double bq = b, aq = a, cq = cv, mq = mv;
            const int oq = o;
            const i64 t = t0 + q;
            if (t == 0) break;
            if (q > 0) {  // the previous frame's loads are requested before this frame's chains run
                o = __builtin_amdgcn_readlane(mysym, q - 1);
                b = act ? Brow[o] : 0.0;
                a = (act && t >= 2) ? arow[(size_t)(t - 2) * sumN] : 0.0;
                mv = (act && t >= 2) ? mrow[(size_t)(t - 1) * K] : 0.0;
                cv = lane == 0 ? crow[(size_t)(t - 1) * nw] : 0.0;
            }
            // the occupancy of frame t
            const double g = a_cur * bh;
            if (act) {
                acc_add(BNrow + 2 * oq, g);
                acc_local(bd, g);
            }
            const double ct = bcast(cq, 0);
            const double u = act ? (bq * bh) / ct : 0.0;
            if (act) acc_local(pic, (mq * pij) * u);  // the expected entries through pi
            // the in-class chain, and on the way what leaves through the class's pi: R = sum_j pi[j] u[j]
            const ChainPair cr = chain_row_pi(u, Arow, pik, N, seg, maxN, single);
            const double acc_b = cr.acc, R = cr.sum;
            // R of this step lives in Xb[steps & 1]: a wave writes that half again two steps on, past the barrier of the
            // step between, which every wave reaches only after its walk and its products of this step
            double* Rt = Xb + (size_t)(steps++ & 1) * K;
            if (head) Rt[k] = R;
            // xi_{t-1}(i, j) = (ah_{t-1}(i) A_ij) u_j for this lane's j
            if (single) {
                for (int i = 0; i < maxN; ++i) {
                    const double xi = (bcast(aq, i) * Acol[i * ld]) * u;
                    if (act) an_add(an_lds, ANl + 2 * (i * ld), ANg + 2 * (i * N), xi);
                }
            } else {
                for (int i = 0; i < maxN; ++i) {
                    const int ii = i < N ? i : 0;
                    const double xi = (lane_read(aq, seg + ii) * Acol[ii * ld]) * u;
                    if (act && i < N) an_add(an_lds, ANl + 2 * (i * ld), ANg + 2 * (i * N), xi);
                }
            }
            double S = 0.0;
            if (GRAM) S = chain_sum(aq, N, seg, maxN, single);  // S_t of this lane's class: ah_{t-1} in state order
            __syncthreads();
            double r = wrow[0] * Rt[0];
            for (int kk = 1; kk < K; ++kk) r = r + wrow[kk] * Rt[kk];
            bh = act ? acc_b + r : 0.0;
            a_cur = aq;
            // the grammar counts of class f = k: this lane's share of the K targets
            if (GRAM && act) {
                i64* crow_l = Cs + (size_t)k * K * 2;
                i64* crow_g = acc_t + (size_t)k * K * 2;
                for (int kk = L.j; kk < K; kk += N) an_add(c_lds, crow_l + 2 * kk, crow_g + 2 * kk, S * (wrow[kk] * Rt[kk]));
            }
        }
    }
    // ---- frame 0: its occupancy is also the count of the first entry ------------------------------------------------------
    if (act) {
        const int o0 = (int)sym[base];
        const double g = a_cur * bh;
        acc_add(BNrow + 2 * o0, g);
        acc_local(bd, g);
        acc_local(pic, g);
        // ---- flush: the lane's sums
        if (bd[0]) atomicAdd((u64*)&BD[2 * L.j], (u64)bd[0]);
        if (bd[1]) atomicAdd((u64*)&BD[2 * L.j + 1], (u64)bd[1]);
        if (pic[0]) atomicAdd((u64*)&PI[2 * L.j], (u64)pic[0]);
        if (pic[1]) atomicAdd((u64*)&PI[2 * L.j + 1], (u64)pic[1]);
    }
    if (an_lds || (GRAM && c_lds)) __syncthreads();
    if (an_lds) {  // the stream's tables into the global ones: a zero word adds nothing
        for (int kk = 0; kk < K; ++kk) {
            const EmbedClassDev ck = classes[kk];
            const int Nk = ck.N, ldk = Nk | 1;
            i64* ANk = acc + ck.acc_at + 2 * Nk;
            for (int x = threadIdx.x; x < 2 * Nk * Nk; x += blockDim.x) {
                const int e = x >> 1, i = e / Nk, j = e - i * Nk;
                const i64 v = ANs[2 * (ck.a_at + i * ldk + j) + (x & 1)];
                if (v != 0) atomicAdd((u64*)&ANk[x], (u64)v);
            }
        }
    }
    if (GRAM && c_lds) {
        for (int x = threadIdx.x; x < cells; x += blockDim.x) {
            const i64 v = Cs[x];
            if (v) atomicAdd((u64*)&acc_t[x], (u64)v);
        }
    }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------
size_t loop_estep_lds_bytes(const SegPlanDev& pl, bool an_lds, bool c_lds, bool a_lds, bool w_lds)
{
    return ((size_t)2 * SEG_MAX_WAVES + (size_t)2 * pl.K + (size_t)pl.sumN + (an_lds ? (size_t)2 * pl.a_words : 0) +
            (c_lds ? (size_t)2 * pl.K * pl.K : 0) + (a_lds ? (size_t)pl.a_words : 0) + (w_lds ? (size_t)2 * pl.K * pl.K : 0)) *
           sizeof(double);
}

void loop_estep_layout(const SegPlanDev& pl, bool gram, bool an_forced, bool c_forced, bool* an_lds, bool* c_lds, bool* a_lds,
                       bool* w_lds)
{
    if (!an_forced) *an_lds = loop_estep_lds_bytes(pl, true, false, false, false) <= SEG_LDS_BYTES;
    if (!gram) *c_lds = false;
    else if (!c_forced) *c_lds = loop_estep_lds_bytes(pl, *an_lds, true, false, false) <= SEG_LDS_BYTES;
    *a_lds = loop_estep_lds_bytes(pl, *an_lds, *c_lds, true, false) <= SEG_LDS_BYTES;
    *w_lds = loop_estep_lds_bytes(pl, *an_lds, *c_lds, *a_lds, true) <= SEG_LDS_BYTES;
}

int launch_loop_estep(const SegPlanDev& pl, const EmbedClassDev* classes, bool an_lds, bool c_lds, bool a_lds, bool w_lds,
                      const unsigned short* sym, const i64* offs, int S, i64 a0, const double* w, double* ahs, double* cs, double* ms,
                      i64* acc, i64* acc_trans, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || pl.slots > SEG_MAX_WAVES) return 1;
    const bool gram = acc_trans != nullptr;
    if (!gram) c_lds = false;
    const size_t lds = loop_estep_lds_bytes(pl, an_lds, c_lds, a_lds, w_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * pl.slots));
#define E2_LEST_LAUNCH(A_LDS, W_LDS, GRAM)                                                                                       \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_loop_estep<A_LDS, W_LDS, GRAM>, hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_loop_estep<A_LDS, W_LDS, GRAM>), grid, block, lds, st, pl, classes, sym, offs, a0, w, ahs, cs, \
                           ms, an_lds, c_lds, acc, acc_trans, mant, exp2, status);                                               \
    } while (0)
#define E2_LEST_GRAM(A_LDS, W_LDS)                                                                                               \
    do {                                                                                                                         \
        if (gram) E2_LEST_LAUNCH(A_LDS, W_LDS, true);                                                                            \
        else E2_LEST_LAUNCH(A_LDS, W_LDS, false);                                                                                \
    } while (0)
    if (a_lds) {
        if (w_lds) E2_LEST_GRAM(true, true);
        else E2_LEST_GRAM(true, false);
    } else {
        if (w_lds) E2_LEST_GRAM(false, true);
        else E2_LEST_GRAM(false, false);
    }
#undef E2_LEST_GRAM
#undef E2_LEST_LAUNCH
    return 0;
}

}  // namespace e2hmm
