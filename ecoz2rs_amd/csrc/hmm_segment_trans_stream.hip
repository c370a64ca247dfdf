// hmm_segment_trans_stream.hip -- HIP kernels (gfx950) of `hmm segment --class-transitions --grammar-continuous`
// (DESIGN.md 4.8.15): the joint Viterbi under class-to-class prices of hmm_segment_trans.hip on a stream that arrives block
// by block and whose old tables are dropped once they are decided, as hmm_segment_stream.hip does it under the one price.
//   k_hmm_segment_trans_stream            one block of one stream per workgroup: k_hmm_segment_trans's step (the chain that
//                                         also yields the class exit before the step's one barrier, E posted to a
//                                         double-buffered LDS array, every lane walking the K sources; the 64-symbol hand-out
//                                         and the early lB request) started from the d the previous block left and ended by
//                                         storing d; the frame-0 rule holds at the absolute frame 0 only.  psi, src, x and E
//                                         go to the ring of the pending frames.
//   k_hmm_segment_trans_coalesce          one workgroup, its threads over the composite states: every live state's path is
//                                         stepped back through the ring in lockstep -- (k, psi), or on ENTER
//                                         (src[k], x[src[k]]) -- until all are in one state or the first pending frame is
//                                         passed.  At close: the maximum of d instead.
//   k_hmm_segment_trans_stream_backtrack  one thread: cls, state, entered, exit_score of the decided frames, and the state the
//                                         path reaches just before them, which must be where the previous commit ended.
// Every d, psi, src, x and E is the closed decode's bit for bit: the same additions and comparisons in the same order
// (hmm_segment_trans_step.h), and a double stored and loaded between two blocks is unchanged.
#include "hmm_segment_common.h"
#include "hmm_segment_trans_step.h"
#include "hmm_segment_trans_stream.h"

namespace e2hmm {

namespace {

constexpr int COALESCE_THREADS = 1024;
constexpr int COALESCE_PER_THREAD = SEG_MAX_SUM_N / COALESCE_THREADS;

}  // namespace

// grid: 1, block: 64 x slots (<= SEG_MAX_WAVES).
// Dynamic LDS: E of two consecutive steps, 2 x K doubles | lA of every class (A_LDS) | ltT (LT_LDS).
template <bool A_LDS, bool LT_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_segment_trans_stream(SegPlanDev pl, const u16* __restrict__ sym, int n,
                                                                                  i64 frame0, const double* __restrict__ ltTg,
                                                                                  const double* d_in, double* d_out,
                                                                                  SegTransRingDev ring, SegStreamState* state)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K;
    double* Eb = (double*)smem;  // [2][K]
    double* lAs = Eb + 2 * K;
    double* lts = lAs + (A_LDS ? pl.a_words : 0);
    const double* lpi = pl.params;
    const double* lAg = lpi + sumN;
    const double* lB = lAg + pl.a_words;
    const int dead = state->status;  // (a symbol >= M in an earlier block: nothing more is decoded)
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) lAs[x] = lAg[x];
    if (LT_LDS)
        for (int x = threadIdx.x; x < K * K; x += blockDim.x) lts[x] = ltTg[x];
    __syncthreads();  // (also: every wave has read the status before thread 0 may write it)
    if (dead != 0) return;
    const double* lA = A_LDS ? lAs : lAg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const double NINF = -__builtin_inf();
    const i64 row0 = frame0 % ring.rows;  // (n <= ring.rows: the block's rows wrap at most once)
    const int par0 = (int)(frame0 & 1);
    int st = 0, bad_at = 0;

    // a lane without a state: N = 0, j = 0, a_at = 0, class 0 in the walk (its reads stay in bounds), d is kept at -inf
    const SegLaneDev L = pl.lanes[wib * 64 + lane];
    const bool act = L.cls >= 0;
    const bool head = act && L.j == 0;  // the lane that posts and stores for its class
    const int c = act ? L.comp : 0, N = L.N, seg = L.seg, k = act ? L.cls : 0;
    const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib]);
    const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib + 1]) != 0;
    const double lpij = act ? lpi[c] : NINF;
    const double* lBrow = lB + (size_t)c * M;
    const double* lAcol = lA + L.a_at + L.j;
    const double* ltk = (LT_LDS ? (const double*)lts : ltTg) + (size_t)k * K;  // lt[f][k] at ltk[f]
    double d = (act && frame0 > 0) ? d_in[c] : NINF;
    for (int t0 = 0; t0 < n && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane (every wave holds the same ones)
        const int m = (n - t0) < 64 ? (n - t0) : 64;
        const int mysym = lane < m ? (int)sym[t0 + lane] : 0;
        int o = __builtin_amdgcn_readlane(mysym, 0);
        double b = (act && o < M) ? lBrow[o] : 0.0;
        for (int q = 0; q < m; ++q) {
            const double bq = b;
            const int oq = o;
            if (q + 1 < m) {  // next step's emission is requested before this step's chain runs
                o = __builtin_amdgcn_readlane(mysym, q + 1);
                b = (act && o < M) ? lBrow[o] : 0.0;
            }
            const int t = t0 + q;
            if (oq >= M) {  // symbol outside the alphabet (workgroup-uniform: no wave reaches a further barrier)
                st = 2;
                bad_at = t;
                break;
            }
            if (frame0 + t == 0) {
                d = lpij + bq;
                continue;
            }
            // the in-class chain, and on the way the class's exit: the greatest d_{t-1}, the lowest state reaching it
            const ChainExit ce = chain_max_exit(d, lAcol, N, seg, maxN, single);
            i64 row = row0 + t;
            if (row >= ring.rows) row -= ring.rows;
            // E of a frame lives in the half of its absolute parity: a wave writes that half again two steps on, past the
            // barrier of the step between, which every wave reaches only after its walk of this step
            double* Et = Eb + (size_t)((par0 + t) & 1) * K;
            if (head) {
                Et[k] = ce.E;
                ring.xs[(size_t)row * K + k] = (u16)ce.x;
                ring.Es[(size_t)row * K + k] = ce.E;
            }
            __syncthreads();
            const Source sw = source_walk(Et, ltk, K);
            double best = ce.best;
            int arg = ce.arg;
            const double xe = sw.base + lpij;
            if (xe > best) {  // (a tie stays in the class)
                best = xe;
                arg = ENTER;
            }
            d = act ? best + bq : NINF;  // (a lane without a state would else carry what it read from lane 0)
            if (act) ring.psi[(size_t)row * sumN + c] = (u16)arg;
            if (head) ring.src[(size_t)row * K + k] = (u16)sw.from;
        }
    }
    if (st == 0 && act) d_out[c] = d;
    if (threadIdx.x == 0 && st == 2) {
        state->status = 2;
        state->bad_frame = frame0 + bad_at;
    }
}

// grid: 1, block: COALESCE_THREADS; thread x follows the states x, x + COALESCE_THREADS, ...
// Dynamic LDS: src | x << 16 of the rows of two consecutive steps, 2 x K words.
__global__ __launch_bounds__(COALESCE_THREADS) void k_hmm_segment_trans_coalesce(int sumN, int K, const u16* __restrict__ comp_cls,
                                                                                 const int* __restrict__ cls_comp0,
                                                                                 const double* __restrict__ d, SegTransRingDev ring,
                                                                                 i64 F, i64 e, int close, SegStreamState* state)
{
    extern __shared__ unsigned int sx[];  // [2][K]
    __shared__ Pair pairs[COALESCE_THREADS / 64];
    __shared__ int lohi[2][COALESCE_THREADS / 64][2];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = COALESCE_THREADS / 64;
    const double NINF = -__builtin_inf();
    if (state->status == 2) {  // (workgroup-uniform; thread 0 writes other fields only)
        if (threadIdx.x == 0) state->fstar = -1;
        return;
    }
    if (close) {  // the end of the stream: the lowest composite index reaching max d, as the closed decode takes it
        double v = NINF;
        int idx = NO_INDEX;
        for (int c = threadIdx.x; c < sumN; c += COALESCE_THREADS) {
            const double x = d[c];
            if (beats(x, c, v, idx)) {
                v = x;
                idx = c;
            }
        }
        block_argmax(v, idx, pairs, wib, lane, nw);
        if (threadIdx.x == 0) {
            state->fstar = e;
            state->a = idx;
            state->logp = v;
            state->status = v == NINF ? 1 : 0;
        }
        return;
    }
    int q[COALESCE_PER_THREAD];
#pragma unroll
    for (int i = 0; i < COALESCE_PER_THREAD; ++i) {
        const int c = (int)threadIdx.x + i * COALESCE_THREADS;
        q[i] = (c < sumN && d[c] > NINF) ? c : -1;
    }
    i64 fstar = -1;
    int a = -1, par = 0;
    i64 row = e % ring.rows;
    for (i64 t = e;; --t) {
        // all live paths in one state at frame t?  the minimum and the maximum of the states over the workgroup
        int lo = NO_INDEX, hi = -1;
#pragma unroll
        for (int i = 0; i < COALESCE_PER_THREAD; ++i)
            if (q[i] >= 0) {
                lo = q[i] < lo ? q[i] : lo;
                hi = q[i] > hi ? q[i] : hi;
            }
        for (int m = 32; m > 0; m >>= 1) {
            const int lo2 = __shfl_xor(lo, m), hi2 = __shfl_xor(hi, m);
            lo = lo2 < lo ? lo2 : lo;
            hi = hi2 > hi ? hi2 : hi;
        }
        if (lane == 0) {
            lohi[par][wib][0] = lo;
            lohi[par][wib][1] = hi;
        }
        // src and x of frame t's row, read once a step for every state's back step (t > F is workgroup-uniform, and then
        // t >= 1: the row was written)
        unsigned int* sxr = sx + (size_t)par * K;
        if (t > F)
            for (int k = threadIdx.x; k < K; k += COALESCE_THREADS)
                sxr[k] = (unsigned int)ring.src[(size_t)row * K + k] | ((unsigned int)ring.xs[(size_t)row * K + k] << 16);
        __syncthreads();  // (the parity alternates: a wave writes this half again only after every wave has passed the next barrier)
        for (int w = 0; w < nw; ++w) {
            const int lo2 = lohi[par][w][0], hi2 = lohi[par][w][1];
            lo = lo2 < lo ? lo2 : lo;
            hi = hi2 > hi ? hi2 : hi;
        }
        par ^= 1;
        if (hi < 0) break;  // no live state: nothing is decided before close
        if (lo == hi) {
            fstar = t;
            a = lo;
            break;
        }
        if (t <= F) break;  // (the walk never leaves the pending frames; frame 0 has no back-pointers)
        const u16* prow = ring.psi + (size_t)row * sumN;
#pragma unroll
        for (int i = 0; i < COALESCE_PER_THREAD; ++i)
            if (q[i] >= 0) {
                const u16 x = prow[q[i]];
                const int k = comp_cls[q[i]];
                if (x == ENTER) {
                    const int f = (int)(sxr[k] & 0xFFFFu);
                    q[i] = cls_comp0[f] + (int)(sxr[f] >> 16);
                } else {
                    q[i] = cls_comp0[k] + (int)x;
                }
            }
        row = row == 0 ? ring.rows - 1 : row - 1;
    }
    if (threadIdx.x == 0) {
        state->fstar = fstar;
        state->a = a;
    }
}

// one thread.  cls / state / entered / exit_score at [frame - F].
__global__ void k_hmm_segment_trans_stream_backtrack(int sumN, int K, const u16* __restrict__ comp_cls,
                                                     const int* __restrict__ cls_comp0, SegTransRingDev ring, i64 F,
                                                     SegStreamState* state, u16* __restrict__ cls, u16* __restrict__ st_out,
                                                     unsigned char* __restrict__ entered, double* __restrict__ exit_score)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const i64 fstar = state->fstar;
    if (state->status == 2 || fstar < F) return;
    int q = state->a, reached = -1;
    i64 row = fstar % ring.rows;
    for (i64 t = fstar; t >= F; --t) {
        const int k = comp_cls[q];
        cls[t - F] = (u16)k;
        st_out[t - F] = (u16)(q - cls_comp0[k]);
        if (t == 0) {
            entered[0] = 1;
            exit_score[0] = 0.0;
            reached = -1;
            break;
        }
        const u16 x = ring.psi[(size_t)row * sumN + q];
        int f = k;
        if (x == ENTER) {
            f = ring.src[(size_t)row * K + k];
            q = cls_comp0[f] + (int)ring.xs[(size_t)row * K + f];
        } else {
            q = cls_comp0[k] + (int)x;
        }
        entered[t - F] = x == ENTER ? 1 : 0;
        exit_score[t - F] = ring.Es[(size_t)row * K + f];  // E_t of the class of frame t - 1
        reached = q;
        row = row == 0 ? ring.rows - 1 : row - 1;
    }
    // the join: the decided frames continue the path of the previous commit (not claimed for a stream that died, status 1)
    state->reached = reached;
    if (F > 0 && state->status == 0 && state->prev_a >= 0 && reached != state->prev_a) state->join_bad = 1;
    state->prev_a = state->a;
}

// ---- launchers ------------------------------------------------------------------------------------------------
int launch_segment_trans_stream(const SegPlanDev& pl, const unsigned short* sym, int n, i64 frame0, const double* ltT,
                                const double* d_in, double* d_out, SegTransRingDev ring, SegStreamState* state, hipStream_t st)
{
    if (n < 1) return 0;
    if (pl.slots < 1 || pl.slots > SEG_MAX_WAVES || (i64)n > ring.rows) return 1;
    bool a_lds, lt_lds;
    segment_trans_layout(pl, &a_lds, &lt_lds);  // (its LDS sum holds SEG_MAX_WAVES pairs more than this kernel's)
    const size_t lds = (size_t)2 * pl.K * 8 + (a_lds ? (size_t)pl.a_words * 8 : 0) + (lt_lds ? (size_t)pl.K * pl.K * 8 : 0);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid(1), block((unsigned)(64 * pl.slots));
#define E2_SEGTS_LAUNCH(A_LDS, LT_LDS)                                                                                             \
    do {                                                                                                                           \
        if (lds > 64 * 1024 &&                                                                                                     \
            hipFuncSetAttribute((const void*)k_hmm_segment_trans_stream<A_LDS, LT_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                                 \
            return 1;                                                                                                              \
        hipLaunchKernelGGL((k_hmm_segment_trans_stream<A_LDS, LT_LDS>), grid, block, lds, st, pl, sym, n, frame0, ltT, d_in, d_out, \
                           ring, state);                                                                                           \
    } while (0)
    if (a_lds) {
        if (lt_lds) E2_SEGTS_LAUNCH(true, true);
        else E2_SEGTS_LAUNCH(true, false);
    } else {
        if (lt_lds) E2_SEGTS_LAUNCH(false, true);
        else E2_SEGTS_LAUNCH(false, false);
    }
#undef E2_SEGTS_LAUNCH
    return 0;
}

void launch_segment_trans_coalesce(const SegPlanDev& pl, const double* d, SegTransRingDev ring, i64 F, i64 e, int close,
                                   SegStreamState* state, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmm_segment_trans_coalesce, dim3(1), dim3(COALESCE_THREADS), (size_t)2 * pl.K * 4, st, pl.sumN, pl.K,
                       pl.comp_cls, pl.cls_comp0, d, ring, F, e, close, state);
}

void launch_segment_trans_stream_backtrack(const SegPlanDev& pl, SegTransRingDev ring, i64 F, SegStreamState* state,
                                           unsigned short* cls, unsigned short* st_out, unsigned char* entered, double* exit_score,
                                           hipStream_t st)
{
    hipLaunchKernelGGL(k_hmm_segment_trans_stream_backtrack, dim3(1), dim3(64), 0, st, pl.sumN, pl.K, pl.comp_cls, pl.cls_comp0, ring,
                       F, state, cls, st_out, entered, exit_score);
}

}  // namespace e2hmm
