// hmm_segment_stream.hip -- HIP kernels (gfx950) of `hmm segment --continuous`: the joint Viterbi of
// hmm_segment.hip on a stream that arrives block by block and whose old back-pointers are dropped once they are decided.
//   k_hmm_segment_stream            one block of one stream per workgroup: k_hmm_segment's two bodies (same packing, in-class
//                                   chain, (value, index) maximum and 64-symbol fetch) started from the d the previous block
//                                   left and ended by storing d; the frame-0 rule holds at the absolute frame 0 only.  psi and g
//                                   go to the ring of the pending frames, G to a staging row of the block.
//   k_hmm_segment_coalesce          one workgroup, its threads over the composite states: every live state's path is stepped
//                                   back through the ring in lockstep until all are in one state (the frames up to there are
//                                   decided) or the first pending frame is passed.  At close: the maximum of d instead.
//   k_hmm_segment_stream_backtrack  one thread: cls, state, entered of the decided frames, and the state the path reaches just
//                                   before them, which must be where the previous commit ended.
// Every d is the closed decode's bit for bit: the same additions in the same order, and a double stored and loaded between
// two blocks is unchanged.
#include "hmm_segment_common.h"
#include "hmm_segment_stream.h"

namespace e2hmm {

namespace {

constexpr int COALESCE_THREADS = 1024;
constexpr int COALESCE_PER_THREAD = SEG_MAX_SUM_N / COALESCE_THREADS;

}  // namespace

// grid: 1, block: 64 x (slots when resident, min(slots, 16) when looped).
// Dynamic LDS: 2 x SEG_MAX_WAVES pairs | lA of every class (A_LDS) | d of two consecutive steps, 2 x sumN doubles (LOOPED).
template <bool LOOPED, bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_segment_stream(SegPlanDev pl, const u16* __restrict__ sym, int n,
                                                                            i64 frame0, double ln_switch, const double* d_in,
                                                                            double* d_out, SegRingDev ring,
                                                                            double* __restrict__ gbest, SegStreamState* state)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Pair* pairs = (Pair*)smem;  // [2][SEG_MAX_WAVES]
    double* lAs = (double*)(pairs + 2 * SEG_MAX_WAVES);
    double* dl = lAs + (A_LDS ? pl.a_words : 0);  // [2][sumN] (LOOPED)
    const int M = pl.M, sumN = pl.sumN;
    const double* lpi = pl.params;
    const double* lAg = lpi + sumN;
    const double* lB = lAg + pl.a_words;
    const int dead = state->status;  // (a symbol >= M in an earlier block: nothing more is decoded)
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) lAs[x] = lAg[x];
    __syncthreads();  // (also: every wave has read the status before thread 0 may write it)
    if (dead != 0) return;
    const double* lA = A_LDS ? lAs : lAg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double NINF = -__builtin_inf();
    const i64 row0 = frame0 % ring.rows;  // (n <= ring.rows: the block's rows wrap at most once)
    int st = 0, calls = 0, bad_at = 0;

    if (!LOOPED) {
        // a lane without a state: N = 0, j = 0, a_at = 0 (its reads stay in bounds), d is kept at -inf
        const SegLaneDev L = pl.lanes[wib * 64 + lane];
        const bool act = L.cls >= 0;
        const int c = act ? L.comp : 0, N = L.N, seg = L.seg;
        const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib]);
        const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib + 1]) != 0;
        const double lpij = act ? lpi[c] : NINF;
        const double* lBrow = lB + (size_t)c * M;
        const double* lAcol = lA + L.a_at + L.j;
        const int myidx = act ? L.comp : NO_INDEX;
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
                    if (threadIdx.x == 0) gbest[0] = 0.0;
                    continue;
                }
                double G = d;
                int g = myidx;
                block_argmax(G, g, pairs + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
                const double base_t = G + ln_switch;
                double best;
                int arg = 0;
                if (single) {  // the slot holds one class: wave-uniform reads
                    best = bcast(d, 0) + lAcol[0];
                    for (int i = 1; i < maxN; ++i) {
                        const double v = bcast(d, i) + lAcol[i * N];
                        if (v > best) {
                            best = v;
                            arg = i;
                        }
                    }
                } else {  // classes of any N_k side by side: every lane runs to the slot's largest N, and counts to its own
                    best = lane_read(d, seg) + lAcol[0];
                    for (int i = 1; i < maxN; ++i) {
                        const int ii = i < N ? i : 0;
                        const double v = lane_read(d, seg + ii) + lAcol[ii * N];
                        if (i < N && v > best) {
                            best = v;
                            arg = i;
                        }
                    }
                }
                const double x = base_t + lpij;
                if (x > best) {  // (a tie stays in the class)
                    best = x;
                    arg = ENTER;
                }
                d = act ? best + bq : NINF;  // (a lane without a state would else carry what it read from lane 0)
                i64 row = row0 + t;
                if (row >= ring.rows) row -= ring.rows;
                if (act) ring.psi[(size_t)row * sumN + c] = (u16)arg;
                if (threadIdx.x == 0) {
                    ring.gsel[row] = g;
                    gbest[t] = G;
                }
            }
        }
        if (st == 0 && act) d_out[c] = d;
    } else {
        const int slots = pl.slots;
        // (a slot's states read and write only that slot's d, and one wave owns the slot: no barrier around the carried d)
        if (frame0 > 0)
            for (int sl = wib; sl < slots; sl += nw) {
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                if (L.cls >= 0) dl[sumN + L.comp] = d_in[L.comp];
            }
        for (int t = 0; t < n; ++t) {
            const int o = (int)sym[t];  // (workgroup-uniform)
            if (o >= M) {
                st = 2;
                bad_at = t;
                break;
            }
            const bool first = frame0 + t == 0;
            const double* dp = dl + ((t - 1) & 1) * sumN;
            double* dn = dl + (t & 1) * sumN;
            double G = NINF;
            int g = NO_INDEX;
            if (!first) {
                for (int sl = wib; sl < slots; sl += nw) {
                    const SegLaneDev L = pl.lanes[sl * 64 + lane];
                    if (L.cls >= 0) {
                        const double x = dp[L.comp];
                        if (beats(x, L.comp, G, g)) {
                            G = x;
                            g = L.comp;
                        }
                    }
                }
                block_argmax(G, g, pairs + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
            }
            const double base_t = G + ln_switch;
            i64 row = row0 + t;
            if (row >= ring.rows) row -= ring.rows;
            for (int sl = wib; sl < slots; sl += nw) {
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                if (L.cls < 0) continue;
                const int c = L.comp, N = L.N;
                const double b = lB[(size_t)c * M + o];
                double dv;
                if (first) {
                    dv = lpi[c] + b;
                } else {
                    const double* dc = dp + (c - L.j);
                    const double* lAcol = lA + L.a_at + L.j;
                    double best = dc[0] + lAcol[0];
                    int arg = 0;
                    for (int i = 1; i < N; ++i) {
                        const double v = dc[i] + lAcol[i * N];
                        if (v > best) {
                            best = v;
                            arg = i;
                        }
                    }
                    const double x = base_t + lpi[c];
                    if (x > best) {
                        best = x;
                        arg = ENTER;
                    }
                    dv = best + b;
                    ring.psi[(size_t)row * sumN + c] = (u16)arg;
                }
                dn[c] = dv;
            }
            if (threadIdx.x == 0) {
                if (!first) ring.gsel[row] = g;
                gbest[t] = first ? 0.0 : G;
            }
        }
        if (st == 0) {
            const double* dfin = dl + ((n - 1) & 1) * sumN;
            for (int sl = wib; sl < slots; sl += nw) {
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                if (L.cls >= 0) d_out[L.comp] = dfin[L.comp];
            }
        }
    }
    if (threadIdx.x == 0 && st == 2) {
        state->status = 2;
        state->bad_frame = frame0 + bad_at;
    }
}

// grid: 1, block: COALESCE_THREADS; thread x follows the states x, x + COALESCE_THREADS, ...
__global__ __launch_bounds__(COALESCE_THREADS) void k_hmm_segment_coalesce(int sumN, const u16* __restrict__ comp_cls,
                                                                           const int* __restrict__ cls_comp0,
                                                                           const double* __restrict__ d, SegRingDev ring, i64 F,
                                                                           i64 e, int close, SegStreamState* state)
{
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
        __syncthreads();  // (the parity alternates: a wave writes this slot again only after every wave has passed the next barrier)
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
        const int g = ring.gsel[row];
#pragma unroll
        for (int i = 0; i < COALESCE_PER_THREAD; ++i)
            if (q[i] >= 0) {
                const u16 x = prow[q[i]];
                q[i] = x == ENTER ? g : cls_comp0[comp_cls[q[i]]] + (int)x;
            }
        row = row == 0 ? ring.rows - 1 : row - 1;
    }
    if (threadIdx.x == 0) {
        state->fstar = fstar;
        state->a = a;
    }
}

// one thread.  cls / state / entered at [frame - F].
__global__ void k_hmm_segment_stream_backtrack(int sumN, const u16* __restrict__ comp_cls, const int* __restrict__ cls_comp0,
                                               SegRingDev ring, i64 F, SegStreamState* state, u16* __restrict__ cls,
                                               u16* __restrict__ st_out, unsigned char* __restrict__ entered)
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
            reached = -1;
            break;
        }
        const u16 x = ring.psi[(size_t)row * sumN + q];
        entered[t - F] = x == ENTER ? 1 : 0;
        q = x == ENTER ? ring.gsel[row] : cls_comp0[k] + (int)x;
        reached = q;
        row = row == 0 ? ring.rows - 1 : row - 1;
    }
    // the join: the decided frames continue the path of the previous commit (not claimed for a stream that died, status 1)
    state->reached = reached;
    if (F > 0 && state->status == 0 && state->prev_a >= 0 && reached != state->prev_a) state->join_bad = 1;
    state->prev_a = state->a;
}

// ---- launchers ------------------------------------------------------------------------------------------------
namespace {

size_t stream_lds_bytes(const SegPlanDev& pl, bool looped, bool a_lds)
{
    return (size_t)2 * SEG_MAX_WAVES * sizeof(Pair) + (a_lds ? (size_t)pl.a_words * 8 : 0) + (looped ? (size_t)2 * pl.sumN * 8 : 0);
}

}  // namespace

int launch_segment_stream(const SegPlanDev& pl, bool looped, const unsigned short* sym, int n, i64 frame0, double ln_switch,
                          const double* d_in, double* d_out, SegRingDev ring, double* gbest, SegStreamState* state, hipStream_t st)
{
    if (n < 1) return 0;
    if (pl.slots < 1 || (!looped && pl.slots > SEG_MAX_WAVES) || (i64)n > ring.rows) return 1;
    const bool a_lds = stream_lds_bytes(pl, looped, true) <= SEG_LDS_BYTES;
    const size_t lds = stream_lds_bytes(pl, looped, a_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const int nw = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    const dim3 grid(1), block((unsigned)(64 * nw));
#define E2_SEG_LAUNCH(LOOPED, A_LDS)                                                                                                 \
    do {                                                                                                                             \
        if (lds > 64 * 1024 &&                                                                                                       \
            hipFuncSetAttribute((const void*)k_hmm_segment_stream<LOOPED, A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,       \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                                   \
            return 1;                                                                                                                \
        hipLaunchKernelGGL((k_hmm_segment_stream<LOOPED, A_LDS>), grid, block, lds, st, pl, sym, n, frame0, ln_switch, d_in, d_out, \
                           ring, gbest, state);                                                                                      \
    } while (0)
    if (looped) {
        if (a_lds) E2_SEG_LAUNCH(true, true);
        else E2_SEG_LAUNCH(true, false);
    } else {
        if (a_lds) E2_SEG_LAUNCH(false, true);
        else E2_SEG_LAUNCH(false, false);
    }
#undef E2_SEG_LAUNCH
    return 0;
}

void launch_segment_coalesce(const SegPlanDev& pl, const double* d, SegRingDev ring, i64 F, i64 e, int close, SegStreamState* state,
                             hipStream_t st)
{
    hipLaunchKernelGGL(k_hmm_segment_coalesce, dim3(1), dim3(COALESCE_THREADS), 0, st, pl.sumN, pl.comp_cls, pl.cls_comp0, d, ring, F,
                       e, close, state);
}

void launch_segment_stream_backtrack(const SegPlanDev& pl, SegRingDev ring, i64 F, SegStreamState* state, unsigned short* cls,
                                     unsigned short* st_out, unsigned char* entered, hipStream_t st)
{
    hipLaunchKernelGGL(k_hmm_segment_stream_backtrack, dim3(1), dim3(64), 0, st, pl.sumN, pl.comp_cls, pl.cls_comp0, ring, F, state,
                       cls, st_out, entered);
}

}  // namespace e2hmm
