// hmm_segment_trans.hip -- HIP kernels (gfx950) of `hmm segment --class-transitions`: the most likely
// path of a whole symbol stream through the class loop when leaving class f for class k costs lt[f][k] -- a K x K matrix
// in the place of hmm_segment.hip's one ln_switch -- in the log domain, bit-exact against the restatement.
//   k_hmm_segment_trans            one workgroup per stream, a wave per slot of hmm_segment.hip's packing (resident body
//                                  only: at most 16 slots).  The in-class chain is k_hmm_segment's; as it visits d of every
//                                  state of the lane's class anyway (ds_bpermute_b32, or v_readlane where the slot holds one
//                                  class), the same loop keeps the class's exit (E, x) = (greatest d, lowest state reaching
//                                  it): the reduction costs one compare a state and no further lane traffic.  The state-0
//                                  lane of class f posts E[f] to a double-buffered LDS array of 2 x K doubles (x[f] is read
//                                  by the backtrack alone and goes to its table only); after the step's one barrier every
//                                  lane of class k walks the K sources itself: base[k], src[k].  ltT[k][f] = lt[f][k], so
//                                  the walk reads consecutive words.
//   k_hmm_segment_trans_backtrack  one thread per stream, in a launch of its own: cls, state, entered, exit_score.
// The model and lt arrive as logarithms (log 0 = -inf): the device adds and compares, nothing else.  Every term is finite
// or -inf and lt <= 0, so no NaN can arise.  Tables, rows relative to psi0: psi (u16, ENTER = 0xFFFF) at
// psi[row * sumN + composite index]; src[row * K + k], xs[row * K + f] (u16) and Es[row * K + f].
// The lane helpers, Pair and block_argmax (called once here, after the last step) are hmm_segment_common.h's.
#include "hmm_segment_common.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x slots (<= SEG_MAX_WAVES).
// Dynamic LDS: SEG_MAX_WAVES pairs | E of two consecutive steps, 2 x K doubles | lA of every class (A_LDS) | ltT (LT_LDS).
template <bool A_LDS, bool LT_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_segment_trans(SegPlanDev pl, const u16* __restrict__ sym,
                                                                           const i64* __restrict__ offs, i64 psi0,
                                                                           const double* __restrict__ ltTg, u16* __restrict__ psi,
                                                                           u16* __restrict__ src, u16* __restrict__ xs,
                                                                           double* __restrict__ Es, double* __restrict__ logp,
                                                                           int* __restrict__ qlast, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Pair* pairs = (Pair*)smem;  // [SEG_MAX_WAVES]
    const int M = pl.M, sumN = pl.sumN, K = pl.K;
    double* Eb = (double*)(pairs + SEG_MAX_WAVES);  // [2][K]
    double* lAs = Eb + 2 * K;
    double* lts = lAs + (A_LDS ? pl.a_words : 0);
    const double* lpi = pl.params;
    const double* lAg = lpi + sumN;
    const double* lB = lAg + pl.a_words;
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) lAs[x] = lAg[x];
    if (LT_LDS)
        for (int x = threadIdx.x; x < K * K; x += blockDim.x) lts[x] = ltTg[x];
    if (A_LDS || LT_LDS) __syncthreads();
    const double* lA = A_LDS ? lAs : lAg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    const double NINF = -__builtin_inf();
    const size_t row0 = (size_t)(base - psi0);
    u16* prow = psi + row0 * sumN;
    u16* srow = src + row0 * K;
    u16* xrow = xs + row0 * K;
    double* Erow = Es + row0 * K;
    int st = 0;

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
    double d = NINF;
    for (i64 t0 = 0; t0 < T && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane (every wave holds the same ones)
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        int o = __builtin_amdgcn_readlane(mysym, 0);
        double b = (act && o < M) ? lBrow[o] : 0.0;
        for (int q = 0; q < n; ++q) {
            const double bq = b;
            const int oq = o;
            if (q + 1 < n) {  // next step's emission is requested before this step's chain runs
                o = __builtin_amdgcn_readlane(mysym, q + 1);
                b = (act && o < M) ? lBrow[o] : 0.0;
            }
            if (oq >= M) {  // symbol outside the alphabet (workgroup-uniform: no wave reaches a further barrier)
                st = 2;
                break;
            }
            const i64 t = t0 + q;
            if (t == 0) {
                d = lpij + bq;
                continue;
            }
            // the in-class chain, and on the way the class's exit: the greatest d_{t-1}, the lowest state reaching it
            double best, E;
            int arg = 0, x = 0;
            if (single) {  // the slot holds one class: wave-uniform reads
                E = bcast(d, 0);
                best = E + lAcol[0];
                for (int i = 1; i < maxN; ++i) {
                    const double di = bcast(d, i);
                    const double v = di + lAcol[i * N];
                    if (di > E) {
                        E = di;
                        x = i;
                    }
                    if (v > best) {
                        best = v;
                        arg = i;
                    }
                }
            } else {  // classes of any N_k side by side: every lane runs to the slot's largest N, and counts to its own
                E = lane_read(d, seg);
                best = E + lAcol[0];
                for (int i = 1; i < maxN; ++i) {
                    const int ii = i < N ? i : 0;
                    const double di = lane_read(d, seg + ii);
                    const double v = di + lAcol[ii * N];
                    if (i < N && di > E) {
                        E = di;
                        x = i;
                    }
                    if (i < N && v > best) {
                        best = v;
                        arg = i;
                    }
                }
            }
            // E of step t lives in Eb[t & 1]: a wave writes that half again at t + 2, past the barrier of t + 1, which
            // every wave reaches only after its walk of step t
            double* Et = Eb + (size_t)(t & 1) * K;
            if (head) {
                Et[k] = E;
                xrow[(size_t)t * K + k] = (u16)x;
                Erow[(size_t)t * K + k] = E;
            }
            __syncthreads();
            // the cheapest way into class k: sources in class order, the lowest wins ties
            double base_t = Et[0] + ltk[0];
            int from = 0;
            for (int f = 1; f < K; ++f) {
                const double v = Et[f] + ltk[f];
                if (v > base_t) {
                    base_t = v;
                    from = f;
                }
            }
            const double xe = base_t + lpij;
            if (xe > best) {  // (a tie stays in the class)
                best = xe;
                arg = ENTER;
            }
            d = act ? best + bq : NINF;  // (a lane without a state would else carry what it read from lane 0)
            if (act) prow[(size_t)t * sumN + c] = (u16)arg;
            if (head) srow[(size_t)t * K + k] = (u16)from;
        }
    }
    double fin = 0.0;  // max d_{T-1} and the lowest composite index reaching it
    int fin_at = 0;
    if (st == 0 && T > 0) {
        fin = d;
        fin_at = act ? L.comp : NO_INDEX;
        block_argmax(fin, fin_at, pairs, wib, lane, nw);
    }
    if (threadIdx.x == 0) {
        if (st == 0 && T > 0 && fin == NINF) st = 1;
        logp[s] = st == 2 ? NINF : fin;
        qlast[s] = fin_at;
        status[s] = st;
    }
}

// one thread per stream of the launch.  cls / state / entered / exit_score are indexed by the absolute offsets; the tables
// as the forward kernel wrote them.  comp_cls[c]: the class of composite index c; cls_comp0[k]: the composite index of (k, 0).
__global__ void k_hmm_segment_trans_backtrack(int sumN, int K, const u16* __restrict__ comp_cls, const int* __restrict__ cls_comp0,
                                              const i64* __restrict__ offs, int S, i64 psi0, const u16* __restrict__ psi,
                                              const u16* __restrict__ src, const u16* __restrict__ xs,
                                              const double* __restrict__ Es, const int* __restrict__ qlast,
                                              const int* __restrict__ status, u16* __restrict__ cls, u16* __restrict__ state,
                                              unsigned char* __restrict__ entered, double* __restrict__ exit_score)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    if (T < 1) return;
    if (status[s] == 2) {
        for (i64 t = 0; t < T; ++t) {
            cls[base + t] = 0xFFFF;
            state[base + t] = 0xFFFF;
            entered[base + t] = 0;
            exit_score[base + t] = t == 0 ? 0.0 : -__builtin_inf();
        }
        return;
    }
    const size_t row0 = (size_t)(base - psi0);
    const u16* ps = psi + row0 * sumN;
    const u16* sr = src + row0 * K;
    const u16* xr = xs + row0 * K;
    const double* Er = Es + row0 * K;
    int q = qlast[s];
    for (i64 t = T - 1; t >= 0; --t) {
        const int k = comp_cls[q];
        cls[base + t] = (u16)k;
        state[base + t] = (u16)(q - cls_comp0[k]);
        if (t == 0) {
            entered[base] = 1;
            exit_score[base] = 0.0;
            break;
        }
        const u16 a = ps[(size_t)t * sumN + q];
        int f = k;
        if (a == ENTER) {
            f = sr[(size_t)t * K + k];
            q = cls_comp0[f] + (int)xr[(size_t)t * K + f];
        } else {
            q = cls_comp0[k] + (int)a;
        }
        entered[base + t] = a == ENTER ? 1 : 0;
        exit_score[base + t] = Er[(size_t)t * K + f];  // E_t of the class of frame t - 1
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------
namespace {
size_t trans_lds_bytes(const SegPlanDev& pl, bool a_lds, bool lt_lds)
{
    return (size_t)SEG_MAX_WAVES * sizeof(Pair) + (size_t)2 * pl.K * 8 + (a_lds ? (size_t)pl.a_words * 8 : 0) +
           (lt_lds ? (size_t)pl.K * pl.K * 8 : 0);
}
}  // namespace

void segment_trans_layout(const SegPlanDev& pl, bool* a_lds, bool* lt_lds)
{
    *a_lds = trans_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;
    *lt_lds = trans_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;
}

int launch_segment_trans(const SegPlanDev& pl, const unsigned short* sym, const i64* offs, int S, i64 psi0, const double* ltT,
                         unsigned short* psi, unsigned short* src, unsigned short* xs, double* Es, double* logp, int* qlast,
                         int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || pl.slots > SEG_MAX_WAVES) return 1;
    bool a_lds, lt_lds;
    segment_trans_layout(pl, &a_lds, &lt_lds);
    const size_t lds = trans_lds_bytes(pl, a_lds, lt_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * pl.slots));
#define E2_SEGT_LAUNCH(A_LDS, LT_LDS)                                                                                            \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_segment_trans<A_LDS, LT_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_segment_trans<A_LDS, LT_LDS>), grid, block, lds, st, pl, sym, offs, psi0, ltT, psi, src, xs,  \
                           Es, logp, qlast, status);                                                                             \
    } while (0)
    if (a_lds) {
        if (lt_lds) E2_SEGT_LAUNCH(true, true);
        else E2_SEGT_LAUNCH(true, false);
    } else {
        if (lt_lds) E2_SEGT_LAUNCH(false, true);
        else E2_SEGT_LAUNCH(false, false);
    }
#undef E2_SEGT_LAUNCH
    return 0;
}

void launch_segment_trans_backtrack(const SegPlanDev& pl, const i64* offs, int S, i64 psi0, const unsigned short* psi,
                                    const unsigned short* src, const unsigned short* xs, const double* Es, const int* qlast,
                                    const int* status, unsigned short* cls, unsigned short* state, unsigned char* entered,
                                    double* exit_score, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(k_hmm_segment_trans_backtrack, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, pl.sumN, pl.K,
                       pl.comp_cls, pl.cls_comp0, offs, S, psi0, psi, src, xs, Es, qlast, status, cls, state, entered,
                       exit_score);
}

}  // namespace e2hmm
