// hmm_segment.hip -- HIP kernels (gfx950) of `hmm segment`: the most likely path of a whole symbol
// stream through the class loop -- the K class models side by side; a path may leave its class at any frame and enter any
// class through that class's pi at the price ln_switch -- in the log domain, bit-exact against the restatement.
//   k_hmm_segment            one workgroup per stream.  The classes are packed in class order into wave-slots of 64 lanes:
//                            class k takes N_k consecutive lanes and never straddles a slot; lane (k, j) is state j.  The
//                            in-class maximisation is k_hmm_viterbi's (d of the other states through ds_bpermute_b32, or
//                            v_readlane where the slot holds one class).  The coupling between the classes is one maximum
//                            per step: every wave reduces (value, composite index) under "greater value, then lower index",
//                            posts its pair to a double-buffered LDS slot, and after the step's one barrier reads all pairs.
//                            Two bodies: resident (<= 16 slots: a wave per slot, d in registers) and looped (a wave takes
//                            several slots in turn, d through a double-buffered LDS array; built to work, not to be fast).
//   k_hmm_segment_backtrack  one thread per stream, in a launch of its own: cls, state, entered.
// The model arrives as logarithms taken on the host (log 0 = -inf): the device adds and compares, nothing else.  Every term
// is finite or -inf and ln_switch <= 0, so no NaN can arise.  psi (u16, ENTER = 0xFFFF) goes to
// psi[(frame - psi0) * sumN + composite index], g_t to gsel[frame - psi0], G_t to gbest[frame] (frame: absolute offset).
#include "hmm_segment_common.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x (slots when resident, min(slots, 16) when looped).
// Dynamic LDS: 2 x SEG_MAX_WAVES pairs | lA of every class (A_LDS) | d of two consecutive steps, 2 x sumN doubles (LOOPED).
template <bool LOOPED, bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_segment(SegPlanDev pl, const u16* __restrict__ sym,
                                                                     const i64* __restrict__ offs, i64 psi0, double ln_switch,
                                                                     u16* __restrict__ psi, int* __restrict__ gsel,
                                                                     double* __restrict__ gbest, double* __restrict__ logp,
                                                                     int* __restrict__ qlast, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Pair* pairs = (Pair*)smem;  // [2][SEG_MAX_WAVES]
    double* lAs = (double*)(pairs + 2 * SEG_MAX_WAVES);
    double* dl = lAs + (A_LDS ? pl.a_words : 0);  // [2][sumN] (LOOPED)
    const int M = pl.M, sumN = pl.sumN;
    const double* lpi = pl.params;
    const double* lAg = lpi + sumN;
    const double* lB = lAg + pl.a_words;
    if (A_LDS) {
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) lAs[x] = lAg[x];
        __syncthreads();
    }
    const double* lA = A_LDS ? lAs : lAg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    const double NINF = -__builtin_inf();
    u16* prow = psi + (size_t)(base - psi0) * sumN;
    int* grow = gsel + (base - psi0);
    double* Grow = gbest + base;
    int st = 0, calls = 0;
    double fin = 0.0;  // max d_{T-1} and the lowest composite index reaching it
    int fin_at = 0;

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
                    if (threadIdx.x == 0) Grow[0] = 0.0;
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
                if (act) prow[(size_t)t * sumN + c] = (u16)arg;
                if (threadIdx.x == 0) {
                    grow[t] = g;
                    Grow[t] = G;
                }
            }
        }
        if (st == 0 && T > 0) {
            fin = d;
            fin_at = myidx;
            block_argmax(fin, fin_at, pairs + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
        }
    } else {
        const int slots = pl.slots;
        for (i64 t = 0; t < T; ++t) {
            const int o = (int)sym[base + t];  // (workgroup-uniform)
            if (o >= M) {
                st = 2;
                break;
            }
            const double* dp = dl + ((t - 1) & 1) * sumN;
            double* dn = dl + (t & 1) * sumN;
            double G = NINF;
            int g = NO_INDEX;
            if (t > 0) {
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
            // (a slot's states read and write only that slot's d, and one wave owns the slot: no barrier between the steps' d)
            for (int sl = wib; sl < slots; sl += nw) {
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                if (L.cls < 0) continue;
                const int c = L.comp, N = L.N;
                const double b = lB[(size_t)c * M + o];
                double dv;
                if (t == 0) {
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
                    prow[(size_t)t * sumN + c] = (u16)arg;
                }
                dn[c] = dv;
            }
            if (threadIdx.x == 0) {
                if (t > 0) grow[t] = g;
                Grow[t] = t > 0 ? G : 0.0;
            }
        }
        if (st == 0 && T > 0) {
            const double* dp = dl + ((T - 1) & 1) * sumN;
            fin = NINF;
            fin_at = NO_INDEX;
            for (int sl = wib; sl < slots; sl += nw) {
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                if (L.cls >= 0) {
                    const double x = dp[L.comp];
                    if (beats(x, L.comp, fin, fin_at)) {
                        fin = x;
                        fin_at = L.comp;
                    }
                }
            }
            block_argmax(fin, fin_at, pairs + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
        }
    }
    if (threadIdx.x == 0) {
        if (st == 0 && T > 0 && fin == NINF) st = 1;
        logp[s] = st == 2 ? NINF : fin;
        qlast[s] = fin_at;
        status[s] = st;
    }
}

// one thread per stream of the launch.  cls / state / entered / gbest are indexed by the absolute offsets; psi and gsel as
// the forward kernel wrote them.  comp_cls[c]: the class of composite index c; cls_comp0[k]: the composite index of (k, 0).
__global__ void k_hmm_segment_backtrack(int sumN, const u16* __restrict__ comp_cls, const int* __restrict__ cls_comp0,
                                        const i64* __restrict__ offs, int S, i64 psi0, const u16* __restrict__ psi,
                                        const int* __restrict__ gsel, const int* __restrict__ qlast,
                                        const int* __restrict__ status, u16* __restrict__ cls, u16* __restrict__ state,
                                        unsigned char* __restrict__ entered, double* __restrict__ gbest)
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
            gbest[base + t] = t == 0 ? 0.0 : -__builtin_inf();
        }
        return;
    }
    const u16* ps = psi + (size_t)(base - psi0) * sumN;
    const int* gs = gsel + (base - psi0);
    int q = qlast[s];
    for (i64 t = T - 1; t >= 0; --t) {
        const int k = comp_cls[q];
        cls[base + t] = (u16)k;
        state[base + t] = (u16)(q - cls_comp0[k]);
        if (t == 0) {
            entered[base] = 1;
            break;
        }
        const u16 a = ps[(size_t)t * sumN + q];
        entered[base + t] = a == ENTER ? 1 : 0;
        q = a == ENTER ? gs[t] : cls_comp0[k] + (int)a;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------
size_t segment_lds_bytes(const SegPlanDev& pl, bool looped, bool a_lds)
{
    return (size_t)2 * SEG_MAX_WAVES * sizeof(Pair) + (a_lds ? (size_t)pl.a_words * 8 : 0) + (looped ? (size_t)2 * pl.sumN * 8 : 0);
}

int launch_segment(const SegPlanDev& pl, bool looped, const unsigned short* sym, const i64* offs, int S, i64 psi0, double ln_switch,
                   unsigned short* psi, int* gsel, double* gbest, double* logp, int* qlast, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || (!looped && pl.slots > SEG_MAX_WAVES)) return 1;
    const bool a_lds = segment_lds_bytes(pl, looped, true) <= SEG_LDS_BYTES;
    const size_t lds = segment_lds_bytes(pl, looped, a_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const int nw = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    const dim3 grid((unsigned)S), block((unsigned)(64 * nw));
#define E2_SEG_LAUNCH(LOOPED, A_LDS)                                                                                             \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_segment<LOOPED, A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,          \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_segment<LOOPED, A_LDS>), grid, block, lds, st, pl, sym, offs, psi0, ln_switch, psi, gsel, gbest, \
                           logp, qlast, status);                                                                                 \
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

void launch_segment_backtrack(const SegPlanDev& pl, const i64* offs, int S, i64 psi0, const unsigned short* psi, const int* gsel,
                              const int* qlast, const int* status, unsigned short* cls, unsigned short* state,
                              unsigned char* entered, double* gbest, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(k_hmm_segment_backtrack, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, pl.sumN, pl.comp_cls,
                       pl.cls_comp0, offs, S, psi0, psi, gsel, qlast, status, cls, state, entered, gbest);
}

}  // namespace e2hmm
