// hmm_align.hip -- HIP kernels (gfx950) of `hmm align`: the most likely path of a whole symbol stream
// through the units of its transcript in their order -- unit l is a copy of the model of class c_l; a path leaves unit l - 1
// for unit l through that class's pi at the price ln_switch, and may pass over an optional unit -- in the log domain,
// bit-exact against the restatement.
//   k_hmm_align            one workgroup per stream.  The units are packed in unit order into wave-slots of 64 lanes as
//                          hmm_segment.hip packs classes; the parameters stay per class (a lane carries its class's rows).
//                          The in-class chain is k_hmm_segment's and yields the unit's exit (E, x) on the way, as
//                          k_hmm_segment_trans does.  The state-0 lane of unit l posts E[l] to a double-buffered LDS array
//                          of 2 x L doubles; after the step's one barrier a lane reads E[l - 1] and, behind an optional
//                          unit, E[l - 2]: two LDS reads, no walk over sources, and no workgroup maximum until the one
//                          after the last step.  Two bodies: resident (<= 16 slots: a wave per slot, d in a register) and
//                          looped (a wave takes several slots in turn, d through a double-buffered LDS array).
//   k_hmm_align_backtrack  one thread per stream, in a launch of its own: unit, state, entered; begin / end of every unit.
// The model arrives as logarithms taken on the host (log 0 = -inf): the device adds and compares, nothing else.  Every term
// is finite or -inf and ln_switch is finite, so no NaN can arise.  Back-pointers, one byte each: psi[t * sumN + composite
// index] = the in-class predecessor or ALIGN_ENTER_1 / ALIGN_ENTER_2; xs[t * L + l] = the exit state of unit l at step t.
#include "hmm_segment_common.h"

namespace e2hmm {

typedef unsigned char u8;

// grid: the streams of the launch, block: 64 x waves.
// Dynamic LDS: SEG_MAX_WAVES pairs | E of two consecutive steps, 2 x max_L doubles | lA of every class (A_LDS) |
// d of two consecutive steps, 2 x max_sumN doubles (LOOPED).
template <bool LOOPED, bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_align(AlignPlanDev pl, const u16* __restrict__ sym,
                                                                   const i64* __restrict__ offs, double ln_switch,
                                                                   u8* __restrict__ tab, double* __restrict__ logp,
                                                                   int* __restrict__ qlast, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Pair* pairs = (Pair*)smem;                      // [SEG_MAX_WAVES]
    double* Eb = (double*)(pairs + SEG_MAX_WAVES);  // [2][max_L]
    double* lAs = Eb + 2 * (size_t)pl.max_L;
    double* dl = lAs + (A_LDS ? pl.a_words : 0);  // [2][max_sumN] (LOOPED)
    const int M = pl.M;
    const double* lpi = pl.params;
    const double* lAg = lpi + pl.sumN_cls;
    const double* lB = lAg + pl.a_words;
    if (A_LDS) {
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) lAs[x] = lAg[x];
        __syncthreads();
    }
    const double* lA = A_LDS ? lAs : lAg;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const AlignStreamDev sd = pl.streams[s];
    const int sumN = sd.sumN, Lu = sd.L, slots = sd.slots;
    const AlignLaneDev* lanes = pl.lanes + sd.lane_at;
    const int* slot_info = pl.slot_info + sd.lane_at / 32;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    const double NINF = -__builtin_inf();
    u8* prow = tab + sd.tab_at;             // [T][sumN]
    u8* xrow = prow + (size_t)T * sumN;     // [T][L]
    int st = 0;
    double fin = 0.0;  // max d_{T-1} over the states that may end the path, and the lowest composite index reaching it
    int fin_at = 0;

    if (!LOOPED) {
        // a lane without a state (a wave without a slot holds none but these): N = 0, j = 0, row = a_at = 0 (its reads stay
        // in bounds), d is kept at -inf
        const bool have = wib < slots;
        AlignLaneDev L = lanes[(have ? wib : 0) * 64 + lane];
        if (!have) L = AlignLaneDev{-1, 0, 0, lane, 0, 0, 0, 0};
        const bool act = L.unit >= 0;
        const bool head = act && L.j == 0;  // the lane that posts and stores for its unit
        const int c = act ? L.comp : 0, N = L.N, seg = L.seg, l = act ? L.unit : 0, flags = L.flags;
        const int maxN = have ? __builtin_amdgcn_readfirstlane(slot_info[2 * wib]) : 0;
        const bool single = have && __builtin_amdgcn_readfirstlane(slot_info[2 * wib + 1]) != 0;
        const double lpij = act ? lpi[L.row] : NINF;
        const double* lBrow = lB + (size_t)L.row * M;
        const double* lAcol = lA + L.a_at + L.j;
        const int l1 = l >= 1 ? l - 1 : 0, l2 = l >= 2 ? l - 2 : 0;
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
                    d = (flags & ALIGN_INIT) ? lpij + bq : NINF;
                    continue;
                }
                // the in-class chain, and on the way the unit's exit: the greatest d_{t-1}, the lowest state reaching it
                double best, E;
                int arg = 0, x = 0;
                if (single) {  // the slot holds one unit: wave-uniform reads
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
                } else {  // units of any N side by side: every lane runs to the slot's largest N, and counts to its own
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
                // every wave reaches only after its reads of step t
                double* Et = Eb + (size_t)(t & 1) * pl.max_L;
                if (head) {
                    Et[l] = E;
                    xrow[(size_t)t * Lu + l] = (u8)x;
                }
                __syncthreads();
                // the way in: from the unit before, or over an optional one when that is strictly better
                double e = (flags & ALIGN_PRED) ? Et[l1] : NINF;
                int code = ALIGN_ENTER_1;
                if (flags & ALIGN_SKIP) {
                    const double e2 = Et[l2];
                    if (e2 > e) {
                        e = e2;
                        code = ALIGN_ENTER_2;
                    }
                }
                const double xe = (e + ln_switch) + lpij;
                if (xe > best) {  // (a tie stays in the unit)
                    best = xe;
                    arg = code;
                }
                d = act ? best + bq : NINF;  // (a lane without a state would else carry what it read from lane 0)
                if (act) prow[(size_t)t * sumN + c] = (u8)arg;
            }
        }
        if (st == 0 && T > 0) {
            const bool last = act && (flags & ALIGN_FINAL);
            fin = last ? d : NINF;
            fin_at = last ? c : NO_INDEX;
            block_argmax(fin, fin_at, pairs, wib, lane, nw);
        }
    } else {
        for (i64 t = 0; t < T; ++t) {
            const int o = (int)sym[base + t];  // (workgroup-uniform)
            if (o >= M) {
                st = 2;
                break;
            }
            const double* dp = dl + ((t - 1) & 1) * (size_t)pl.max_sumN;
            double* dn = dl + (t & 1) * (size_t)pl.max_sumN;
            double* Et = Eb + (size_t)(t & 1) * pl.max_L;  // (the halves alternate as in the resident body)
            if (t > 0) {
                // every unit's exit from d_{t-1}, by its state-0 lane
                for (int sl = wib; sl < slots; sl += nw) {
                    const AlignLaneDev L = lanes[sl * 64 + lane];
                    if (L.unit < 0 || L.j != 0) continue;
                    const double* dc = dp + L.comp;
                    double E = dc[0];
                    int x = 0;
                    for (int i = 1; i < L.N; ++i)
                        if (dc[i] > E) {
                            E = dc[i];
                            x = i;
                        }
                    Et[L.unit] = E;
                    xrow[(size_t)t * Lu + L.unit] = (u8)x;
                }
                __syncthreads();
            }
            // (a slot's states read and write only that slot's d, and one wave owns the slot: no barrier between the steps' d)
            for (int sl = wib; sl < slots; sl += nw) {
                const AlignLaneDev L = lanes[sl * 64 + lane];
                if (L.unit < 0) continue;
                const int c = L.comp, N = L.N, l = L.unit;
                const double b = lB[(size_t)L.row * M + o];
                const double lpij = lpi[L.row];
                double dv;
                if (t == 0) {
                    dv = (L.flags & ALIGN_INIT) ? lpij + b : NINF;
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
                    double e = (L.flags & ALIGN_PRED) ? Et[l >= 1 ? l - 1 : 0] : NINF;
                    int code = ALIGN_ENTER_1;
                    if (L.flags & ALIGN_SKIP) {
                        const double e2 = Et[l >= 2 ? l - 2 : 0];
                        if (e2 > e) {
                            e = e2;
                            code = ALIGN_ENTER_2;
                        }
                    }
                    const double xe = (e + ln_switch) + lpij;
                    if (xe > best) {
                        best = xe;
                        arg = code;
                    }
                    dv = best + b;
                    prow[(size_t)t * sumN + c] = (u8)arg;
                }
                dn[c] = dv;
            }
        }
        if (st == 0 && T > 0) {
            const double* dp = dl + ((T - 1) & 1) * (size_t)pl.max_sumN;
            fin = NINF;
            fin_at = NO_INDEX;
            for (int sl = wib; sl < slots; sl += nw) {
                const AlignLaneDev L = lanes[sl * 64 + lane];
                if (L.unit >= 0 && (L.flags & ALIGN_FINAL)) {
                    const double x = dp[L.comp];
                    if (beats(x, L.comp, fin, fin_at)) {
                        fin = x;
                        fin_at = L.comp;
                    }
                }
            }
            block_argmax(fin, fin_at, pairs, wib, lane, nw);
        }
    }
    if (threadIdx.x == 0) {
        if (st == 0 && T > 0 && fin == NINF) st = 1;
        logp[s] = st == 2 ? NINF : fin;
        qlast[s] = fin_at;
        status[s] = st;
    }
}

// one thread per stream of the launch.  unit / state / entered are indexed by the absolute offsets, begin / end by the
// stream's unit_at; the tables as the forward kernel wrote them.
__global__ void k_hmm_align_backtrack(const AlignStreamDev* __restrict__ streams, const u16* __restrict__ comp_unit,
                                      const int* __restrict__ unit_comp0, const i64* __restrict__ offs, int S,
                                      const u8* __restrict__ tab, const int* __restrict__ qlast, const int* __restrict__ status,
                                      u16* __restrict__ unit, u16* __restrict__ state, u8* __restrict__ entered,
                                      i64* __restrict__ begin, i64* __restrict__ end)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const AlignStreamDev sd = streams[s];
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    i64* bg = begin + sd.unit_at;
    i64* en = end + sd.unit_at;
    for (int l = 0; l < sd.L; ++l) {
        bg[l] = -1;
        en[l] = -1;
    }
    if (T < 1) return;
    if (status[s] == 2) {
        for (i64 t = 0; t < T; ++t) {
            unit[base + t] = 0xFFFF;
            state[base + t] = 0xFFFF;
            entered[base + t] = 0;
        }
        return;
    }
    const int sumN = sd.sumN, Lu = sd.L;
    const u8* ps = tab + sd.tab_at;
    const u8* xr = ps + (size_t)T * sumN;
    const u16* cu = comp_unit + sd.comp_at;
    const int* c0 = unit_comp0 + sd.unit_at;
    int q = qlast[s];
    en[cu[q]] = T;
    for (i64 t = T - 1; t >= 0; --t) {
        const int l = cu[q];
        unit[base + t] = (u16)l;
        state[base + t] = (u16)(q - c0[l]);
        if (t == 0) {
            entered[base] = 1;
            bg[l] = 0;
            break;
        }
        const u8 a = ps[(size_t)t * sumN + q];
        if (a >= ALIGN_ENTER_1) {
            const int f = a == ALIGN_ENTER_1 ? l - 1 : l - 2;
            entered[base + t] = 1;
            bg[l] = t;
            en[f] = t;
            q = c0[f] + (int)xr[(size_t)t * Lu + f];
        } else {
            entered[base + t] = 0;
            q = c0[l] + (int)a;
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------
size_t align_lds_bytes(int max_L, int max_sumN, int a_words, bool looped, bool a_lds)
{
    return (size_t)SEG_MAX_WAVES * sizeof(Pair) + (size_t)2 * max_L * 8 + (a_lds ? (size_t)a_words * 8 : 0) +
           (looped ? (size_t)2 * max_sumN * 8 : 0);
}

int launch_align(const AlignPlanDev& pl, bool looped, int waves, const unsigned short* sym, const i64* offs, int S, double ln_switch,
                 unsigned char* tab, double* logp, int* qlast, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (waves < 1 || waves > SEG_MAX_WAVES) return 1;
    const bool a_lds = align_lds_bytes(pl.max_L, pl.max_sumN, pl.a_words, looped, true) <= SEG_LDS_BYTES;
    const size_t lds = align_lds_bytes(pl.max_L, pl.max_sumN, pl.a_words, looped, a_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_ALIGN_LAUNCH(LOOPED, A_LDS)                                                                                           \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_align<LOOPED, A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,            \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_align<LOOPED, A_LDS>), grid, block, lds, st, pl, sym, offs, ln_switch, tab, logp, qlast, status); \
    } while (0)
    if (looped) {
        if (a_lds) E2_ALIGN_LAUNCH(true, true);
        else E2_ALIGN_LAUNCH(true, false);
    } else {
        if (a_lds) E2_ALIGN_LAUNCH(false, true);
        else E2_ALIGN_LAUNCH(false, false);
    }
#undef E2_ALIGN_LAUNCH
    return 0;
}

void launch_align_backtrack(const AlignPlanDev& pl, const i64* offs, int S, const unsigned char* tab, const int* qlast,
                            const int* status, unsigned short* unit, unsigned short* state, unsigned char* entered, i64* begin,
                            i64* end, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(k_hmm_align_backtrack, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, pl.streams, pl.comp_unit,
                       pl.unit_comp0, offs, S, tab, qlast, status, unit, state, entered, begin, end);
}

}  // namespace e2hmm
