// hmm_segment_trans_looped.hip -- the looped bodies of `hmm segment --class-transitions` and of its session
// `--grammar-continuous` (gfx950; DESIGN.md 4.8.8 and 4.8.15, "The looped body"): the joint Viterbi under class-to-class prices
// of hmm_segment_trans.hip and hmm_segment_trans_stream.hip for classes that take any number of wave-slots.  The contract is
// the resident bodies', comparison for comparison: the same chains in state order, the same walk over the K sources in class
// order, the same tables in the same layouts, so the backtrack, the coalescence and the session's backtrack are reused as they
// are.
//   k_hmm_segment_trans_looped         one workgroup per stream, min(slots, 16) waves; wave w serves the slots w, w + nw,
//                                      w + 2 nw, .. in turn, and lane l of slot sl is the state pl.lanes[sl * 64 + l] for the
//                                      whole stream.
//   k_hmm_segment_trans_stream_looped  the same body on one block of one open stream: started from d_in, ended by storing
//                                      d_out, its rows in the ring; the frame-0 rule at the absolute frame 0 only; nothing is
//                                      decoded once the session's status is set.
// A frame is two passes over the wave's slots around ONE barrier (hmm_segment_trans_looped_step.h):
//   before it     per served slot, the state's d of the previous frame comes from LDS into a register, chain_max_exit runs
//                 through ds_bpermute_b32 / v_readlane_b32 exactly as in the resident stream kernel, the head lane posts E to
//                 Eb[parity][k] and stores x and E; best and arg go to LDS.
//   after it      per served slot, source_walk over Eb[parity], ENTER against best (a tie stays in the class), d = best + b;
//                 psi by every state's lane, src by the head lane.
// Why one barrier suffices: Eb is double-buffered by the frame's absolute parity.  The half written in the first pass of
// frame t is read in the second pass of frame t, behind the barrier of t.  It is written again in the first pass of frame
// t + 2, and a wave gets there only past the barrier of frame t + 1, which every wave reaches only after its second pass of
// frame t, that is after its last read of that half.  The carried arrays (d, best, arg: one word per composite state) are
// touched by the state's own lane alone, in program order: no other lane ever reads them, so they need no fence and no barrier.
//   emissions     lB[c][o_t] is requested at the head of a slot's turn behind the barrier, ahead of the walk, which hides it.
//   status        the symbol check of a frame comes before its arithmetic and before its barrier and reads a wave-uniform
//                 value every wave holds alike: status 2 is workgroup-uniform, no wave waits at a barrier the others skip.
//   the end       the closed stream's maximum of d_{T-1} runs over every served slot's d under "greater value, then lower
//                 composite index" and then through block_argmax, as in k_hmm_segment<LOOPED>.
//   A, ltT        in LDS behind the mandatory arrays when they fit, A first (segment_trans_looped_layout): four instantiations
//                 per kernel.
// The 64-symbol hand-out is the resident body's; no bit depends on it.  Compiled with -ffp-contract=off.
#include "hmm_segment_trans_looped_step.h"
#include "hmm_segment_trans_stream.h"

namespace e2hmm {

namespace {

// Dynamic LDS of both kernels (segment_trans_looped_lds_bytes): SEG_MAX_WAVES pairs (the closed stream's last maximum) | E of
// two consecutive frames, 2 x K doubles | d, sumN doubles | best, sumN doubles | lA of every class (A_LDS) | ltT (LT_LDS) |
// arg, sumN ints (last: everything before it is a multiple of 8 bytes).
template <bool A_LDS, bool LT_LDS>
struct LoopedLds {
    Pair* pairs;
    double* Eb;
    LoopedCarry cy;
    const double* lA;
    const double* ltT;
    // stages A and ltT; the caller's next barrier publishes them
    __device__ __forceinline__ LoopedLds(unsigned char* smem, const SegPlanDev& pl, const double* lAg, const double* ltTg)
    {
        const int K = pl.K, sumN = pl.sumN;
        pairs = (Pair*)smem;
        Eb = (double*)(pairs + SEG_MAX_WAVES);
        cy.d = Eb + 2 * (size_t)K;
        cy.best = cy.d + sumN;
        double* lAs = cy.best + sumN;
        double* lts = lAs + (A_LDS ? pl.a_words : 0);
        cy.arg = (int*)(lts + (LT_LDS ? (size_t)K * K : 0));
        if (A_LDS)
            for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) lAs[x] = lAg[x];
        if (LT_LDS)
            for (int x = threadIdx.x; x < K * K; x += blockDim.x) lts[x] = ltTg[x];
        lA = A_LDS ? lAs : lAg;
        ltT = LT_LDS ? lts : ltTg;
    }
};

}  // namespace

// grid: the streams of the launch, block: 64 x min(slots, SEG_MAX_WAVES).  Arguments and tables: k_hmm_segment_trans's.
template <bool A_LDS, bool LT_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_segment_trans_looped(SegPlanDev pl, const u16* __restrict__ sym,
                                                                                  const i64* __restrict__ offs, i64 psi0,
                                                                                  const double* __restrict__ ltTg, u16* __restrict__ psi,
                                                                                  u16* __restrict__ src, u16* __restrict__ xs,
                                                                                  double* __restrict__ Es, double* __restrict__ logp,
                                                                                  int* __restrict__ qlast, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K, slots = pl.slots;
    const double* lpi = pl.params;
    const double* lAg = lpi + sumN;
    const double* lB = lAg + pl.a_words;
    const LoopedLds<A_LDS, LT_LDS> lds(smem, pl, lAg, ltTg);
    if (A_LDS || LT_LDS) __syncthreads();
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    const double NINF = -__builtin_inf();
    const size_t row0 = (size_t)(base - psi0);
    int st = 0;
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
            if (t == 0) {
                for (int sl = wib; sl < slots; sl += nw) looped_first_turn(pl, sl, lane, o, lpi, lB, lds.cy);
                continue;
            }
            const size_t r = row0 + (size_t)t;
            const LoopedRows row{psi + r * sumN, src + r * K, xs + r * K, Es + r * K};
            double* Et = lds.Eb + (size_t)(t & 1) * K;
            for (int sl = wib; sl < slots; sl += nw) looped_exit_turn(pl, sl, lane, lds.lA, lds.cy, Et, row);
            __syncthreads();
            for (int sl = wib; sl < slots; sl += nw) looped_enter_turn(pl, sl, lane, o, lpi, lB, lds.ltT, lds.cy, Et, row);
        }
    }
    double fin = 0.0;  // max d_{T-1} and the lowest composite index reaching it
    int fin_at = 0;
    if (st == 0 && T > 0) {
        fin = NINF;
        fin_at = NO_INDEX;
        for (int sl = wib; sl < slots; sl += nw) {
            const SegLaneDev L = pl.lanes[sl * 64 + lane];
            if (L.cls >= 0) {
                const double x = lds.cy.d[L.comp];
                if (beats(x, L.comp, fin, fin_at)) {
                    fin = x;
                    fin_at = L.comp;
                }
            }
        }
        block_argmax(fin, fin_at, lds.pairs, wib, lane, nw);
    }
    if (threadIdx.x == 0) {
        if (st == 0 && T > 0 && fin == NINF) st = 1;
        logp[s] = st == 2 ? NINF : fin;
        qlast[s] = fin_at;
        status[s] = st;
    }
}

// grid: 1, block: 64 x min(slots, SEG_MAX_WAVES).  Arguments and the ring: k_hmm_segment_trans_stream's.
template <bool A_LDS, bool LT_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_segment_trans_stream_looped(SegPlanDev pl, const u16* __restrict__ sym, int n,
                                                                                         i64 frame0, const double* __restrict__ ltTg,
                                                                                         const double* d_in, double* d_out,
                                                                                         SegTransRingDev ring, SegStreamState* state)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K, slots = pl.slots;
    const double* lpi = pl.params;
    const double* lAg = lpi + sumN;
    const double* lB = lAg + pl.a_words;
    const int dead = state->status;  // (a symbol >= M in an earlier block: nothing more is decoded)
    const LoopedLds<A_LDS, LT_LDS> lds(smem, pl, lAg, ltTg);
    __syncthreads();  // (also: every wave has read the status before thread 0 may write it)
    if (dead != 0) return;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const i64 row0 = frame0 % ring.rows;  // (n <= ring.rows: the block's rows wrap at most once)
    int st = 0, bad_at = 0;
    if (frame0 > 0)  // d of the frame before the block, each state by its own lane
        for (int sl = wib; sl < slots; sl += nw) {
            const SegLaneDev L = pl.lanes[sl * 64 + lane];
            if (L.cls >= 0) lds.cy.d[L.comp] = d_in[L.comp];
        }
    for (int t0 = 0; t0 < n && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane (every wave holds the same ones)
        const int m = (n - t0) < 64 ? (n - t0) : 64;
        const int mysym = lane < m ? (int)sym[t0 + lane] : 0;
        for (int q = 0; q < m; ++q) {
            const int o = __builtin_amdgcn_readlane(mysym, q);
            const int t = t0 + q;
            if (o >= M) {  // symbol outside the alphabet (workgroup-uniform: no wave reaches a further barrier)
                st = 2;
                bad_at = t;
                break;
            }
            if (frame0 + t == 0) {
                for (int sl = wib; sl < slots; sl += nw) looped_first_turn(pl, sl, lane, o, lpi, lB, lds.cy);
                continue;
            }
            i64 r = row0 + t;
            if (r >= ring.rows) r -= ring.rows;
            const LoopedRows row{ring.psi + (size_t)r * sumN, ring.src + (size_t)r * K, ring.xs + (size_t)r * K, ring.Es + (size_t)r * K};
            // E of a frame lives in the half of its absolute parity
            double* Et = lds.Eb + (size_t)((frame0 + t) & 1) * K;
            for (int sl = wib; sl < slots; sl += nw) looped_exit_turn(pl, sl, lane, lds.lA, lds.cy, Et, row);
            __syncthreads();
            for (int sl = wib; sl < slots; sl += nw) looped_enter_turn(pl, sl, lane, o, lpi, lB, lds.ltT, lds.cy, Et, row);
        }
    }
    if (st == 0)
        for (int sl = wib; sl < slots; sl += nw) {
            const SegLaneDev L = pl.lanes[sl * 64 + lane];
            if (L.cls >= 0) d_out[L.comp] = lds.cy.d[L.comp];
        }
    if (threadIdx.x == 0 && st == 2) {
        state->status = 2;
        state->bad_frame = frame0 + bad_at;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------
// mandatory: the pairs, E of two frames, and d, best (doubles) and arg (int) per composite state; A, then ltT, where they fit
size_t segment_trans_looped_lds_bytes(const SegPlanDev& pl, bool a_lds, bool lt_lds)
{
    return (size_t)SEG_MAX_WAVES * sizeof(Pair) + (size_t)2 * pl.K * 8 + (size_t)pl.sumN * (8 + 8 + 4) +
           (a_lds ? (size_t)pl.a_words * 8 : 0) + (lt_lds ? (size_t)pl.K * pl.K * 8 : 0);
}

void segment_trans_looped_layout(const SegPlanDev& pl, bool* a_lds, bool* lt_lds)
{
    *a_lds = segment_trans_looped_lds_bytes(pl, true, false) <= SEG_LDS_BYTES;
    *lt_lds = segment_trans_looped_lds_bytes(pl, *a_lds, true) <= SEG_LDS_BYTES;
}

#define E2_SEGTL_LAUNCH(KERNEL, A_LDS, LT_LDS, ...)                                                                              \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)KERNEL<A_LDS, LT_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,                  \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((KERNEL<A_LDS, LT_LDS>), grid, block, lds, st, __VA_ARGS__);                                          \
    } while (0)
#define E2_SEGTL_DISPATCH(KERNEL, ...)                                                                                           \
    do {                                                                                                                         \
        if (a_lds) {                                                                                                             \
            if (lt_lds) E2_SEGTL_LAUNCH(KERNEL, true, true, __VA_ARGS__);                                                        \
            else E2_SEGTL_LAUNCH(KERNEL, true, false, __VA_ARGS__);                                                              \
        } else {                                                                                                                 \
            if (lt_lds) E2_SEGTL_LAUNCH(KERNEL, false, true, __VA_ARGS__);                                                       \
            else E2_SEGTL_LAUNCH(KERNEL, false, false, __VA_ARGS__);                                                             \
        }                                                                                                                        \
    } while (0)

int launch_segment_trans_looped(const SegPlanDev& pl, const unsigned short* sym, const i64* offs, int S, i64 psi0, const double* ltT,
                                unsigned short* psi, unsigned short* src, unsigned short* xs, double* Es, double* logp, int* qlast,
                                int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (pl.slots < 1 || segment_trans_looped_lds_bytes(pl, false, false) > SEG_LDS_BYTES) return 1;
    bool a_lds, lt_lds;
    segment_trans_looped_layout(pl, &a_lds, &lt_lds);
    const size_t lds = segment_trans_looped_lds_bytes(pl, a_lds, lt_lds);
    const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
    E2_SEGTL_DISPATCH(k_hmm_segment_trans_looped, pl, sym, offs, psi0, ltT, psi, src, xs, Es, logp, qlast, status);
    return 0;
}

int launch_segment_trans_stream_looped(const SegPlanDev& pl, const unsigned short* sym, int n, i64 frame0, const double* ltT,
                                       const double* d_in, double* d_out, SegTransRingDev ring, SegStreamState* state, hipStream_t st)
{
    if (n < 1) return 0;
    if (pl.slots < 1 || (i64)n > ring.rows || segment_trans_looped_lds_bytes(pl, false, false) > SEG_LDS_BYTES) return 1;
    bool a_lds, lt_lds;
    segment_trans_looped_layout(pl, &a_lds, &lt_lds);
    const size_t lds = segment_trans_looped_lds_bytes(pl, a_lds, lt_lds);
    const int waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    const dim3 grid(1), block((unsigned)(64 * waves));
    E2_SEGTL_DISPATCH(k_hmm_segment_trans_stream_looped, pl, sym, n, frame0, ltT, d_in, d_out, ring, state);
    return 0;
}
#undef E2_SEGTL_DISPATCH
#undef E2_SEGTL_LAUNCH

}  // namespace e2hmm
