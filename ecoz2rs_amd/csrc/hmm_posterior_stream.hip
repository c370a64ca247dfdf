// hmm_posterior_stream.hip -- HIP kernels (gfx950) of `hmm segment --continuous-posteriors`: the class
// posteriors of hmm_posterior.hip on a stream of unknown length, window by window.  A launch serves one window of one session
// (grid 1): it advances the forward pass from the last forwarded frame to the window's end w, then runs the backward pass from
// w - 1 (bh = 1.0) down to lo, the first frame that was not delivered yet, and stores the posteriors of [lo, emit_hi) -- those of
// the look-ahead frames [emit_hi, w) are computed and dropped.  What is delivered for frame t is row t of the closed pass on
// the prefix o[0 : w), bit for bit: no arithmetic is new, every operation is one IEEE double operation in 4.8.7's order (the
// unit is compiled with -ffp-contract=off), and the two bodies are 4.8.7's with its packing, chains, block_sum, 64-symbol
// hand-out and odd leading dimension of A.
//   k_hmm_loop_posteriors_stream          the resident body: a wave per slot, at most 16 slots.
//   k_hmm_loop_posteriors_stream_looped   the looped body: min(slots, 16) waves, wave w serves the slots w, w + nw, .. in turn.
// What differs from the closed kernels:
//   ring        ah_t, c_t and the symbol of frame t live in row t % rows of PostRingDev (rows = B + L, any value >= 1: the row
//               of a frame is counted up or down with a wrap, and a chunk's 64 symbols are fetched at (row + lane) % rows).
//               As in the closed pass a lane loads only what it stored itself -- in this launch or in an earlier one.
//   start       the forward pass of a launch with f0 > 0 takes ah_{f0-1} from its ring row, read by the lane that owns the
//               state; the t = 0 rule applies at the absolute frame 0 alone.
//   looped end  the looped body keeps x_t in LDS (sv) and forms ah_t = x_t / c_t at the head of the slot's next turn, so after
//               the last frame of a launch ah_{w-1} would exist nowhere.  Behind the forward loop every wave therefore takes one
//               more turn through its slots that only divides sv[c] by c_{w-1} and stores the quotient to the ring -- the same
//               division, by the same lane, that the closed body makes at the head of its backward pass.  The backward pass
//               then reads ah_{w-1} from the ring like every other frame, and so does the next launch's forward start.  (sv is
//               touched by a state's own lane only: no barrier is needed for it.)
//   scaling     the scale_step pair (p, E) is read from and written back to the session's PostStreamState.
//   events      status 2 (a symbol >= M, checked before the frame's arithmetic) and status 1 (!(c_t > 0)) are workgroup-uniform
//               as in 4.8.7; thread 0 records status and frame in the state, no row is written, and every later launch returns
//               after reading the state.
// Scratch in registers only; nothing transcendental runs here.
#include "hmm_lane.h"
#include "hmm_posterior_stream.h"

namespace e2hmm {

namespace {

// row - 1 and row + 1 in a ring of `rows`
__device__ __forceinline__ i64 ring_prev(i64 row, i64 rows) { return row == 0 ? rows - 1 : row - 1; }
__device__ __forceinline__ i64 ring_next(i64 row, i64 rows) { return row + 1 == rows ? 0 : row + 1; }

}  // namespace

// grid: 1, block: 64 x slots.  Dynamic LDS and pl.params: k_hmm_loop_posteriors'.
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_loop_posteriors_stream(SegPlanDev pl, PostRingDev ring, i64 f0, i64 w,
                                                                                   i64 lo, i64 emit_hi, double sw,
                                                                                   double* __restrict__ post, PostStreamState* state)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* parts = (double*)smem;  // [2][SEG_MAX_WAVES]
    double* As = parts + 2 * SEG_MAX_WAVES;
    const int M = pl.M, sumN = pl.sumN, K = pl.K;
    const double* pig = pl.params;
    const double* eg = pig + sumN;
    const double* Ag = eg + sumN;
    const double* Bg = Ag + pl.a_words;
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
    int st = state->status;
    double p = state->p;
    i64 E = state->E;
    __syncthreads();  // (A is in place, and every wave has read the state before thread 0 writes it)
    if (st != 0) return;  // (workgroup-uniform) the session met an event in an earlier launch
    const double* A = A_LDS ? As : Ag;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const i64 rows = ring.rows;
    // a lane without a state: N = 0, j = 0, a_at = 0, ld = 0 (its reads stay in bounds), its values are kept at +0.0
    const SegLaneDev L = pl.lanes[wib * 64 + lane];
    const bool act = L.cls >= 0;
    const int c = act ? L.comp : 0, N = L.N, seg = L.seg, ld = act ? (N | 1) : 0;
    const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib]);
    const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * wib + 1]) != 0;
    const double pij = act ? pig[c] : 0.0;
    const double ej = act ? eg[c] : 0.0;
    const double* Brow = Bg + (size_t)c * M;
    const double* Acol = A + L.a_at + L.j;               // A[i][j] at Acol[i * ld]
    const double* Arow = A + L.a_at + (size_t)L.j * ld;  // A[j][i] at Arow[i]
    double* arow = ring.ah + c;                          // ah_t of this state at arow[(t % rows) * sumN]
    double* crow = ring.c + wib;                         // c_t of this wave at crow[(t % rows) * nw]
    int calls = 0;
    i64 evf = -1;

    // ---- forward: ah_t and c_t of the frames [f0, w); the first event in frame order decides the status --------------
    i64 r = f0 % rows;  // the ring row of the frame at hand
    double ah = (act && f0 > 0) ? arow[(size_t)ring_prev(r, rows) * sumN] : 0.0;
    for (i64 t0 = f0; t0 < w && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane (every wave holds the same ones)
        const int n = (int)((w - t0) < 64 ? (w - t0) : 64);
        const int mysym = lane < n ? (int)ring.sym[(r + lane) % rows] : 0;
        int o = __builtin_amdgcn_readlane(mysym, 0);
        double b = (act && o < M) ? Brow[o] : 0.0;
        for (int q = 0; q < n; ++q) {
            const double bq = b;
            const int oq = o;
            if (q + 1 < n) {  // next step's emission is requested before this step's chain runs
                o = __builtin_amdgcn_readlane(mysym, q + 1);
                b = (act && o < M) ? Brow[o] : 0.0;
            }
            const i64 t = t0 + q;
            if (oq >= M) {  // symbol outside the alphabet (workgroup-uniform: no wave reaches a further barrier)
                st = 2;
                evf = t;
                break;
            }
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
                evf = t;
                break;
            }
            ah = x / ct;
            if (act) arow[(size_t)r * sumN] = ah;
            if (lane == 0) crow[(size_t)r * nw] = ct;
            scale_step(ct, p, E);
            r = ring_next(r, rows);
        }
    }
    if (threadIdx.x == 0) {
        if (st == 0) {
            state->p = p;
            state->E = E;
        } else {
            state->status = st;
            state->frame = evf;
        }
    }
    if (st != 0) return;  // (workgroup-uniform) the launch delivers no row

    // ---- backward: bh_t from bh_{t+1} over [lo, w), and the posterior of every frame below emit_hi ----------------------
    double bh = act ? 1.0 : 0.0;
    for (i64 hi = w; hi > lo; hi -= 64) {
        const i64 t0 = hi - 64 < lo ? lo : hi - 64;
        const int n = (int)(hi - t0);
        const i64 r0 = t0 % rows;
        const int mysym = lane < n ? (int)ring.sym[(r0 + lane) % rows] : 0;
        // what frame t = t0 + q needs: B[j][o_t], c_t (bh_{t-1} from bh_t) and ah_t (the posterior of t)
        i64 rr = (r0 + n - 1) % rows;
        int o = __builtin_amdgcn_readlane(mysym, n - 1);
        double b = act ? Brow[o] : 0.0;
        double a = act ? arow[(size_t)rr * sumN] : 0.0;
        double cv = lane == 0 ? crow[(size_t)rr * nw] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double bq = b, aq = a, cq = cv;
            if (q > 0) {  // the previous frame's loads are requested before this frame's chains run
                rr = ring_prev(rr, rows);
                o = __builtin_amdgcn_readlane(mysym, q - 1);
                b = act ? Brow[o] : 0.0;
                a = act ? arow[(size_t)rr * sumN] : 0.0;
                cv = lane == 0 ? crow[(size_t)rr * nw] : 0.0;
            }
            const i64 t = t0 + q;
            const double g = aq * bh;
            const double sum = chain_sum(g, N, seg, maxN, single);
            if (act && L.j == 0 && t < emit_hi) post[(size_t)(t - lo) * K + L.cls] = sum;
            if (t == lo) break;
            const double ct = bcast(cq, 0);
            const double u = act ? (bq * bh) / ct : 0.0;
            const double R = block_sum(pij * u, parts + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
            const double rs = sw * R;
            const double acc = chain_row(u, Arow, N, seg, maxN, single);
            bh = act ? acc + rs : 0.0;
        }
    }
}

// grid: 1, block: 64 x min(slots, 16).  Dynamic LDS and pl.params: k_hmm_loop_posteriors_looped's.
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_loop_posteriors_stream_looped(SegPlanDev pl, PostRingDev ring, i64 f0,
                                                                                          i64 w, i64 lo, i64 emit_hi, double sw,
                                                                                          double* __restrict__ post,
                                                                                          PostStreamState* state)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int M = pl.M, sumN = pl.sumN, K = pl.K, slots = pl.slots;
    double* parts = (double*)smem;           // [2][slots]
    double* sv = parts + 2 * (size_t)slots;  // [sumN]
    double* As = sv + sumN;
    const double* pig = pl.params;
    const double* eg = pig + sumN;
    const double* Ag = eg + sumN;
    const double* Bg = Ag + pl.a_words;
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
    int st = state->status;
    double p = state->p;
    i64 E = state->E;
    __syncthreads();  // (A is in place, and every wave has read the state before thread 0 writes it)
    if (st != 0) return;  // (workgroup-uniform) the session met an event in an earlier launch
    const double* A = A_LDS ? As : Ag;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const i64 rows = ring.rows;
    double* crow = ring.c + wib;  // c_t of this wave at crow[(t % rows) * nw]
    int calls = 0;
    i64 evf = -1;

    // ---- forward: x_t and c_t of the frames [f0, w); the first event in frame order decides the status ----------------
    double cprev = 1.0;  // c_{t-1}
    i64 r = f0 % rows;   // the ring row of the frame at hand
    for (i64 t0 = f0; t0 < w && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane (every wave holds the same ones)
        const int n = (int)((w - t0) < 64 ? (w - t0) : 64);
        const int mysym = lane < n ? (int)ring.sym[(r + lane) % rows] : 0;
        for (int q = 0; q < n; ++q) {
            const int o = __builtin_amdgcn_readlane(mysym, q);
            const i64 t = t0 + q;
            if (o >= M) {  // symbol outside the alphabet (workgroup-uniform: no wave reaches a further barrier)
                st = 2;
                evf = t;
                break;
            }
            double* pt = parts + (size_t)(calls++ & 1) * slots;
            double* aprev = ring.ah + (size_t)ring_prev(r, rows) * sumN;  // ah_{t-1} of the state c at aprev[c]
            for (int sl = wib; sl < slots; sl += nw) {
                // a lane without a state: N = 0, j = 0, a_at = 0, ld = 0 (its reads stay in bounds), its values are kept at +0.0
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                const bool act = L.cls >= 0;
                const int c = act ? L.comp : 0, N = L.N, ld = act ? (N | 1) : 0;
                const double bq = act ? Bg[(size_t)c * M + o] : 0.0;  // requested before the turn's chain runs
                double x;
                if (t == 0) {
                    x = act ? pig[c] * bq : 0.0;
                } else {
                    const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl]);
                    const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl + 1]) != 0;
                    const double ej = act ? eg[c] : 0.0;
                    double ah;  // ah_{t-1} of this state
                    if (t == f0) {  // (workgroup-uniform) the launch's first frame: what an earlier launch left in the ring
                        ah = act ? aprev[c] : 0.0;
                    } else {
                        ah = act ? sv[c] / cprev : 0.0;
                        if (act) aprev[c] = ah;
                    }
                    const double acc = chain_col(ah, A + L.a_at + L.j, ld, N, L.seg, maxN, single);
                    x = act ? (acc + ej) * bq : 0.0;
                }
                if (act) sv[c] = x;
                const double v = slot_sum(x);
                if (lane == 0) pt[sl] = v;
            }
            __syncthreads();
            const double ct = slots_sum(pt, slots);
            if (!(ct > 0.0)) {  // (the same bits in every lane: workgroup-uniform)
                st = 1;
                evf = t;
                break;
            }
            if (lane == 0) crow[(size_t)r * nw] = ct;
            scale_step(ct, p, E);
            cprev = ct;
            r = ring_next(r, rows);
        }
    }
    if (threadIdx.x == 0) {
        if (st == 0) {
            state->p = p;
            state->E = E;
        } else {
            state->status = st;
            state->frame = evf;
        }
    }
    if (st != 0) return;  // (workgroup-uniform) the launch delivers no row
    if (w > f0) {  // ah_{w-1} is still x_{w-1} in sv: finished and stored before the launch ends (the file header)
        double* alast = ring.ah + (size_t)ring_prev(r, rows) * sumN;
        for (int sl = wib; sl < slots; sl += nw) {
            const SegLaneDev L = pl.lanes[sl * 64 + lane];
            if (L.cls >= 0) alast[L.comp] = sv[L.comp] / cprev;
        }
    }

    // ---- backward: bh_t from u_{t+1} and R_{t+1}, the posterior of frame t below emit_hi, then u_t ------------------------
    double R = 0.0;
    for (i64 hi = w; hi > lo; hi -= 64) {
        const i64 t0 = hi - 64 < lo ? lo : hi - 64;
        const int n = (int)(hi - t0);
        const i64 r0 = t0 % rows;
        const int mysym = lane < n ? (int)ring.sym[(r0 + lane) % rows] : 0;
        i64 rr = (r0 + n - 1) % rows;  // the ring row of the frame at hand
        double cv = lane == 0 ? crow[(size_t)rr * nw] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double cq = cv;
            const double* at = ring.ah + (size_t)rr * sumN;  // ah_t of the state c at at[c]
            if (q > 0) {  // the previous frame's c, a frame ahead
                rr = ring_prev(rr, rows);
                cv = lane == 0 ? crow[(size_t)rr * nw] : 0.0;
            }
            const int o = __builtin_amdgcn_readlane(mysym, q);
            const i64 t = t0 + q;
            const double ct = bcast(cq, 0);
            const double rs = sw * R;
            double* pt = parts + (size_t)(calls++ & 1) * slots;
            for (int sl = wib; sl < slots; sl += nw) {
                const SegLaneDev L = pl.lanes[sl * 64 + lane];
                const bool act = L.cls >= 0;
                const int c = act ? L.comp : 0, N = L.N, ld = act ? (N | 1) : 0;
                const int maxN = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl]);
                const bool single = __builtin_amdgcn_readfirstlane(pl.slot_info[2 * sl + 1]) != 0;
                const double bq = act ? Bg[(size_t)c * M + o] : 0.0;  // requested before the turn's chains run
                const double a = act ? at[c] : 0.0;
                double bh;
                if (t == w - 1) {  // (workgroup-uniform)
                    bh = act ? 1.0 : 0.0;
                } else {
                    const double u1 = act ? sv[c] : 0.0;  // u_{t+1} of this state
                    const double acc = chain_row(u1, A + L.a_at + (size_t)L.j * ld, N, L.seg, maxN, single);
                    bh = act ? acc + rs : 0.0;
                }
                const double sum = chain_sum(a * bh, N, L.seg, maxN, single);
                if (act && L.j == 0 && t < emit_hi) post[(size_t)(t - lo) * K + L.cls] = sum;
                if (t == lo) continue;  // (workgroup-uniform)
                const double u = act ? (bq * bh) / ct : 0.0;
                if (act) sv[c] = u;
                const double pij = act ? pig[c] : 0.0;
                const double v = slot_sum(pij * u);
                if (lane == 0) pt[sl] = v;
            }
            if (t == lo) break;
            __syncthreads();
            R = slots_sum(pt, slots);
        }
    }
}

// ---- launcher ----------------------------------------------------------------------------------------------------------
int launch_loop_posteriors_stream(const SegPlanDev& pl, bool looped, PostRingDev ring, long long f0, long long w, long long lo,
                                  long long emit_hi, double sw, double* post, PostStreamState* state, hipStream_t st)
{
    if (pl.slots < 1 || ring.rows < 1 || lo < 0 || lo >= w || emit_hi <= lo || emit_hi > w || f0 < 0 || f0 > w || w - lo > ring.rows ||
        w - f0 > ring.rows)
        return 1;
    bool a_lds;
    size_t lds;
    int waves;
    if (looped) {
        if (posteriors_looped_lds_bytes(pl, false) > SEG_LDS_BYTES) return 1;
        a_lds = posteriors_looped_lds_bytes(pl, true) <= SEG_LDS_BYTES;
        lds = posteriors_looped_lds_bytes(pl, a_lds);
        waves = pl.slots < SEG_MAX_WAVES ? pl.slots : SEG_MAX_WAVES;
    } else {
        if (pl.slots > SEG_MAX_WAVES) return 1;
        a_lds = posteriors_a_in_lds(pl);
        lds = (size_t)2 * SEG_MAX_WAVES * sizeof(double) + (a_lds ? (size_t)pl.a_words * 8 : 0);
        waves = pl.slots;
    }
    const dim3 grid(1), block((unsigned)(64 * waves));
#define E2_POST_STREAM_LAUNCH(KERNEL)                                                                                            \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEG_LDS_BYTES) != hipSuccess) \
            return 1;                                                                                                            \
        hipLaunchKernelGGL(KERNEL, grid, block, lds, st, pl, ring, f0, w, lo, emit_hi, sw, post, state);                          \
    } while (0)
    if (looped) {
        if (a_lds) E2_POST_STREAM_LAUNCH(k_hmm_loop_posteriors_stream_looped<true>);
        else E2_POST_STREAM_LAUNCH(k_hmm_loop_posteriors_stream_looped<false>);
    } else {
        if (a_lds) E2_POST_STREAM_LAUNCH(k_hmm_loop_posteriors_stream<true>);
        else E2_POST_STREAM_LAUNCH(k_hmm_loop_posteriors_stream<false>);
    }
#undef E2_POST_STREAM_LAUNCH
    return 0;
}

}  // namespace e2hmm
