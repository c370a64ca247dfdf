// hmm_embed_looped.hip -- the looped body of the embedded E-step (gfx950; `hmm learn --embedded`): the
// forward-backward pass of hmm_embed.hip for a stream whose units take any number of wave-slots.  The contract is the
// resident body's, bit for bit: the same chains in state order, the same global sum (a butterfly over the 64 lanes of each
// slot, then the slots in slot order), the same limbs, log_prob and status.
//   k_hmm_embed_fb_looped      one workgroup per stream, min(slots, 16) waves; wave w owns the slots w, w + nw, w + 2 nw, ..
//                              and a composite state belongs to one lane for the whole stream (k_hmm_align<true, .>'s
//                              hand-out).  What the resident body keeps in a register per state lives in two LDS arrays of
//                              max_sumN doubles: forward ah_{t-1} and x_t / ah_t (the halves alternate), backward W (bh_t,
//                              then u_t, then the row chain's sum, each written by the state's own lane) and P (ah_{t-1},
//                              posted by the lane that stored it).  A unit never straddles a slot, so the chains of a unit
//                              read only what their own wave wrote; the coupling between the units (V forward, R backward)
//                              and the partial sums of the global sum go through LDS behind a barrier, as in the resident
//                              body.  Two barriers a forward step, one a backward step.
// Scratch of a stream, at scr + (its offset - a0) * row_words, in the resident body's layout: ah_t at [t * sumN + composite
// index] and m_t behind it (T * sumN further) by the state's lane, c_t at [2 * T * sumN + t] by thread 0 (the first of the
// resident body's 16 columns); the backward pass loads only what the same lane stored, thread 0 hands c_t out through LDS.
// Where the counts go (exact integer limb sums, so the routes are interchangeable bit for bit): gamma -> BN, BD and PI, and
// m u -> PI by global atomics per frame (a lane serves several states, so no register can hold a state's sum over the
// stream); xi -> AN as in the resident body (the workgroup's LDS table where it fits, else global atomics).
#include "hmm_limbs.h"

namespace e2hmm {

namespace {

// what a wave wrote to LDS is read by other lanes of the same wave: the accesses keep their order
__device__ __forceinline__ void wave_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

}  // namespace

// grid: the streams of the launch, block: 64 x min(the most slots of a stream, 16).
// Dynamic LDS: 2 x max_slots partials | V / R of two consecutive steps, 2 x max_L doubles | the two per-state arrays,
// 2 x max_sumN doubles | A of every class (A_LDS) | the AN limb table, 2 x a_words int64 at the padded positions of A (an_lds).
// pl.params and pl.classes as k_hmm_embed_fb takes them; pl.max_L, max_slots and max_sumN: the largest of the launch's streams.
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_embed_fb_looped(EmbedPlanDev pl, int max_slots, int max_sumN,
                                                                            const u16* __restrict__ sym, const i64* __restrict__ offs,
                                                                            i64 a0, i64 row_words, int an_lds, double* scr,
                                                                            i64* __restrict__ acc, double* __restrict__ mant,
                                                                            i64* __restrict__ exp2, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* parts = (double*)smem;                   // [2][max_slots]
    double* Vb = parts + 2 * (size_t)max_slots;      // [2][max_L]
    double* sa = Vb + 2 * (size_t)pl.max_L;          // [2][max_sumN]
    double* As = sa + 2 * (size_t)max_sumN;
    i64* ANs = (i64*)(As + (A_LDS ? pl.a_words : 0));  // [a_words][hi, lo]
    const int M = pl.M, sumC = pl.sumN_cls;
    const double* pig = pl.params;
    const double* eg = pig + sumC;
    const double* Ag = eg + sumC;
    const double* Bg = Ag + pl.a_words;
    if (A_LDS)
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
    if (an_lds)
        for (int x = threadIdx.x; x < 2 * pl.a_words; x += blockDim.x) ANs[x] = 0;
    __syncthreads();
    const double* A = A_LDS ? As : Ag;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const AlignStreamDev sd = pl.streams[s];
    const int sumN = sd.sumN, slots = sd.slots;
    const AlignLaneDev* lanes = pl.lanes + sd.lane_at;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    double* arow = scr + (size_t)(base - a0) * row_words;  // ah_t of the state c at arow[t * sumN + c]
    double* mrow = arow + (size_t)T * sumN;                 // m_t
    double* crow = mrow + (size_t)T * sumN;                 // c_t at crow[t]
    // (kept in vector registers: the kernel's uniform values would else not all fit the scalar file)
    asm volatile("" : "+v"(arow), "+v"(mrow), "+v"(crow));
    int st = T < 1 ? 1 : 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward: ah_t, m_t and c_t of every frame; the first event in frame order decides the status ---------------
    for (i64 t = 0; t < T; ++t) {
        const int o = (int)sym[base + t];  // (workgroup-uniform)
        if (o >= M) {  // symbol outside the alphabet, before the frame's arithmetic (no wave reaches a further barrier)
            st = 2;
            break;
        }
        const double* ap = sa + (size_t)((t - 1) & 1) * max_sumN;  // ah_{t-1}
        double* xn = sa + (size_t)(t & 1) * max_sumN;              // x_t, then ah_t
        // the mass of step t - 1 lives in Vb[t & 1]: a wave writes that half again at t + 2, past the barriers of t and
        // t + 1, which every wave reaches only after its reads of step t
        double* Vp = Vb + (size_t)(t & 1) * pl.max_L;
        if (t > 0) {
            // every unit's normalised mass Vn = ah_{t-1}[l][0] + ah_{t-1}[l][1] + .. by its state-0 lane
            for (int sl = wib; sl < slots; sl += nw) {
                const AlignLaneDev L = lanes[sl * 64 + lane];
                if (L.unit < 0 || L.j != 0) continue;
                const double* dc = ap + L.comp;
                double Vn = dc[0];
                for (int i = 1; i < L.N; ++i) Vn = Vn + dc[i];
                Vp[L.unit] = Vn;
            }
            __syncthreads();
        }
        double* pt = parts + (size_t)(calls++ & 1) * max_slots;
        for (int sl = wib; sl < slots; sl += nw) {
            const AlignLaneDev L = lanes[sl * 64 + lane];
            double x = 0.0;
            if (L.unit >= 0) {
                const int c = L.comp, N = L.N, l = L.unit, ld = N | 1;
                const double bq = Bg[(size_t)L.row * M + o];
                double m = 0.0;
                if (t == 0) {
                    x = (L.flags & ALIGN_INIT) ? pig[L.row] * bq : 0.0;
                } else {
                    // the in-unit chain over a column of A
                    const double* dc = ap + (c - L.j);
                    const double* Acol = A + pl.classes[pl.row_cls[L.row]].a_at + L.j;  // A[i][j] at Acol[i * ld]
                    double a = dc[0] * Acol[0];
                    for (int i = 1; i < N; ++i) a = a + dc[i] * Acol[i * ld];
                    // the entering mass: from the unit before, and over an optional one
                    if (L.flags & ALIGN_PRED) {
                        double in = Vp[l - 1];
                        if (L.flags & ALIGN_SKIP) in = in + Vp[l - 2];
                        m = in * eg[L.row];
                    }
                    x = (a + m) * bq;  // (unit 0 has no m: + 0.0 leaves the bits of a >= 0)
                }
                xn[c] = x;
                mrow[(size_t)t * sumN + c] = m;
            }
            const double v = slot_sum(x);
            if (lane == 0) pt[sl] = v;
        }
        __syncthreads();
        double ct = pt[0];
        for (int w = 1; w < slots; ++w) ct = ct + pt[w];
        if (!(ct > 0.0)) {  // (the same bits in every lane: workgroup-uniform)
            st = 1;
            break;
        }
        for (int sl = wib; sl < slots; sl += nw) {
            const AlignLaneDev L = lanes[sl * 64 + lane];
            if (L.unit < 0) continue;
            const double ah = xn[L.comp] / ct;
            xn[L.comp] = ah;
            arow[(size_t)t * sumN + L.comp] = ah;
        }
        wave_order();  // (the next step's chains read what the wave's other lanes wrote)
        if (threadIdx.x == 0) crow[t] = ct;
        scale_step(ct, p, E);
    }
    double Z = 0.0;
    if (st == 0) {  // (workgroup-uniform) the mass of the states that may hold the last frame
        const double* af = sa + (size_t)((T - 1) & 1) * max_sumN;
        double* pt = parts + (size_t)(calls++ & 1) * max_slots;
        for (int sl = wib; sl < slots; sl += nw) {
            const AlignLaneDev L = lanes[sl * 64 + lane];
            const double v = slot_sum((L.unit >= 0 && (L.flags & ALIGN_FINAL)) ? af[L.comp] : 0.0);
            if (lane == 0) pt[sl] = v;
        }
        __syncthreads();
        Z = pt[0];
        for (int w = 1; w < slots; ++w) Z = Z + pt[w];
        if (!(Z > 0.0)) st = 1;
        else scale_step(Z, p, E);
    }
    if (threadIdx.x == 0) {
        mant[s] = st == 0 ? p : 0.0;
        exp2[s] = st == 0 ? E : 0;
        status[s] = st;
    }
    // the stream's mark at the classes it names: `used`, or `skipped` (then it adds nothing else)
    for (int sl = wib; sl < slots; sl += nw) {
        const AlignLaneDev L = lanes[sl * 64 + lane];
        if (L.unit < 0 || L.j != 0 || !(L.flags & EMBED_FIRST)) continue;
        const EmbedClassDev cd = pl.classes[pl.row_cls[L.row]];
        i64* counts = acc + cd.acc_at + 2 * ((i64)cd.N + (i64)cd.N * cd.N + cd.N + (i64)cd.N * M + cd.N);
        atomicAdd((u64*)&counts[st == 0 ? 0 : 1], (u64)1);
    }
    if (st != 0) return;  // (workgroup-uniform)

    // ---- backward: bh_t from bh_{t+1}, and the counts of every frame ---------------------------------------------------
    // W[c]: bh_{t+1}'s in-unit part on entry to step t (the successors' R is added then), u_t while the chains run, the row
    // chain's sum on exit.  P[c]: ah_t on entry, ah_{t-1} while the chains run.  c_t comes from thread 0 through cb[t & 1].
    double* W = sa;
    double* P = sa + max_sumN;
    double* cb = parts;
    {
        const double* af = sa + (size_t)((T - 1) & 1) * max_sumN;
        const double zinv = 1.0 / Z;
        for (int sl = wib; sl < slots; sl += nw) {
            const AlignLaneDev L = lanes[sl * 64 + lane];
            if (L.unit < 0) continue;
            const double a_last = af[L.comp];  // (each lane moves its own entry: read before either write)
            P[L.comp] = a_last;
            W[L.comp] = (L.flags & ALIGN_FINAL) ? zinv : 0.0;
        }
        __syncthreads();  // (the partial sums of Z are read: cb may be written)
        if (threadIdx.x == 0 && T > 1) cb[(T - 1) & 1] = crow[T - 1];
        __syncthreads();
    }
    for (i64 t = T - 1; t >= 0; --t) {
        const int o = (int)sym[base + t];
        const double c_nx = (threadIdx.x == 0 && t > 1) ? crow[t - 1] : 0.0;  // requested ahead of the step's chains
        const double ct = t > 0 ? cb[t & 1] : 1.0;
        double* Rt = Vb + (size_t)(t & 1) * pl.max_L;              // (the halves alternate as in the forward pass)
        const double* Rn = Vb + (size_t)((t + 1) & 1) * pl.max_L;  // R of step t + 1
        for (int sl = wib; sl < slots; sl += nw) {
            const AlignLaneDev L = lanes[sl * 64 + lane];
            const bool act = L.unit >= 0;
            const int c = act ? L.comp : 0, N = L.N, l = act ? L.unit : 0, j = L.j, ld = N | 1;
            const EmbedClassDev cd = pl.classes[act ? pl.row_cls[L.row] : 0];
            // the class's accumulators: PI[N] | AN[N][N] | AD[N] | BN[N][M] | BD[N] | used, skipped -- [hi, lo] pairs
            i64* PI = acc + cd.acc_at;
            i64* AN = PI + 2 * cd.N;
            i64* BN = AN + 2 * (i64)cd.N * cd.N + 2 * cd.N;
            i64* BD = BN + 2 * (i64)cd.N * M;
            double u = 0.0, a_prev = 0.0;
            if (act) {
                double bh = W[c];
                if (t < T - 1 && (L.flags & EMBED_SUCC)) {
                    double r = Rn[l + 1];
                    if (L.flags & EMBED_SUCC2) r = r + Rn[l + 2];
                    bh = bh + r;
                }
                const double g = P[c] * bh;
                acc_add(BN + 2 * ((i64)j * M + o), g);
                acc_add(BD + 2 * j, g);
                if (t == 0) acc_add(PI + 2 * j, g);
                if (t > 0) {
                    u = (Bg[(size_t)L.row * M + o] * bh) / ct;
                    if (L.flags & ALIGN_PRED) acc_add(PI + 2 * j, mrow[(size_t)t * sumN + c] * u);  // the expected entries through pi
                    a_prev = arow[(size_t)(t - 1) * sumN + c];
                }
            }
            if (t == 0) continue;  // (workgroup-uniform)
            wave_order();
            if (act) {
                W[c] = u;
                P[c] = a_prev;
            }
            wave_order();
            double a = 0.0;
            if (act) {
                const double* uu = W + (c - j);
                const double* pp = P + (c - j);
                if (j == 0) {  // the unit's entry sum R = e_0 u_0 + e_1 u_1 + .. in state order
                    const double* eu = eg + L.row;
                    double R = eu[0] * uu[0];
                    for (int i = 1; i < N; ++i) R = R + eu[i] * uu[i];
                    Rt[l] = R;
                }
                // the in-unit chain over a row of A, and xi_{t-1}(i, j) = (ah_{t-1}(i) A_ij) u_j for this lane's j
                const double* Arow = A + cd.a_at + (size_t)j * ld;  // A[j][i] at Arow[i]
                const double* Acol = A + cd.a_at + j;               // A[i][j] at Acol[i * ld]
                a = Arow[0] * uu[0];
                for (int i = 1; i < N; ++i) a = a + Arow[i] * uu[i];
                for (int i = 0; i < N; ++i) {
                    const double xi = (pp[i] * Acol[i * ld]) * u;
                    an_add(an_lds != 0, ANs + 2 * (cd.a_at + i * ld + j), AN + 2 * (i * N + j), xi);
                }
            }
            wave_order();
            if (act) W[c] = a;
        }
        if (t == 0) break;
        if (threadIdx.x == 0 && t > 1) cb[(t - 1) & 1] = c_nx;
        __syncthreads();
    }
    // ---- flush: the workgroup's AN table -------------------------------------------------------------------------------
    if (an_lds) {
        __syncthreads();
        for (int k = 0; k < pl.K; ++k) {
            const EmbedClassDev ck = pl.classes[k];
            const int Nk = ck.N, ldk = Nk | 1;
            i64* ANk = acc + ck.acc_at + 2 * Nk;
            for (int x = threadIdx.x; x < 2 * Nk * Nk; x += blockDim.x) {
                const int e = x >> 1, i = e / Nk, j = e - i * Nk;
                const i64 v = ANs[2 * (ck.a_at + i * ldk + j) + (x & 1)];
                if (v != 0) atomicAdd((u64*)&ANk[x], (u64)v);
            }
        }
    }
}

// ---- launcher -----------------------------------------------------------------------------------------------------
// two per-state arrays: the forward pass keeps ah_{t-1} next to x_t / ah_t, the backward pass W next to P; bh, u and the
// row chain's sum take turns in W, so a third array is not needed
size_t embed_looped_lds_bytes(int max_L, int max_slots, int max_sumN, int a_words, bool a_lds, bool an_lds)
{
    return (size_t)2 * max_slots * sizeof(double) + (size_t)2 * max_L * 8 + (size_t)2 * max_sumN * 8 +
           (a_lds ? (size_t)a_words * 8 : 0) + (an_lds ? (size_t)a_words * 16 : 0);
}

int launch_embed_fb_looped(const EmbedPlanDev& pl, bool a_lds, bool an_lds, int max_slots, int max_sumN, const unsigned short* sym,
                           const i64* offs, int S, i64 a0, i64 row_words, double* scr, i64* acc, double* mant, i64* exp2, int* status,
                           hipStream_t st)
{
    if (S < 1) return 0;
    if (max_slots < 1 || max_sumN < 1 || pl.max_L < 1) return 1;
    const int waves = max_slots < SEG_MAX_WAVES ? max_slots : SEG_MAX_WAVES;
    const size_t lds = embed_looped_lds_bytes(pl.max_L, max_slots, max_sumN, pl.a_words, a_lds, an_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_EMBED_LOOPED_LAUNCH(A_LDS)                                                                                            \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_embed_fb_looped<A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,          \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_embed_fb_looped<A_LDS>), grid, block, lds, st, pl, max_slots, max_sumN, sym, offs, a0, row_words, \
                           an_lds ? 1 : 0, scr, acc, mant, exp2, status);                                                        \
    } while (0)
    if (a_lds) E2_EMBED_LOOPED_LAUNCH(true);
    else E2_EMBED_LOOPED_LAUNCH(false);
#undef E2_EMBED_LOOPED_LAUNCH
    return 0;
}

}  // namespace e2hmm
