// hmm_align_posterior_looped.hip -- the looped body of `hmm align --posteriors` (gfx950): the pass of
// hmm_align_posterior.hip for a stream whose units take any number of wave-slots.  The contract is the resident body's, bit for
// bit: the same chains in state order, the same global sum (a butterfly over the 64 lanes of each slot, then the slots in slot
// order), the same G, En and per-unit sums, log_prob and status.
//   k_hmm_align_posteriors_looped  one workgroup per stream, min(slots, 16) waves; wave w owns the slots w, w + nw, w + 2 nw, ..
//                              and a composite state belongs to one lane for the whole stream (k_hmm_embed_fb_looped's
//                              hand-out).  The forward pass is that kernel's, with its scratch layout.  The backward pass is
//                              that kernel's without xi, limbs and atomics: the two per-state LDS arrays W and P carry bh_t
//                              next to ah_t while the unit's state-0 lane forms G, then u_t next to m_t while it forms En and
//                              R, then the row chain's sum next to ah_{t-1}.  A lane heads several units, so the three sums of
//                              En, d En and d d En cannot stay in registers: they live in three LDS arrays of max_L doubles
//                              that only the unit's state-0 lane reads and writes (no barrier guards them), in descending t
//                              as in the resident body, and go to out.w once after the last step.
//                              Two barriers a forward step, one a backward step.
// Scratch of a stream as in hmm_embed_looped.hip: ah_t at [t * sumN + composite index] and m_t behind it (T * sumN further) by
// the state's lane, c_t at [2 * T * sumN + t] by thread 0; the backward pass loads only what the same lane stored, thread 0
// hands c_t out through LDS.  The outputs are zeroed by the host: a stream of status != 0 writes none of them, and a frame
// whose path_unit names no unit keeps its 0.0.
#include "hmm_lane.h"

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
// 2 x max_sumN doubles | the per-unit sums w0, w1, w2, 3 x max_L doubles | A of every class (A_LDS).
// pl as k_hmm_align_posteriors takes it; pl.max_L, max_slots and max_sumN: the largest of the launch's streams.
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_align_posteriors_looped(EmbedPlanDev pl, int max_slots, int max_sumN,
                                                                                    const u16* __restrict__ sym,
                                                                                    const i64* __restrict__ offs, i64 a0, i64 row_words,
                                                                                    double* scr, AlignPostDev out, double* __restrict__ mant,
                                                                                    i64* __restrict__ exp2, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* parts = (double*)smem;                   // [2][max_slots]
    double* Vb = parts + 2 * (size_t)max_slots;      // [2][max_L]
    double* sa = Vb + 2 * (size_t)pl.max_L;          // [2][max_sumN]
    double* ws = sa + 2 * (size_t)max_sumN;          // [3][max_L]
    double* As = ws + 3 * (size_t)pl.max_L;
    const int M = pl.M, sumC = pl.sumN_cls;
    const double* pig = pl.params;
    const double* eg = pig + sumC;
    const double* Ag = eg + sumC;
    const double* Bg = Ag + pl.a_words;
    // (kept in vector registers: the kernel's uniform values would else not all fit the scalar file)
    asm volatile("" : "+v"(pig), "+v"(eg), "+v"(Bg));
    if (A_LDS) {
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
        __syncthreads();
    }
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
    asm volatile("" : "+v"(arow), "+v"(mrow), "+v"(crow));  // (as pig, eg and Bg above)
    int st = T < 1 ? 1 : 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward (k_hmm_embed_fb_looped's): ah_t, m_t and c_t of every frame; the first event in frame order decides the status
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
        if (t > 0) {  // (workgroup-uniform)
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
        const double ct = slots_sum(pt, slots);
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
        Z = slots_sum(pt, slots);
        if (!(Z > 0.0)) st = 1;
        else scale_step(Z, p, E);
    }
    if (threadIdx.x == 0) {
        mant[s] = st == 0 ? p : 0.0;
        exp2[s] = st == 0 ? E : 0;
        status[s] = st;
    }
    if (st != 0) return;  // (workgroup-uniform) every output of the stream keeps the host's 0.0

    // ---- backward: bh_t from bh_{t+1}; G_t and En_t of every unit, and the unit's three sums over the frames ----------------
    // W[c]: bh_{t+1}'s in-unit part on entry to step t, bh_t (the successors' R added) while G is formed, u_t while En, R and the
    // chains run, the row chain's sum on exit.  P[c]: ah_t on entry and while G is formed, m_t while En is formed, ah_{t-1} on
    // exit.  c_t comes from thread 0 through cb[t & 1].
    double* W = sa;
    double* P = sa + max_sumN;
    double* cb = parts;
    double* w0s = ws;
    double* w1s = ws + pl.max_L;
    double* w2s = ws + 2 * (size_t)pl.max_L;
    {
        const double* af = sa + (size_t)((T - 1) & 1) * max_sumN;
        const double zinv = 1.0 / Z;
        for (int sl = wib; sl < slots; sl += nw) {
            const AlignLaneDev L = lanes[sl * 64 + lane];
            if (L.unit < 0) continue;
            const double a_last = af[L.comp];  // (each lane moves its own entry: read before either write)
            P[L.comp] = a_last;
            W[L.comp] = (L.flags & ALIGN_FINAL) ? zinv : 0.0;
            if (L.j == 0) w0s[L.unit] = 0.0, w1s[L.unit] = 0.0, w2s[L.unit] = 0.0;  // (its head alone touches them)
        }
        __syncthreads();  // (the partial sums of Z are read: cb may be written)
        if (threadIdx.x == 0 && T > 1) cb[(T - 1) & 1] = crow[T - 1];
        __syncthreads();
    }
    double* occ = out.occ ? out.occ + out.occ_at[s] : nullptr;  // G_t[l] at occ[t * L + l]
    double* post = out.post_path + base;
    double* wout = out.w + sd.unit_at;
    const i64* ref = out.ref ? out.ref + sd.unit_at : nullptr;
    const u16* punit = out.path_unit ? out.path_unit + base : nullptr;
    asm volatile("" : "+v"(occ), "+v"(post), "+v"(wout), "+v"(ref), "+v"(punit));  // (as arow, mrow and crow above)
    for (i64 t = T - 1; t >= 0; --t) {
        const int o = (int)sym[base + t];
        const int pu = punit ? (int)punit[t] : 0xFFFF;  // the decoded path's unit (0xFFFF: no unit)
        const double c_nx = (threadIdx.x == 0 && t > 1) ? crow[t - 1] : 0.0;  // requested ahead of the step's chains
        const double ct = t > 0 ? cb[t & 1] : 1.0;
        double* Rt = Vb + (size_t)(t & 1) * pl.max_L;              // (the halves alternate as in the forward pass)
        const double* Rn = Vb + (size_t)((t + 1) & 1) * pl.max_L;  // R of step t + 1
        for (int sl = wib; sl < slots; sl += nw) {
            const AlignLaneDev L = lanes[sl * 64 + lane];
            const bool act = L.unit >= 0;
            const bool head = act && L.j == 0;  // the lane that posts, stores and sums for its unit
            const int c = act ? L.comp : 0, N = L.N, l = act ? L.unit : 0, j = L.j, ld = N | 1;
            const int a_at = act ? pl.classes[pl.row_cls[L.row]].a_at : 0;
            const i64 rf = (head && ref) ? ref[l] : 0;
            double bh = 0.0, u = 0.0, m = 0.0, a_prev = 0.0;
            if (act) {
                bh = W[c];
                if (t < T - 1 && (L.flags & EMBED_SUCC)) {
                    double r = Rn[l + 1];
                    if (L.flags & EMBED_SUCC2) r = r + Rn[l + 2];
                    bh = bh + r;
                }
                if (t > 0) {
                    u = (Bg[(size_t)L.row * M + o] * bh) / ct;
                    m = mrow[(size_t)t * sumN + c];
                    a_prev = arow[(size_t)(t - 1) * sumN + c];
                }
                W[c] = bh;  // (its own entry)
            }
            wave_order();
            double G = 0.0;
            if (head) {  // the occupancy G = ah_0 bh_0 + ah_1 bh_1 + .. in state order
                const double* aa = P + c;
                const double* bb = W + c;
                G = aa[0] * bb[0];
                for (int i = 1; i < N; ++i) G = G + aa[i] * bb[i];
                if (occ) occ[(size_t)t * sd.L + l] = G;
                if (pu == l) post[t] = G;
            }
            if (t == 0) {  // (workgroup-uniform) En_0 = G_0, and nothing is left to carry back
                if (head) {
                    const double d = (double)(t - rf);
                    w0s[l] = w0s[l] + G;
                    w1s[l] = w1s[l] + d * G;
                    w2s[l] = w2s[l] + (d * d) * G;
                }
                continue;
            }
            wave_order();
            if (act) {
                W[c] = u;
                P[c] = m;
            }
            wave_order();
            double a = 0.0;
            if (act) {
                const double* uu = W + (c - j);
                if (j == 0) {
                    // the unit's entry sum R = e_0 u_0 + e_1 u_1 + .. and the expected entries through pi En = m_0 u_0 + m_1 u_1 + ..,
                    // each in state order
                    const double* eu = eg + L.row;
                    const double* mm = P + c;
                    double R = eu[0] * uu[0], En = mm[0] * uu[0];
                    for (int i = 1; i < N; ++i) {
                        R = R + eu[i] * uu[i];
                        En = En + mm[i] * uu[i];
                    }
                    Rt[l] = R;
                    if (!(L.flags & ALIGN_PRED)) En = 0.0;  // (unit 0 is entered at frame 0 only)
                    const double d = (double)(t - rf);
                    w0s[l] = w0s[l] + En;
                    w1s[l] = w1s[l] + d * En;
                    w2s[l] = w2s[l] + (d * d) * En;
                }
                // the in-unit chain over a row of A
                const double* Arow = A + a_at + (size_t)j * ld;  // A[j][i] at Arow[i]
                a = Arow[0] * uu[0];
                for (int i = 1; i < N; ++i) a = a + Arow[i] * uu[i];
            }
            wave_order();
            if (act) {
                W[c] = a;
                P[c] = a_prev;
            }
        }
        if (t == 0) break;  // (workgroup-uniform)
        if (threadIdx.x == 0 && t > 1) cb[(t - 1) & 1] = c_nx;
        __syncthreads();
    }
    // ---- the per-unit sums, each by the lane that formed it ----------------------------------------------------------------
    for (int sl = wib; sl < slots; sl += nw) {
        const AlignLaneDev L = lanes[sl * 64 + lane];
        if (L.unit < 0 || L.j != 0) continue;
        const int l = L.unit;
        wout[l] = w0s[l];
        wout[out.units + l] = w1s[l];
        wout[2 * out.units + l] = w2s[l];
    }
}

// ---- launcher -----------------------------------------------------------------------------------------------------
// the looped E-step's mandatory arrays (the partial sums, V / R, the two per-state arrays) and the three per-unit sums
size_t align_post_looped_lds_bytes(int max_L, int max_slots, int max_sumN, int a_words, bool a_lds)
{
    return embed_looped_lds_bytes(max_L, max_slots, max_sumN, a_words, a_lds, false) + (size_t)3 * max_L * sizeof(double);
}

int launch_align_posteriors_looped(const EmbedPlanDev& pl, bool a_lds, int max_slots, int max_sumN, const unsigned short* sym,
                                   const i64* offs, int S, i64 a0, i64 row_words, double* scr, const AlignPostDev& out, double* mant,
                                   i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (max_slots < 1 || max_sumN < 1 || pl.max_L < 1) return 1;
    const int waves = max_slots < SEG_MAX_WAVES ? max_slots : SEG_MAX_WAVES;
    const size_t lds = align_post_looped_lds_bytes(pl.max_L, max_slots, max_sumN, pl.a_words, a_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_ALIGN_POST_LOOPED_LAUNCH(A_LDS)                                                                                         \
    do {                                                                                                                           \
        if (lds > 64 * 1024 &&                                                                                                     \
            hipFuncSetAttribute((const void*)k_hmm_align_posteriors_looped<A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                                 \
            return 1;                                                                                                              \
        hipLaunchKernelGGL((k_hmm_align_posteriors_looped<A_LDS>), grid, block, lds, st, pl, max_slots, max_sumN, sym, offs, a0,  \
                           row_words, scr, out, mant, exp2, status);                                                               \
    } while (0)
    if (a_lds) E2_ALIGN_POST_LOOPED_LAUNCH(true);
    else E2_ALIGN_POST_LOOPED_LAUNCH(false);
#undef E2_ALIGN_POST_LOOPED_LAUNCH
    return 0;
}

}  // namespace e2hmm
