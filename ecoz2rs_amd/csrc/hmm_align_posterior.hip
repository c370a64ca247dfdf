// hmm_align_posterior.hip -- HIP kernel (gfx950) of `hmm align --posteriors`: how sure the alignment is.
// The scaled forward-backward of the embedded E-step (hmm_embed.hip, 4.8.11) over the chain of a stream's units, with the same
// operations in the same order -- c_t, Z, ah, bh, u, log_prob and the status are that kernel's bits -- but what it adds into the
// class accumulators is kept here per unit and per frame: the occupancy G_t[l] = the sum over the unit's states of ah bh, the
// entry mass En_t[l] = the sum of m u, and per unit the three sums of En, d En and d d En over the frames (d = t - ref[l]).
//   k_hmm_align_posteriors     one workgroup per stream, a wave per slot of k_hmm_align's packing (resident only: at most 16
//                              slots).  The forward pass is k_hmm_embed_fb's.  The backward pass has no xi, no limb and no
//                              atomic: next to the entry sum R it forms two more in-unit sums in state order (G and En) before
//                              the step's one barrier; the unit's state-0 lane stores G, keeps the three sums in registers over
//                              the whole stream and writes them once.
// Nothing transcendental runs here: sw and e = sw * pi come from the host.  Every operation is one IEEE double operation in
// the contract's order (the unit is compiled with -ffp-contract=off).  All terms are >= 0 and idle lanes carry +0.0.
// Scratch of a stream as in hmm_embed.hip: ah_t at [t * sumN + composite index] and m_t behind it by the state's lane, c_t at
// [2 * T * sumN + t * slots + wave] by each wave's lane 0; the backward pass loads only what the same lane stored, so no
// visibility between waves is needed.  The outputs are zeroed by the host: a stream of status != 0 writes none of them, and a
// frame whose path_unit names no unit keeps its 0.0.
#include "hmm_lane.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x waves (at least the most slots of a stream).
// Dynamic LDS: 2 x SEG_MAX_WAVES partials | Vn / R of two consecutive steps, 2 x max_L doubles | A of every class (A_LDS).
// pl: k_hmm_embed_fb's plan (of classes only a_at is read: no accumulator is addressed); pl.params: pi | e = sw * pi | A
// (leading dimension N_k | 1) | B.
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_align_posteriors(EmbedPlanDev pl, const u16* __restrict__ sym,
                                                                             const i64* __restrict__ offs, i64 a0, i64 row_words,
                                                                             double* scr, AlignPostDev out, double* __restrict__ mant,
                                                                             i64* __restrict__ exp2, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* parts = (double*)smem;             // [2][SEG_MAX_WAVES]
    double* Vb = parts + 2 * SEG_MAX_WAVES;    // [2][max_L]
    double* As = Vb + 2 * (size_t)pl.max_L;
    const int M = pl.M, sumC = pl.sumN_cls;
    const double* pig = pl.params;
    const double* eg = pig + sumC;
    const double* Ag = eg + sumC;
    const double* Bg = Ag + pl.a_words;
    if (A_LDS) {
        for (int x = threadIdx.x; x < pl.a_words; x += blockDim.x) As[x] = Ag[x];
        __syncthreads();
    }
    const double* A = A_LDS ? As : Ag;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int s = (int)blockIdx.x;
    const AlignStreamDev sd = pl.streams[s];
    const int sumN = sd.sumN, slots = sd.slots;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    // a lane without a state (a wave without a slot holds none but these): N = 0, j = 0, row = a_at = ld = 0 (its reads stay
    // in bounds), its values are kept at +0.0
    const bool have = wib < slots;
    AlignLaneDev L = pl.lanes[sd.lane_at + (have ? wib : 0) * 64 + lane];
    if (!have) L = AlignLaneDev{-1, 0, 0, lane, 0, 0, 0, 0};
    const bool act = L.unit >= 0;
    const bool head = act && L.j == 0;  // the lane that posts, stores and sums for its unit
    const int c = act ? L.comp : 0, N = L.N, seg = L.seg, l = act ? L.unit : 0, flags = act ? L.flags : 0;
    const int ld = act ? (N | 1) : 0;
    const int a_at = act ? pl.classes[pl.row_cls[L.row]].a_at : 0;  // (the lane's own a_at counts N x N words: k_hmm_align's)
    const int* slot_info = pl.slot_info + sd.lane_at / 32;
    const int maxN = have ? __builtin_amdgcn_readfirstlane(slot_info[2 * wib]) : 0;
    const bool single = !have || __builtin_amdgcn_readfirstlane(slot_info[2 * wib + 1]) != 0;
    const double pij = act ? pig[L.row] : 0.0;
    const double ej = act ? eg[L.row] : 0.0;
    const double* Brow = Bg + (size_t)L.row * M;
    const double* Acol = A + a_at + L.j;               // A[i][j] at Acol[i * ld]
    const double* Arow = A + a_at + (size_t)L.j * ld;  // A[j][i] at Arow[i]
    double* arow = scr + (size_t)(base - a0) * row_words + c;  // ah_t of this state at arow[t * sumN]
    double* mrow = arow + (size_t)T * sumN;                    // m_t
    double* crow = scr + (size_t)(base - a0) * row_words + (size_t)2 * T * sumN + (have ? wib : 0);  // c_t at crow[t * slots]
    const int l1 = l >= 1 ? l - 1 : 0, l2 = l >= 2 ? l - 2 : 0;
    int st = T < 1 ? 1 : 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward (k_hmm_embed_fb's): ah_t, m_t and c_t of every frame; the first event in frame order decides the status ----
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
            double x, m = 0.0;
            if (t == 0) {
                x = (flags & ALIGN_INIT) ? pij * bq : 0.0;
            } else {
                // the in-unit chain, and on the way the unit's mass Vn = ah_{t-1}[l][0] + ah_{t-1}[l][1] + ..
                const ChainPair cv = chain_col_mass(ah, Acol, ld, N, seg, maxN, single);
                const double a = cv.acc, Vn = cv.sum;
                // the mass of step t - 1 lives in Vb[t & 1]: a wave writes that half again at t + 2, past the barriers of t and
                // t + 1, which every wave reaches only after its reads of step t
                double* Vp = Vb + (size_t)(t & 1) * pl.max_L;
                if (head) Vp[l] = Vn;
                __syncthreads();
                // the entering mass: from the unit before, and over an optional one
                if (flags & ALIGN_PRED) {
                    double in = Vp[l1];
                    if (flags & ALIGN_SKIP) in = in + Vp[l2];
                    m = in * ej;
                }
                x = (a + m) * bq;  // (unit 0 has no m: + 0.0 leaves the bits of a >= 0)
            }
            if (!act) x = 0.0;
            const double ct = block_sum(x, parts + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
            if (!(ct > 0.0)) {  // (the same bits in every lane: workgroup-uniform)
                st = 1;
                break;
            }
            ah = x / ct;
            if (act) {
                arow[(size_t)t * sumN] = ah;
                mrow[(size_t)t * sumN] = m;
            }
            if (have && lane == 0) crow[(size_t)t * slots] = ct;
            scale_step(ct, p, E);
        }
    }
    double Z = 0.0;
    if (st == 0) {  // (workgroup-uniform) the mass of the states that may hold the last frame
        Z = block_sum((flags & ALIGN_FINAL) ? ah : 0.0, parts + (calls++ & 1) * SEG_MAX_WAVES, wib, lane, nw);
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
    double bh = (flags & ALIGN_FINAL) ? 1.0 / Z : 0.0;
    double a_cur = ah;  // ah_{T-1}; every earlier one was stored by this very lane
    // what the step t -> t - 1 needs from the scratch: c_t, m_t and ah_{t-1}, requested a step ahead
    double cq = (have && lane == 0 && T > 1) ? crow[(size_t)(T - 1) * slots] : 0.0;
    double mq = (act && T > 1) ? mrow[(size_t)(T - 1) * sumN] : 0.0;
    double a_prev = (act && T > 1) ? arow[(size_t)(T - 2) * sumN] : 0.0;
    const i64 rf = (head && out.ref) ? out.ref[sd.unit_at + l] : 0;
    double* occ = out.occ ? out.occ + out.occ_at[s] : nullptr;  // G_t[l] at occ[t * L + l]
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    for (i64 t0 = ((T - 1) / 64) * 64; t0 >= 0; t0 -= 64) {
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        // the decoded path's unit of these frames, handed out as the symbols are (0xFFFF: no unit)
        const int mypu = (out.path_unit && lane < n) ? (int)out.path_unit[base + t0 + lane] : 0xFFFF;
        int o = __builtin_amdgcn_readlane(mysym, n - 1);
        double b = act ? Brow[o] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double bq = b;
            const i64 t = t0 + q;
            const double c_nx = (have && lane == 0 && t > 1) ? crow[(size_t)(t - 1) * slots] : 0.0;
            const double m_nx = (act && t > 1) ? mrow[(size_t)(t - 1) * sumN] : 0.0;
            const double a_nx = (act && t > 1) ? arow[(size_t)(t - 2) * sumN] : 0.0;
            if (q > 0) {
                o = __builtin_amdgcn_readlane(mysym, q - 1);
                b = act ? Brow[o] : 0.0;
            }
            const int pu = __builtin_amdgcn_readlane(mypu, q);
            const double g = a_cur * bh;
            const double G = chain_sum(g, N, seg, maxN, single);
            if (head) {
                if (occ) occ[(size_t)t * sd.L + l] = G;
                if (pu == l) out.post_path[base + t] = G;
            }
            double u = 0.0, En = G;  // (En_0 = G_0)
            if (t > 0) {
                const double ct = bcast(cq, 0);
                u = act ? (bq * bh) / ct : 0.0;
                En = chain_sum(mq * u, N, seg, maxN, single);  // the expected entries through pi
                if (!(flags & ALIGN_PRED)) En = 0.0;          // (unit 0 is entered at frame 0 only)
            }
            const double d = (double)(t - rf);
            w0 = w0 + En;
            w1 = w1 + d * En;
            w2 = w2 + (d * d) * En;
            if (t == 0) break;
            const double R = chain_sum(ej * u, N, seg, maxN, single);
            double* Rt = Vb + (size_t)(t & 1) * pl.max_L;  // (the halves alternate as in the forward pass)
            if (head) Rt[l] = R;
            // the in-unit chain over a row of A
            const double a = chain_row(u, Arow, N, seg, maxN, single);
            __syncthreads();
            if (flags & EMBED_SUCC) {
                double r = Rt[l + 1];
                if (flags & EMBED_SUCC2) r = r + Rt[l + 2];
                bh = a + r;
            } else {
                bh = act ? a : 0.0;
            }
            a_cur = a_prev;
            cq = c_nx, mq = m_nx, a_prev = a_nx;
        }
    }
    if (head) {
        out.w[sd.unit_at + l] = w0;
        out.w[out.units + sd.unit_at + l] = w1;
        out.w[2 * out.units + sd.unit_at + l] = w2;
    }
}

// ---- launcher -------------------------------------------------------------------------------------------------------
size_t align_post_lds_bytes(int max_L, int a_words, bool a_lds)
{
    return (size_t)2 * SEG_MAX_WAVES * sizeof(double) + (size_t)2 * max_L * 8 + (a_lds ? (size_t)a_words * 8 : 0);
}

int launch_align_posteriors(const EmbedPlanDev& pl, bool a_lds, int waves, const unsigned short* sym, const i64* offs, int S, i64 a0,
                            i64 row_words, double* scr, const AlignPostDev& out, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (waves < 1 || waves > SEG_MAX_WAVES) return 1;
    const size_t lds = align_post_lds_bytes(pl.max_L, pl.a_words, a_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_ALIGN_POST_LAUNCH(A_LDS)                                                                                                \
    do {                                                                                                                           \
        if (lds > 64 * 1024 &&                                                                                                     \
            hipFuncSetAttribute((const void*)k_hmm_align_posteriors<A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,           \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                                 \
            return 1;                                                                                                              \
        hipLaunchKernelGGL((k_hmm_align_posteriors<A_LDS>), grid, block, lds, st, pl, sym, offs, a0, row_words, scr, out, mant,   \
                           exp2, status);                                                                                          \
    } while (0)
    if (a_lds) E2_ALIGN_POST_LAUNCH(true);
    else E2_ALIGN_POST_LAUNCH(false);
#undef E2_ALIGN_POST_LAUNCH
    return 0;
}

}  // namespace e2hmm
