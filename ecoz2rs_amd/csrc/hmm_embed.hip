// hmm_embed.hip -- HIP kernels (gfx950) of `hmm learn --embedded`: Baum-Welch over whole streams and the
// order of their units, without boundaries.  Unit l of a stream is a copy of the model of class c_l; mass leaves unit l - 1
// (or l - 2 over an optional unit) for unit l through that class's pi at the price sw = exp(ln_switch).  A scaled
// forward-backward in the linear domain runs over this chain, and the expected counts of every unit are added to the exact
// int64 limb accumulators of the unit's CLASS, bit-exact against the restatement.
//   k_hmm_embed_fb             one workgroup per stream, a wave per slot of k_hmm_align's packing (resident only: at most 16
//                              slots).  The in-unit sums are chains in state order (v_readlane where the slot holds one unit,
//                              else ds_bpermute_b32); the forward pass reads a column of A, the backward pass a row.  The
//                              coupling between the units is an LDS array of 2 x L doubles written by each unit's state-0
//                              lane and read after a barrier -- forward the unit's normalised mass of the step before, summed
//                              on the way of the chain (a second barrier next to the one of the global sum c_t; measured
//                              8 to 14 % faster than posting the unnormalised mass with the partial sum),
//                              backward its entry sum R.
//   k_hmm_embed_rowsum         AD[i] = the integer sum of row i of AN, once the streams are done
//   k_hmm_reestimate_embedded  M-step, one thread per parameter, every class in one launch
//   k_hmm_embed_adjustb        the floor at epsilon of every class that was re-estimated
// Nothing transcendental runs here: sw and e = sw * pi come from the host.  Every operation is one IEEE double operation in
// the contract's order (the unit is compiled with -ffp-contract=off).  All terms are >= 0 and idle lanes carry +0.0.
// Scratch of a stream, at scr + (its offset - a0) * row_words: ah_t at [t * sumN + composite index] and m_t behind it
// (T * sumN further) by the state's lane, c_t at [2 * T * sumN + t * slots + wave] by each wave's lane 0; the backward pass
// loads only what the same lane stored, so no visibility between waves is needed.
// Where the counts go (all of them exact integer limb sums, so the routes are interchangeable bit for bit):
//   gamma -> BD, gamma_0 and m u -> PI : per-lane registers over the stream, one global atomic per limb at the end
//   gamma -> BN[j][o_t] : global atomics (N x M words per class: spread out)
//   xi -> AN : a workgroup-wide LDS table over all classes (ds_add_u64), flushed with global atomics at the end; where the
//              table does not fit, global atomics straight away
#include "hmm_limbs.h"

namespace e2hmm {

// grid: the streams of the launch, block: 64 x waves (at least the most slots of a stream).
// Dynamic LDS: 2 x SEG_MAX_WAVES partials | Vn / R of two consecutive steps, 2 x max_L doubles | A of every class (A_LDS) |
// the AN limb table, 2 x a_words int64 at the padded positions of A (an_lds).
// pl.params: pi (sumN_cls) | e = sw * pi (sumN_cls) | A (a_words; class k at classes[k].a_at, leading dimension N_k | 1: odd,
// so that the rows the backward pass reads and the columns the forward pass reads both spread over the LDS banks) | B
// (sumN_cls rows of M).
template <bool A_LDS>
__global__ __launch_bounds__(64 * SEG_MAX_WAVES) void k_hmm_embed_fb(EmbedPlanDev pl, const u16* __restrict__ sym,
                                                                     const i64* __restrict__ offs, i64 a0, i64 row_words, int an_lds,
                                                                     double* scr, i64* __restrict__ acc, double* __restrict__ mant,
                                                                     i64* __restrict__ exp2, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* parts = (double*)smem;             // [2][SEG_MAX_WAVES]
    double* Vb = parts + 2 * SEG_MAX_WAVES;    // [2][max_L]
    double* As = Vb + 2 * (size_t)pl.max_L;
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
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    // a lane without a state (a wave without a slot holds none but these): N = 0, j = 0, row = a_at = ld = 0 (its reads stay
    // in bounds), its values are kept at +0.0
    const bool have = wib < slots;
    AlignLaneDev L = pl.lanes[sd.lane_at + (have ? wib : 0) * 64 + lane];
    if (!have) L = AlignLaneDev{-1, 0, 0, lane, 0, 0, 0, 0};
    const bool act = L.unit >= 0;
    const bool head = act && L.j == 0;  // the lane that posts for its unit
    const int c = act ? L.comp : 0, N = L.N, seg = L.seg, l = act ? L.unit : 0, flags = act ? L.flags : 0;
    const int ld = act ? (N | 1) : 0;
    const EmbedClassDev cd = pl.classes[act ? pl.row_cls[L.row] : 0];
    const int a_at = act ? cd.a_at : 0;
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
    // the class's accumulators: PI[N] | AN[N][N] | AD[N] | BN[N][M] | BD[N] | used, skipped -- [hi, lo] pairs
    i64* PI = acc + cd.acc_at;
    i64* AN = PI + 2 * cd.N;
    i64* BN = AN + 2 * (i64)cd.N * cd.N + 2 * cd.N;
    i64* BD = BN + 2 * (i64)cd.N * M;
    i64* counts = BD + 2 * cd.N;
    const int l1 = l >= 1 ? l - 1 : 0, l2 = l >= 2 ? l - 2 : 0;
    int st = T < 1 ? 1 : 0, calls = 0;
    double p = 0.5;
    i64 E = 1;

    // ---- forward: ah_t, m_t and c_t of every frame; the first event in frame order decides the status ---------------
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
                // (hmm_lane.h's chain_col_mass, written out: with the call this kernel's registers were allocated otherwise --
                // docs/HISTORY.md; a change to that chain is made in both places)
                double a, Vn;
                if (single) {  // the slot holds one unit: wave-uniform reads
                    Vn = bcast(ah, 0);
                    a = Vn * Acol[0];
                    for (int i = 1; i < maxN; ++i) {
                        const double h = bcast(ah, i);
                        a = a + h * Acol[i * ld];
                        Vn = Vn + h;
                    }
                } else {  // units of any N side by side: every lane runs to the slot's largest N, and counts to its own
                    Vn = lane_read(ah, seg);
                    a = Vn * Acol[0];
                    for (int i = 1; i < maxN; ++i) {
                        const int ii = i < N ? i : 0;
                        const double h = lane_read(ah, seg + ii);
                        const double v = h * Acol[ii * ld];
                        if (i < N) {
                            a = a + v;
                            Vn = Vn + h;
                        }
                    }
                }
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
    if (st != 0) {  // (workgroup-uniform) the stream adds nothing but its mark at the classes it names
        if (head && (flags & EMBED_FIRST)) atomicAdd((u64*)&counts[1], (u64)1);
        return;
    }

    // ---- backward: bh_t from bh_{t+1}, and the counts of every frame ---------------------------------------------------
    double bh = (flags & ALIGN_FINAL) ? 1.0 / Z : 0.0;
    double a_cur = ah;  // ah_{T-1}; every earlier one was stored by this very lane
    // what the step t -> t - 1 needs from the scratch: c_t, m_t and ah_{t-1}, requested a step ahead
    double cq = (have && lane == 0 && T > 1) ? crow[(size_t)(T - 1) * slots] : 0.0;
    double mq = (act && T > 1) ? mrow[(size_t)(T - 1) * sumN] : 0.0;
    double a_prev = (act && T > 1) ? arow[(size_t)(T - 2) * sumN] : 0.0;
    i64 bd[2] = {0, 0}, pic[2] = {0, 0};
    for (i64 t0 = ((T - 1) / 64) * 64; t0 >= 0; t0 -= 64) {
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        int o = __builtin_amdgcn_readlane(mysym, n - 1);
        double b = act ? Brow[o] : 0.0;
        for (int q = n - 1; q >= 0; --q) {
            const double bq = b;
            const int oq = o;
            const i64 t = t0 + q;
            const double c_nx = (have && lane == 0 && t > 1) ? crow[(size_t)(t - 1) * slots] : 0.0;
            const double m_nx = (act && t > 1) ? mrow[(size_t)(t - 1) * sumN] : 0.0;
            const double a_nx = (act && t > 1) ? arow[(size_t)(t - 2) * sumN] : 0.0;
            if (q > 0) {
                o = __builtin_amdgcn_readlane(mysym, q - 1);
                b = act ? Brow[o] : 0.0;
            }
            const double g = a_cur * bh;
            if (act) {
                acc_add(BN + 2 * ((i64)L.j * M + oq), g);
                acc_local(bd, g);
                if (t == 0) acc_local(pic, g);
            }
            if (t == 0) break;
            const double ct = bcast(cq, 0);
            const double u = act ? (bq * bh) / ct : 0.0;
            if (flags & ALIGN_PRED) acc_local(pic, mq * u);  // the expected entries through pi
            const double R = chain_sum(ej * u, N, seg, maxN, single);
            double* Rt = Vb + (size_t)(t & 1) * pl.max_L;  // (the halves alternate as in the forward pass)
            if (head) Rt[l] = R;
            // the in-unit chain over a row of A, and xi_{t-1}(i, j) = (ah_{t-1}(i) A_ij) u_j for this lane's j
            double a;
            if (single) {
                a = Arow[0] * bcast(u, 0);
                for (int i = 1; i < maxN; ++i) a = a + Arow[i] * bcast(u, i);
                for (int i = 0; i < maxN; ++i) {
                    const double xi = (bcast(a_prev, i) * Acol[i * ld]) * u;
                    if (act) an_add(an_lds != 0, ANs + 2 * (a_at + i * ld + L.j), AN + 2 * (i * N + L.j), xi);
                }
            } else {
                a = Arow[0] * lane_read(u, seg);
                for (int i = 1; i < maxN; ++i) {
                    const int ii = i < N ? i : 0;
                    const double v = Arow[ii] * lane_read(u, seg + ii);
                    if (i < N) a = a + v;
                }
                for (int i = 0; i < maxN; ++i) {
                    const int ii = i < N ? i : 0;
                    const double xi = (lane_read(a_prev, seg + ii) * Acol[ii * ld]) * u;
                    if (act && i < N) an_add(an_lds != 0, ANs + 2 * (a_at + i * ld + L.j), AN + 2 * (i * N + L.j), xi);
                }
            }
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
    // ---- flush: per-lane sums, the stream's mark at its classes, the workgroup's AN table --------------------------------
    if (act) {
        if (bd[0]) atomicAdd((u64*)&BD[2 * L.j], (u64)bd[0]);
        if (bd[1]) atomicAdd((u64*)&BD[2 * L.j + 1], (u64)bd[1]);
        if (pic[0]) atomicAdd((u64*)&PI[2 * L.j], (u64)pic[0]);
        if (pic[1]) atomicAdd((u64*)&PI[2 * L.j + 1], (u64)pic[1]);
    }
    if (head && (flags & EMBED_FIRST)) atomicAdd((u64*)&counts[0], (u64)1);
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

// grid: (ceil(max N / 64), K).  AD[i] = the sum of row i of AN, both limbs
__global__ void k_hmm_embed_rowsum(const EmbedClassDev* __restrict__ classes, i64* __restrict__ acc)
{
    const EmbedClassDev cd = classes[blockIdx.y];
    const int N = cd.N, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const i64* AN = acc + cd.acc_at + 2 * N + 2 * (i64)i * N;
    i64 hi = 0, lo = 0;
    for (int j = 0; j < N; ++j) {
        hi += AN[2 * j];
        lo += AN[2 * j + 1];
    }
    i64* AD = acc + cd.acc_at + 2 * N + 2 * (i64)N * N;
    AD[2 * i] = hi;
    AD[2 * i + 1] = lo;
}

// M-step, grid: (ceil(max P / 256), K): thread x of class k = parameter x of its dense block pi | A | B at
// params + param_at.  pi is divided by the sum of its own counts (entries through pi, not sequences); each quotient applies
// only where its denominator is > 0, so a class that no transcript names keeps every byte.
__global__ void k_hmm_reestimate_embedded(const EmbedClassDev* __restrict__ classes, int M, const i64* __restrict__ acc,
                                          double* __restrict__ params)
{
    const EmbedClassDev cd = classes[blockIdx.y];
    const int N = cd.N;
    const i64 x = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= (i64)N + (i64)N * N + (i64)N * M) return;
    const i64* PI = acc + cd.acc_at;
    const i64* AN = PI + 2 * N;
    const i64* AD = AN + 2 * (i64)N * N;
    const i64* BN = AD + 2 * N;
    const i64* BD = BN + 2 * (i64)N * M;
    double* pi = params + cd.param_at;
    double* A = pi + N;
    double* B = A + (size_t)N * N;
    if (x < N) {
        i64 hi = 0, lo = 0;
        for (int j = 0; j < N; ++j) {
            hi += PI[2 * j];
            lo += PI[2 * j + 1];
        }
        const double den = e2vq::unfix(hi, lo, ACC_SHIFT);
        if (den > 0.0) pi[x] = e2vq::unfix(PI[2 * x], PI[2 * x + 1], ACC_SHIFT) / den;
    } else if (x < N + (i64)N * N) {
        const i64 e = x - N;
        const int i = (int)(e / N);
        const double den = e2vq::unfix(AD[2 * i], AD[2 * i + 1], ACC_SHIFT);
        if (den > 0.0) A[e] = e2vq::unfix(AN[2 * e], AN[2 * e + 1], ACC_SHIFT) / den;
    } else {
        const i64 e = x - N - (i64)N * N;
        const int j = (int)(e / M);
        const double den = e2vq::unfix(BD[2 * j], BD[2 * j + 1], ACC_SHIFT);
        if (den > 0.0) B[e] = e2vq::unfix(BN[2 * e], BN[2 * e + 1], ACC_SHIFT) / den;
    }
}

// grid: (ceil(max N / 64), K).  hmm_adjustb of every class some status-0 stream names: floor at epsilon, then the row
// divided by its sequential sum (one thread per state; k_hmm_adjustb's row, copied)
__global__ void k_hmm_embed_adjustb(const EmbedClassDev* __restrict__ classes, int M, const i64* __restrict__ acc, double epsilon,
                                    double* __restrict__ params)
{
    const EmbedClassDev cd = classes[blockIdx.y];
    const int N = cd.N, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const i64 used = acc[cd.acc_at + 2 * ((i64)N + (i64)N * N + N + (i64)N * M + N)];
    if (used < 1) return;
    double* row = params + cd.param_at + N + (size_t)N * N + (size_t)j * M;
    double s = 0.0;
    for (int k = 0; k < M; ++k) {
        double v = row[k];
        if (v < epsilon) {
            v = epsilon;
            row[k] = v;
        }
        s = s + v;
    }
    for (int k = 0; k < M; ++k) row[k] = row[k] / s;
}

// ---- launchers ------------------------------------------------------------------------------------------------
size_t embed_lds_bytes(int max_L, int a_words, bool a_lds, bool an_lds)
{
    return (size_t)2 * SEG_MAX_WAVES * sizeof(double) + (size_t)2 * max_L * 8 + (a_lds ? (size_t)a_words * 8 : 0) +
           (an_lds ? (size_t)a_words * 16 : 0);
}

int launch_embed_fb(const EmbedPlanDev& pl, bool a_lds, bool an_lds, int waves, const unsigned short* sym, const i64* offs, int S,
                    i64 a0, i64 row_words, double* scr, i64* acc, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (S < 1) return 0;
    if (waves < 1 || waves > SEG_MAX_WAVES) return 1;
    const size_t lds = embed_lds_bytes(pl.max_L, pl.a_words, a_lds, an_lds);
    if (lds > SEG_LDS_BYTES) return 1;
    const dim3 grid((unsigned)S), block((unsigned)(64 * waves));
#define E2_EMBED_LAUNCH(A_LDS)                                                                                                   \
    do {                                                                                                                         \
        if (lds > 64 * 1024 &&                                                                                                   \
            hipFuncSetAttribute((const void*)k_hmm_embed_fb<A_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,                 \
                                (int)SEG_LDS_BYTES) != hipSuccess)                                                               \
            return 1;                                                                                                            \
        hipLaunchKernelGGL((k_hmm_embed_fb<A_LDS>), grid, block, lds, st, pl, sym, offs, a0, row_words, an_lds ? 1 : 0, scr, acc, \
                           mant, exp2, status);                                                                                  \
    } while (0)
    if (a_lds) E2_EMBED_LAUNCH(true);
    else E2_EMBED_LAUNCH(false);
#undef E2_EMBED_LAUNCH
    return 0;
}

void launch_embed_rowsum(const EmbedClassDev* classes, int K, int max_N, i64* acc, hipStream_t st)
{
    if (K < 1) return;
    hipLaunchKernelGGL(k_hmm_embed_rowsum, dim3((unsigned)((max_N + 63) / 64), (unsigned)K), dim3(64), 0, st, classes, acc);
}

void launch_reestimate_embedded(const EmbedClassDev* classes, int K, int M, i64 max_P, int max_N, const i64* acc, double epsilon,
                                double* params, hipStream_t st)
{
    if (K < 1) return;
    hipLaunchKernelGGL(k_hmm_reestimate_embedded, dim3((unsigned)((max_P + 255) / 256), (unsigned)K), dim3(256), 0, st, classes, M, acc,
                       params);
    if (epsilon > 0.0)
        hipLaunchKernelGGL(k_hmm_embed_adjustb, dim3((unsigned)((max_N + 63) / 64), (unsigned)K), dim3(64), 0, st, classes, M, acc,
                           epsilon, params);
}

}  // namespace e2hmm
