// hmm_scan.hip -- HIP kernels (gfx950) of `hmm scan`: the scaled forward pass of k_hmm_score over the
// windows of resident symbol streams.
//   k_hmm_scan     a workgroup takes a RUN of consecutive windows of one stream and one model: it stages the model's A and
//                  the span of symbols the run covers ((count - 1) hop + L of them) in LDS once and scores every window of
//                  the run from there -- overlapping windows are never materialised.  G = floor(64 / N) windows share a
//                  wave, lane g N + j = state j of window g (the packing of k_hmm_score_grid; here every segment has the
//                  same model, so a lane holds one column of A); G = 1 is one window per wave with k_hmm_score's
//                  wave-uniform v_readlane sums.
//   k_hmm_scan_wg  more than 64 states: one workgroup per (window, model), thread j = state j (k_hmm_score_wg on the
//                  window table).  Built to work, not to be fast.
//   k_scan_top2    per window the best and the second-best model, ranked as `hmm classify` ranks (ties: the later model
//                  first), so that the host fetches two results per window instead of K.
// Every lane performs k_hmm_score's operations in k_hmm_score's order: each result is, bit for bit, what e2vq_hmm_score
// returns for the window's symbols passed as a sequence of their own.  The step body is a copy of k_hmm_score_grid's, not
// a shared __device__ function: sharing it would move the register allocation of the existing kernels (docs/HISTORY.md).
#include "hmm_lane.h"

namespace e2hmm {

constexpr int SCAN_WAVES = 4;

// grid: (runs, models of this launch).  ks[blockIdx.y] = the model's index k in `models` (all of N states); results at
// [w * K + k].  A run's windows lie in one stream, start in non-decreasing order, and its last window ends last.
// STAGED: the dynamic LDS has room behind A for the longest span among the runs (span_lds symbols); else (a window longer
// than SCAN_SPAN_CAP) the symbols are read from global memory.  (Two instantiations: one body with a run-time choice made
// the compiler read both through flat loads.)
template <bool STAGED>
__global__ __launch_bounds__(64 * SCAN_WAVES) void k_hmm_scan(const ModelDev* __restrict__ models, const int* __restrict__ ks,
                                                               int K, int N, int G, const ScanWin* __restrict__ wins,
                                                               const ScanRun* __restrict__ runs,
                                                               const unsigned short* __restrict__ sym,
                                                               const i64* __restrict__ offs, int span_lds,
                                                               double* __restrict__ mant, i64* __restrict__ exp2,
                                                               int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int GN = G * N;
    double* As = (double*)smem;  // [N][G N]: element (i, lane) at i G N + lane, the same A in every segment
    unsigned short* ls = (unsigned short*)(As + N * GN);
    const int k = ks[blockIdx.y];
    const ModelDev md = models[k];
    const int M = md.M;
    const ScanRun run = runs[blockIdx.x];
    const ScanWin wf = wins[run.w0], wl = wins[run.w0 + run.count - 1];
    const i64 sbase = offs[wf.stream] + wf.first;  // the span's first symbol
    const i64 span = wl.first + wl.len - wf.first;
    for (int x = threadIdx.x; x < N * GN; x += blockDim.x) {
        const int i = x / GN, l = x - i * GN;
        As[x] = md.A[i * N + l % N];
    }
    if (STAGED)
        for (int x = threadIdx.x; x < (int)span && x < span_lds; x += blockDim.x) ls[x] = sym[sbase + x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int g = lane / N;
    const bool seg_ok = g < G;
    const int seg = seg_ok ? g * N : 0, j = seg_ok ? lane - seg : 0;
    const double pij = seg_ok ? md.pi[j] : 0.0;
    const double* Brow = md.B + (size_t)j * M;
    const double* Acol = As + (seg_ok ? lane : 0);
    for (int r0 = wib * G; r0 < run.count; r0 += SCAN_WAVES * G) {  // (wave-uniform)
        const int wi = r0 + g;
        const bool act = seg_ok && wi < run.count;
        const ScanWin w = wins[run.w0 + (act ? wi : r0)];
        const int len = act ? w.len : 0;
        const i64 rel = w.first - wf.first;  // the window's first symbol within the span
        int lmax = len;
        for (int d = 32; d > 0; d >>= 1) lmax = max(lmax, __shfl_xor(lmax, d));
        double al = 0.0, p = 0.5;
        i64 E = 1;
        int st = act ? 0 : 3;  // (3: no window in this segment)
        int o = len > 0 ? (STAGED ? (int)ls[(int)rel] : (int)sym[sbase + rel]) : 0;
        double b = (act && o < M) ? Brow[o] : 0.0;
        for (int t = 0; t < lmax; ++t) {
            const double bq = b;
            const int oq = o;
            if (t + 1 < lmax) {  // next step's emission probability is requested before this step's chain runs
                o = t + 1 < len ? (STAGED ? (int)ls[(int)rel + t + 1] : (int)sym[sbase + rel + t + 1]) : 0;
                b = (act && o < M) ? Brow[o] : 0.0;
            }
            if (st == 0 && t < len && oq >= M) st = 2;  // symbol outside the model's alphabet: this window stops
            double nx;
            if (t == 0) {
                nx = pij * bq;
            } else {
                double acc = 0.0;
                int i = 0;
                if (G == 1)  // one window to the wave: wave-uniform reads, as in k_hmm_score
                    for (; i < N; ++i) acc = fma(bcast(al, i), Acol[i * GN], acc);
                for (; i + 4 <= N; i += 4) {
                    const double x0 = lane_read(al, seg + i), x1 = lane_read(al, seg + i + 1);
                    const double x2 = lane_read(al, seg + i + 2), x3 = lane_read(al, seg + i + 3);
                    const double a0 = Acol[i * GN], a1 = Acol[(i + 1) * GN], a2 = Acol[(i + 2) * GN], a3 = Acol[(i + 3) * GN];
                    acc = fma(x0, a0, acc);
                    acc = fma(x1, a1, acc);
                    acc = fma(x2, a2, acc);
                    acc = fma(x3, a3, acc);
                }
                for (; i < N; ++i) acc = fma(lane_read(al, seg + i), Acol[i * GN], acc);
                nx = acc * bq;
            }
            if (!seg_ok) nx = 0.0;
            double c = 0.0;
            int i = 0;
            if (G == 1)
                for (; i < N; ++i) c = c + bcast(nx, i);
            for (; i + 4 <= N; i += 4) {
                const double x0 = lane_read(nx, seg + i), x1 = lane_read(nx, seg + i + 1);
                const double x2 = lane_read(nx, seg + i + 2), x3 = lane_read(nx, seg + i + 3);
                c = c + x0;
                c = c + x1;
                c = c + x2;
                c = c + x3;
            }
            for (; i < N; ++i) c = c + lane_read(nx, seg + i);
            if (st == 0 && t < len) {
                if (!(c > 0.0)) {
                    st = 1;
                } else {
                    al = nx / c;
                    scale_step(c, p, E);
                }
            }
            if (!__any(st == 0 && t + 1 < len)) break;
        }
        if (act && j == 0) {
            const size_t idx = (size_t)(run.w0 + wi) * K + k;
            mant[idx] = st == 0 ? p : 0.0;
            exp2[idx] = st == 0 ? E : 0;
            status[idx] = st;
        }
    }
}

// grid: (windows of this launch, models of this launch); ks as above; w0: the first window of the launch
__global__ void k_hmm_scan_wg(const ModelDev* __restrict__ models, const int* __restrict__ ks, int K,
                              const ScanWin* __restrict__ wins, int w0, const unsigned short* __restrict__ sym,
                              const i64* __restrict__ offs, double* __restrict__ mant, i64* __restrict__ exp2,
                              int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* als = (double*)smem;
    const int k = ks[blockIdx.y], wi = w0 + (int)blockIdx.x;
    const ModelDev md = models[k];
    const int N = md.N, M = md.M;
    double* nxs = als + N;
    const int j = threadIdx.x;
    const bool act = j < N;
    const int jj = act ? j : 0;
    const ScanWin w = wins[wi];
    const i64 base = offs[w.stream] + w.first;
    const i64 T = w.len;
    double p = 0.5;
    i64 E = 1;
    int st = 0;
    for (i64 t = 0; t < T; ++t) {
        const int o = (int)sym[base + t];
        if (o >= M) {
            st = 2;
            break;
        }
        const double b = md.B[(size_t)jj * M + o];
        double nx;
        if (t == 0) {
            nx = md.pi[jj] * b;
        } else {
            double acc = 0.0;
            for (int i = 0; i < N; ++i) acc = fma(als[i], md.A[(size_t)i * N + jj], acc);
            nx = acc * b;
        }
        if (act) nxs[j] = nx;
        __syncthreads();
        double c = 0.0;
        for (int i = 0; i < N; ++i) c = c + nxs[i];
        if (!(c > 0.0)) {  // (every thread holds the same c)
            st = 1;
            break;
        }
        if (act) als[j] = nx / c;
        __syncthreads();
        scale_step(c, p, E);
    }
    if (j == 0) {
        const size_t idx = (size_t)wi * K + k;
        mant[idx] = st == 0 ? p : 0.0;
        exp2[idx] = st == 0 ? E : 0;
        status[idx] = st;
    }
}

// One thread per window.  P = mant 2^exp2 with mant in [0.5, 1) orders as (exp2, mant); a result whose status is not 0 is
// P = 0.  `hmm classify` sorts ascending and stably and reads the ranking from the end: among equal scores the model
// given later ranks first.  top[2 w], top[2 w + 1] = best, second (-1 when K = 1); tmant / texp: their P (0, 0 for P = 0).
__global__ void k_scan_top2(const double* __restrict__ mant, const i64* __restrict__ exp2, const int* __restrict__ status,
                            i64 W, int K, int* __restrict__ top, double* __restrict__ tmant, i64* __restrict__ texp)
{
    const i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= W) return;
    const double* m = mant + w * K;
    const i64* e = exp2 + w * K;
    const int* s = status + w * K;
    int b1 = -1, b2 = -1;
    double m1 = 0.0, m2 = 0.0;
    i64 e1 = 0, e2 = 0;
    bool v1 = false, v2 = false;
    for (int k = 0; k < K; ++k) {
        const bool v = s[k] == 0;
        const double mk = v ? m[k] : 0.0;
        const i64 ek = v ? e[k] : 0;
        // less(k, x): P_k < P_x
        const bool lt1 = b1 >= 0 && (v ? (v1 && (ek != e1 ? ek < e1 : mk < m1)) : v1);
        if (!lt1) {
            b2 = b1, m2 = m1, e2 = e1, v2 = v1;
            b1 = k, m1 = mk, e1 = ek, v1 = v;
        } else {
            const bool lt2 = b2 >= 0 && (v ? (v2 && (ek != e2 ? ek < e2 : mk < m2)) : v2);
            if (!lt2) b2 = k, m2 = mk, e2 = ek, v2 = v;
        }
    }
    top[2 * w] = b1;
    top[2 * w + 1] = b2;
    tmant[2 * w] = m1;
    tmant[2 * w + 1] = m2;
    texp[2 * w] = e1;
    texp[2 * w + 1] = e2;
}

// ---- launchers ------------------------------------------------------------------------------------------------
int scan_waves() { return SCAN_WAVES; }

// (1: the arguments name no launch this file can make, and nothing was launched)
int launch_scan(const ModelDev* models, const int* ks, int nk, int K, int N, int G, const ScanWin* wins, const ScanRun* runs,
                int nruns, int span_lds, const unsigned short* sym, const i64* offs, double* mant, i64* exp2, int* status,
                hipStream_t st)
{
    if (nruns < 1 || nk < 1 || N < 1 || N > WAVE_N || G < 1 || G * N > WAVE_N || span_lds < 0 || span_lds > SCAN_SPAN_CAP) return 1;
    const size_t lds = (size_t)N * G * N * 8 + (size_t)span_lds * 2;
    // grid.y carries the models: at most 65535 per launch, more in further launches
    for (int k0 = 0; k0 < nk; k0 += 65535) {
        const int kn = nk - k0 < 65535 ? nk - k0 : 65535;
        if (span_lds > 0)
            hipLaunchKernelGGL(k_hmm_scan<true>, dim3((unsigned)nruns, (unsigned)kn), dim3(64 * SCAN_WAVES), lds, st, models, ks + k0, K,
                               N, G, wins, runs, sym, offs, span_lds, mant, exp2, status);
        else
            hipLaunchKernelGGL(k_hmm_scan<false>, dim3((unsigned)nruns, (unsigned)kn), dim3(64 * SCAN_WAVES), lds, st, models, ks + k0, K,
                               N, G, wins, runs, sym, offs, span_lds, mant, exp2, status);
    }
    return 0;
}

int launch_scan_wg(const ModelDev* models, const int* ks, int nk, int K, int maxN, const ScanWin* wins, long long W,
                   const unsigned short* sym, const i64* offs, double* mant, i64* exp2, int* status, hipStream_t st)
{
    if (W < 1 || nk < 1 || maxN < 1 || maxN > MAX_N) return 1;
    for (int k0 = 0; k0 < nk; k0 += 65535) {
        const int kn = nk - k0 < 65535 ? nk - k0 : 65535;
        for (i64 w0 = 0; w0 < W; w0 += 1 << 20) {
            const int wn = (int)(W - w0 < (1 << 20) ? W - w0 : (1 << 20));
            hipLaunchKernelGGL(k_hmm_scan_wg, dim3((unsigned)wn, (unsigned)kn), dim3((unsigned)((maxN + 63) & ~63)),
                               (size_t)2 * maxN * 8, st, models, ks + k0, K, wins, (int)w0, sym, offs, mant, exp2, status);
        }
    }
    return 0;
}

void launch_scan_top2(const double* mant, const i64* exp2, const int* status, long long W, int K, int* top, double* tmant,
                      i64* texp, hipStream_t st)
{
    if (W < 1 || K < 1) return;
    hipLaunchKernelGGL(k_scan_top2, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, mant, exp2, status, W, K, top, tmant, texp);
}

}  // namespace e2hmm
