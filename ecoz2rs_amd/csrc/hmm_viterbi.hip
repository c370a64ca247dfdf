// hmm_viterbi.hip -- HIP kernels (gfx950) of HMM decoding: the most likely state sequence Q* of every sequence under
// one model (Viterbi), in the log domain, bit-exact against the restatement of DESIGN.md 4.8.1.
//   k_hmm_viterbi     N <= 64: one wavefront per sequence, lane j = state j (the layout of k_hmm_score)
//   k_hmm_viterbi_wg  65 <= N <= 512: one workgroup per sequence, thread j = state j, d through LDS
//   k_hmm_backtrack   one thread per sequence: q_{T-1}, then q_t = psi_{t+1}[q_{t+1}]
// The model arrives as logarithms taken on the host (lpi, lA, lB; log 0 = -inf): the device adds and compares, nothing
// else.  Per step and state j:  best = d[0] + lA[0][j], arg = 0;  for i = 1 .. N-1: v = d[i] + lA[i][j], v > best ->
// (best, arg) = (v, i);  d'[j] = best + lB[j][o_t], psi_t[j] = arg.  The strict > gives ties to the lowest index.
// psi is written as u16 at psi[(offs[s] - psi0 + t) * N + j] by the forward kernels and read back by the backtrack in
// a launch of its own (the kernel boundary orders the stores before the loads).  PATH = false: no psi, no backtrack.
#include "hmm_lane.h"

namespace e2hmm {

static constexpr int VIT_WAVES = 4;

// grid: ceil(S / VIT_WAVES) workgroups of VIT_WAVES waves, N x N doubles of LDS (lA, row i = from-state).
// Out (index s of this launch): logp, qlast (the lowest state reaching logp; PATH only), status.
template <bool PATH>
__global__ __launch_bounds__(64 * VIT_WAVES) void k_hmm_viterbi(ModelDev md, const u16* __restrict__ sym,
                                                                 const i64* __restrict__ offs, int S, i64 psi0,
                                                                 u16* __restrict__ psi, double* __restrict__ logp,
                                                                 int* __restrict__ qlast, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lAs = (double*)smem;
    const int N = md.N, M = md.M;
    for (int x = threadIdx.x; x < N * N; x += blockDim.x) lAs[x] = md.A[x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int s = blockIdx.x * VIT_WAVES + wib;
    if (s >= S) return;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    const bool act = lane < N;
    const int jj = act ? lane : 0;
    const double lpij = md.pi[jj];
    const double* lBrow = md.B + (size_t)jj * M;
    u16* prow = PATH ? psi + (size_t)(base - psi0) * N + jj : nullptr;
    double d = 0.0;
    int st = 0;
    for (i64 t0 = 0; t0 < T && st == 0; t0 += 64) {
        // this chunk's symbols: one per lane, handed out by readlane
        const int n = (int)((T - t0) < 64 ? (T - t0) : 64);
        const int mysym = lane < n ? (int)sym[base + t0 + lane] : 0;
        int o = __builtin_amdgcn_readlane(mysym, 0);
        double b = o < M ? lBrow[o] : 0.0;
        for (int q = 0; q < n; ++q) {
            const double bq = b;
            const int oq = o;
            if (q + 1 < n) {  // next step's emission is requested before this step's chain runs
                o = __builtin_amdgcn_readlane(mysym, q + 1);
                b = o < M ? lBrow[o] : 0.0;
            }
            if (oq >= M) {  // symbol outside the model's alphabet (wave-uniform)
                st = 2;
                break;
            }
            if (t0 + q == 0) {
                d = lpij + bq;
            } else {
                double best = bcast(d, 0) + lAs[jj];
                int arg = 0;
                for (int i = 1; i < N; ++i) {
                    const double v = bcast(d, i) + lAs[i * N + jj];
                    if (v > best) {
                        best = v;
                        arg = i;
                    }
                }
                d = best + bq;
                if (PATH && act) prow[(size_t)(t0 + q) * N] = (u16)arg;
            }
        }
    }
    // termination: the lowest state reaching max_j d_{T-1}[j]
    double best = T > 0 ? bcast(d, 0) : 0.0;
    int arg = 0;
    if (T > 0)
        for (int j = 1; j < N; ++j) {
            const double v = bcast(d, j);
            if (v > best) {
                best = v;
                arg = j;
            }
        }
    if (lane == 0) {
        if (st == 0 && best == -__builtin_inf()) st = 1;
        logp[s] = st == 2 ? -__builtin_inf() : best;
        if (PATH) qlast[s] = arg;
        status[s] = st;
    }
}

// grid: S workgroups of ceil(N / 64) waves; LDS: d of two consecutive steps (2 x N doubles), one barrier per step.
// lA is read from global memory (column access: consecutive threads, consecutive addresses).
template <bool PATH>
__global__ __launch_bounds__(MAX_N) void k_hmm_viterbi_wg(ModelDev md, const u16* __restrict__ sym,
                                                          const i64* __restrict__ offs, int S, i64 psi0,
                                                          u16* __restrict__ psi, double* __restrict__ logp,
                                                          int* __restrict__ qlast, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = md.N, M = md.M;
    double* ds = (double*)smem;  // [2][N]: step t writes ds[(t & 1) * N + j], reads the other half
    const int s = (int)blockIdx.x;
    const int j = threadIdx.x;
    const bool act = j < N;
    const int jj = act ? j : 0;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    const double* lBrow = md.B + (size_t)jj * M;
    const double* lAcol = md.A + jj;
    u16* prow = PATH ? psi + (size_t)(base - psi0) * N + jj : nullptr;
    int st = 0;
    for (i64 t = 0; t < T; ++t) {
        const int o = (int)sym[base + t];  // (workgroup-uniform)
        if (o >= M) {
            st = 2;
            break;
        }
        const double b = lBrow[o];
        double d;
        if (t == 0) {
            d = md.pi[jj] + b;
        } else {
            const double* dp = ds + ((t - 1) & 1) * N;
            double best = dp[0] + lAcol[0];
            int arg = 0;
            for (int i = 1; i < N; ++i) {
                const double v = dp[i] + lAcol[(size_t)i * N];
                if (v > best) {
                    best = v;
                    arg = i;
                }
            }
            d = best + b;
            if (PATH && act) prow[(size_t)t * N] = (u16)arg;
        }
        // (the half written here was last read in step t - 1, before the barrier that ended it)
        if (act) ds[(t & 1) * N + j] = d;
        __syncthreads();
    }
    if (j == 0) {
        double best = 0.0;
        int arg = 0;
        if (st == 0 && T > 0) {
            const double* dp = ds + ((T - 1) & 1) * N;
            best = dp[0];
            for (int i = 1; i < N; ++i)
                if (dp[i] > best) {
                    best = dp[i];
                    arg = i;
                }
            if (best == -__builtin_inf()) st = 1;
        }
        logp[s] = st == 2 ? -__builtin_inf() : best;
        if (PATH) qlast[s] = arg;
        status[s] = st;
    }
}

// one thread per sequence of the launch; path is indexed by the absolute offsets, psi as the forward kernels wrote it
__global__ void k_hmm_backtrack(int N, const i64* __restrict__ offs, int S, i64 psi0, const u16* __restrict__ psi,
                                const int* __restrict__ qlast, const int* __restrict__ status, u16* __restrict__ path)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const i64 base = offs[s];
    const i64 T = offs[s + 1] - base;
    if (T < 1) return;
    u16* p = path + base;
    if (status[s] == 2) {
        for (i64 t = 0; t < T; ++t) p[t] = 0xFFFF;
        return;
    }
    const u16* ps = psi + (size_t)(base - psi0) * N;
    int q = qlast[s];
    p[T - 1] = (u16)q;
    for (i64 t = T - 2; t >= 0; --t) {
        q = ps[(size_t)(t + 1) * N + q];
        p[t] = (u16)q;
    }
}

void launch_viterbi(const ModelDev& lm, const unsigned short* sym, const i64* offs, int S, i64 psi0, unsigned short* psi,
                    double* logp, int* qlast, int* status, hipStream_t st)
{
    if (S < 1) return;
    if (lm.N > WAVE_N) {
        const dim3 block((unsigned)((lm.N + 63) & ~63));
        const size_t lds = (size_t)2 * lm.N * 8;
        if (psi)
            hipLaunchKernelGGL(k_hmm_viterbi_wg<true>, dim3((unsigned)S), block, lds, st, lm, sym, offs, S, psi0, psi, logp, qlast, status);
        else
            hipLaunchKernelGGL(k_hmm_viterbi_wg<false>, dim3((unsigned)S), block, lds, st, lm, sym, offs, S, psi0, psi, logp, qlast, status);
        return;
    }
    const dim3 grid((unsigned)((S + VIT_WAVES - 1) / VIT_WAVES));
    const size_t lds = (size_t)lm.N * lm.N * 8;
    if (psi)
        hipLaunchKernelGGL(k_hmm_viterbi<true>, grid, dim3(64 * VIT_WAVES), lds, st, lm, sym, offs, S, psi0, psi, logp, qlast, status);
    else
        hipLaunchKernelGGL(k_hmm_viterbi<false>, grid, dim3(64 * VIT_WAVES), lds, st, lm, sym, offs, S, psi0, psi, logp, qlast, status);
}

void launch_backtrack(int N, const i64* offs, int S, i64 psi0, const unsigned short* psi, const int* qlast, const int* status,
                      unsigned short* path, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(k_hmm_backtrack, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, N, offs, S, psi0, psi, qlast, status,
                       path);
}

}  // namespace e2hmm
