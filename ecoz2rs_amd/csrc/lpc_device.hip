// lpc_device.hip -- LPC analysis of signal frames (`ecoz2 lpc`), the arithmetic of the reference's Rust text:
// frame pipeline src/lpc/lpc_rs.rs:104-160 (mean removal, pre-emphasis, Hamming), lpca1 src/lpc/lpca_rs.rs:28-75
// (autocorrelation + Levinson-Durbin) and the gain normalisation of lpc_rs.rs:126-131.  Every operation is the IEEE
// double operation of that text, in its order (the build has -ffp-contract=off: no FMA is formed), so the frames are
// bit-identical to a sequential restatement.
//
// Lane-per-frame path (k_lpc_lane<NC, MODE>): one lane owns one frame.  The autocorrelation is streamed over the later
// sample index n: at step n every lag i <= n adds w[n - i] * w[n], which visits k = n - i in increasing order -- the
// sequential sum of lpca1 -- and each lag ends by itself at n = win - 1.  The last NC windowed samples live in a ring
// of VGPRs; the loop is unrolled by NC so every ring index is static.  Only the first NC steps need a per-lag
// predicate, and it is static there (i <= j).  Levinson then runs in registers, unrolled on NC.
// Generic path (k_lpc_block<MODE>): one block per frame, the windowed frame in LDS, one thread per lag, any P <= 80.
#include "lpc_device.h"
#include "lpc_levinson.h"

namespace e2lpc {

namespace {

enum { kSignal = 0, kWindowed = 1 };

// The windowed sample at n of a signal frame: x = s[n] - mean, pre-emphasis y = x[n] - 0.95 x[n-1] (computed from
// the mean-removed value of n - 1, which the reference's downward loop has not yet overwritten), then y * h[n].
struct SignalSrc {
    const int32_t* s;
    const double* h;
    double mean;
    double prev;  // s[n - 1] - mean
    template <bool FIRST>
    __device__ __forceinline__ double next(int n)
    {
        const double x = (double)s[n] - mean;
        const double y = FIRST ? x : x - 0.95 * prev;
        prev = x;
        return y * h[n];
    }
};

struct WindowedSrc {
    const double* x;
    template <bool FIRST>
    __device__ __forceinline__ double next(int n)
    {
        return x[n];
    }
};

// autocorrelation r[i] = sum_{k=0}^{win-1-i} w[k] w[k+i], sequential in k (lpca_rs.rs:31-38)
template <int NC, class Src>
__device__ __forceinline__ void autocorrelation(Src& src, int win, double (&r)[NC])
{
    double ring[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) r[i] = 0.0;
    // first NC samples: lag i exists from n = i on
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (j < win) {
            const double w = j == 0 ? src.template next<true>(j) : src.template next<false>(j);
            ring[j] = w;
#pragma unroll
            for (int i = 0; i <= j; ++i) r[i] = r[i] + ring[j - i] * w;
        }
    }
    int n0 = NC;
    for (; n0 + NC <= win; n0 += NC) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double w = src.template next<false>(n0 + j);
            ring[j] = w;
#pragma unroll
            for (int i = 0; i < NC; ++i) r[i] = r[i] + ring[(j - i + NC) % NC] * w;
        }
    }
    // tail: fewer than NC samples left (win is uniform across the wave: a scalar branch per step)
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (n0 + j < win) {
            const double w = src.template next<false>(n0 + j);
            ring[j] = w;
#pragma unroll
            for (int i = 0; i < NC; ++i) r[i] = r[i] + ring[(j - i + NC) % NC] * w;
        }
    }
}

template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_lpc_lane(const int32_t* __restrict__ samples, const Frame* __restrict__ tab,
                                                  const double* __restrict__ h, const double* __restrict__ xw, int xn,
                                                  int64_t nframes, double* __restrict__ out, double* __restrict__ rc_out,
                                                  double* __restrict__ a_out, double* __restrict__ pe_out,
                                                  int32_t* __restrict__ status)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t wave0 = f - (threadIdx.x & (kWave - 1));
    if (wave0 >= nframes) return;  // whole wave past the end (uniform)
    const bool real_frame = f < nframes && (MODE == kWindowed || tab[f].start >= 0);
    double r[NC];
    if (MODE == kSignal) {
        // win and h_off are the same for the whole wave (host contract): read them once as scalars
        const int win = __builtin_amdgcn_readfirstlane(tab[wave0].win);
        const int h_off = __builtin_amdgcn_readfirstlane(tab[wave0].h_off);
        const int64_t start = real_frame ? tab[f].start : 0;
        const int32_t* s = samples + start;
        double sum = 0.0;  // sequential sum left to right (lpc_rs.rs:146-153)
        for (int n = 0; n < win; ++n) sum = sum + (double)s[n];
        SignalSrc src{s, h + h_off, sum / (double)win, 0.0};
        autocorrelation<NC>(src, win, r);
    } else {
        WindowedSrc src{xw + (real_frame ? f : 0) * (int64_t)xn};
        autocorrelation<NC>(src, xn, r);
    }
    double rc[NC], a[NC], pe;
    const int st = levinson<NC>(r, rc, a, pe);
    if (!real_frame) return;
    status[f] = st;
    double* o = out + f * NC;
    if (MODE == kSignal) {
        // gain normalisation, lpc_rs.rs:126-131 (status 0 implies pe > 0); failed frames are zero rows
#pragma unroll
        for (int i = 0; i < NC; ++i) o[i] = st == 0 ? r[i] / pe : 0.0;
    } else {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            o[i] = r[i];
            rc_out[f * NC + i] = rc[i];
            a_out[f * NC + i] = a[i];
        }
        pe_out[f] = pe;
    }
}

// ---- generic path: one 128-thread block per frame ----------------------------------------------------------------
constexpr int kBlock = 128;

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_lpc_block(int P, const int32_t* __restrict__ samples,
                                                      const Frame* __restrict__ tab, const double* __restrict__ h,
                                                      const double* __restrict__ xw, int xn, int64_t nframes,
                                                      double* __restrict__ out, double* __restrict__ rc_out,
                                                      double* __restrict__ a_out, double* __restrict__ pe_out,
                                                      int32_t* __restrict__ status)
{
    __shared__ double w[kGenericMaxWin];
    __shared__ double r[E2VQ_LPC_MAX_P + 1], rc[E2VQ_LPC_MAX_P + 1], a[E2VQ_LPC_MAX_P + 1];
    __shared__ double mean_s, pe_s;
    __shared__ int st_s;
    const int NC = P + 1;
    const int tid = threadIdx.x;
    for (int64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
        int win;
        if (MODE == kSignal) {
            const Frame fr = tab[f];
            if (fr.start < 0) continue;  // padding entry (uniform across the block)
            win = fr.win;
            const int32_t* s = samples + fr.start;
            const double* hh = h + fr.h_off;
            if (tid == 0) {
                double sum = 0.0;
                for (int n = 0; n < win; ++n) sum = sum + (double)s[n];
                mean_s = sum / (double)win;
            }
            __syncthreads();
            const double mean = mean_s;
            for (int n = tid; n < win; n += kBlock) {
                const double x = (double)s[n] - mean;
                const double y = n == 0 ? x : x - 0.95 * ((double)s[n - 1] - mean);
                w[n] = y * hh[n];
            }
        } else {
            win = xn;
            for (int n = tid; n < win; n += kBlock) w[n] = xw[f * (int64_t)xn + n];
        }
        __syncthreads();
        for (int i = tid; i < NC; i += kBlock) {
            double sum = 0.0;
            for (int k = 0; k < win - i; ++k) sum = sum + w[k] * w[k + i];
            r[i] = sum;
            rc[i] = 0.0;
            a[i] = 0.0;
        }
        __syncthreads();
        if (tid == 0) {  // Levinson-Durbin, lpca_rs.rs:40-72
            int st = 0;
            double pe = 0.0;
            if (0.0 == r[0]) {
                st = 1;
            } else {
                pe = r[0];
                a[0] = 1.0;
                for (int k = 1; k <= P; ++k) {
                    double sum = 0.0;
                    for (int i = 1; i <= k; ++i) sum = sum - a[k - i] * r[i];
                    const double akk = sum / pe;
                    rc[k] = akk;
                    a[k] = akk;
                    for (int i = 1; i <= (k >> 1); ++i) {
                        const double ai = a[i], aj = a[k - i];
                        a[i] = ai + akk * aj;
                        a[k - i] = aj + akk * ai;
                    }
                    pe = pe * (1.0 - akk * akk);
                    if (pe <= 0.0) {
                        st = 2;
                        break;
                    }
                }
            }
            st_s = st;
            pe_s = pe;
            status[f] = st;
            if (MODE == kWindowed) pe_out[f] = pe;
        }
        __syncthreads();
        const int st = st_s;
        const double pe = pe_s;
        for (int i = tid; i < NC; i += kBlock) {
            if (MODE == kSignal) {
                out[f * NC + i] = st == 0 ? r[i] / pe : 0.0;
            } else {
                out[f * NC + i] = r[i];
                rc_out[f * NC + i] = rc[i];
                a_out[f * NC + i] = a[i];
            }
        }
        __syncthreads();  // LDS is reused by the next frame
    }
}

unsigned lane_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
unsigned block_grid(int64_t n) { return (unsigned)(n < 65536 ? n : 65536); }

}  // namespace

bool lane_path(int P)
{
#define E2LPC_HAS(nc) || (P + 1 == nc)
    return false E2VQ_LPC_NC_LIST(E2LPC_HAS);
#undef E2LPC_HAS
}

int launch_signals(int P, const int32_t* samples, const Frame* tab, int64_t n_entries, const double* h, double* out,
                   int32_t* status, hipStream_t stream)
{
    if (n_entries <= 0) return 0;
    switch (P + 1) {
#define E2LPC_CASE(nc)                                                                                                 \
    case nc:                                                                                                          \
        hipLaunchKernelGGL((k_lpc_lane<nc, kSignal>), dim3(lane_blocks(n_entries)), dim3(256), 0, stream, samples, tab, \
                           h, nullptr, 0, n_entries, out, nullptr, nullptr, nullptr, status);                          \
        return hipGetLastError() == hipSuccess ? 0 : 1;
        E2VQ_LPC_NC_LIST(E2LPC_CASE)
#undef E2LPC_CASE
        default:
            hipLaunchKernelGGL((k_lpc_block<kSignal>), dim3(block_grid(n_entries)), dim3(kBlock), 0, stream, P, samples,
                               tab, h, nullptr, 0, n_entries, out, nullptr, nullptr, nullptr, status);
            return hipGetLastError() == hipSuccess ? 0 : 1;
    }
}

int launch_windowed(int P, const double* x, int n, int64_t nframes, double* r, double* rc, double* a, double* pe,
                    int32_t* status, hipStream_t stream)
{
    if (nframes <= 0) return 0;
    switch (P + 1) {
#define E2LPC_CASE(nc)                                                                                                 \
    case nc:                                                                                                          \
        hipLaunchKernelGGL((k_lpc_lane<nc, kWindowed>), dim3(lane_blocks(nframes)), dim3(256), 0, stream, nullptr,     \
                           nullptr, nullptr, x, n, nframes, r, rc, a, pe, status);                                     \
        return hipGetLastError() == hipSuccess ? 0 : 1;
        E2VQ_LPC_NC_LIST(E2LPC_CASE)
#undef E2LPC_CASE
        default:
            hipLaunchKernelGGL((k_lpc_block<kWindowed>), dim3(block_grid(nframes)), dim3(kBlock), 0, stream, P, nullptr,
                               nullptr, nullptr, x, n, nframes, r, rc, a, pe, status);
            return hipGetLastError() == hipSuccess ? 0 : 1;
    }
}

}  // namespace e2lpc
