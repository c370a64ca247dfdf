// lpc_features.hip -- LPC features of stored vectors (`prd show --predictors / -k / --cepstrum`, e2vq_lpc_features):
// the Levinson recursion lpca_r (src/lpc/lpca_r_rs.rs, restated by e2vq_io::lpca_r_host) and Papamichalis' cepstrum
// recursion (src/lpc/lpca_cepstrum_rs.rs) on every row r (P + 1 doubles).  Each step is the IEEE double operation of the
// Rust text in its order (-ffp-contract=off), so every output except c[0] is bit-identical to a sequential restatement;
// c[0] = log(sqrt(pe)) uses the device log here, and the host path replaces it with the C library's.
//
// Lane path (k_feat_lane<NC, STAGE>): one lane per frame, NC = P + 1 from the LPC kernel's lane set.  Levinson runs in
// registers (lpc_levinson.h).  The cepstrum recursion for i > P reads only c[i - P .. i - 1]: those live in a ring of P
// registers, and the loop over i is unrolled by P so that every ring index is static; Q is a runtime value.
// STAGE: a wave's 64 input rows (contiguous in memory) are loaded into LDS with coalesced loads, and its rc / a rows and
// column chunks of c leave through LDS the same way; used up to NC = 37 (kStageMaxNC, measured in DESIGN.md 8.1).
// Generic path (k_feat_generic): one thread per frame, arrays in private memory, any 1 <= P <= 80.
#include "lpc_device.h"
#include "lpc_levinson.h"

#include <utility>

namespace e2lpc {

namespace {

// LDS staging pays up to NC = 37 (2 waves per SIMD); at NC = 41 (286 VGPRs, 1 wave per SIMD) its barriers have nothing
// to overlap with and the direct loads and stores are faster
constexpr int kStageMaxNC = 37;
constexpr int kCW = 16;        // columns of c per LDS chunk (one 128-byte line per row)
constexpr int kCWP = kCW + 1;  // padded row stride of the c chunk in LDS (odd: no bank conflicts)

struct FeatOut {
    int32_t* status;
    double* pe;
    double* rc;
    double* a;
    double* c;
};

// writes the columns of c of a wave's frames [f0, f0 + nv); STAGE collects kCW columns in LDS per store round
template <bool STAGE>
struct CWriter {
    double* c;
    double* tile;  // STAGE: 64 x kCWP doubles
    int64_t f0;
    int nv, lane, Q;
    __device__ __forceinline__ void put(int i, double v)
    {
        if (!STAGE) {
            if (lane < nv) c[(f0 + lane) * Q + i] = v;
            return;
        }
        const int col = i % kCW;
        tile[lane * kCWP + col] = v;
        if (col == kCW - 1 || i == Q - 1) {  // uniform: i and Q are the same for the whole wave
            const int w = col + 1, base = i - col;
            __syncthreads();
            for (int e = lane; e < nv * w; e += kWave) {
                const int row = e / w, cc = e - row * w;
                c[(f0 + row) * Q + base + cc] = tile[row * kCWP + cc];
            }
            __syncthreads();
        }
    }
};

template <class F, int... J>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, J...>)
{
    (f(std::integral_constant<int, J>{}), ...);
}

// one NC-wide output row per lane (rc or a); STAGE: the wave's 64 rows (contiguous) leave LDS with coalesced stores
template <int NC, bool STAGE>
__device__ __forceinline__ void store_rows(double* dst, const double (&v)[NC], double* tile, int64_t f0, int nv, int lane)
{
    if (!dst) return;  // uniform
    if (STAGE) {
#pragma unroll
        for (int i = 0; i < NC; ++i) tile[lane * NC + i] = v[i];
        __syncthreads();
        double* d = dst + f0 * NC;
        for (int e = lane; e < nv * NC; e += kWave) d[e] = tile[e];
        __syncthreads();
    } else if (lane < nv) {
#pragma unroll
        for (int i = 0; i < NC; ++i) dst[(f0 + lane) * NC + i] = v[i];
    }
}

template <int NC, bool STAGE>
__global__ __launch_bounds__(kWave) void k_feat_lane(const double* __restrict__ frames, int64_t T, int Q, FeatOut o)
{
    constexpr int P = NC - 1;
    __shared__ double tile[STAGE ? kWave * (NC > kCWP ? NC : kCWP) : 1];
    const int lane = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * kWave;
    const int64_t f = f0 + lane;
    const int nv = T - f0 < kWave ? (int)(T - f0) : kWave;
    const bool real = lane < nv;

    double r[NC];
    if (STAGE) {
        const double* src = frames + f0 * NC;
        for (int e = lane; e < nv * NC; e += kWave) tile[e] = src[e];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NC; ++i) r[i] = real ? tile[lane * NC + i] : 0.0;
        __syncthreads();
    } else {
#pragma unroll
        for (int i = 0; i < NC; ++i) r[i] = real ? frames[f * NC + i] : 0.0;
    }
    double rc[NC], a[NC], pe;
    const int st = levinson<NC>(r, rc, a, pe);
    if (real && o.status) o.status[f] = st;
    if (real && o.pe) o.pe[f] = pe;
    store_rows<NC, STAGE>(o.rc, rc, tile, f0, nv, lane);
    store_rows<NC, STAGE>(o.a, a, tile, f0, nv, lane);
    if (!o.c) return;

    // cepstrum, lpca_cepstrum_rs.rs: c[0] = ln(sqrt(pe)), c[1] = -a[1], then the two sums; c[j] sits in ring[(j-1) % P]
    CWriter<STAGE> cw{o.c, tile, f0, nv, lane, Q};
    double ring[P];
    cw.put(0, log(sqrt(pe)));
    ring[0] = -a[1];
    cw.put(1, ring[0]);
#pragma unroll
    for (int i = 2; i <= P; ++i) {
        double sum = a[i];
#pragma unroll
        for (int k = 1; k < i; ++k) sum = sum + ((double)(i - k) * ring[i - k - 1]) * a[k];
        ring[i - 1] = -sum / (double)i;
        cw.put(i, ring[i - 1]);
    }
    // unrolled by P through an index sequence (the loop unroller gives up on bodies this large at NC >= 37)
    for (int i0 = P + 1; i0 < Q; i0 += P) {
        static_for([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const int i = i0 + j;
            if (i < Q) {  // uniform
                double sum = 0.0;
#pragma unroll
                for (int k = 1; k <= P; ++k) sum = sum + ((double)(i - k) * ring[(j - k + P) % P]) * a[k];
                ring[j] = -sum / (double)i;  // (i - 1) % P == j: c[i - P] is the last read of this slot
                cw.put(i, ring[j]);
            }
        }, std::make_integer_sequence<int, P>{});
    }
}

// ---- generic path: one thread per frame, any order up to 80 -------------------------------------------------------
constexpr int kRing = 128;  // > E2VQ_LPC_MAX_P, power of two

__global__ __launch_bounds__(kWave) void k_feat_generic(int P, const double* __restrict__ frames, int64_t T, int Q,
                                                        FeatOut o)
{
    const int64_t f = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (f >= T) return;
    const int NC = P + 1;
    const double* r = frames + f * NC;
    double rc[E2VQ_LPC_MAX_P + 1], a[E2VQ_LPC_MAX_P + 1], c[kRing];
    for (int i = 0; i < NC; ++i) rc[i] = a[i] = 0.0;
    double pe = 0.0;
    int st = 0;
    if (0.0 == r[0]) {  // lpca_r_rs.rs:8-43
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
    if (o.status) o.status[f] = st;
    if (o.pe) o.pe[f] = pe;
    for (int i = 0; i < NC; ++i) {
        if (o.rc) o.rc[f * NC + i] = rc[i];
        if (o.a) o.a[f * NC + i] = a[i];
    }
    if (!o.c) return;
    double* cf = o.c + f * Q;
    cf[0] = log(sqrt(pe));
    c[1] = -a[1];
    cf[1] = c[1];
    for (int i = 2; i < Q; ++i) {
        double sum = i <= P ? a[i] : 0.0;
        const int kend = i <= P ? i - 1 : P;
        for (int k = 1; k <= kend; ++k) sum = sum + ((double)(i - k) * c[(i - k) & (kRing - 1)]) * a[k];
        c[i & (kRing - 1)] = -sum / (double)i;
        cf[i] = c[i & (kRing - 1)];
    }
}

unsigned wave_blocks(int64_t n) { return (unsigned)((n + kWave - 1) / kWave); }

}  // namespace

int launch_features(int P, int Q, const double* frames, int64_t T, int32_t* status, double* pe, double* rc, double* a,
                    double* c, hipStream_t stream)
{
    if (T <= 0) return 0;
    const FeatOut o{status, pe, rc, a, c};
    switch (P + 1) {
#define E2LPC_CASE(nc)                                                                                                 \
    case nc:                                                                                                          \
        hipLaunchKernelGGL((k_feat_lane<nc, (nc <= kStageMaxNC)>), dim3(wave_blocks(T)), dim3(kWave), 0, stream,       \
                           frames, T, Q, o);                                                                           \
        return hipGetLastError() == hipSuccess ? 0 : 1;
        E2VQ_LPC_NC_LIST(E2LPC_CASE)
#undef E2LPC_CASE
        default:
            hipLaunchKernelGGL(k_feat_generic, dim3(wave_blocks(T)), dim3(kWave), 0, stream, P, frames, T, Q, o);
            return hipGetLastError() == hipSuccess ? 0 : 1;
    }
}

}  // namespace e2lpc
