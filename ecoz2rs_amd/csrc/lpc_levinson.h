// lpc_levinson.h -- the Levinson-Durbin recursion of the reference's Rust text in registers, unrolled on NC = P + 1.
// Shared by the analysis kernels (lpc_device.hip) and the feature kernels (lpc_features.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>

namespace e2lpc {

// Levinson-Durbin, lpca_rs.rs:40-72 (= lpca_r_rs.rs:8-43).  rc / a keep zeros where the recursion stopped early.
template <int NC>
__device__ __forceinline__ int levinson(const double (&r)[NC], double (&rc)[NC], double (&a)[NC], double& pe_out)
{
#pragma unroll
    for (int i = 0; i < NC; ++i) rc[i] = a[i] = 0.0;
    pe_out = 0.0;
    if (0.0 == r[0]) return 1;
    double pe = r[0];
    a[0] = 1.0;
#pragma unroll
    for (int k = 1; k < NC; ++k) {
        double sum = 0.0;
#pragma unroll
        for (int i = 1; i <= k; ++i) sum = sum - a[k - i] * r[i];
        const double akk = sum / pe;
        rc[k] = akk;
        a[k] = akk;
#pragma unroll
        for (int i = 1; i <= (k >> 1); ++i) {
            const double ai = a[i], aj = a[k - i];
            a[i] = ai + akk * aj;
            a[k - i] = aj + akk * ai;
        }
        pe = pe * (1.0 - akk * akk);
        if (pe <= 0.0) {
            pe_out = pe;
            return 2;
        }
    }
    pe_out = pe;
    return 0;
}

}  // namespace e2lpc
