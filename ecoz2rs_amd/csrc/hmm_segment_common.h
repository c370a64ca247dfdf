// hmm_segment_common.h -- device helpers the forward kernels of `hmm segment` share (hmm_segment.hip: a closed stream;
// hmm_segment_stream.hip: one block of an open one) and of `hmm align` (hmm_align.hip) share: the pair a wave posts per step,
// reads of d from another lane, and the workgroup's (value, index) maximum.  Device code only.  Internal.
#pragma once
#include "hmm_device.h"

namespace e2hmm {

typedef long long i64;
typedef unsigned short u16;

namespace {

constexpr u16 ENTER = 0xFFFF;
constexpr int NO_INDEX = 0x7fffffff;

struct Pair {  // what a wave posts per step
    double v;
    int idx, pad;
};

__device__ __forceinline__ double bcast(double x, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double lane_read(double x, int src)
{
    const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(x));
    return __hiloint2double(hi, lo);
}

// greater value, then lower index: a total order on the pairs of distinct indices, so the result does not depend on the tree
__device__ __forceinline__ bool beats(double v2, int i2, double v, int i) { return v2 > v || (v2 == v && i2 < i); }

// the workgroup's maximum of (v, idx): in every lane on return.  slot: the nw pairs of this call's parity -- two calls
// apart a wave writes the same slot again, and between them lies a barrier every wave passes only after its reads.
__device__ __forceinline__ void block_argmax(double& v, int& idx, Pair* slot, int wib, int lane, int nw)
{
    for (int m = 32; m > 0; m >>= 1) {
        const double v2 = __shfl_xor(v, m);
        const int i2 = __shfl_xor(idx, m);
        if (beats(v2, i2, v, idx)) {
            v = v2;
            idx = i2;
        }
    }
    if (lane == 0) {
        slot[wib].v = v;
        slot[wib].idx = idx;
    }
    __syncthreads();
    v = slot[0].v;
    idx = slot[0].idx;
    for (int w = 1; w < nw; ++w) {
        const double v2 = slot[w].v;
        const int i2 = slot[w].idx;
        if (beats(v2, i2, v, idx)) {
            v = v2;
            idx = i2;
        }
    }
}

}  // namespace

}  // namespace e2hmm
