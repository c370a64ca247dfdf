// hmm_segment_common.h -- what the max-sum decoders share on the device (hmm_segment.hip: a closed stream;
// hmm_segment_stream.hip: one block of an open one; hmm_segment_trans.hip: class-to-class prices; hmm_align.hip: a known class
// order): the marks of the psi tables, the pair a wave posts per step, and the workgroup's (value, index) maximum.  Reads of d
// from another lane are hmm_lane.h's.  Device code only.  Internal.
#pragma once
#include "hmm_lane.h"

namespace e2hmm {

namespace {

constexpr u16 ENTER = 0xFFFF;
constexpr int NO_INDEX = 0x7fffffff;

struct Pair {  // what a wave posts per step
    double v;
    int idx, pad;
};

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
