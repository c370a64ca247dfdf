// hmm_limbs.h -- the limb accumulators of the E-steps (hmm_embed.hip, hmm_embed_looped.hip, hmm_trans_estep.hip, hmm_loop_estep.hip), written once: an expected
// count becomes two int32 limbs by the fix2_mul route (fix2's limbs for every input, by full-rate operations -- vq_fixed.h) and
// is added to int64 cells; a zero limb adds nothing, so no atomic is issued for it.  (hmm_device.hip's acc_add / acc_local are
// other functions: the fix2 route, every limb added.  This header does not reach that unit.)  Device code only.  Internal.
#pragma once
#include "hmm_lane.h"
#include "vq_fixed.h"

namespace e2hmm {

namespace {

constexpr double ACC_SCALE = (double)(1 << ACC_SHIFT);

__device__ __forceinline__ void acc_local(i64 (&cell)[2], double x)
{
    int hi, lo;
    e2vq::fix2_mul(x, ACC_SCALE, hi, lo);
    cell[0] += (i64)hi;
    cell[1] += (i64)lo;
}

__device__ __forceinline__ void acc_add(i64* cell, double x)
{
    int hi, lo;
    e2vq::fix2_mul(x, ACC_SCALE, hi, lo);
    if (hi) atomicAdd((u64*)&cell[0], (u64)(i64)hi);
    if (lo) atomicAdd((u64*)&cell[1], (u64)(i64)lo);
}

// one xi into its AN cell: the workgroup's LDS table (ds_add_u64) or the class's block in global memory
__device__ __forceinline__ void an_add(bool an_lds, i64* lds_cell, i64* g_cell, double x)
{
    int hi, lo;
    e2vq::fix2_mul(x, ACC_SCALE, hi, lo);
    if (an_lds) {
        if (hi) atomicAdd((u64*)&lds_cell[0], (u64)(i64)hi);
        if (lo) atomicAdd((u64*)&lds_cell[1], (u64)(i64)lo);
    } else {
        if (hi) atomicAdd((u64*)&g_cell[0], (u64)(i64)hi);
        if (lo) atomicAdd((u64*)&g_cell[1], (u64)(i64)lo);
    }
}

}  // namespace

}  // namespace e2hmm
