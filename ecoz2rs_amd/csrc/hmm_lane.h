// hmm_lane.h -- the lane helpers of every HMM kernel unit, written once: reads of a double from another lane, the scaled
// product P = p * 2^E, the sums over a slot and over a workgroup, and the in-class (in-unit) chains in state order.  The chains
// are the bit-exactness contract of the sum-product kernels: each is the same IEEE operations in the same order as its
// restatement, so a change to that contract is made here and nowhere else.  Every function is a __forceinline__ leaf: a unit
// that includes this header compiles to what it compiled to with copies of its own (docs/HISTORY.md).  Kernel bodies are not
// shared here, and for a reason (the same entry).  Device code only.  Internal.
#pragma once
#include "hmm_device.h"

namespace e2hmm {

typedef long long i64;
typedef unsigned long long u64;
typedef unsigned short u16;

namespace {

// the value of x in lane `lane`, which is wave-uniform: two v_readlane_b32
__device__ __forceinline__ double bcast(double x, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// the value of x in lane `src` (its own for every lane: ds_bpermute_b32, two dwords per double)
__device__ __forceinline__ double lane_read(double x, int src)
{
    const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(x));
    return __hiloint2double(hi, lo);
}

// P = p * 2^E with p in [0.5, 1): one more factor c (frexp is exact; the product rounds once)
__device__ __forceinline__ void scale_step(double c, double& p, i64& E)
{
    int e, e2;
    const double m = frexp(c, &e);
    p = frexp(p * m, &e2);
    E += (i64)e + (i64)e2;
}

// the sum of v over every lane of the workgroup: the same bits in every lane on return.  slot: the nw partials of this
// call's parity -- two calls apart a wave writes the same slot again, and between them lies a barrier every wave passes only
// after its reads (block_argmax's pattern).
__device__ __forceinline__ double block_sum(double v, double* slot, int wib, int lane, int nw)
{
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m);
    if (lane == 0) slot[wib] = v;
    __syncthreads();
    v = slot[0];
    for (int w = 1; w < nw; ++w) v = v + slot[w];
    return v;
}

// the looped bodies' block_sum in two halves.  The slot's part: a butterfly over its 64 lanes (the same bits in every lane)
__device__ __forceinline__ double slot_sum(double v)
{
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

// ... and the whole once every slot has posted: the partials in slot order from slot 0
__device__ __forceinline__ double slots_sum(const double* pt, int slots)
{
    double v = pt[0];
    for (int w = 1; w < slots; ++w) v = v + pt[w];
    return v;
}

// ---- the chains: sums over the states of the lane's class (or unit), in state order.  N: the states of the lane's class,
// seg: its first lane, maxN: the slot's largest N (wave-uniform).  `single`: the slot holds one class, so the reads are
// wave-uniform (v_readlane); else classes of any N_k lie side by side, every lane runs to maxN and counts to its own N.

// sum_j v_j
__device__ __forceinline__ double chain_sum(double v, int N, int seg, int maxN, bool single)
{
    double sum;
    if (single) {
        sum = bcast(v, 0);
        for (int j = 1; j < maxN; ++j) sum = sum + bcast(v, j);
    } else {
        sum = lane_read(v, seg);
        for (int j = 1; j < maxN; ++j) {
            const int jj = j < N ? j : 0;
            const double w = lane_read(v, seg + jj);
            if (j < N) sum = sum + w;
        }
    }
    return sum;
}

// sum_i v_i * Acol[i * ld] (the forward chain: a column of A)
__device__ __forceinline__ double chain_col(double v, const double* Acol, int ld, int N, int seg, int maxN, bool single)
{
    double acc;
    if (single) {
        acc = bcast(v, 0) * Acol[0];
        for (int i = 1; i < maxN; ++i) acc = acc + bcast(v, i) * Acol[i * ld];
    } else {
        acc = lane_read(v, seg) * Acol[0];
        for (int i = 1; i < maxN; ++i) {
            const int ii = i < N ? i : 0;
            const double w = lane_read(v, seg + ii) * Acol[ii * ld];
            if (i < N) acc = acc + w;
        }
    }
    return acc;
}

// what the two chains below return: the chain over A, and the second sum that rides on its reads.  (Returned as a pair, not
// through a reference: with a reference the callers' schedules moved -- docs/HISTORY.md.)
struct ChainPair {
    double acc, sum;
};

// chain_col, and on the way sum = sum_i v_i (the mass of the class): the chain reads every v_i anyway, one add a state
__device__ __forceinline__ ChainPair chain_col_mass(double v, const double* Acol, int ld, int N, int seg, int maxN, bool single)
{
    double acc, S;
    if (single) {
        S = bcast(v, 0);
        acc = S * Acol[0];
        for (int i = 1; i < maxN; ++i) {
            const double vi = bcast(v, i);
            acc = acc + vi * Acol[i * ld];
            S = S + vi;
        }
    } else {
        S = lane_read(v, seg);
        acc = S * Acol[0];
        for (int i = 1; i < maxN; ++i) {
            const int ii = i < N ? i : 0;
            const double vi = lane_read(v, seg + ii);
            const double w = vi * Acol[ii * ld];
            if (i < N) {
                acc = acc + w;
                S = S + vi;
            }
        }
    }
    return ChainPair{acc, S};
}

// sum_j Arow[j] * v_j (the backward chain: a row of A)
__device__ __forceinline__ double chain_row(double v, const double* Arow, int N, int seg, int maxN, bool single)
{
    double acc;
    if (single) {
        acc = Arow[0] * bcast(v, 0);
        for (int j = 1; j < maxN; ++j) acc = acc + Arow[j] * bcast(v, j);
    } else {
        acc = Arow[0] * lane_read(v, seg);
        for (int j = 1; j < maxN; ++j) {
            const int jj = j < N ? j : 0;
            const double w = Arow[jj] * lane_read(v, seg + jj);
            if (j < N) acc = acc + w;
        }
    }
    return acc;
}

// chain_row, and on the way sum = sum_j pik[j] * v_j (what leaves the class through its pi)
__device__ __forceinline__ ChainPair chain_row_pi(double v, const double* Arow, const double* pik, int N, int seg, int maxN,
                                                  bool single)
{
    double acc, R;
    if (single) {
        const double v0 = bcast(v, 0);
        acc = Arow[0] * v0;
        R = pik[0] * v0;
        for (int j = 1; j < maxN; ++j) {
            const double vj = bcast(v, j);
            acc = acc + Arow[j] * vj;
            R = R + pik[j] * vj;
        }
    } else {
        const double v0 = lane_read(v, seg);
        acc = Arow[0] * v0;
        R = pik[0] * v0;
        for (int j = 1; j < maxN; ++j) {
            const int jj = j < N ? j : 0;
            const double vj = lane_read(v, seg + jj);
            const double w = Arow[jj] * vj;
            const double pw = pik[jj] * vj;
            if (j < N) {
                acc = acc + w;
                R = R + pw;
            }
        }
    }
    return ChainPair{acc, R};
}

}  // namespace

}  // namespace e2hmm
