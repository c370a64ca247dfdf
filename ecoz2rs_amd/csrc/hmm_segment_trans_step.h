// hmm_segment_trans_step.h -- the two halves of a step of the joint Viterbi under class-to-class prices,
// written once: the in-class chain that also yields the class's exit, and the walk over the K sources of a destination class.
// Each is the same IEEE additions and comparisons in the same order as the restatement (`transcribe`), so a change to that
// contract is made here.  hmm_segment_trans_stream.hip and the looped bodies (hmm_segment_trans_looped_step.h) use them; k_hmm_segment_trans (hmm_segment_trans.hip) still carries
// its own copies -- moving it here is a change with a measurement of its own.  Both are __forceinline__ leaves.
// Device code only.  Internal.
#pragma once
#include "hmm_lane.h"

namespace e2hmm {

namespace {

// what the chain returns (a struct, not references: hmm_lane.h's ChainPair says why)
struct ChainExit {
    double best;  // max_i d[i] + lA[i][j], the lowest i wins ties
    double E;     // max_i d[i], the class's exit
    int arg;      // the i of best
    int x;        // the lowest i reaching E
};

// d: the lane's d of the previous frame.  lAcol: lA of the lane's class at column j (row i at lAcol[i * N]).  N: the states of
// the lane's class, seg: its first lane, maxN: the slot's largest N (wave-uniform).  `single`: the slot holds one class, so
// the reads are wave-uniform (v_readlane); else classes of any N_k lie side by side, every lane runs to maxN and counts to N.
__device__ __forceinline__ ChainExit chain_max_exit(double d, const double* lAcol, int N, int seg, int maxN, bool single)
{
    double best, E;
    int arg = 0, x = 0;
    if (single) {
        E = bcast(d, 0);
        best = E + lAcol[0];
        for (int i = 1; i < maxN; ++i) {
            const double di = bcast(d, i);
            const double v = di + lAcol[i * N];
            if (di > E) {
                E = di;
                x = i;
            }
            if (v > best) {
                best = v;
                arg = i;
            }
        }
    } else {
        E = lane_read(d, seg);
        best = E + lAcol[0];
        for (int i = 1; i < maxN; ++i) {
            const int ii = i < N ? i : 0;
            const double di = lane_read(d, seg + ii);
            const double v = di + lAcol[ii * N];
            if (i < N && di > E) {
                E = di;
                x = i;
            }
            if (i < N && v > best) {
                best = v;
                arg = i;
            }
        }
    }
    return ChainExit{best, E, arg, x};
}

struct Source {
    double base;  // max_f E[f] + lt[f][k]
    int from;     // the lowest f reaching it
};

// the cheapest way into class k: Et[f] = E of class f, ltk[f] = lt[f][k] (a row of the transposed prices: consecutive words)
__device__ __forceinline__ Source source_walk(const double* Et, const double* ltk, int K)
{
    double base = Et[0] + ltk[0];
    int from = 0;
    for (int f = 1; f < K; ++f) {
        const double v = Et[f] + ltk[f];
        if (v > base) {
            base = v;
            from = f;
        }
    }
    return Source{base, from};
}

}  // namespace

}  // namespace e2hmm
