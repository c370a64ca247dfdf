// hmm_segment_stream.h -- device-side interface of the streaming joint Viterbi (hmm_segment_stream.hip):
// the forward pass of one block of an open stream, the coalescence test over the frames that are not final yet, and
// the backtrack of the frames it decides.  Packing, parameters and recursion are launch_segment's (hmm_device.h).
// Internal.
#pragma once
#include "hmm_device.h"

namespace e2hmm {

// The ring of the pending frames: frame f keeps psi at psi[(f % rows) * sumN + composite index] and g at gsel[f % rows].
struct SegRingDev {
    unsigned short* psi;
    int* gsel;
    long long rows;
};

// What a session keeps on the device between its launches (zeroed at open; prev_a = -1).
struct SegStreamState {
    long long fstar;      // the last coalescence: the latest frame all live paths share, -1: none
    long long bad_frame;  // status 2: the absolute frame of the symbol >= M
    double logp;          // close: max d of the last frame
    int a;                // the composite state at fstar
    int prev_a;           // the a of the previous commit (-1: none yet)
    int reached;          // the state the last backtrack reached at F - 1 (-1: F = 0)
    int join_bad;         // 1: `reached` differed from prev_a
    int status;           // 0, or 2 once a symbol >= M was met (every later launch then returns at once), 1 at close: all dead
    int pad;
};

// One block: n symbols from `sym` on, the first at the absolute frame frame0.  d_in / d_out: sumN doubles in composite
// order (d_in is not read at frame0 = 0).  gbest: G of the block's frames, n doubles.  looped: the body that takes any
// number of slots.  Returns 1 when the shape cannot be launched.
int launch_segment_stream(const SegPlanDev& pl, bool looped, const unsigned short* sym, int n, long long frame0, double ln_switch,
                          const double* d_in, double* d_out, SegRingDev ring, double* gbest, SegStreamState* state, hipStream_t st);
// The coalescence of the live paths from frame e back to frame F (the first that is not final), d: d of frame e.  Writes
// state->fstar / a.  close: no walk -- fstar = e, a = the lowest composite index reaching max d; logp and status 1 are set.
void launch_segment_coalesce(const SegPlanDev& pl, const double* d, SegRingDev ring, long long F, long long e, int close,
                             SegStreamState* state, hipStream_t st);
// cls / state / entered of the frames F .. fstar at [frame - F], from (fstar, a); the state reached at F - 1 is compared with
// prev_a, and a becomes prev_a.  Nothing when fstar < F.
void launch_segment_stream_backtrack(const SegPlanDev& pl, SegRingDev ring, long long F, SegStreamState* state, unsigned short* cls,
                                     unsigned short* st_out, unsigned char* entered, hipStream_t st);

}  // namespace e2hmm
