// hmm_segment_trans_stream.h -- device-side interface of the streaming joint Viterbi under class-to-class prices
// (hmm_segment_trans_stream.hip): hmm_segment_stream.h's three launches with launch_segment_trans's
// recursion and tables.  The session's device state is hmm_segment_stream.h's SegStreamState.  Internal.
#pragma once
#include "hmm_segment_stream.h"

namespace e2hmm {

// The ring of the pending frames: frame f keeps, at row r = f % rows, psi at psi[r * sumN + composite index], src at
// src[r * K + k], x at xs[r * K + f'] and E at Es[r * K + f'] (2 sumN + 12 K bytes a frame).
struct SegTransRingDev {
    unsigned short* psi;
    unsigned short* src;
    unsigned short* xs;
    double* Es;
    long long rows;
};

// One block under the prices ltT (transposed, as launch_segment_trans takes them): n symbols from `sym` on, the first at
// the absolute frame frame0.  d_in / d_out: sumN doubles in composite order (d_in is not read at frame0 = 0).  At most
// SEG_MAX_WAVES slots.  Returns 1 when the shape cannot be launched.
int launch_segment_trans_stream(const SegPlanDev& pl, const unsigned short* sym, int n, long long frame0, const double* ltT,
                                const double* d_in, double* d_out, SegTransRingDev ring, SegStreamState* state, hipStream_t st);
// The looped body of the same block step (hmm_segment_trans_looped.hip; LDS as launch_segment_trans_looped): any number of
// slots, the same d_out and the same ring rows bit for bit
int launch_segment_trans_stream_looped(const SegPlanDev& pl, const unsigned short* sym, int n, long long frame0, const double* ltT,
                                       const double* d_in, double* d_out, SegTransRingDev ring, SegStreamState* state, hipStream_t st);
// launch_segment_coalesce with the back step of the matrix: (k, psi), or on ENTER (src[k], x[src[k]])
void launch_segment_trans_coalesce(const SegPlanDev& pl, const double* d, SegTransRingDev ring, long long F, long long e, int close,
                                   SegStreamState* state, hipStream_t st);
// launch_segment_stream_backtrack, and exit_score of the frames F .. fstar at [frame - F] (0.0 at the absolute frame 0)
void launch_segment_trans_stream_backtrack(const SegPlanDev& pl, SegTransRingDev ring, long long F, SegStreamState* state,
                                           unsigned short* cls, unsigned short* st_out, unsigned char* entered, double* exit_score,
                                           hipStream_t st);

}  // namespace e2hmm
