// hmm_posterior_stream.h -- device-side interface of the streamed class posteriors (hmm_posterior_stream.hip, DESIGN.md
// 4.8.17): one window of one open stream per launch -- the forward pass advanced to the window's end, then a backward pass
// from there down to the first frame that was not delivered yet.  Packing, parameter block and arithmetic are
// launch_loop_posteriors' (hmm_device.h).  Internal.
#pragma once
#include "hmm_device.h"

namespace e2hmm {

// The ring of the last `rows` frames: frame t keeps ah_t at ah[(t % rows) * sumN + composite index], c_t at
// c[(t % rows) * waves + wave] (a copy per wave of the workgroup) and its symbol at sym[t % rows].
struct PostRingDev {
    double* ah;
    double* c;
    unsigned short* sym;
    long long rows;
};

// What a session keeps on the device between its launches (at open: p = 0.5, E = 1, status = 0, frame = -1).
struct PostStreamState {
    double p;         // P(the frames forwarded so far) = p 2^E, p in [0.5, 1)
    long long E;
    long long frame;  // status != 0: the absolute frame of the event
    int status;       // 0; 1: !(c_t > 0) at `frame`; 2: a symbol >= M at `frame`.  Every later launch returns at once
    int pad;
};

// One window.  The forward pass runs over the frames [f0, w) (f0: the frames forwarded so far; their symbols and, for
// f0 > 0, ah of frame f0 - 1 are in the ring), the backward pass from w - 1 (bh = 1.0) down to lo, and the posteriors of
// the frames [lo, emit_hi) go to post[(t - lo) * K + class].  0 <= lo < w, lo < emit_hi <= w, f0 <= w, w - lo <= ring.rows
// and w - f0 <= ring.rows.  looped: the body that takes any number of slots.  An event (status) of the forward pass is
// recorded in *state and no row is written.  Returns 1 when the shape cannot be launched.
int launch_loop_posteriors_stream(const SegPlanDev& pl, bool looped, PostRingDev ring, long long f0, long long w, long long lo,
                                  long long emit_hi, double sw, double* post, PostStreamState* state, hipStream_t st);

}  // namespace e2hmm
