// lpc_device.h -- LPC analysis kernels (lpc_device.hip) as seen by the host driver (lpc_host.cpp).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define E2VQ_LPC_MAX_P 80  // the generic (block per frame) path serves any order up to this one

// Orders with a lane-per-frame instantiation (NC = P + 1): the prefilter's orders of the VQ path (vq_device.h)
#ifndef E2VQ_LPC_NC_LIST
#define E2VQ_LPC_NC_LIST(X) X(13) X(17) X(21) X(25) X(29) X(33) X(37) X(41)
#endif

namespace e2lpc {

// One analysis frame of the signal-batch launch.  The table is laid out in waves of 64 entries; within one wave every
// entry has the same win and h_off (the host pads at each change), so the Hamming table is read with scalar loads.
// start < 0 marks a padding entry: it computes on frame 0 of the batch's samples and writes nothing.
struct Frame {
    int64_t start;  // index of the frame's first sample in the batch's int32 sample buffer
    int32_t win;    // window length in samples
    int32_t h_off;  // offset of the window's Hamming table in the batch's table buffer
};

constexpr int kWave = 64;
// generic path: the windowed frame sits in LDS (doubles)
constexpr int kGenericMaxWin = 7680;

// frames of integer signals: out = (r / pe) row-major nframes x (P + 1) and status per table entry (padding entries
// are left untouched); status 0 / 1 (r0 == 0) / 2 (prediction error <= 0), failed rows are zeros
int launch_signals(int P, const int32_t* samples, const Frame* tab, int64_t n_entries, const double* h, double* out,
                   int32_t* status, hipStream_t stream);
// Levinson on already-windowed frames x (nframes x n, row-major): r, rc, a (nframes x (P + 1)), pe, status
int launch_windowed(int P, const double* x, int n, int64_t nframes, double* r, double* rc, double* a, double* pe,
                    int32_t* status, hipStream_t stream);
// features of stored LPC vectors (lpc_features.hip): frames T x (P + 1) -> status, pe, rc, a (T x (P + 1)), c (T x Q);
// a NULL output is neither computed nor stored (c == NULL: no cepstrum); c[0] = log(sqrt(pe)) from the device log.
int launch_features(int P, int Q, const double* frames, int64_t T, int32_t* status, double* pe, double* rc, double* a,
                    double* c, hipStream_t stream);
// true when order P has a lane-per-frame instantiation (else the generic path runs)
bool lane_path(int P);

}  // namespace e2lpc
