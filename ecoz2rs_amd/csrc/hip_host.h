// hip_host.h -- the host-side HIP plumbing of the entry points (vq_entry.cpp, vq_host.cpp, the hmm_*.cpp units, lpc_host.cpp):
// error check, device check, handles that release themselves, and the fan-out over worker threads.  Host code only.
// Internal.
#pragma once
#include "../../include/ecoz2_vq.h"
#include "vq_io.h"

#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <thread>
#include <utility>
#include <vector>

// errors: the message of the calling thread (e2vq_last_error); e2vq_set_error (vq_io.h) returns 1
char* e2vq_err_buf();  // 1024 bytes, thread-local
int e2vq_env_int(const char* name, int dflt);  // vq_entry.cpp

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return e2vq_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

namespace e2hip {

// the number of HIP devices; 0 (with the error set) when there is none
inline int device_count()
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        e2vq_set_error("no HIP device available (%s); this library has no CPU path",
                       e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return 0;
    }
    return n;
}

// `device` exists and is the calling thread's current device
inline int require_device(int device)
{
    const int n = device_count();
    if (n == 0) return 1;
    if (device < 0 || device >= n) return e2vq_set_error("device %d not in [0, %d)", device, n);
    HIPCHK(hipSetDevice(device));
    return 0;
}

// ECOZ2_VQ_DEVICE: the device of a single-device call, the first device of a sharded one
inline int env_device() { return e2vq_env_int("ECOZ2_VQ_DEVICE", 0); }
// ECOZ2_VQ_GPUS = N: sequences, predictor files or classes are dealt in contiguous shares to N workers, worker w on device
// (ECOZ2_VQ_DEVICE + w) % device count -- workers beyond the device count share devices, which is how the 1-GPU tests run
inline int env_workers()
{
    const int n = e2vq_env_int("ECOZ2_VQ_GPUS", 1);
    return n < 1 ? 1 : (n > 64 ? 64 : n);
}

// worker w of a sharded call runs on device (dev0 + w) % ndev: workers beyond the device count share devices
inline int worker_device(int dev0, int w, int ndev) { return (dev0 + w) % ndev; }

// part i of `parts` contiguous shares of [0, total), the first total % parts of them one longer
inline void split_range(long long total, int parts, int i, long long* lo, long long* hi)
{
    const long long base = total / parts, rem = total % parts;
    *lo = i * base + std::min<long long>(i, rem);
    *hi = *lo + base + (i < rem ? 1 : 0);
}

// runs fn(w) for w = 0 .. n - 1, worker 0 on the calling thread; the message of the lowest-numbered failing worker
// becomes the calling thread's
template <typename Fn>
int run_workers(int n, Fn fn)
{
    std::vector<int> rcs((size_t)n, 0);
    std::vector<std::string> errs((size_t)n);
    std::vector<std::thread> th;
    auto body = [&](int w) {
        rcs[(size_t)w] = fn(w);
        if (rcs[(size_t)w]) errs[(size_t)w] = e2vq_last_error();
    };
    for (int w = 1; w < n; ++w) th.emplace_back(body, w);
    body(0);
    for (auto& t : th) t.join();
    for (int w = 0; w < n; ++w)
        if (rcs[(size_t)w]) {
            if (w > 0) snprintf(e2vq_err_buf(), 1024, "%s", errs[(size_t)w].c_str());
            return rcs[(size_t)w];
        }
    return 0;
}

// Room for `count` T's, on the device (DeviceBuffer) or pinned on the host (PinnedBuffer), freed on destruction.
// reserve() only ever grows the buffer (without keeping its contents) and allocates at least one element.
template <typename T, bool Pinned>
class HipBuffer {
  public:
    HipBuffer() = default;
    HipBuffer(HipBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    HipBuffer& operator=(HipBuffer&& o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
        return *this;
    }
    ~HipBuffer() { free(); }

    int reserve(size_t count)
    {
        if (p_ && count <= n_) return 0;
        free();
        count = std::max<size_t>(count, 1);
        if (Pinned)
            HIPCHK(hipHostMalloc((void**)&p_, count * sizeof(T), hipHostMallocDefault));
        else
            HIPCHK(hipMalloc((void**)&p_, count * sizeof(T)));
        n_ = count;
        return 0;
    }
    // (device buffers) reserve `count`, then copy them in on `st`
    int upload(const T* src, size_t count, hipStream_t st)
    {
        if (reserve(count)) return 1;
        if (count) HIPCHK(hipMemcpyAsync(p_, src, count * sizeof(T), hipMemcpyHostToDevice, st));
        return 0;
    }
    T* get() const { return p_; }
    T* release()  // the caller owns the memory from now on
    {
        n_ = 0;
        return std::exchange(p_, nullptr);
    }

  private:
    void free()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <typename T>
using DeviceBuffer = HipBuffer<T, false>;
template <typename T>
using PinnedBuffer = HipBuffer<T, true>;

// A non-blocking stream on the current device.  Its destructor waits for the stream before destroying it: buffers
// declared before a Stream are released only once no copy or kernel queued on it can still touch them.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream()
    {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
    int create()
    {
        HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return 0;
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event()
    {
        if (e) (void)hipEventDestroy(e);
    }
    int create(unsigned flags = hipEventDefault)
    {
        HIPCHK(hipEventCreateWithFlags(&e, flags));
        return 0;
    }
};

// the time between two events recorded on one stream around a kernel
struct KernelTimer {
    Event start, stop;
    int create() { return start.create() || stop.create(); }
    int elapsed_ms(float* ms)
    {
        HIPCHK(hipEventElapsedTime(ms, start.e, stop.e));
        return 0;
    }
};

}  // namespace e2hip
