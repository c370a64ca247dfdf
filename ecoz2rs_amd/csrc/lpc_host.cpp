// lpc_host.cpp -- `ecoz2 lpc`: .wav -> .prd on the GPU (kernels in lpc_device.hip), the WAV reader, the frame count of
// src/lpc/lpc_rs.rs:203-218, the reference's per-frame helper ecoz2_lpca (host code: src/ecoz2_lib/lpca_c.rs:7-17) and
// the session-level entries (e2vq_lpc_*).  The arithmetic contract is DESIGN.md section 8.
#include "../../include/ecoz2_vq.h"
#include "host_util.h"
#include "lpc_device.h"
#include "vq_io.h"
#include "vq_session.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <chrono>
#include <map>
#include <string>
#include <thread>
#include <vector>

using namespace e2hip;

namespace {

// ---- WAV ---------------------------------------------------------------------------------------------------------
struct Wav {
    int sample_rate = 0, bits = 0, channels = 0, format = 0;
    int64_t N = 0;         // samples (mono frames)
    int64_t data_off = 0;  // byte offset of the data chunk's payload
};

uint32_t le32(const unsigned char* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t le16(const unsigned char* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// RIFF/WAVE, mono, 16/24/32-bit integer PCM (WAVE_FORMAT_PCM, or WAVE_FORMAT_EXTENSIBLE with the PCM subformat)
int wav_parse(const char* path, Wav& w)
{
    FILE* f = fopen(path, "rb");
    if (!f) return e2vq_set_error("%s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fileno(f), &st) != 0) {
        fclose(f);
        return e2vq_set_error("%s: cannot stat", path);
    }
    const int64_t size = st.st_size;
    unsigned char h[12];
    int rc = 0;
    if (fread(h, 1, 12, f) != 12 || memcmp(h, "RIFF", 4) != 0 || memcmp(h + 8, "WAVE", 4) != 0) {
        fclose(f);
        return e2vq_set_error("%s: not a RIFF/WAVE file", path);
    }
    bool have_fmt = false;
    int64_t pos = 12;
    for (;;) {
        unsigned char ch[8];
        if (fseeko(f, (off_t)pos, SEEK_SET) != 0 || fread(ch, 1, 8, f) != 8) {
            rc = e2vq_set_error("%s: truncated WAV file (no data chunk)", path);
            break;
        }
        const uint32_t len = le32(ch + 4);
        if (!memcmp(ch, "fmt ", 4)) {
            unsigned char fm[40] = {0};
            if (len < 16 || fread(fm, 1, len < 40 ? len : 40, f) != (len < 40 ? len : 40)) {
                rc = e2vq_set_error("%s: truncated fmt chunk", path);
                break;
            }
            w.format = le16(fm);
            w.channels = le16(fm + 2);
            w.sample_rate = (int)le32(fm + 4);
            w.bits = le16(fm + 14);
            const int block_align = le16(fm + 12);
            if (w.format == 0xFFFE) {  // WAVE_FORMAT_EXTENSIBLE: the subformat GUID starts with the format code
                if (len < 40) {
                    rc = e2vq_set_error("%s: truncated WAVE_FORMAT_EXTENSIBLE fmt chunk", path);
                    break;
                }
                w.format = le16(fm + 24);
            }
            if (w.format != 1) {
                rc = e2vq_set_error("%s: unsupported WAV format: %s (format code %d); mono 16/24/32-bit integer PCM only",
                                    path, w.format == 3 ? "IEEE float" : "not integer PCM", w.format);
                break;
            }
            if (w.channels != 1) {
                rc = e2vq_set_error("%s: unsupported WAV format: %d channels; mono 16/24/32-bit integer PCM only", path,
                                    w.channels);
                break;
            }
            if ((w.bits != 16 && w.bits != 24 && w.bits != 32) || block_align != w.bits / 8) {
                rc = e2vq_set_error("%s: unsupported WAV format: %d-bit samples (block align %d); mono 16/24/32-bit "
                                    "integer PCM only", path, w.bits, block_align);
                break;
            }
            if (w.sample_rate <= 0) {
                rc = e2vq_set_error("%s: sample rate %d", path, w.sample_rate);
                break;
            }
            have_fmt = true;
        } else if (!memcmp(ch, "data", 4)) {
            if (!have_fmt) {
                rc = e2vq_set_error("%s: data chunk before the fmt chunk", path);
                break;
            }
            w.data_off = pos + 8;
            if (w.data_off + (int64_t)len > size) {
                rc = e2vq_set_error("%s: truncated WAV file: data chunk of %u bytes, %lld present", path, len,
                                    (long long)(size - w.data_off));
                break;
            }
            w.N = (int64_t)len / (w.bits / 8);
            break;
        }
        pos += 8 + (int64_t)len + (len & 1);  // chunks are padded to an even size
    }
    fclose(f);
    return rc;
}

// the samples of a parsed file as int32 (exact: the integer value of each sample)
int wav_read(const char* path, const Wav& w, int32_t* out)
{
    FILE* f = fopen(path, "rb");
    if (!f) return e2vq_set_error("%s: %s", path, strerror(errno));
    int rc = 0;
    const int B = w.bits / 8;
    if (fseeko(f, (off_t)w.data_off, SEEK_SET) != 0) rc = e2vq_set_error("%s: seek failed", path);
    if (!rc && B == 4) {
        if (fread(out, 4, (size_t)w.N, f) != (size_t)w.N) rc = e2vq_set_error("%s: truncated data", path);
    } else if (!rc) {
        const int64_t CH = 1 << 16;
        std::vector<unsigned char> buf((size_t)(CH * B));
        for (int64_t i0 = 0; i0 < w.N && !rc; i0 += CH) {
            const int64_t n = std::min(CH, w.N - i0);
            if (fread(buf.data(), (size_t)B, (size_t)n, f) != (size_t)n) {
                rc = e2vq_set_error("%s: truncated data", path);
                break;
            }
            const unsigned char* p = buf.data();
            if (B == 2) {
                for (int64_t i = 0; i < n; ++i) out[i0 + i] = (int16_t)le16(p + 2 * i);
            } else {
                for (int64_t i = 0; i < n; ++i) {
                    const uint32_t u = p[3 * i] | (p[3 * i + 1] << 8) | ((uint32_t)p[3 * i + 2] << 16);
                    out[i0 + i] = (int32_t)(u << 8) >> 8;  // sign-extend 24 bits
                }
            }
        }
    }
    fclose(f);
    return rc;
}

// ---- frame geometry (lpc_rs.rs:203-218) ----------------------------------------------------------------------------
// *T = -1: the signal is shorter than one window
int frame_geometry(int64_t N, int sample_rate, int W_ms, int O_ms, int* win, int* off, int64_t* T)
{
    const int64_t wv = (int64_t)W_ms * sample_rate / 1000, ov = (int64_t)O_ms * sample_rate / 1000;
    if (W_ms < 0 || O_ms < 0 || sample_rate <= 0) return e2vq_set_error("lpc: bad window arguments");
    if (ov == 0) return e2vq_set_error("lpc: offset of %d ms at %d Hz is zero samples", O_ms, sample_rate);
    if (wv < 2 || wv > INT32_MAX) return e2vq_set_error("lpc: window of %lld samples", (long long)wv);
    *win = (int)wv;
    *off = (int)ov;
    if (wv > N) {
        *T = -1;
        return 0;
    }
    int64_t t = (N - (wv - ov)) / ov;
    if ((t - 1) * ov + wv > N) t -= 1;  // discard the last section if incomplete
    *T = t;
    return 0;
}

// Hamming window of lpc_rs.rs:72-76 with the C library's cos
void hamming(int win, double* h)
{
    for (int n = 0; n < win; ++n) h[n] = 0.54 - 0.46 * cos(((double)(n * 2) * M_PI) / (double)(win - 1));
}

// One batch of signals analysed by one launch: samples concatenated, a frame table in waves of 64 with the same window
// per wave, one Hamming table per window length.
struct BatchSignal {
    int64_t sample_base, N, T, first_entry;
    int win, off, h_off;
};

struct Batch {
    std::vector<BatchSignal> sig;
    std::vector<e2lpc::Frame> tab;
    std::vector<double> h;
    int64_t samples = 0;

    void add(int64_t N, int win, int off, int64_t T)
    {
        int h_off = -1;
        for (const BatchSignal& s : sig)  // a window length seen before reuses its table
            if (s.win == win) h_off = s.h_off;
        if (h_off < 0) {
            h_off = (int)h.size();
            h.resize(h.size() + (size_t)win);
            hamming(win, h.data() + h_off);
        }
        if (!sig.empty() && sig.back().win != win) pad();
        BatchSignal b{samples, N, T, (int64_t)tab.size(), win, off, h_off};
        for (int64_t t = 0; t < T; ++t) tab.push_back({samples + t * off, win, h_off});
        sig.push_back(b);
        samples += N;
    }
    void pad()  // up to the next multiple of a wave, same window as the last entry
    {
        while (tab.size() % e2lpc::kWave) tab.push_back({-1, tab.back().win, tab.back().h_off});
    }
};

// device analysis of one batch whose samples are in h_samples (host, pinned or not); results to out/status (host)
struct Analyzer {
    int device = 0, P = 0;
    DeviceBuffer<int32_t> d_samples, d_status;
    DeviceBuffer<e2lpc::Frame> d_tab;
    DeviceBuffer<double> d_h, d_out;
    KernelTimer* timer = nullptr;  // optional: recorded around the kernel
    Stream st;

    int init(int dev, int p)
    {
        if (require_device(dev)) return 1;
        device = dev;
        P = p;
        return st.create();
    }
    // enqueue: copies in, kernel; results stay on the device (d_out / d_status)
    int launch(Batch& b, const int32_t* h_samples)
    {
        b.pad();
        const int NC = P + 1;
        const int64_t E = (int64_t)b.tab.size();
        if (E == 0) return 0;
        if (!e2lpc::lane_path(P))
            for (const auto& s : b.sig)
                if (s.win > e2lpc::kGenericMaxWin)
                    return e2vq_set_error("lpc: order %d runs the generic path, whose window limit is %d samples (got %d)",
                                          P, e2lpc::kGenericMaxWin, s.win);
        HIPCHK(hipSetDevice(device));
        if (d_samples.reserve((size_t)std::max<int64_t>(b.samples, 1)) || d_tab.reserve((size_t)E) || d_h.reserve(b.h.size()) ||
            d_out.reserve((size_t)E * NC) || d_status.reserve((size_t)E))
            return 1;
        HIPCHK(hipMemcpyAsync(d_samples.get(), h_samples, (size_t)b.samples * 4, hipMemcpyHostToDevice, st.s));
        HIPCHK(hipMemcpyAsync(d_tab.get(), b.tab.data(), (size_t)E * sizeof(e2lpc::Frame), hipMemcpyHostToDevice, st.s));
        HIPCHK(hipMemcpyAsync(d_h.get(), b.h.data(), b.h.size() * 8, hipMemcpyHostToDevice, st.s));
        if (timer) HIPCHK(hipEventRecord(timer->start.e, st.s));
        if (e2lpc::launch_signals(P, d_samples.get(), d_tab.get(), E, d_h.get(), d_out.get(), d_status.get(), st.s))
            return e2vq_set_error("lpc kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        if (timer) HIPCHK(hipEventRecord(timer->stop.e, st.s));
        // the host tables must stay alive until the copies are done: the caller synchronises before reusing them
        return 0;
    }
};

std::string class_of(const std::string& path)
{
    std::string dir = path;
    const size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? std::string(".") : dir.substr(0, slash);
    if (dir.empty()) dir = "/";
    std::string name = dir.substr(dir.find_last_of('/') == std::string::npos ? 0 : dir.find_last_of('/') + 1);
    if (name.empty() || name == "." || name == "..") {
        char buf[4096];
        if (realpath(dir.c_str(), buf)) {
            const std::string r(buf);
            name = r.substr(r.find_last_of('/') + 1);
        }
    }
    return name;
}

}  // namespace

// ---- the reference's per-frame helper (host) ------------------------------------------------------------------------
// lpca1, src/lpc/lpca_rs.rs:28-75: autocorrelation (sequential sums) then Levinson-Durbin; the same operations as the
// kernel.  rc[0] is not written (as lpca1); a[0] = 1 once r[0] != 0.
extern "C" int ecoz2_lpca(double* x, int n, int p, double* r, double* rc, double* a, double* pe)
{
    if (!x || !r || !rc || !a || !pe || n < 0 || p < 0 || p >= n) {
        e2vq_set_error("ecoz2_lpca: bad arguments (n = %d, p = %d)", n, p);
        return -1;
    }
    for (int i = 0; i <= p; ++i) {
        double sum = 0.0;
        for (int k = 0; k < n - i; ++k) sum += x[k] * x[k + i];
        r[i] = sum;
    }
    *pe = 0.0;
    const double r0 = r[0];
    if (0.0 == r0) return 1;
    double e = r0;
    a[0] = 1.0;
    for (int k = 1; k <= p; ++k) {
        double sum = 0.0;
        for (int i = 1; i <= k; ++i) sum -= a[k - i] * r[i];
        const double akk = sum / e;
        rc[k] = akk;
        a[k] = akk;
        for (int i = 1; i <= (k >> 1); ++i) {
            const double ai = a[i], aj = a[k - i];
            a[i] = ai + akk * aj;
            a[k - i] = aj + akk * ai;
        }
        e *= 1.0 - akk * akk;
        if (e <= 0.0) {
            *pe = e;
            return 2;
        }
    }
    *pe = e;
    return 0;
}

// ---- session-level entries ------------------------------------------------------------------------------------------
extern "C" int e2vq_wav_info(const char* path, int* sample_rate, int64_t* num_samples, int* bits_per_sample)
{
    if (!path) return e2vq_set_error("e2vq_wav_info: bad arguments");
    Wav w;
    if (wav_parse(path, w)) return 1;
    if (sample_rate) *sample_rate = w.sample_rate;
    if (num_samples) *num_samples = w.N;
    if (bits_per_sample) *bits_per_sample = w.bits;
    return 0;
}

extern "C" int e2vq_wav_read(const char* path, int32_t* samples, int64_t capacity)
{
    if (!path || !samples) return e2vq_set_error("e2vq_wav_read: bad arguments");
    Wav w;
    if (wav_parse(path, w)) return 1;
    if (w.N > capacity) return e2vq_set_error("%s: %lld samples exceed the buffer", path, (long long)w.N);
    return wav_read(path, w, samples);
}

extern "C" int e2vq_lpc_frame_count(int64_t num_samples, int sample_rate, int W_ms, int O_ms, int* win, int* off,
                                    int64_t* T)
{
    int wv = 0, ov = 0;
    int64_t t = 0;
    if (frame_geometry(num_samples, sample_rate, W_ms, O_ms, &wv, &ov, &t)) return 1;
    if (win) *win = wv;
    if (off) *off = ov;
    if (T) *T = t;
    return 0;
}

namespace {
thread_local float g_last_kernel_ms = -1.f;  // e2vq_lpc_last_kernel_ms
}

extern "C" int e2vq_lpc_last_kernel_ms(float* ms)
{
    if (!ms) return e2vq_set_error("e2vq_lpc_last_kernel_ms: bad arguments");
    *ms = g_last_kernel_ms;
    return 0;
}

extern "C" int e2vq_lpc_analyze(int device, int P, int W_ms, int O_ms, const int32_t* samples, int64_t num_samples,
                                int sample_rate, void* frames, int32_t* status, int64_t capacity, int64_t* T_out,
                                int on_device)
{
    if (P < 1 || P > E2VQ_LPC_MAX_P) return e2vq_set_error("lpc: prediction order %d out of range [1, %d]", P, E2VQ_LPC_MAX_P);
    if (!samples || num_samples < 0 || !T_out) return e2vq_set_error("e2vq_lpc_analyze: bad arguments");
    int win, off;
    int64_t T;
    if (frame_geometry(num_samples, sample_rate, W_ms, O_ms, &win, &off, &T)) return 1;
    if (T < 0) return e2vq_set_error("lpc: signal too short: %lld samples, window %d", (long long)num_samples, win);
    *T_out = T;
    if (!frames) return 0;  // size query
    if (!status) return e2vq_set_error("e2vq_lpc_analyze: bad arguments");
    if (T > capacity) return e2vq_set_error("lpc: %lld frames exceed the buffer of %lld", (long long)T, (long long)capacity);
    Analyzer an;
    if (an.init(device, P)) return 1;
    Batch b;
    b.add(num_samples, win, off, T);
    KernelTimer timer;
    if (timer.create()) return 1;
    an.timer = &timer;
    if (an.launch(b, samples)) return 1;
    const int NC = P + 1;
    const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(frames, an.d_out.get(), (size_t)T * NC * 8, k, an.st.s));
    HIPCHK(hipMemcpyAsync(status, an.d_status.get(), (size_t)T * 4, k, an.st.s));
    HIPCHK(hipStreamSynchronize(an.st.s));
    return timer.elapsed_ms(&g_last_kernel_ms);
}

extern "C" int e2vq_lpca_batch(int device, int P, const double* x, int n, int64_t count, double* r, double* rc, double* a,
                               double* pe, int32_t* status)
{
    if (P < 1 || P > E2VQ_LPC_MAX_P || n <= P || count < 0 || !x || !r || !rc || !a || !pe || !status)
        return e2vq_set_error("e2vq_lpca_batch: bad arguments (P = %d, n = %d)", P, n);
    if (!e2lpc::lane_path(P) && n > e2lpc::kGenericMaxWin)
        return e2vq_set_error("e2vq_lpca_batch: order %d runs the generic path, whose frame limit is %d samples", P,
                              e2lpc::kGenericMaxWin);
    if (!device_count()) return 1;
    if (count == 0) return 0;
    DeviceBuffer<double> dx, dr, drc, da, dpe;
    DeviceBuffer<int32_t> dst;
    Analyzer an;
    if (an.init(device, P)) return 1;
    const int NC = P + 1;
    if (dx.reserve((size_t)count * n) || dr.reserve((size_t)count * NC) || drc.reserve((size_t)count * NC) ||
        da.reserve((size_t)count * NC) || dpe.reserve((size_t)count) || dst.reserve((size_t)count))
        return 1;
    HIPCHK(hipMemcpyAsync(dx.get(), x, (size_t)count * n * 8, hipMemcpyHostToDevice, an.st.s));
    if (e2lpc::launch_windowed(P, dx.get(), n, count, dr.get(), drc.get(), da.get(), dpe.get(), dst.get(), an.st.s))
        return e2vq_set_error("lpca kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIPCHK(hipMemcpyAsync(r, dr.get(), (size_t)count * NC * 8, hipMemcpyDeviceToHost, an.st.s));
    HIPCHK(hipMemcpyAsync(rc, drc.get(), (size_t)count * NC * 8, hipMemcpyDeviceToHost, an.st.s));
    HIPCHK(hipMemcpyAsync(a, da.get(), (size_t)count * NC * 8, hipMemcpyDeviceToHost, an.st.s));
    HIPCHK(hipMemcpyAsync(pe, dpe.get(), (size_t)count * 8, hipMemcpyDeviceToHost, an.st.s));
    HIPCHK(hipMemcpyAsync(status, dst.get(), (size_t)count * 4, hipMemcpyDeviceToHost, an.st.s));
    HIPCHK(hipStreamSynchronize(an.st.s));
    return 0;
}

// ---- ecoz2_lpc_signals ----------------------------------------------------------------------------------------------
namespace {

struct Job {
    std::string path, cls, out;
    Wav w;
    int win = 0, off = 0;
    int64_t T = 0;
};

// samples per batch (int32): two pinned staging buffers of this size; a longer signal gets a batch of its own
constexpr int64_t kBatchSamples = (int64_t)1 << 25;

// reads the files of jobs [a, b) into dst (concatenated), up to `threads` files at a time
int read_batch(const std::vector<Job>& jobs, size_t a, size_t b, int32_t* dst, int threads, std::string& err)
{
    std::vector<int64_t> base(b - a + 1, 0);
    for (size_t i = a; i < b; ++i) base[i - a + 1] = base[i - a] + jobs[i].w.N;
    std::vector<int> rcs(b - a, 0);
    std::vector<std::string> errs(b - a);
    std::vector<std::thread> th;
    const int nt = std::max(1, std::min(threads, (int)(b - a)));
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            for (size_t i = a + (size_t)t; i < b; i += (size_t)nt) {
                rcs[i - a] = wav_read(jobs[i].path.c_str(), jobs[i].w, dst + base[i - a]);
                if (rcs[i - a]) errs[i - a] = e2vq_last_error();
            }
        });
    for (auto& x : th) x.join();
    for (size_t i = 0; i < rcs.size(); ++i)
        if (rcs[i]) {
            err = errs[i];
            return 1;
        }
    return 0;
}

}  // namespace

extern "C" int ecoz2_lpc_signals(int P, int W_ms, int O_ms, int minpc, float split, const char* const* sgn_filenames,
                                 int n, float mintrpt, int verbose)
{
    e2host::FlushStdout flush_at_return;
    if (P < 1 || P > E2VQ_LPC_MAX_P) return e2vq_set_error("lpc: prediction order %d out of range [1, %d]", P, E2VQ_LPC_MAX_P);
    if (n < 0 || (n > 0 && !sgn_filenames)) return e2vq_set_error("ecoz2_lpc_signals: bad arguments");
    if (W_ms <= 0 || O_ms <= 0) return e2vq_set_error("lpc: window %d ms / offset %d ms", W_ms, O_ms);
    if (!device_count()) return 1;
    if (split != 0.f) printf("NOTE: split (%g) is deprecated and ignored; all predictors go to data/predictors\n", (double)split);

    // classes: the name of each signal's parent directory (notes.md:73-79)
    std::map<std::string, std::vector<std::string>> by_class;
    for (int i = 0; i < n; ++i) {
        if (!sgn_filenames[i]) return e2vq_set_error("ecoz2_lpc_signals: NULL file name");
        by_class[class_of(sgn_filenames[i])].push_back(sgn_filenames[i]);
    }
    printf("Number of classes: %zu\n", by_class.size());
    std::vector<Job> jobs;
    std::vector<std::string> header_of_job;  // lines printed before a job's own (class header, skips)
    std::string pending;
    const std::string root = std::string(e2host::out_root()) + "/data/predictors/";
    for (const auto& kv : by_class) {
        char line[1024];
        snprintf(line, sizeof line, "class '%s': %zu\n", kv.first.c_str(), kv.second.size());
        pending += line;
        if ((int)kv.second.size() < minpc) {
            snprintf(line, sizeof line, "  (fewer than minpc = %d signals: class skipped)\n", minpc);
            pending += line;
            continue;
        }
        for (const auto& path : kv.second) {
            Job j;
            j.path = path;
            j.cls = kv.first;
            j.out = root + kv.first + "/" + e2vq_io::basename_noext(path.c_str()) + ".prd";
            if (wav_parse(path.c_str(), j.w)) return 1;
            if (frame_geometry(j.w.N, j.w.sample_rate, W_ms, O_ms, &j.win, &j.off, &j.T)) return 1;
            if (j.T < 0) {
                snprintf(line, sizeof line, "  %s\nERROR: lpa_on_signal: signal too short (%lld samples, window %d): skipped\n",
                         path.c_str(), (long long)j.w.N, j.win);
                pending += line;
                continue;
            }
            header_of_job.push_back(pending);
            pending.clear();
            jobs.push_back(std::move(j));
        }
    }
    if (jobs.empty()) {
        fputs(pending.c_str(), stdout);
        return 0;
    }

    // batches of consecutive jobs
    std::vector<size_t> cut{0};
    for (size_t i = 0, s = 0; i < jobs.size(); ++i) {
        if (s > 0 && s + jobs[i].w.N > (size_t)kBatchSamples) {
            cut.push_back(i);
            s = 0;
        }
        s += (size_t)jobs[i].w.N;
    }
    cut.push_back(jobs.size());
    const size_t nb = cut.size() - 1;
    auto batch_samples = [&](size_t k) {
        int64_t s = 0;
        for (size_t i = cut[k]; i < cut[k + 1]; ++i) s += jobs[i].w.N;
        return s;
    };

    PinnedBuffer<int32_t> stage[2];
    PinnedBuffer<double> h_out;
    std::vector<int32_t> h_status;
    Analyzer an;  // (after the buffers its stream copies into: see Stream)
    if (an.init(env_device(), P)) return 1;
    const int NC = P + 1;
    std::vector<double> keep;
    const int threads = e2vq_io::io_threads();
    using clock = std::chrono::steady_clock;
    std::vector<clock::time_point> t_read(nb);

    // reader thread: batch k + 1 is read while batch k is analysed and written
    std::string rerr;
    int rrc = 0;
    auto read_into = [&](size_t k) {
        t_read[k] = clock::now();
        rrc = read_batch(jobs, cut[k], cut[k + 1], stage[k & 1].get(), threads, rerr);
    };
    if (stage[0].reserve((size_t)batch_samples(0))) return 1;
    read_into(0);
    if (rrc) return e2vq_set_error("%s", rerr.c_str());
    for (size_t k = 0; k < nb; ++k) {
        Batch b;
        for (size_t i = cut[k]; i < cut[k + 1]; ++i) b.add(jobs[i].w.N, jobs[i].win, jobs[i].off, jobs[i].T);
        if (an.launch(b, stage[k & 1].get())) return 1;
        const int64_t E = (int64_t)b.tab.size();
        if (h_out.reserve((size_t)E * NC)) return 1;
        h_status.resize((size_t)E);
        HIPCHK(hipMemcpyAsync(h_out.get(), an.d_out.get(), (size_t)E * NC * 8, hipMemcpyDeviceToHost, an.st.s));
        HIPCHK(hipMemcpyAsync(h_status.data(), an.d_status.get(), (size_t)E * 4, hipMemcpyDeviceToHost, an.st.s));
        std::thread reader;
        if (k + 1 < nb) {
            if (stage[(k + 1) & 1].reserve((size_t)batch_samples(k + 1))) return 1;
            reader = std::thread(read_into, k + 1);
        }
        const hipError_t se = hipStreamSynchronize(an.st.s);
        int rc = se == hipSuccess ? 0 : e2vq_set_error("lpc: %s", hipGetErrorString(se));
        for (size_t i = cut[k]; i < cut[k + 1] && !rc; ++i) {
            const Job& j = jobs[i];
            const BatchSignal& s = b.sig[i - cut[k]];
            fputs(header_of_job[i].c_str(), stdout);
            printf("  %s\n", j.path.c_str());
            printf("lpa_on_signal: P=%d numSamples=%lld sampleRate=%d winSize=%d offset=%d T=%lld\n", P, (long long)j.w.N,
                   j.w.sample_rate, j.win, j.off, (long long)j.T);
            const double* rows = h_out.get() + (size_t)s.first_entry * NC;
            const int32_t* sts = h_status.data() + s.first_entry;
            int64_t good = 0;
            for (int64_t t = 0; t < j.T; ++t) good += sts[t] == 0;
            const double* payload = rows;
            if (good != j.T) {  // frames whose Levinson recursion failed are left out
                keep.resize((size_t)good * NC);
                int64_t o = 0;
                for (int64_t t = 0; t < j.T; ++t)
                    if (sts[t] == 0) memcpy(keep.data() + (size_t)(o++) * NC, rows + (size_t)t * NC, (size_t)NC * 8);
                payload = keep.data();
            }
            rc = e2vq_prd_write(j.out.c_str(), j.cls.c_str(), P, payload, good);
            if (rc) break;
            if (good != j.T)
                printf("%s: '%s': predictor saved (%lld vectors; %lld frames left out: Levinson status != 0)\n",
                       j.out.c_str(), j.cls.c_str(), (long long)good, (long long)(j.T - good));
            else
                printf("%s: '%s': predictor saved\n", j.out.c_str(), j.cls.c_str());
            const double secs = std::chrono::duration<double>(clock::now() - t_read[k]).count();
            if (secs >= (double)mintrpt) printf("  processing took: %.2fs\n", secs);
            if (verbose) printf("  batch %zu/%zu: %lld frames\n", k + 1, nb, (long long)j.T);
        }
        if (reader.joinable()) reader.join();
        if (rc) return 1;
        if (rrc) return e2vq_set_error("%s", rerr.c_str());
    }
    fputs(pending.c_str(), stdout);
    return 0;
}

// ---- e2vq_lpc_features: features of stored LPC vectors (lpc_features.hip) ------------------------------------------
extern "C" int e2vq_lpc_features(int device, int P, int Q, const double* frames, int64_t T, int32_t* status, double* pe,
                                 double* rc, double* a, double* c, int on_device)
{
    if (P < 1 || P > E2VQ_LPC_MAX_P) return e2vq_set_error("lpc features: prediction order %d out of range [1, %d]", P, E2VQ_LPC_MAX_P);
    if (Q < 0 || (Q > 0 && Q <= P)) return e2vq_set_error("lpc features: cepstrum length %d must be > prediction order %d", Q, P);
    if (Q > E2VQ_LPC_FEATURES_MAX_Q)
        return e2vq_set_error("lpc features: cepstrum length %d exceeds the limit of %d", Q, E2VQ_LPC_FEATURES_MAX_Q);
    if (!frames || T < 0) return e2vq_set_error("e2vq_lpc_features: bad arguments");
    if (Q == 0) c = nullptr;
    if (!device_count()) return 1;
    if (T == 0) return 0;
    DeviceBuffer<double> din, dpe, drc, da, dc;
    DeviceBuffer<int32_t> dst;
    Analyzer an;
    if (an.init(device, P)) return 1;
    const int NC = P + 1;
    if (on_device) {
        KernelTimer timer;
        if (timer.create()) return 1;
        HIPCHK(hipEventRecord(timer.start.e, an.st.s));
        if (e2lpc::launch_features(P, Q, frames, T, status, pe, rc, a, c, an.st.s))
            return e2vq_set_error("lpc features kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        HIPCHK(hipEventRecord(timer.stop.e, an.st.s));
        HIPCHK(hipStreamSynchronize(an.st.s));
        return timer.elapsed_ms(&g_last_kernel_ms);
    }
    // host memory: chunks of frames through device buffers; c[0] is then replaced by the C library's log(sqrt(pe))
    const int64_t CH = std::min<int64_t>(T, (int64_t)1 << 18);
    const bool need_pe = pe || c;
    if (din.reserve((size_t)CH * NC) || (status && dst.reserve((size_t)CH)) || (need_pe && dpe.reserve((size_t)CH)) ||
        (rc && drc.reserve((size_t)CH * NC)) || (a && da.reserve((size_t)CH * NC)) || (c && dc.reserve((size_t)CH * Q)))
        return 1;
    std::vector<double> pe_tmp;
    if (c && !pe) pe_tmp.resize((size_t)CH);
    for (int64_t t0 = 0; t0 < T; t0 += CH) {
        const int64_t n = std::min(CH, T - t0);
        HIPCHK(hipMemcpyAsync(din.get(), frames + t0 * NC, (size_t)n * NC * 8, hipMemcpyHostToDevice, an.st.s));
        if (e2lpc::launch_features(P, Q, din.get(), n, status ? dst.get() : nullptr, need_pe ? dpe.get() : nullptr,
                                   rc ? drc.get() : nullptr, a ? da.get() : nullptr, c ? dc.get() : nullptr, an.st.s))
            return e2vq_set_error("lpc features kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        double* pe_h = pe ? pe + t0 : pe_tmp.data();
        if (status) HIPCHK(hipMemcpyAsync(status + t0, dst.get(), (size_t)n * 4, hipMemcpyDeviceToHost, an.st.s));
        if (need_pe) HIPCHK(hipMemcpyAsync(pe_h, dpe.get(), (size_t)n * 8, hipMemcpyDeviceToHost, an.st.s));
        if (rc) HIPCHK(hipMemcpyAsync(rc + t0 * NC, drc.get(), (size_t)n * NC * 8, hipMemcpyDeviceToHost, an.st.s));
        if (a) HIPCHK(hipMemcpyAsync(a + t0 * NC, da.get(), (size_t)n * NC * 8, hipMemcpyDeviceToHost, an.st.s));
        if (c) HIPCHK(hipMemcpyAsync(c + t0 * Q, dc.get(), (size_t)n * Q * 8, hipMemcpyDeviceToHost, an.st.s));
        HIPCHK(hipStreamSynchronize(an.st.s));
        if (c)
            for (int64_t t = 0; t < n; ++t) c[(t0 + t) * Q] = log(sqrt(pe_h[t]));
    }
    return 0;
}
