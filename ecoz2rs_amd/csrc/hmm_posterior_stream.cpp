// hmm_posterior_stream.cpp -- `hmm segment --continuous-posteriors`: a session that takes one symbol stream
// of unknown length in feeds of any length and delivers the class posteriors of `hmm segment --posteriors` block by block, each
// block once a look-ahead of L frames behind it has been fed (the kernels of hmm_posterior_stream.hip); and the file form that
// feeds consecutive pieces of one recording to a `--continuous` session and to a posterior session.  Shape checks, models,
// packing, its device side and the body choice are hmm_class_loop.cpp's, the parameter block hmm_transcript.cpp's, the input
// stage hmm_input.cpp's (hmm_host.h).
// The schedule: block b = the frames [b B, (b + 1) B) is delivered by the launch of window b, which is queued as soon as
// w_b = (b + 1) B + L symbols have been fed; the launch advances the forward pass to w_b and walks back to b B.  The ring has
// B + L rows (ah, c, symbol): what window b's forward pass and the symbols behind it overwrite belongs to block b - 1, whose
// launch precedes them on the session's stream.  close queues one launch to the end of the stream over all undelivered blocks.
#include "hmm_host.h"
#include "hmm_posterior_stream.h"

#include <memory>

using namespace e2hmm_host;
using e2hmm::PostStreamState;

struct e2vq_posterior_stream {
    int device = 0, K = 0, M = 0, sumN = 0, waves = 0;
    bool looped = false;  // the body, fixed at open (ECOZ2_HMM_POSTERIOR_BODY)
    double sw = 0.0;      // exp(ln_switch)
    i64 B = 0, L = 0, R = 0;  // block, look-ahead, ring rows = B + L
    i64 dev_bytes = 0;
    // device: parameters, packing and plan; the ring (d_ah, d_c, d_sym); the staging buffer of one launch's posteriors (d_post,
    // B + L rows: what the launch of close may emit); the session's state
    ClassLoopDev loop;
    DeviceBuffer<double> d_ah, d_c, d_post;
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<PostStreamState> d_state;
    // pinned host: the rows of the launches since the last wait, and the state
    PinnedBuffer<double> h_post;
    PinnedBuffer<PostStreamState> h_state;
    e2hmm::PostRingDev ring{};
    KernelTimer all;
    bool timing = false;  // all.start is recorded and not yet closed by a wait
    float kernel_ms = 0.f;
    // the stream so far
    i64 fed = 0;       // symbols given
    i64 fwd = 0;       // frames the forward pass has been queued for
    i64 next_b = 0;    // the first block no launch has been queued for
    i64 ready = 0;     // frames delivered
    i64 taken = 0;     // frames handed out
    i64 launches = 0, walked = 0;  // launches queued; frames their backward passes walk
    bool closed = false;
    int status = 0;
    i64 ev_frame = -1;
    double log_prob = 0.0;
    struct Queued {  // a launch since the last wait: its window end, and its rows in h_post
        i64 w, count;
        size_t at;
    };
    std::vector<Queued> queued;
    size_t h_used = 0;           // doubles of h_post the stream is filling
    std::vector<double> f_post;  // delivered rows not yet taken, [taken, ready)
    Stream st;  // (after the buffers: see Stream)
};

namespace {

typedef e2vq_posterior_stream Session;

// The refusals of a session that e2vq_hmm_segment_posteriors does not make: host only.
int check_block(const char* who, i64 block, i64 lookahead)
{
    if (block < 1) return e2vq_set_error("%s: a block of %lld frames (at least 1)", who, (long long)block);
    if (lookahead < 0) return e2vq_set_error("%s: a look-ahead of %lld frames (at least 0)", who, (long long)lookahead);
    return 0;
}

// The models (checked by segment_check_shape, posteriors_check_slots with `body` and posteriors_check_params; all of one M)
// on the device and an empty session.
int stream_open(const char* who, int device, const LoopModels& lm, double ln_switch, i64 B, i64 L, LoopBody body, Session** out)
{
    const int K = lm.K(), M = lm.M;
    const SegPacking pk = pack_slots(lm.Ns, posteriors_a_ld);
    const int sumN = pk.sumN;
    const bool looped = runs_looped(body, pk.slots);
    const int waves = body_waves(looped, pk.slots);
    const double sw = exp(ln_switch);  // (-inf: 0.0)
    const std::vector<double> params = embed_params(lm, pk, sw);
    // a ring row: ah (sumN doubles), c (a double a wave) and the symbol.  Counted with it, though no part of the ring: the staging
    // buffer of one launch's posteriors, B + L rows of K doubles -- a feed's launch fills B of them, the launch of close up to
    // B + L - 1 (every undelivered block in one backward pass)
    const i64 row = 8 * ((i64)sumN + waves + K) + 2;
    const bool fits = B <= ((i64)1 << 40) && L <= ((i64)1 << 40);  // (beyond: the byte count below would overflow)
    const i64 R = fits ? B + L : 0;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    std::unique_ptr<Session> sp(new Session);
    Session& s = *sp;
    s.device = device, s.K = K, s.M = M, s.sumN = sumN, s.waves = waves, s.looped = looped, s.sw = sw, s.B = B, s.L = L, s.R = R;
    if (s.st.create() || s.all.create()) return 1;
    const hipStream_t st = s.st.s;
    if (s.loop.upload(pk, params, K, M, st) || s.d_state.reserve(1) || s.h_state.reserve(1)) return 1;
    if (!fits || s.d_ah.reserve((size_t)R * sumN) || s.d_c.reserve((size_t)R * waves) || s.d_sym.reserve((size_t)R) ||
        s.d_post.reserve((size_t)R * K)) {
        const std::string why = fits ? e2vq_last_error() : "the size is out of range";
        (void)hipStreamSynchronize(st);  // (`params` and the packing are locals)
        (void)hipGetLastError();         // (the failed allocation is reported here, not by the next call's check)
        if (!fits) return e2vq_set_error("%s: no room for the ring of %lld + %lld frames x %d states: %s", who, (long long)B, (long long)L, sumN, why.c_str());
        return e2vq_set_error("%s: no room for the ring of %lld frames x %d states (%lld bytes: block %lld + look-ahead %lld): %s", who,
                              (long long)R, sumN, (long long)(R * row), (long long)B, (long long)L, why.c_str());
    }
    s.dev_bytes = s.loop.bytes + R * row + (i64)sizeof(PostStreamState);
    PostStreamState init{};
    init.p = 0.5, init.E = 1, init.frame = -1;
    *s.h_state.get() = init;
    HIPCHK(hipMemcpyAsync(s.d_state.get(), s.h_state.get(), sizeof init, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // (`params` and the packing are locals)
    s.ring = e2hmm::PostRingDev{s.d_ah.get(), s.d_c.get(), s.d_sym.get(), R};
    *out = sp.release();
    return 0;
}

// queues the copy of n symbols, the frames t .. t + n - 1, to their ring rows (n <= R)
int queue_symbols(Session& s, const unsigned short* src, i64 t, i64 n, hipMemcpyKind kind)
{
    if (n < 1) return 0;
    const i64 row = t % s.R, first = std::min(n, s.R - row);
    HIPCHK(hipMemcpyAsync(s.d_sym.get() + row, src, (size_t)first * 2, kind, s.st.s));
    if (n > first) HIPCHK(hipMemcpyAsync(s.d_sym.get(), src + first, (size_t)(n - first) * 2, kind, s.st.s));
    return 0;
}

// queues one launch: the forward pass to w, the backward pass down to the first undelivered frame, the rows of [lo, emit_hi)
// and their copy to h_post
int queue_window(Session& s, i64 w, i64 emit_hi)
{
    const hipStream_t st = s.st.s;
    const i64 lo = s.next_b * s.B, count = emit_hi - lo;
    if (!s.timing) {
        HIPCHK(hipEventRecord(s.all.start.e, st));
        s.timing = true;
    }
    if (e2hmm::launch_loop_posteriors_stream(s.loop.pl, s.looped, s.ring, s.fwd, w, lo, emit_hi, s.sw, s.d_post.get(), s.d_state.get(), st))
        return e2vq_set_error("hmm segment --continuous-posteriors: %d wave-slots of %d states cannot be launched", s.loop.pl.slots, s.sumN);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.h_post.get() + s.h_used, s.d_post.get(), (size_t)count * s.K * 8, hipMemcpyDeviceToHost, st));
    s.queued.push_back(Session::Queued{w, count, s.h_used});
    s.h_used += (size_t)count * s.K;
    s.fwd = w;
    s.launches += 1;
    s.walked += w - lo;
    return 0;
}

// The one wait of a feed or of close, and what the launches since the last one delivered.  A launch whose forward pass met an
// event, and every launch behind it, delivered nothing.  Returns 2 when this wait found a symbol outside the alphabet.
int wait_and_deliver(Session& s)
{
    const hipStream_t st = s.st.s;
    if (s.timing) HIPCHK(hipEventRecord(s.all.stop.e, st));
    HIPCHK(hipMemcpyAsync(s.h_state.get(), s.d_state.get(), sizeof(PostStreamState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (s.timing) {
        float ms = 0.f;
        if (s.all.elapsed_ms(&ms)) return 1;
        s.kernel_ms += ms;
        s.timing = false;
    }
    const PostStreamState& hs = *s.h_state.get();
    for (const Session::Queued& q : s.queued) {
        if (hs.status != 0 && q.w > hs.frame) break;
        s.f_post.insert(s.f_post.end(), s.h_post.get() + q.at, s.h_post.get() + q.at + (size_t)q.count * s.K);
        s.ready += q.count;
    }
    s.queued.clear();
    s.h_used = 0;
    if (hs.status != 0 && s.status == 0) {
        s.status = hs.status;
        s.ev_frame = hs.frame;
        if (hs.status == 2) return 2;
    }
    return 0;
}

int bad_symbol(const char* who, const Session& s)
{
    return e2vq_set_error("%s: the symbol at frame %lld is outside the models' alphabet of %d; the session takes no more symbols", who,
                          (long long)s.ev_frame, s.M);
}

int stream_feed(const char* who, Session& s, const void* sym, i64 n, bool on_device)
{
    if (s.status == 1) {  // the loop cannot emit the stream: the symbols count, nothing else happens
        s.fed += n;
        return 0;
    }
    const unsigned short* src = (const unsigned short*)sym;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const i64 B = s.B, L = s.L, avail = s.fed + n;
    // the windows this feed completes: the blocks b >= next_b with (b + 1) B + L <= avail
    const i64 nwin = avail >= L ? std::max<i64>((avail - L) / B - s.next_b, 0) : 0;
    if (s.h_post.reserve((size_t)(nwin * B) * s.K)) return 1;  // (empty: every feed ends with a wait)
    i64 o = 0;  // symbols of the feed queued
    for (i64 i = 0; i < nwin; ++i) {
        const i64 w = (s.next_b + 1) * B + L;
        if (queue_symbols(s, src + o, s.fed + o, w - (s.fed + o), kind)) return 1;
        o = w - s.fed;
        if (queue_window(s, w, (s.next_b + 1) * B)) return 1;
        s.next_b += 1;
    }
    // the remainder waits in the ring: fewer symbols than the next window lacks, in rows of delivered blocks
    if (queue_symbols(s, src + o, s.fed + o, n - o, kind)) return 1;
    s.fed += n;
    const int rc = wait_and_deliver(s);
    return rc == 2 ? bad_symbol(who, s) : rc;
}

// Returns 2 when the close itself met a symbol outside the alphabet (the session is closed all the same).
int stream_close(Session& s)
{
    int rc = 0;
    if (s.status == 0 && s.fed > s.next_b * s.B) {  // the undelivered blocks: fewer than B + L frames
        if (s.h_post.reserve((size_t)(s.fed - s.next_b * s.B) * s.K) || queue_window(s, s.fed, s.fed)) return 1;
        rc = wait_and_deliver(s);
        if (rc == 1) return 1;
    }
    if (s.status == 0) {
        const PostStreamState& hs = *s.h_state.get();
        s.log_prob = e2hmm_host::log_prob(hs.p, hs.E);
    } else {  // every row that was not delivered is +0.0
        s.f_post.insert(s.f_post.end(), (size_t)(s.fed - s.ready) * s.K, 0.0);
        s.ready = s.fed;
        s.log_prob = -INFINITY;
    }
    s.closed = true;
    return rc;
}

}  // namespace

extern "C" int e2vq_hmm_posterior_stream_open(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                              const double* const* Bs, double ln_switch, int64_t block, int64_t lookahead,
                                              e2vq_posterior_stream** out)
{
    const char* who = "e2vq_hmm_posterior_stream_open";
    LoopModels lm;
    LoopBody body = LoopBody::Resident;
    if (loop_check_args(who, K, Ns, pis, As, Bs, out != nullptr) || segment_check_shape(who, K, Ns) || segment_check_switch(who, ln_switch) ||
        posteriors_body(&body) || posteriors_check_slots(who, K, Ns, body) || check_block(who, block, lookahead) ||
        lm.from_arrays(K, Ns, M, pis, As, Bs))
        return 1;
    for (const Hmm& h : lm.models)
        if (posteriors_check_params(h)) return 1;
    return stream_open(who, device, lm, ln_switch, block, lookahead, body, out);
}

extern "C" int e2vq_hmm_posterior_stream_feed(e2vq_posterior_stream* s, const void* sym, int64_t n, int sym_on_device, int64_t* ready_frames)
{
    const char* who = "e2vq_hmm_posterior_stream_feed";
    if (!s) return e2vq_set_error("%s: NULL session", who);
    if (s->closed) return e2vq_set_error("%s: the session is closed", who);
    if (s->status == 2)
        return e2vq_set_error("%s: the session met a symbol outside the alphabet at frame %lld and takes no more symbols", who,
                              (long long)s->ev_frame);
    if (n < 0 || (n > 0 && !sym)) return e2vq_set_error("%s: bad arguments", who);
    HIPCHK(hipSetDevice(s->device));
    const int rc = n > 0 ? stream_feed(who, *s, sym, n, sym_on_device != 0) : 0;
    if (ready_frames) *ready_frames = s->ready;
    return rc;
}

extern "C" int e2vq_hmm_posterior_stream_close(e2vq_posterior_stream* s, double* log_prob, int* status, int64_t* ready_frames)
{
    const char* who = "e2vq_hmm_posterior_stream_close";
    if (!s) return e2vq_set_error("%s: NULL session", who);
    if (s->closed) return e2vq_set_error("%s: the session is closed", who);
    HIPCHK(hipSetDevice(s->device));
    const int rc = stream_close(*s);
    if (rc == 1) return 1;
    if (log_prob) *log_prob = s->log_prob;
    if (status) *status = s->status;
    if (ready_frames) *ready_frames = s->ready;
    return rc == 2 ? bad_symbol(who, *s) : 0;
}

extern "C" int e2vq_hmm_posterior_stream_take(e2vq_posterior_stream* s, int64_t max_frames, double* post, int64_t* first_frame, int64_t* count)
{
    if (!s) return e2vq_set_error("e2vq_hmm_posterior_stream_take: NULL session");
    if (max_frames < 0) return e2vq_set_error("e2vq_hmm_posterior_stream_take: bad arguments");
    const size_t c = (size_t)std::min<i64>(max_frames, s->ready - s->taken), words = c * (size_t)s->K;
    if (post) std::copy(s->f_post.begin(), s->f_post.begin() + (std::ptrdiff_t)words, post);
    s->f_post.erase(s->f_post.begin(), s->f_post.begin() + (std::ptrdiff_t)words);
    if (first_frame) *first_frame = s->taken;
    if (count) *count = (int64_t)c;
    s->taken += (i64)c;
    return 0;
}

extern "C" int e2vq_hmm_posterior_stream_kernel_ms(e2vq_posterior_stream* s, float* ms)
{
    if (!s || !ms) return e2vq_set_error("e2vq_hmm_posterior_stream_kernel_ms: %s", s ? "bad arguments" : "NULL session");
    *ms = s->kernel_ms;
    return 0;
}

extern "C" int e2vq_hmm_posterior_stream_stats(e2vq_posterior_stream* s, int64_t* device_bytes, int64_t* ring_rows, int64_t* launches,
                                               int64_t* backward_frames)
{
    if (!s) return e2vq_set_error("e2vq_hmm_posterior_stream_stats: NULL session");
    if (device_bytes) *device_bytes = s->dev_bytes;
    if (ring_rows) *ring_rows = s->R;
    if (launches) *launches = s->launches;
    if (backward_frames) *backward_frames = s->walked;
    return 0;
}

extern "C" void e2vq_hmm_posterior_stream_free(e2vq_posterior_stream* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

namespace {

struct PostHolder {
    Session* s = nullptr;
    ~PostHolder() { e2vq_hmm_posterior_stream_free(s); }
};
struct SegHolder {
    e2vq_segment_stream* s = nullptr;
    ~SegHolder() { e2vq_hmm_segment_stream_free(s); }
};

}  // namespace

// `hmm segment --continuous-posteriors`: the inputs are consecutive pieces of one recording.  Each is staged once and fed, on
// the device, to a `--continuous` session (unchanged: through its C entry points) and to a posterior session; the report of the
// whole run is e2vq_hmm_segment_report_posteriors'.  The host keeps the T K doubles of the posteriors for that report.
extern "C" int e2vq_hmm_segment_continuous_files_posteriors(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                                            const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                                            double ln_switch, const char* name, const char* csv_dir_or_file,
                                                            const char* frames_dir, int64_t block, int64_t lookahead)
{
    const char* who = "e2vq_hmm_segment_continuous_files_posteriors";
    FlushStdout flush_on_return;
    LoopModels fm;
    LoopBody body = LoopBody::Resident;
    if (files_given(who, model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
    if (!name || !*name) return e2vq_set_error("%s: the recording needs a name", who);
    if (segment_check_switch(who, ln_switch) || window_ms_ok(who, W_ms, O_ms) || fm.load_checked(who, model_filenames, num_models) ||
        posteriors_body(&body) || posteriors_check_slots(who, fm.K(), fm.Ns.data(), body) || check_block(who, block, lookahead))
        return 1;
    for (const Hmm& h : fm.models)
        if (posteriors_check_params(h)) return 1;
    SymInputs si;
    if (sym_inputs_check(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, nullptr, si)) return 1;
    std::string csv = csv_dir_or_file ? csv_dir_or_file : "";
    if (!csv.empty() && !ends_with(csv, ".csv")) csv += std::string("/") + name + ".csv";
    const std::string fcsv = frames_dir && *frames_dir ? frames_csv_path(frames_dir, name) : "";
    const int K = fm.K(), device = env_device();
    std::vector<const double*> pis, As, Bs;
    for (const Hmm* h : fm.ms) pis.push_back(h->pi.data()), As.push_back(h->A.data()), Bs.push_back(h->B.data());
    SegHolder seg;
    PostHolder post;
    if (e2vq_hmm_segment_stream_open(device, K, fm.Ns.data(), fm.M, pis.data(), As.data(), Bs.data(), ln_switch, &seg.s) ||
        stream_open(who, device, fm, ln_switch, block, lookahead, body, &post.s))
        return 1;
    Session& s = *post.s;
    SymStage stg;
    if (stg.open(device, si)) return 1;
    for (const SymInput& in : si.inputs) {
        int64_t T = 0;
        // (the stage waits for its stream before it returns, and a feed waits for its session's: the buffer is free again)
        if (stg.input(in, si, P, W_ms, O_ms, &T)) return 1;
        if (T < 1) continue;
        if (stream_feed(who, s, stg.d_sym.get(), T, true) || e2vq_hmm_segment_stream_feed(seg.s, stg.d_sym.get(), T, 1, nullptr)) {
            if (s.status == 2)
                return e2vq_set_error("%s: a symbol outside the models' alphabet of %d (frame %lld of %s)", in.path.c_str(), fm.M,
                                      (long long)s.ev_frame, name);
            return 1;
        }
    }
    double lp = 0.0;
    int seg_status = 0;
    int64_t T = 0;
    const int rc = stream_close(s);
    if (rc == 1 || e2vq_hmm_segment_stream_close(seg.s, &lp, &seg_status, &T)) return 1;
    if (s.status == 2 || seg_status == 2)
        return e2vq_set_error("%s: a symbol outside the models' alphabet of %d (frame %lld)", name, fm.M, (long long)s.ev_frame);
    const size_t n = (size_t)std::max<int64_t>(T, 1);
    std::vector<uint16_t> cls(n);
    std::vector<uint8_t> entered(n);
    std::vector<double> gbest(n);
    if (e2vq_hmm_segment_stream_take(seg.s, T, cls.data(), nullptr, entered.data(), gbest.data(), nullptr, nullptr)) return 1;
    return e2vq_hmm_segment_report_posteriors(name, T, K, fm.names.data(), W_ms, O_ms, cls.data(), entered.data(), gbest.data(), lp, ln_switch,
                                              s.f_post.data(), csv.empty() ? nullptr : csv.c_str(), fcsv.empty() ? nullptr : fcsv.c_str());
}
