// hmm_segment_stream.cpp -- `hmm segment --continuous`: a decoder session that takes one symbol stream of
// unknown length in feeds of any length, runs the joint Viterbi of `hmm segment` on it block by block (the kernels of
// hmm_segment_stream.hip), keeps the back-pointers of the undecided frames alone -- in a ring on the device -- and hands the
// frames out as soon as every surviving path agrees on them; and the file form that feeds consecutive pieces of one recording
// to one session.  Shape checks, models, packing and its device side are hmm_class_loop.cpp's, the input stage hmm_input.cpp's
// (hmm_host.h).
// A session has two modes, and one schedule serves both: under the one switch penalty, or -- `matrix` --
// under a K x K matrix of class-to-class prices (`--class-transitions --grammar-continuous`, hmm_segment_trans_stream.hip, or
// the looped block step of hmm_segment_trans_looped.hip where ECOZ2_HMM_SEGMENT_TRANS_BODY chose it when the session opened).
// Only the launches, the ring's allocations and the results of a commit differ.
#include "hmm_host.h"
#include "hmm_segment_trans_stream.h"

#include <memory>

using namespace e2hmm_host;
using e2hmm::SegStreamState;

struct e2vq_segment_stream {
    int device = 0, K = 0, M = 0, sumN = 0;
    bool looped = false;  // the body of the block step, fixed at open (under a matrix: ECOZ2_HMM_SEGMENT_TRANS_BODY)
    bool matrix = false;  // class-to-class prices: the ring holds psi, src, x and E, a commit yields exit_score
    double ln_switch = 0.0;
    i64 B = 0;         // frames of a block
    i64 C = 0;         // frames the pending budget holds; the ring has C + B - 1 rows (the last B - 1: the remainder at close)
    i64 dev_bytes = 0;
    // device: parameters, packing and plan (as segment_device uploads them), the ring, the carried d, O(B) staging, the session's state
    ClassLoopDev loop;
    DeviceBuffer<double> d_d, d_gstage;
    DeviceBuffer<int> d_gsel;
    DeviceBuffer<unsigned short> d_psi, d_blk;
    DeviceBuffer<SegStreamState> d_state;
    // matrix: the prices transposed, the ring's src / x / E, and exit_score of one commit (8 bytes more a pending frame)
    DeviceBuffer<double> d_ltT, d_Es, d_score;
    DeviceBuffer<unsigned short> d_src, d_xs;
    PinnedBuffer<double> h_score;
    e2hmm::SegTransRingDev tring{};
    // device and pinned host: cls / state / entered of one commit (5 bytes a pending frame); G of the blocks since the last wait
    DeviceBuffer<unsigned short> d_cls, d_st;
    DeviceBuffer<unsigned char> d_entered;
    PinnedBuffer<unsigned short> h_cls, h_st;
    PinnedBuffer<unsigned char> h_entered;
    PinnedBuffer<double> h_g;
    PinnedBuffer<SegStreamState> h_state;
    e2hmm::SegRingDev ring{};
    KernelTimer all, commit_t;
    bool timing = false;  // all.start is recorded and not yet closed by a wait
    float kernel_ms = 0.f, commit_ms = 0.f;
    // the stream so far
    i64 fed = 0;        // symbols given
    i64 p = 0;          // frames processed (the forward pass has been queued for them)
    i64 r = 0;          // symbols buffered in d_blk
    i64 F = 0;          // frames final
    i64 taken = 0;      // frames handed out
    i64 g_queued = 0;   // doubles of h_g the stream is filling
    i64 peak_pending = 0;
    int dcur = 0;       // which half of d_d holds d of frame p - 1
    bool dirty = false;  // frames were processed since the last coalescence
    bool closed = false;
    int status = 0;
    i64 bad_frame = -1;
    double log_prob = 0.0;
    // final frames not yet taken, [taken, F); G of the pending frames, [F, p)
    std::vector<uint16_t> f_cls, f_st;
    std::vector<uint8_t> f_entered;
    // (matrix: f_g holds exit_score, which the backtrack writes; pend_g stays empty)
    std::vector<double> f_g, pend_g;
    Stream st;  // (after the buffers: see Stream)
};

namespace {

typedef e2vq_segment_stream Session;

const char* const ENV_BLOCK = "ECOZ2_HMM_SEGMENT_STREAM_BLOCK";
const char* const ENV_PENDING = "ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES";

double* d_half(Session& s, int which) { return s.d_d.get() + (size_t)which * s.sumN; }

const char* flag_of(const Session& s) { return s.matrix ? "--grammar-continuous" : "--continuous"; }

// The models (checked by segment_check_shape; all of one M) on the device and an empty session.  lt: the K x K prices of a
// matrix session (checked by trans_check_lt), or null under the one ln_switch.  Every refusal comes before the first HIP call.
// trans_body: the body of a matrix session (what segment_trans_body gave).
int stream_open(const char* who, int device, const LoopModels& lm, double ln_switch, const double* lt, Session** out,
                LoopBody trans_body = LoopBody::Resident)
{
    const int K = lm.K(), M = lm.M;
    const char* bv = getenv(ENV_BLOCK);
    const i64 B = bv && *bv ? atoll(bv) : 4096;
    if (B < 1 || B > ((i64)1 << 24)) return e2vq_set_error("%s: %s=%s: a block of 1 .. %d frames", who, ENV_BLOCK, bv, 1 << 24);
    const SegPacking pk = pack_slots(lm.Ns);
    const int sumN = pk.sumN;
    bool looped = false;
    if (lt ? trans_check_slots(who, K, lm.Ns.data(), trans_body) : loop_body_looped("ECOZ2_HMM_SEGMENT_BODY", pk.slots, &looped))
        return 1;
    if (lt) looped = runs_looped(trans_body, pk.slots);
    const i64 row = 2 * (i64)sumN + (lt ? 12 * (i64)K : 4), budget = env_bytes(ENV_PENDING, (i64)256 << 20), C = budget / row;
    if (C < 2 * B)
        return lt ? e2vq_set_error("%s: %s=%lld holds %lld pending frames of %d states and %d classes (%lld bytes a frame): fewer than "
                                   "two blocks of %lld", who, ENV_PENDING, (long long)budget, (long long)C, sumN, K, (long long)row, (long long)B)
                  : e2vq_set_error("%s: %s=%lld holds %lld pending frames of %d states (%lld bytes a frame): fewer than two blocks of %lld", who,
                                   ENV_PENDING, (long long)budget, (long long)C, sumN, (long long)row, (long long)B);
    const std::vector<double> params = loop_log_params(lm, pk);
    const std::vector<double> ltT = lt ? trans_transposed(K, lt) : std::vector<double>();
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    std::unique_ptr<Session> sp(new Session);
    Session& s = *sp;
    s.device = device, s.K = K, s.M = M, s.sumN = sumN, s.ln_switch = ln_switch, s.B = B, s.C = C;
    s.looped = looped;
    s.matrix = lt != nullptr;
    const i64 rows = C + B - 1;
    if (s.st.create() || s.all.create() || s.commit_t.create()) return 1;
    const hipStream_t st = s.st.s;
    if (s.loop.upload(pk, params, K, M, st) || s.d_d.reserve((size_t)2 * sumN) || s.d_blk.reserve((size_t)B) || s.d_state.reserve(1) ||
        s.h_state.reserve(1) || (s.matrix ? s.d_ltT.upload(ltT.data(), ltT.size(), st) : s.d_gstage.reserve((size_t)B)))
        return 1;
    if (s.d_psi.reserve((size_t)rows * sumN) ||
        (s.matrix ? s.d_src.reserve((size_t)rows * K) || s.d_xs.reserve((size_t)rows * K) || s.d_Es.reserve((size_t)rows * K)
                  : s.d_gsel.reserve((size_t)rows))) {
        const std::string why = e2vq_last_error();
        return e2vq_set_error("%s: no room for the ring of %lld pending frames x %d states (%lld bytes; %s bounds it): %s", who,
                              (long long)rows, sumN, (long long)(rows * row), ENV_PENDING, why.c_str());
    }
    // (besides the ring: the carried d, the block's symbols, and G of a block or the K x K prices)
    s.dev_bytes = s.loop.bytes + rows * row + (i64)2 * sumN * 8 + (s.matrix ? B * 2 + (i64)K * K * 8 : B * 10) + (i64)sizeof(SegStreamState);
    SegStreamState zero{};
    zero.fstar = -1, zero.bad_frame = -1, zero.prev_a = -1, zero.reached = -1;
    *s.h_state.get() = zero;
    HIPCHK(hipMemcpyAsync(s.d_state.get(), s.h_state.get(), sizeof zero, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // (`params` and the packing are locals)
    s.ring = e2hmm::SegRingDev{s.d_psi.get(), s.d_gsel.get(), rows};
    s.tring = e2hmm::SegTransRingDev{s.d_psi.get(), s.d_src.get(), s.d_xs.get(), s.d_Es.get(), rows};
    *out = sp.release();
    return 0;
}

// queues the forward pass of n symbols at `blk` (device) as the frames p .. p + n - 1, and under the one price the copy of
// their G
int queue_block(Session& s, const unsigned short* blk, i64 n)
{
    const hipStream_t st = s.st.s;
    if (!s.timing) {
        HIPCHK(hipEventRecord(s.all.start.e, st));
        s.timing = true;
    }
    const auto trans_launch = s.looped ? e2hmm::launch_segment_trans_stream_looped : e2hmm::launch_segment_trans_stream;
    if (s.matrix ? trans_launch(s.loop.pl, blk, (int)n, s.p, s.d_ltT.get(), d_half(s, s.dcur), d_half(s, s.dcur ^ 1), s.tring,
                                s.d_state.get(), st)
                 : e2hmm::launch_segment_stream(s.loop.pl, s.looped, blk, (int)n, s.p, s.ln_switch, d_half(s, s.dcur), d_half(s, s.dcur ^ 1),
                                                s.ring, s.d_gstage.get(), s.d_state.get(), st))
        return e2vq_set_error("hmm segment %s: %d wave-slots of %d states cannot be launched", flag_of(s), s.loop.pl.slots, s.sumN);
    HIPCHK(hipGetLastError());
    if (!s.matrix) {
        HIPCHK(hipMemcpyAsync(s.h_g.get() + s.g_queued, s.d_gstage.get(), (size_t)n * 8, hipMemcpyDeviceToHost, st));
        s.g_queued += n;
    }
    s.dcur ^= 1;
    s.p += n;
    s.dirty = true;
    s.peak_pending = std::max(s.peak_pending, s.p - s.F);
    return 0;
}

// The one wait of a feed: the coalescence over the pending frames (close: the end of the stream instead), the backtrack of
// what it decides, and their results.  Returns 2 when a symbol outside the alphabet was met (s.status, s.bad_frame).
int commit(Session& s, bool close)
{
    const hipStream_t st = s.st.s;
    const i64 pend = s.p - s.F;
    // (at close the maximum of d is wanted even where every frame is final already)
    const bool walk = (pend > 0 && s.dirty) || (close && s.p > 0);
    if (walk) {
        size_t cap = 1024;
        while ((i64)cap < pend) cap *= 2;
        if (s.d_cls.reserve(cap) || s.d_st.reserve(cap) || s.d_entered.reserve(cap) || s.h_cls.reserve(cap) || s.h_st.reserve(cap) ||
            s.h_entered.reserve(cap) || (s.matrix && (s.d_score.reserve(cap) || s.h_score.reserve(cap))))
            return 1;
        if (!s.timing) {
            HIPCHK(hipEventRecord(s.all.start.e, st));
            s.timing = true;
        }
        HIPCHK(hipEventRecord(s.commit_t.start.e, st));
        if (s.matrix) e2hmm::launch_segment_trans_coalesce(s.loop.pl, d_half(s, s.dcur), s.tring, s.F, s.p - 1, close ? 1 : 0, s.d_state.get(), st);
        else e2hmm::launch_segment_coalesce(s.loop.pl, d_half(s, s.dcur), s.ring, s.F, s.p - 1, close ? 1 : 0, s.d_state.get(), st);
        HIPCHK(hipGetLastError());
        if (s.matrix)
            e2hmm::launch_segment_trans_stream_backtrack(s.loop.pl, s.tring, s.F, s.d_state.get(), s.d_cls.get(), s.d_st.get(),
                                                         s.d_entered.get(), s.d_score.get(), st);
        else
            e2hmm::launch_segment_stream_backtrack(s.loop.pl, s.ring, s.F, s.d_state.get(), s.d_cls.get(), s.d_st.get(), s.d_entered.get(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s.commit_t.stop.e, st));
    }
    if (s.timing) HIPCHK(hipEventRecord(s.all.stop.e, st));
    if (walk) {
        HIPCHK(hipMemcpyAsync(s.h_state.get(), s.d_state.get(), sizeof(SegStreamState), hipMemcpyDeviceToHost, st));
        if (pend > 0) {
            HIPCHK(hipMemcpyAsync(s.h_cls.get(), s.d_cls.get(), (size_t)pend * 2, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(s.h_st.get(), s.d_st.get(), (size_t)pend * 2, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(s.h_entered.get(), s.d_entered.get(), (size_t)pend, hipMemcpyDeviceToHost, st));
            if (s.matrix) HIPCHK(hipMemcpyAsync(s.h_score.get(), s.d_score.get(), (size_t)pend * 8, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    if (s.timing) {
        float ms = 0.f;
        if (s.all.elapsed_ms(&ms)) return 1;
        s.kernel_ms += ms;
        if (walk) {
            if (s.commit_t.elapsed_ms(&ms)) return 1;
            s.commit_ms += ms;
        }
        s.timing = false;
    }
    s.pend_g.insert(s.pend_g.end(), s.h_g.get(), s.h_g.get() + s.g_queued);
    s.g_queued = 0;
    if (!walk) return 0;
    s.dirty = false;
    const SegStreamState& hs = *s.h_state.get();
    if (hs.status == 2) {
        s.status = 2;
        s.bad_frame = hs.bad_frame;
        return 2;
    }
    if (hs.join_bad)
        return e2vq_set_error("hmm segment %s: internal error: the frames decided from %lld on reach state %d at frame %lld, where "
                              "the previous commit ended in another", flag_of(s), (long long)s.F, hs.reached, (long long)(s.F - 1));
    if (hs.fstar >= s.F) {
        const size_t c = (size_t)(hs.fstar - s.F + 1);
        s.f_cls.insert(s.f_cls.end(), s.h_cls.get(), s.h_cls.get() + c);
        s.f_st.insert(s.f_st.end(), s.h_st.get(), s.h_st.get() + c);
        s.f_entered.insert(s.f_entered.end(), s.h_entered.get(), s.h_entered.get() + c);
        if (s.matrix) {
            s.f_g.insert(s.f_g.end(), s.h_score.get(), s.h_score.get() + c);
        } else {
            s.f_g.insert(s.f_g.end(), s.pend_g.begin(), s.pend_g.begin() + (std::ptrdiff_t)c);
            s.pend_g.erase(s.pend_g.begin(), s.pend_g.begin() + (std::ptrdiff_t)c);
        }
        s.F += (i64)c;
    }
    if (close) {
        s.log_prob = hs.logp;
        s.status = hs.status;
    }
    return 0;
}

int ring_full(const char* who, const Session& s, i64 n)
{
    if (s.matrix)
        return e2vq_set_error("%s: %lld frames are pending and %lld more do not fit the %lld that %s holds (where every price is -inf, or "
                              "the finite ones do not connect the classes, paths of different classes never meet, and nothing is decided "
                              "before close); the session can still be closed",
                              who, (long long)(s.p - s.F), (long long)n, (long long)s.C, ENV_PENDING);
    return e2vq_set_error("%s: %lld frames are pending and %lld more do not fit the %lld that %s holds (with ln_switch = -inf paths of "
                          "different classes never meet, and nothing is decided before close); the session can still be closed",
                          who, (long long)(s.p - s.F), (long long)n, (long long)s.C, ENV_PENDING);
}

int bad_symbol(const char* who, const Session& s)
{
    return e2vq_set_error("%s: the symbol at frame %lld is outside the models' alphabet of %d; the session takes no more symbols", who,
                          (long long)s.bad_frame, s.M);
}

int usable(const char* who, Session* s)
{
    if (!s) return e2vq_set_error("%s: NULL session", who);
    if (s->closed) return e2vq_set_error("%s: the session is closed", who);
    if (s->status == 2) return e2vq_set_error("%s: the session met a symbol outside the alphabet at frame %lld and takes no more symbols", who, (long long)s->bad_frame);
    return 0;
}

// room for n more pending frames within the budget: a coalescence first where frames were processed since the last one
int make_room(const char* who, Session& s, i64 n)
{
    if (s.p - s.F + n <= s.C) return 0;
    if (s.dirty) {
        const int rc = commit(s, false);
        if (rc) return rc;
    }
    return s.p - s.F + n <= s.C ? 0 : ring_full(who, s, n);
}

int stream_feed(const char* who, Session& s, const void* sym, i64 n, bool on_device)
{
    const hipStream_t st = s.st.s;
    const unsigned short* src = (const unsigned short*)sym;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const i64 B = s.B, nblk = (s.r + n) / B;
    if (!s.matrix && s.h_g.reserve((size_t)(nblk * B))) return 1;  // (empty: every feed ends with a wait)
    i64 o = 0;  // symbols of the feed taken
    int rc = 0;
    while (s.r + (n - o) >= B) {
        if ((rc = make_room(who, s, B)) != 0) break;
        const unsigned short* blk = src + o;
        if (s.r > 0 || !on_device) {  // the block is put together behind the buffered symbols
            HIPCHK(hipMemcpyAsync(s.d_blk.get() + s.r, src + o, (size_t)(B - s.r) * 2, kind, st));
            blk = s.d_blk.get();
        }
        if (queue_block(s, blk, B)) return 1;
        o += B - s.r;
        s.r = 0;
    }
    if (rc == 0 && n - o > 0) {  // the remainder waits in the session
        HIPCHK(hipMemcpyAsync(s.d_blk.get() + s.r, src + o, (size_t)(n - o) * 2, kind, st));
        s.r += n - o;
        o = n;
    }
    if (rc == 1) {  // the pending frames are full: what the processed blocks took stays, the rest of the feed is dropped
        s.fed += o;
        const std::string why = e2vq_last_error();
        HIPCHK(hipStreamSynchronize(st));
        return e2vq_set_error("%s (%lld of the feed's %lld symbols were taken)", why.c_str(), (long long)o, (long long)n);
    }
    if (rc == 0) rc = commit(s, false);  // the one coalescence and the one wait of the feed
    s.fed += rc == 2 ? n : o;
    if (rc == 2) return bad_symbol(who, s);
    return rc;
}

int stream_flush(const char* who, Session& s)
{
    if (s.r == 0) return 0;
    int rc = make_room(who, s, s.r);
    if (rc == 1) return 1;
    if (rc == 0) {
        if (!s.matrix && s.h_g.reserve((size_t)s.r)) return 1;
        if (queue_block(s, s.d_blk.get(), s.r)) return 1;
        s.r = 0;
        rc = commit(s, false);
    }
    return rc == 2 ? bad_symbol(who, s) : rc;
}

int stream_close(Session& s)
{
    if (s.status != 2) {
        if (s.r > 0) {  // (the ring's last B - 1 rows are kept for this)
            if (!s.matrix && s.h_g.reserve((size_t)s.r)) return 1;
            if (queue_block(s, s.d_blk.get(), s.r)) return 1;
            s.r = 0;
        }
        if (commit(s, true) == 1) return 1;
    }
    if (s.status == 2) {  // the frames that were not final get the fill of a stream of status 2
        const size_t c = (size_t)(s.fed - s.F);
        s.f_cls.insert(s.f_cls.end(), c, (uint16_t)0xFFFF);
        s.f_st.insert(s.f_st.end(), c, (uint16_t)0xFFFF);
        s.f_entered.insert(s.f_entered.end(), c, (uint8_t)0);
        s.f_g.insert(s.f_g.end(), c, -INFINITY);
        if (s.matrix && s.F == 0 && c > 0) s.f_g[s.f_g.size() - c] = 0.0;  // (exit_score of the absolute frame 0, as the closed decode fills it)
        s.pend_g.clear();
        s.F = s.fed;
        s.log_prob = -INFINITY;
    }
    s.closed = true;
    return 0;
}

}  // namespace

extern "C" int e2vq_hmm_segment_stream_open(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                            const double* const* Bs, double ln_switch, e2vq_segment_stream** out)
{
    const char* who = "e2vq_hmm_segment_stream_open";
    LoopModels lm;
    if (loop_check_args(who, K, Ns, pis, As, Bs, out != nullptr) || segment_check_shape(who, K, Ns) || segment_check_switch(who, ln_switch) ||
        lm.from_arrays(K, Ns, M, pis, As, Bs) || lm.logs())
        return 1;
    return stream_open(who, device, lm, ln_switch, nullptr, out);
}

// the same session under a K x K matrix of class-to-class prices; feed, flush, close, take, kernel_ms,
// stats and free above serve it
extern "C" int e2vq_hmm_segment_trans_stream_open(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                                  const double* const* Bs, const double* lt, e2vq_segment_stream** out)
{
    const char* who = "e2vq_hmm_segment_trans_stream_open";
    LoopModels lm;
    LoopBody body = LoopBody::Resident;
    if (loop_check_args(who, K, Ns, pis, As, Bs, lt != nullptr && out != nullptr) || segment_check_shape(who, K, Ns) ||
        trans_check_lt(who, K, lt) || segment_trans_body(&body) || lm.from_arrays(K, Ns, M, pis, As, Bs) || lm.logs())
        return 1;
    return stream_open(who, device, lm, 0.0, lt, out, body);
}

extern "C" int e2vq_hmm_segment_stream_feed(e2vq_segment_stream* s, const void* sym, int64_t n, int sym_on_device, int64_t* final_frames)
{
    const char* who = "e2vq_hmm_segment_stream_feed";
    if (usable(who, s)) return 1;
    if (n < 0 || (n > 0 && !sym)) return e2vq_set_error("%s: bad arguments", who);
    HIPCHK(hipSetDevice(s->device));
    const int rc = n > 0 ? stream_feed(who, *s, sym, n, sym_on_device != 0) : 0;
    if (final_frames) *final_frames = s->F;
    return rc;
}

extern "C" int e2vq_hmm_segment_stream_flush(e2vq_segment_stream* s, int64_t* final_frames)
{
    const char* who = "e2vq_hmm_segment_stream_flush";
    if (usable(who, s)) return 1;
    HIPCHK(hipSetDevice(s->device));
    const int rc = stream_flush(who, *s);
    if (final_frames) *final_frames = s->F;
    return rc;
}

extern "C" int e2vq_hmm_segment_stream_close(e2vq_segment_stream* s, double* log_prob, int* status, int64_t* final_frames)
{
    const char* who = "e2vq_hmm_segment_stream_close";
    if (!s) return e2vq_set_error("%s: NULL session", who);
    if (s->closed) return e2vq_set_error("%s: the session is closed", who);
    HIPCHK(hipSetDevice(s->device));
    if (stream_close(*s)) return 1;
    if (log_prob) *log_prob = s->log_prob;
    if (status) *status = s->status;
    if (final_frames) *final_frames = s->F;
    return 0;
}

extern "C" int e2vq_hmm_segment_stream_take(e2vq_segment_stream* s, int64_t max_frames, uint16_t* cls, uint16_t* state, uint8_t* entered,
                                            double* gbest, int64_t* first_frame, int64_t* count)
{
    if (!s) return e2vq_set_error("e2vq_hmm_segment_stream_take: NULL session");
    if (max_frames < 0) return e2vq_set_error("e2vq_hmm_segment_stream_take: bad arguments");
    const size_t c = (size_t)std::min<i64>(max_frames, s->F - s->taken);
    if (cls) std::copy(s->f_cls.begin(), s->f_cls.begin() + (std::ptrdiff_t)c, cls);
    if (state) std::copy(s->f_st.begin(), s->f_st.begin() + (std::ptrdiff_t)c, state);
    if (entered) std::copy(s->f_entered.begin(), s->f_entered.begin() + (std::ptrdiff_t)c, entered);
    if (gbest) std::copy(s->f_g.begin(), s->f_g.begin() + (std::ptrdiff_t)c, gbest);
    s->f_cls.erase(s->f_cls.begin(), s->f_cls.begin() + (std::ptrdiff_t)c);
    s->f_st.erase(s->f_st.begin(), s->f_st.begin() + (std::ptrdiff_t)c);
    s->f_entered.erase(s->f_entered.begin(), s->f_entered.begin() + (std::ptrdiff_t)c);
    s->f_g.erase(s->f_g.begin(), s->f_g.begin() + (std::ptrdiff_t)c);
    if (first_frame) *first_frame = s->taken;
    if (count) *count = (int64_t)c;
    s->taken += (i64)c;
    return 0;
}

extern "C" int e2vq_hmm_segment_stream_kernel_ms(e2vq_segment_stream* s, float* ms)
{
    if (!s || !ms) return e2vq_set_error("e2vq_hmm_segment_stream_kernel_ms: %s", s ? "bad arguments" : "NULL session");
    *ms = s->kernel_ms;
    return 0;
}

extern "C" int e2vq_hmm_segment_stream_stats(e2vq_segment_stream* s, int64_t* peak_pending, int64_t* device_bytes, float* commit_ms)
{
    if (!s) return e2vq_set_error("e2vq_hmm_segment_stream_stats: NULL session");
    if (peak_pending) *peak_pending = s->peak_pending;
    if (device_bytes) *device_bytes = s->dev_bytes + std::max<i64>(s->peak_pending, 1024) * (s->matrix ? 13 : 5);
    if (commit_ms) *commit_ms = s->commit_ms;
    return 0;
}

extern "C" void e2vq_hmm_segment_stream_free(e2vq_segment_stream* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

namespace {

// The file forms: the inputs are consecutive pieces of one recording.  Each piece is turned into symbols on its own (a .wav is
// analysed by itself: no LPC window straddles two files) and fed to one session, which is then closed.  lt: as stream_open.
struct Holder {
    Session* s = nullptr;
    ~Holder() { e2vq_hmm_segment_stream_free(s); }
};

int decode_pieces(const char* who, const LoopModels& fm, const SymInputs& si, int P, int W_ms, int O_ms, double ln_switch, const double* lt,
                  const char* name, Holder& hold, LoopBody trans_body = LoopBody::Resident)
{
    const int device = env_device();
    if (stream_open(who, device, fm, ln_switch, lt, &hold.s, trans_body)) return 1;  // (makes the device current)
    Session& s = *hold.s;
    SymStage stg;
    if (stg.open(device, si)) return 1;
    for (const SymInput& in : si.inputs) {
        int64_t T = 0;
        // (the stage waits for its stream before it returns, and a feed waits for the session's: the buffer is free again)
        if (stg.input(in, si, P, W_ms, O_ms, &T)) return 1;
        if (T > 0 && stream_feed(who, s, stg.d_sym.get(), T, true)) {
            if (s.status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d (frame %lld of %s)", in.path.c_str(), fm.M, (long long)s.bad_frame, name);
            return 1;
        }
    }
    if (stream_close(s)) return 1;
    if (s.status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d (frame %lld)", name, fm.M, (long long)s.bad_frame);
    return 0;
}

std::string csv_of(const char* csv_dir_or_file, const char* name)
{
    std::string csv = csv_dir_or_file ? csv_dir_or_file : "";
    if (!csv.empty() && !(csv.size() >= 4 && csv.compare(csv.size() - 4, 4, ".csv") == 0)) csv += std::string("/") + name + ".csv";
    return csv;
}

}  // namespace

// `hmm segment --continuous`: the report is that of the whole run.
extern "C" int e2vq_hmm_segment_continuous_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                                 const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                                 double ln_switch, const char* name, const char* csv_dir_or_file)
{
    const char* who = "e2vq_hmm_segment_continuous_files";
    FlushStdout flush_on_return;
    LoopModels fm;
    if (files_given(who, model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
    if (!name || !*name) return e2vq_set_error("%s: the recording needs a name", who);
    if (segment_check_switch(who, ln_switch) || window_ms_ok(who, W_ms, O_ms) || fm.load_checked(who, model_filenames, num_models) ||
        fm.logs(model_filenames))
        return 1;
    SymInputs si;
    if (sym_inputs_check(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, nullptr, si)) return 1;
    const std::string csv = csv_of(csv_dir_or_file, name);
    Holder hold;
    if (decode_pieces(who, fm, si, P, W_ms, O_ms, ln_switch, nullptr, name, hold)) return 1;
    const Session& s = *hold.s;
    return e2vq_hmm_segment_report(name, s.F, (int)num_models, fm.names.data(), W_ms, O_ms, s.f_cls.data(), s.f_entered.data(), s.f_g.data(),
                                   s.log_prob, ln_switch, csv.empty() ? nullptr : csv.c_str());
}

// `hmm segment --class-transitions --grammar-continuous`: the same under the transitions file, read and permuted as
// e2vq_hmm_segment_trans_files reads it; the effective price is the file's plus ln_switch.
extern "C" int e2vq_hmm_segment_trans_continuous_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                                       const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                                       double ln_switch, const char* transitions_csv, const char* name,
                                                       const char* csv_dir_or_file)
{
    const char* who = "e2vq_hmm_segment_trans_continuous_files";
    FlushStdout flush_on_return;
    LoopModels fm;
    if (files_given(who, model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
    if (!name || !*name) return e2vq_set_error("%s: the recording needs a name", who);
    if (!transitions_csv || !*transitions_csv) return e2vq_set_error("%s: no class-transitions file", who);
    if (segment_check_switch(who, ln_switch) || window_ms_ok(who, W_ms, O_ms) || fm.load_checked(who, model_filenames, num_models)) return 1;
    const int K = fm.K();
    LoopBody body = LoopBody::Resident;
    if (segment_trans_body(&body) || trans_check_slots(who, K, fm.Ns.data(), body) || check_names(who, K, fm.names.data())) return 1;
    std::vector<double> lt;
    if (transitions_read(transitions_csv, K, fm.names.data(), lt)) return 1;
    for (double& v : lt) v = v + ln_switch;  // the effective price
    if (fm.logs(model_filenames)) return 1;
    SymInputs si;
    if (sym_inputs_check(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, nullptr, si)) return 1;
    const std::string csv = csv_of(csv_dir_or_file, name);
    Holder hold;
    if (decode_pieces(who, fm, si, P, W_ms, O_ms, ln_switch, lt.data(), name, hold, body)) return 1;
    const Session& s = *hold.s;
    return e2vq_hmm_segment_trans_report(name, s.F, K, fm.names.data(), W_ms, O_ms, s.f_cls.data(), s.f_entered.data(), s.f_g.data(),
                                         s.log_prob, ln_switch, lt.data(), csv.empty() ? nullptr : csv.c_str());
}
