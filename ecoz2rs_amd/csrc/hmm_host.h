// hmm_host.h -- what the host units of the HMM consumers share (hmm_model.cpp: models, files, sequences; hmm_train.cpp:
// Baum-Welch; hmm_classify.cpp: forward scoring and the classification reports; hmm_decode.cpp: Viterbi and scan;
// hmm_class_loop.cpp: segment, its posteriors and its class-to-class prices, the body choice, slot check and forward table of
// every pass with a looped body; hmm_transitions.cpp: the file and the estimator of those prices; hmm_input.cpp: inputs to
// device symbols, label files; hmm_segment_stream.cpp: the streaming segment decoder; hmm_transcript.cpp: what the commands
// that take a transcript share; hmm_align.cpp: forced alignment; hmm_embed.cpp:
// embedded Baum-Welch on transcribed streams; hmm_align_posterior.cpp: the posteriors of the alignment; hmm_trans_train.cpp:
// Baum-Welch for the class-to-class prices; hmm_loop_train.cpp: Baum-Welch for the class models under the class loop;
// hmm_posterior_stream.cpp: the streamed class posteriors).
// The host loads files, draws the initial model, sequences the launches, takes the logarithm of the (mantissa, exponent)
// pairs the kernels return and the stopping decision, and prints the reports; every sum over states, time or sequences
// that defines a model or a score runs on the GPU (no CPU fallback: without a HIP device the entry points fail).
// Definitions (file layout, generator, scaled Baum-Welch with exact fixed-point sums, stopping rule): this repo's own,
// written down in oracle/hmm_oracle.h and DESIGN.md.  Internal.
#pragma once
#include "../../include/ecoz2_classify.h"
#include "../../include/ecoz2_vq.h"
#include "hip_host.h"
#include "hmm_device.h"
#include "host_util.h"
#include "vq_io.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <map>
#include <string>
#include <vector>

namespace e2hmm_host {
using namespace e2hip;
using namespace e2host;
using e2hmm::ModelDev;
typedef long long i64;

// ---- model (hmm_model.cpp) -----------------------------------------------------------------------------------------
extern uint64_t g_rng;  // the generator's state (ecoz2_set_random_seed); hmm_init draws from it

struct Hmm {
    std::string class_name;
    int N = 0, M = 0;
    std::vector<double> pi, A, B;
    void resize(int n, int m)
    {
        N = n;
        M = m;
        pi.assign((size_t)n, 0.0);
        A.assign((size_t)n * n, 0.0);
        B.assign((size_t)n * m, 0.0);
    }
    // pi | A | B as one flat block of params() doubles: how every device parameter buffer holds a model
    size_t params() const { return pi.size() + A.size() + B.size(); }
    void pack(double* q) const
    {
        std::copy(pi.begin(), pi.end(), q);
        std::copy(A.begin(), A.end(), q + pi.size());
        std::copy(B.begin(), B.end(), q + pi.size() + A.size());
    }
    void unpack(const double* q)
    {
        std::copy(q, q + pi.size(), pi.begin());
        std::copy(q + pi.size(), q + pi.size() + A.size(), A.begin());
        std::copy(q + pi.size() + A.size(), q + params(), B.begin());
    }
    // the model as the device sees it, its block at `base`
    ModelDev dev(const double* base) const { return ModelDev{N, M, base, base + N, base + N + (size_t)N * N}; }
};

// the shapes a model may have
inline bool shape_ok(int N, int M) { return N >= 1 && N <= e2hmm::MAX_N && M >= 1 && M <= 65536; }

int hmm_init(Hmm& h, int type);
int hmm_save(const std::string& path, const Hmm& h);
int hmm_load(const char* path, Hmm& h);
int load_models(const char* const* files, unsigned n, std::vector<Hmm>& models);
int log_model(const Hmm& h, std::vector<double>& flat);
// a model from the caller's arrays and back
int model_from_arrays(int N, int M, const double* pi, const double* A, const double* B, Hmm& h);
void model_to_arrays(const Hmm& h, double* pi, double* A, double* B);
// K models of one M from per-model arrays; ms: pointers to them
int models_from_arrays(int K, const int* Ns, int M, const double* const* pis, const double* const* As, const double* const* Bs,
                       std::vector<Hmm>& models, std::vector<const Hmm*>& ms);

// natural log of mant * 2^exp2 (oracle: e2h_log_prob)
inline double log_prob(double mant, i64 exp2)
{
    if (!(mant > 0.0)) return -INFINITY;
    return log(mant) + (double)exp2 * M_LN2;
}

// a byte budget from the environment, at least 1
inline i64 env_bytes(const char* name, i64 dflt)
{
    const char* v = getenv(name);
    return std::max<i64>(v && *v ? atoll(v) : dflt, 1);
}

// ---- sequences (hmm_model.cpp) -------------------------------------------------------------------------------------
struct SeqSet {
    std::vector<std::string> files, classes;
    std::vector<uint16_t> sym;  // concatenated
    std::vector<i64> offs;      // S + 1
    int M = -1;                 // codebook size (all equal, unless loaded with mixed_M)
    std::vector<int> Ms;        // each file's codebook size
    int S() const { return (int)files.size(); }
};

// mixed_M: files of different codebook sizes are accepted (ss.M is then the first file's)
int load_sequences(const char* const* files, unsigned n, SeqSet& ss, bool mixed_M = false);
// S + 1 offsets that start at 0 and never decrease (the kernels index the symbols with them)
int check_offsets(const int64_t* offs, int S);

// Host sequences on the device, and the stream the call works on.  The symbols are uploaded, or the caller's device
// pointer is adopted; nothing here synchronises.  Declare it after every buffer and host mirror the stream's work
// touches (a Trainer, a Scores): its Stream then waits before they are released (see Stream).
struct DevSeqs {
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<i64> d_offs;
    std::vector<i64> h_offs;              // of a slice: its offsets, from 0
    const unsigned short* sym = nullptr;  // d_sym, or the adopted pointer
    Stream st;                            // (after the buffers: see Stream)
    // the stream and n symbols alone (the offsets stay with the caller)
    int symbols(const void* src, size_t n, bool on_device = false)
    {
        if (st.create()) return 1;
        if (!on_device && d_sym.upload((const unsigned short*)src, n, st.s)) return 1;
        sym = on_device ? (const unsigned short*)src : d_sym.get();
        return 0;
    }
    // for an array-level entry point: the offsets checked and the device made current, then symbols()
    int open(int device, const void* src, const int64_t* offs, int S, bool on_device)
    {
        return check_offsets(offs, S) || require_device(device) || symbols(src, (size_t)offs[S], on_device);
    }
    // S whole sequences
    int upload(const uint16_t* src, const i64* offs, int S) { return symbols(src, (size_t)offs[S]) || d_offs.upload(offs, (size_t)S + 1, st.s); }
    // the sequences [s0, s1) of a set
    int upload_slice(const SeqSet& ss, i64 s0, i64 s1)
    {
        const i64 a = ss.offs[(size_t)s0];
        for (i64 i = s0; i <= s1; ++i) h_offs.push_back(ss.offs[(size_t)i] - a);
        return upload(ss.sym.data() + a, h_offs.data(), (int)(s1 - s0));
    }
};

// ---- many models at once -------------------------------------------------------------------
// The sequences a batch's models work on: host symbols and S + 1 offsets from 0.  Each model takes a range of them; the
// models of different N of one class and M share theirs, the classes of `--all-classes` have disjoint ones.
struct SeqStore {
    const uint16_t* sym = nullptr;
    const i64* offs = nullptr;
};

// The sequences of one batch (of trainings or of scorings): the jobs' ranges [s_lo, s_hi) of the store merged into
// disjoint runs that follow one another, so that a sequence goes to the device once however many jobs use it.
struct BatchSeqs {
    std::vector<std::pair<int, int>> merged;  // the runs, as ranges of the store, ascending
    std::vector<int> run_at;                  // batch index of each run's first sequence
    std::vector<i64> offs;                    // the batch's sequences: their symbol offsets, from 0
    BatchSeqs(std::vector<std::pair<int, int>> ranges, const SeqStore& ss);
    int local(int s) const;  // batch index of the store's sequence s (one of a range given)
    int upload_symbols(const SeqStore& ss, unsigned short* d_sym, hipStream_t st) const;  // d_sym: offs.back() symbols
};

// the checks the array-level grid entry points make of model k; then: the (offset, end) ranges of `what` do not overlap
int grid_model_check(int k, int N, int M, i64 seq_lo, i64 seq_hi, int S, i64 param_off);
int check_disjoint(std::vector<std::pair<i64, i64>> ranges, const char* what);

// ---- scores (hmm_classify.cpp) -----------------------------------------------------------------------------------------
// P(O) = mant * 2^exp2 and the status of scored sequences: the device slots the kernels fill and their host mirrors
// (Host: HostVec, or PinnedBuffer where the copy back must not wait for the host).  reserve() makes the device slots
// only; the host mirrors are made by download(), after the launches, so that a large result set is allocated while the
// kernels run -- or ahead of time by reserve_host(), which pinned mirrors need.
template <typename T>
struct HostVec {
    std::vector<T> v;
    int reserve(size_t n) { return v.resize(std::max(n, v.size())), 0; }
    T* get() { return v.data(); }
    const T* get() const { return v.data(); }
};
template <template <typename> class Host>
struct ScoresT {
    DeviceBuffer<double> d_mant;
    DeviceBuffer<i64> d_exp;
    DeviceBuffer<int> d_status;
    Host<double> mant;
    Host<i64> exp2;
    Host<int> status;
    int reserve(size_t n) { return d_mant.reserve(n) || d_exp.reserve(n) || d_status.reserve(n); }
    int reserve_host(size_t n) { return mant.reserve(n) || exp2.reserve(n) || status.reserve(n); }
    // enqueues the copy of the first n results to the host mirrors (the caller synchronises)
    int download(size_t n, hipStream_t st)
    {
        if (reserve_host(n)) return 1;
        if (!n) return 0;
        HIPCHK(hipMemcpyAsync(mant.get(), d_mant.get(), n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(exp2.get(), d_exp.get(), n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(status.get(), d_status.get(), n * 4, hipMemcpyDeviceToHost, st));
        return 0;
    }
    bool ok(size_t i) const { return status.get()[i] == 0; }
    // natural log; -inf when the model cannot emit the sequence or a symbol is outside its alphabet
    double log_prob(size_t i) const { return ok(i) ? e2hmm_host::log_prob(mant.get()[i], exp2.get()[i]) : -INFINITY; }
    // result i into the caller's arrays (any may be null)
    void get(size_t i, double* m, int64_t* e, int* s, double* lp) const
    {
        if (m) *m = mant.get()[i];
        if (e) *e = exp2.get()[i];
        if (s) *s = status.get()[i];
        if (lp) *lp = log_prob(i);
    }
    // status and natural log of the first n results into the caller's arrays (either may be null)
    void get_all(size_t n, int* s, double* lp) const
    {
        for (size_t i = 0; i < n; ++i) get(i, nullptr, nullptr, s ? s + i : nullptr, lp ? lp + i : nullptr);
    }
};
typedef ScoresT<HostVec> Scores;

struct DevModels {  // a set of models on the device
    DeviceBuffer<double> params;  // all pi | A | B, model after model
    DeviceBuffer<ModelDev> table;
    std::vector<ModelDev> host;
    int maxN = 0;
    int upload(const std::vector<const Hmm*>& ms, hipStream_t st);
};

// scores of S device-resident sequences under K models: sc[s * K + k]
int score_device(const std::vector<const Hmm*>& ms, const unsigned short* d_sym, const i64* d_offs, int S, hipStream_t st, Scores& sc);

// ---- decoding: what hmm_decode.cpp, hmm_class_loop.cpp, hmm_segment_stream.cpp and hmm_transcript.cpp share ------------
// The launches of a decoder whose table takes `row` bytes a frame: whole sequences [s0, s1) up to the budget of the
// environment variable `env` (default 256 MiB), a longer sequence alone; *max_frames: the most frames of a launch
// (hmm_decode.cpp)
std::vector<std::pair<int, int>> plan_chunks(const char* env, i64 row, const i64* hoffs, int S, i64* max_frames);

// the body of every e2vq_*_last_kernel_ms export
inline int last_kernel_ms(const char* who, float value, float* ms)
{
    if (!ms) return e2vq_set_error("%s: bad arguments", who);
    *ms = value;
    return 0;
}

// the first refusals of an array-level entry point over K models (scan and the class loop): K >= 1, then the arrays (`rest`: the entry point's own pointers and counts)
int loop_check_args(const char* who, int K, const int* Ns, const double* const* pis, const double* const* As, const double* const* Bs,
                    bool rest);
// S >= 0, and symbols wherever the offsets count any
inline bool syms_given(const void* sym, const int64_t* offs, int S) { return S >= 0 && !(!sym && S > 0 && offs && offs[S] > 0); }

// the refusals every file form opens with, and the one of its frame geometry
inline int files_given(const char* who, const void* models, unsigned num_models, bool inputs)
{
    if (!models || num_models < 1) return e2vq_set_error("%s: no models", who);
    if (!inputs) return e2vq_set_error("%s: no inputs", who);
    return 0;
}
inline int window_ms_ok(const char* who, int W_ms, int O_ms)
{
    return W_ms < 1 || O_ms < 1 ? e2vq_set_error("%s: window %d ms / offset %d ms", who, W_ms, O_ms) : 0;
}

// the per-frame table of an input in `dir`: <dir>/<the input's name without directory and extension>.csv; frames_csv_distinct:
// no two inputs may share one ("%s and %s would both write %s"; dir empty: no table is written, nothing is refused)
std::string frames_csv_path(const std::string& dir, const char* input_filename);
int frames_csv_distinct(const std::string& dir, const char* const* input_filenames, int num_inputs);

// The models of `hmm scan` / `hmm segment`: loaded, all of one M
struct FilesModels {
    std::vector<Hmm> models;
    std::vector<const Hmm*> ms;
    std::vector<const char*> names;  // the classes'
    int M = 0;
    int load(const char* const* files, unsigned n)
    {
        if (load_models(files, n, models)) return 1;
        M = models[0].M;
        for (unsigned k = 0; k < n; ++k) {
            if (models[k].M != M) return e2vq_set_error("%s: model has M=%d but %s has M=%d", files[k], models[k].M, files[0], M);
            ms.push_back(&models[k]);
            names.push_back(models[k].class_name.c_str());
        }
        return 0;
    }
};

// ---- the class loop (hmm_class_loop.cpp): what `hmm segment` in all its forms and `hmm align` share ---------------------
// the shapes and the price the class loop takes (`who`: the entry point named in the message)
int segment_check_shape(const char* who, int K, const int* Ns);
int segment_check_switch(const char* who, double ln_switch);

// The models of a class-loop call, all of one M, from the caller's arrays or from files (then with `names`): their N and,
// once logs() has run, log_model of each.  The checks between these steps stay with the entry point, in its own order.
struct LoopModels : FilesModels {
    std::vector<int> Ns;
    std::vector<std::vector<double>> lflats;
    int K() const { return (int)ms.size(); }
    int from_arrays(int K, const int* Ns, int M, const double* const* pis, const double* const* As, const double* const* Bs);
    int load_checked(const char* who, const char* const* files, unsigned n);  // load(), then segment_check_shape
    int logs(const char* const* files = nullptr);  // files: a failure is prefixed with the model's file name
};

// where the trainers that re-estimate given models write them: <out_dir>/<class>.hmm for every class of fm, in class order; a
// path that names an input model's file is refused ("%s would overwrite an input model")
int model_out_paths(const char* who, const char* out_dir, const LoopModels& fm, const char* const* model_filenames, unsigned num_models,
                    std::vector<std::string>& out_paths);

// The packing of the classes into wave-slots of 64 lanes that the class-loop decoders share: class after class, a class
// that does not fit the open slot opens the next.  a_ld(N): the leading dimension of a class's A in the device block
// (a_at / a_words count N x a_ld(N) words a class).
struct SegPacking {
    int sumN = 0, a_words = 0, slots = 0;
    std::vector<int> comp0, a_at;            // [K]: composite index of state 0, offset of A
    std::vector<int> slot_info;              // [slots][2]: the largest N of the slot, 1 when the slot holds one class
    std::vector<e2hmm::SegLaneDev> lanes;    // [slots][64]
    std::vector<uint16_t> comp_cls;          // [sumN]
};
inline int a_ld_dense(int N) { return N; }  // A as N x N
SegPacking pack_slots(const std::vector<int>& Ns, int (*a_ld)(int) = a_ld_dense);

// the logarithms as the Viterbi kernels of the class loop read them: lpi of every class | lA of every class | lB of every
// class, each class at its place in `pk` (a packing of the classes with a_ld(N) = N)
std::vector<double> loop_log_params(const LoopModels& lm, const SegPacking& pk);
// the body of a class-loop kernel: looped where `slots` exceed a workgroup's waves or the variable `env_name` says
// "looped" (slots = 0: whether it says so); a value other than "resident" or "looped" is refused
int loop_body_looped(const char* env_name, int slots, bool* looped);

// The body of a pass whose looped kernel is opt-in: resident (more than 16 wave-slots are refused), looped, or resident up to
// 16 slots and looped above.  opt_in_body is the one reader of the variables: unset, empty or "resident" / "looped" / "auto" of
// `env_name` -> *body; any other value is refused with "<env_name>=<v>: auto, resident or looped".  The five readers below name
// their variable; each entry point calls its reader once.  runs_looped: whether a packing (or a transcript) of `slots` runs the
// looped kernels under `body`.  body_waves: the waves of a workgroup, each of which stores its copy of c_t.
enum class LoopBody { Resident, Looped, Auto };
int opt_in_body(const char* env_name, LoopBody* body);
bool runs_looped(LoopBody body, int slots);
int body_waves(bool looped, int slots);
int embed_body(LoopBody* body);          // ECOZ2_HMM_EMBED_BODY: the E-step of `hmm learn --embedded`
int align_post_body(LoopBody* body);     // ECOZ2_HMM_ALIGN_POSTERIOR_BODY: `hmm align --posteriors` (4.8.12)
int posteriors_body(LoopBody* body);     // ECOZ2_HMM_POSTERIOR_BODY: `hmm segment --posteriors` (4.8.7)
int segment_trans_body(LoopBody* body);  // ECOZ2_HMM_SEGMENT_TRANS_BODY: `--class-transitions` and its session (4.8.8 / 4.8.15)
// ECOZ2_HMM_TRANS_FB_BODY: `--grammar-posteriors` (4.8.13) and the E-step of `hmm transitions --em` (4.8.14);
// e2vq_hmm_segment_trans_posteriors, e2vq_hmm_segment_trans_files_posteriors (whose decode follows the same choice),
// e2vq_hmm_transitions_estep, e2vq_hmm_train_transitions and e2vq_hmm_learn_transitions_files read it, and nothing else does
int trans_fb_body(LoopBody* body);

// the shape of a packing as the *_lds_bytes and *_layout functions of hmm_device.h read it (no table, no device pointer)
e2hmm::SegPlanDev loop_shape(const SegPacking& pk, int K, int M = 0);
// The slot check of a pass that has a looped body (host only).  Resident: more than 16 slots are refused, word for word as
// before the looped body existed (`resident_has` closes that message).  Looped: `looped_lds`, the mandatory LDS bytes of the
// looped body for this shape, must fit -- with segment_check_shape's caps they always do; the check stands for the day a cap
// moves.  `looped_of` names the looped body in that refusal; classes: the pass runs under class-to-class prices and the refusal
// counts the K classes too.
int check_body_slots(const char* who, const SegPacking& pk, int K, LoopBody body, const char* resident_has, const char* looped_of,
                     size_t looped_lds, bool classes = true);
// that check for the decoder under class-to-class prices (`hmm segment --class-transitions` and its session, DESIGN.md 4.8.8 /
// 4.8.15; body: what segment_trans_body gave, or trans_fb_body where the decode follows the posteriors)
int trans_check_slots(const char* who, int K, const int* Ns, LoopBody body);
// and for the sum-product pass under the one price (`hmm segment --posteriors`, DESIGN.md 4.8.7, and the posterior session of
// hmm_posterior_stream.cpp, 4.8.17; body: what posteriors_body gave)
int posteriors_check_slots(const char* who, int K, const int* Ns, LoopBody body);
// the K x K prices transposed, ltT[k * K + f] = lt[f * K + k]: a lane of class k walks its sources along consecutive words
std::vector<double> trans_transposed(int K, const double* lt);

// A packing on the device: the parameter block, the four tables of `pk`, and the plan the kernels take.  upload() only
// enqueues: the host vectors must outlive the stream's copies, and this struct the stream's kernels (a local is declared
// before the DevSeqs / Stream whose stream works on it, or the function waits for that stream before it returns).
struct ClassLoopDev {
    DeviceBuffer<double> params;
    DeviceBuffer<e2hmm::SegLaneDev> lanes;
    DeviceBuffer<int> slot_info, comp0;
    DeviceBuffer<unsigned short> comp_cls;
    e2hmm::SegPlanDev pl{};
    i64 bytes = 0;  // of the five buffers
    int upload(const SegPacking& pk, const std::vector<double>& host_params, int K, int M, hipStream_t st);
};

// The forward table of a sum-product pass through the class loop (hmm_class_loop.cpp: --posteriors, --grammar-posteriors;
// hmm_trans_train.cpp; hmm_loop_train.cpp): per frame ah (sumN doubles), c (one double a wave) and, where the pass keeps one,
// a third array of `extra` doubles (the loop trainer's m_t, K a frame).  reserve() cuts the S streams of h_offs into launches
// of whole streams whose rows of 8 (sumN + waves + extra) bytes stay within ECOZ2_HMM_POSTERIOR_CHUNK_BYTES (plan_chunks) and
// makes room for the largest; a failure is refused as "<prefix>: no room for the forward table of ...".
struct ForwardTable {
    DeviceBuffer<double> d_ah, d_c, d_x;
    std::vector<std::pair<int, int>> chunks;
    i64 max_frames = 0;
    int reserve(const char* prefix, int sumN, int waves, int extra, const i64* h_offs, int S);
};

// What the sum-product passes under class-to-class prices share (hmm_class_loop.cpp: --grammar-posteriors;
// hmm_trans_train.cpp: transitions --em; hmm_loop_train.cpp: learn --loop).  check_resident: where only the resident layout
// exists, a packing of more than 16 slots is refused (`what_has` closes the message).  posteriors_a_ld: the leading dimension
// N | 1 of a class's A.
// posteriors_check_params: a negative, NaN or infinite parameter is refused.  trans_check_lt: every price <= 0 or -inf.
// trans_prices: w = exp(lt) and its transpose.  trans_params: pi | A (N | 1) | B at the places of `pk`.
int check_resident(const char* who, int slots, const char* what_has);
int posteriors_a_ld(int N);
int posteriors_check_params(const Hmm& h);
int trans_check_lt(const char* who, int K, const double* lt);
std::vector<double> trans_prices(int K, const double* lt);
std::vector<double> trans_params(const LoopModels& lm, const SegPacking& pk);
// (hmm_trans_train.cpp) alpha: finite and at least 0.  trans_mstep: the M-step of 4.8.14 on the host -- row f of ln_p (K x K) from
// the 2 K^2 limb words of acc; a -inf entry stays, a row without mass keeps its bytes.
int trans_check_alpha(const char* who, double alpha);
void trans_mstep(int K, const i64* acc, double alpha, double* ln_p);

// ---- transcripts (hmm_transcript.cpp): what `hmm align`, `hmm learn --embedded` and `hmm align --posteriors` share --------
// What the host decides about a call before the device is touched: the packing of every stream's units, the device tables
// that describe it, and the launches (consecutive streams of one body whose tables and LDS fit together).
struct AlignPlan {
    std::vector<e2hmm::AlignStreamDev> streams;  // tab_at: relative to the first stream of its launch
    std::vector<e2hmm::AlignLaneDev> lanes;
    std::vector<int> slot_info, unit_comp0;
    std::vector<uint16_t> comp_unit;
    struct Launch {
        int s0, s1, waves, max_L, max_sumN;
        bool looped;
        i64 bytes;
    };
    std::vector<Launch> launches;
    i64 max_bytes = 0;
    SegPacking cls;  // the classes: their rows in the parameter block (comp0, a_at, sumN, a_words)
};
// the checks of the transcripts and the price, the packing and the launches: host only (`who`: the entry point named in
// the messages).  embedded: the caller is the embedded forward-backward pass -- every refusal stays (the bound of
// ECOZ2_HMM_ALIGN_TABLE_BYTES on a stream too, worded for a caller without back-pointers), but ECOZ2_HMM_ALIGN_BODY is not
// read and no launches are cut.  own_looped_lds: the caller has a looped body of its own and holds a stream of more than 16
// slots against that body's LDS sum, not against k_hmm_align's
int align_plan(const char* who, int K, const int* Ns, const i64* offs, int S, const int32_t* units, const i64* unit_offs,
               const uint8_t* optional, double ln_switch, AlignPlan& ap, bool embedded = false, bool own_looped_lds = false);
// may unit l hold frame 0 / the last frame (opt: the stream's flags, or null)
bool unit_is_initial(int l, const uint8_t* opt);
bool unit_is_final(int l, int L, const uint8_t* opt);

// the first checks of an array-level entry point that takes transcripts: the arguments, the shapes, the models (into lm, with
// their logarithms) and the offsets
int transcript_check_args(const char* who, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                          const double* const* Bs, const void* sym, const int64_t* offs, int S, const int32_t* units,
                          const int64_t* unit_offs, LoopModels& lm);

// The transcripts of a file form: the labels of each file in their order, the filler (an optional unit) around and between
// them.  File f's units are units.data() + unit_offs[f], unit_offs[f + 1] - unit_offs[f] of them.
struct Transcripts {
    std::vector<int32_t> units;
    std::vector<uint8_t> optional;
    std::vector<i64> unit_offs = std::vector<i64>(1, 0);
    int filler = -1;  // the filler's class, or -1
    int set_filler(const char* who, const LoopModels& fm, const char* filler_class);  // null or empty: none
    int add_labels(const char* who, const LoopModels& fm, const char* path);          // the next file's
    const int32_t* u(int f) const { return units.data() + unit_offs[(size_t)f]; }  // file f's
    const uint8_t* o(int f) const { return optional.data() + unit_offs[(size_t)f]; }
    i64 L(int f) const { return unit_offs[(size_t)f + 1] - unit_offs[(size_t)f]; }
};

// The plan of the embedded forward-backward pass (hmm_embed.hip, hmm_align_posterior.hip): align_plan's packing of every
// stream with the successor flags, the classes' A at the leading dimension N | 1, what ECOZ2_HMM_EMBED_A says and the
// launches.  Whether A goes to LDS is the caller's decision (a_lds; each kernel has its own LDS sum).
// The body of a stream (hmm_embed.hip / hmm_embed_looped.hip) is the caller's choice: resident for every stream (more than 16
// wave-slots are refused), looped for every stream, or resident up to 16 slots and looped above.  A launch has one body:
// the launches of plan_chunks are cut further where the body changes and where the looped streams' largest shapes no longer
// fit LDS together.
struct EStepPlan {
    AlignPlan ap;
    SegPacking cls;                              // the classes, A with the leading dimension N | 1
    std::vector<e2hmm::EmbedClassDev> classes;   // N and a_at; the caller's own places are 0
    std::vector<uint16_t> row_cls;
    i64 row_words = 0, max_frames = 0;
    int M = 0, max_L = 0, max_slots = 0;         // max_*: over the streams of the resident body
    bool a_forced = false, a_lds = false;        // ECOZ2_HMM_EMBED_A is set; A in LDS
    std::vector<std::pair<int, int>> chunks;
    std::vector<uint8_t> looped;                 // [S]: the stream's body
    struct Shape {                               // of a launch of the looped body: the largest among its streams
        bool looped = false;
        int max_L = 0, max_slots = 0, max_sumN = 0;
    };
    std::vector<Shape> shapes;                   // per chunk
};
// `what` closes the refusal of a stream of more than 16 wave-slots that would run resident; first_flags: EMBED_FIRST on a
// class's first unit; body: the caller's choice (the embedded E-step: what embed_body gave; the alignment posteriors: what
// align_post_body gave), held against each stream's slots; looped_unit_bytes: what the caller's looped body keeps in LDS per unit
// on top of embed_looped_lds_bytes' mandatory part (the alignment posteriors: the three per-unit sums), counted wherever a looped
// stream or launch is held against LDS
int estep_plan(const char* who, int K, const int* Ns, int M, const i64* offs, int S, const int32_t* units, const i64* unit_offs,
               const uint8_t* optional, double ln_switch, const char* what, bool first_flags, LoopBody body, EStepPlan& p,
               size_t looped_unit_bytes = 0);
// "lds" / "global" / unset of the variable `name` -> *forced (whether it is set) and *lds; any other value is refused
int embed_route(const char* name, bool* forced, bool* lds);
// pi of every class | e = sw pi | A of every class, row i at i (N | 1) | B of every class
std::vector<double> embed_params(const LoopModels& lm, const SegPacking& pk, double sw);

// An EStepPlan on the device: its six tables and the forward tables' scratch.  upload() only enqueues: the plan and the
// offsets must outlive the stream's copies, and this struct the stream's kernels (a local or member declared before the
// DevSeqs / SymStage whose stream works on it, or the function waits for that stream before it returns).
struct EStepDev {
    DeviceBuffer<e2hmm::AlignLaneDev> lanes;
    DeviceBuffer<e2hmm::AlignStreamDev> streams;
    DeviceBuffer<int> slot_info;
    DeviceBuffer<e2hmm::EmbedClassDev> classes;
    DeviceBuffer<unsigned short> row_cls;
    DeviceBuffer<i64> offs;
    DeviceBuffer<double> scr;
    int upload(const EStepPlan& p, const i64* h_offs, int S, hipStream_t st);
    int scratch(const char* who, const EStepPlan& p);  // room for the largest launch
    // what a kernel takes for the launch that starts at stream s0 (offs.get() + s0 are its offsets)
    e2hmm::EmbedPlanDev plan(const EStepPlan& p, int s0, const double* d_params) const;
};

// the reports of `hmm align`: the validation both share (`rest`: the caller's own pointers) -> the optional units passed
// over, or -1; the time in seconds of frame * O_ms + W_ms; a visited unit's score; the header line and the per-class counts
int align_report_check(const char* who, const char* name, int64_t T, int K, const char* const* class_names, int L, const int32_t* units,
                       const uint8_t* optional, const int64_t* begin, const int64_t* end, const double* score, bool rest);
inline double align_time_s(int64_t frame, int O_ms, int W_ms = 0) { return (double)(frame * O_ms + W_ms) / 1000.0; }
inline double align_unit_score(const double* score, const int64_t* begin, const int64_t* end, int l, double ln_switch)
{
    return score[end[l] - 1] - (begin[l] == 0 ? 0.0 : score[begin[l] - 1] + ln_switch);
}
void align_report_head(const char* name, int64_t T, int K, const char* const* class_names, int L, const int32_t* units,
                       const int64_t* begin, const int64_t* end, int skipped, double log_prob, double ln_switch);

inline std::string fmt_17g(double v)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

inline bool ends_with(const std::string& s, const char* ext)
{
    const size_t n = strlen(ext);
    return s.size() >= n && s.compare(s.size() - n, n, ext) == 0;
}

// ---- the transitions file (hmm_transitions.cpp) -----------------------------------------------------------------------------
// class names that can head its columns: K >= 1 of them, none empty or with a separator, no two equal
int check_names(const char* who, int K, const char* const* names);
// the file's matrix in the order of `names` (the models' classes): lt[f * K + k], each value <= 0 or -inf
int transitions_read(const char* path, int K, const char* const* names, std::vector<double>& lt);

// ---- inputs (hmm_input.cpp) -------------------------------------------------------------------------------------------------
std::vector<std::string> split_on(const std::string& s, char sep);
// the lines of a text file without their line ends; a last line without one counts, trailing empty lines do not
int read_lines(const char* path, std::vector<std::string>& lines);

// The labelled units of one file, in their order: a segment CSV (column `class`, in row order) or a tab-separated selection
// table (column `Type`, sorted by `Begin Time (s)`; equal times keep their row order).  The first line that is no '#'
// comment is the header.  `hmm transitions` counts their successions, `hmm align` aligns to them.
struct LabelRow {
    std::string label;
    size_t line;  // of the file, from 1
};
int read_label_file(const char* path, std::vector<LabelRow>& rows);

// input -> device symbols: the stage `hmm scan`, `hmm segment` and `hmm align` share
struct SymInput {
    std::string path, csv;
    int kind = 0;  // 0 .wav, 1 .prd, 2 .seq
    int sample_rate = 0;
    int64_t samples = 0, T = 0;
};
struct SymInputs {
    bool have_cb = false, need_cb = false;
    int cbP = 0, cbM = 0;
    std::vector<double> refl;
    std::vector<SymInput> inputs;
};
// the checks of the inputs against the models' M and the codebook, and the codebook itself: host only, no file written
int sym_inputs_check(const char* who, int M, const char* cb_filename, const char* const* input_filenames, int num_inputs, int P,
                     int W_ms, int O_ms, const char* csv_dir_or_file, SymInputs& si);
struct VqSessionHolder {
    e2vq_session* s = nullptr;
    ~VqSessionHolder()
    {
        if (s) e2vq_session_destroy(s);
    }
};
// The device side of the inputs of one call: the buffers they reuse (the symbols of the current input in d_sym), the
// stream, and the quantize session where an input needs the codebook.
struct SymStage {
    DeviceBuffer<double> d_frames;
    DeviceBuffer<int32_t> d_status;
    DeviceBuffer<unsigned short> d_sym;
    int device = 0;
    Stream st;  // (after the buffers: see Stream)
    VqSessionHolder vq;
    // the stream and the session on `device`, which the caller has made current (require_device)
    int open(int device, const SymInputs& si);
    // one input to symbols in d_sym (read and uploaded once; frames and symbols stay on the device): *T_out of them.
    // Waits for the stream before it returns.
    int input(const SymInput& in, const SymInputs& si, int P, int W_ms, int O_ms, int64_t* T_out);
    // every input to symbols, one after the other, gathered in one device buffer: d_all holds them all, offs their
    // num_inputs + 1 offsets from 0 (the trainers over whole streams: an E-step is then one call)
    int gather(const char* who, const SymInputs& si, int P, int W_ms, int O_ms, DeviceBuffer<unsigned short>& d_all, std::vector<i64>& offs);
};
// What the commands that work input by input do once their own checks have passed (`who`: the entry point): the check of
// the inputs and the codebook against M, still on the host alone; then one SymStage, and for every input its symbols on
// the device followed by the command's work on them, run(input, T, d_sym, stream).
int run_on_files(const char* who, int M, const char* cb_filename, const char* const* input_filenames, int num_inputs, int P, int W_ms,
                 int O_ms, const char* csv_dir_or_file,
                 const std::function<int(const SymInput&, int64_t, const unsigned short*, hipStream_t)>& run);

}  // namespace e2hmm_host
