// hmm_class_loop.cpp -- the class loop of all models on the GPU: the joint Viterbi through it (`hmm segment`, DESIGN.md
// 4.8.6, hmm_segment.hip), the class posteriors under it (`--posteriors`, 4.8.7, hmm_posterior.hip) and the same loop under
// a matrix of class-to-class prices (`--class-transitions`, 4.8.8, hmm_segment_trans.hip and, above 16 wave-slots or on
// request, hmm_segment_trans_looped.hip: ECOZ2_HMM_SEGMENT_TRANS_BODY) with the posteriors under that
// matrix (`--grammar-posteriors`, 4.8.13, hmm_posterior_trans.hip and, above 16 wave-slots or on request,
// hmm_posterior_trans_looped.hip: ECOZ2_HMM_TRANS_FB_BODY), with their reports and their
// array and file entry points (one file form, segment_files, for all four of them); and what every class-loop pass shares
// (hmm_host.h): the shape checks, the packing into wave-slots, the models with their logarithms, the parameter block, the
// device side of a packing, and for the passes with a looped body the choice of the body (LoopBody, opt_in_body, runs_looped,
// body_waves), the slot check (check_body_slots) and the forward table (ForwardTable).
#include "hmm_host.h"

namespace e2hmm_host {

int segment_check_shape(const char* who, int K, const int* Ns)
{
    if (K < 1) return e2vq_set_error("%s: %d models (at least 1)", who, K);
    i64 sum = 0;
    for (int k = 0; k < K; ++k) {
        if (Ns[k] < 1 || Ns[k] > e2hmm::SEG_MAX_N)
            return e2vq_set_error("%s: model %d has N=%d states (1 .. %d)", who, k, Ns[k], e2hmm::SEG_MAX_N);
        sum += Ns[k];
    }
    if (sum > e2hmm::SEG_MAX_SUM_N)
        return e2vq_set_error("%s: %lld states in all models (at most %d)", who, (long long)sum, e2hmm::SEG_MAX_SUM_N);
    return 0;
}

int segment_check_switch(const char* who, double ln_switch)
{
    if (std::isnan(ln_switch) || ln_switch > 0.0)
        return e2vq_set_error("%s: ln_switch = %g: the logarithm of a price, at most 0 (-inf forbids a new segment)", who, ln_switch);
    return 0;
}

SegPacking pack_slots(const std::vector<int>& Ns, int (*a_ld)(int))
{
    SegPacking pk;
    const int K = (int)Ns.size();
    pk.comp0.resize((size_t)K);
    pk.a_at.resize((size_t)K);
    for (int k = 0; k < K; ++k) {
        pk.comp0[(size_t)k] = pk.sumN;
        pk.a_at[(size_t)k] = pk.a_words;
        pk.sumN += Ns[(size_t)k];
        pk.a_words += Ns[(size_t)k] * a_ld(Ns[(size_t)k]);
    }
    pk.comp_cls.resize((size_t)pk.sumN);
    int fill = 64;  // lanes taken of the current slot (64: none is open)
    for (int k = 0; k < K; ++k) {
        const int N = Ns[(size_t)k];
        if (fill + N > 64) {
            const int l0 = (int)pk.lanes.size();
            pk.lanes.resize((size_t)l0 + 64);
            for (int l = 0; l < 64; ++l) pk.lanes[(size_t)(l0 + l)] = e2hmm::SegLaneDev{-1, 0, 0, l, 0, 0};
            pk.slot_info.push_back(0);
            pk.slot_info.push_back(0);
            fill = 0;
        }
        const size_t l0 = pk.lanes.size() - 64;
        for (int j = 0; j < N; ++j) {
            pk.lanes[l0 + (size_t)(fill + j)] = e2hmm::SegLaneDev{k, j, N, fill, pk.comp0[(size_t)k] + j, pk.a_at[(size_t)k]};
            pk.comp_cls[(size_t)(pk.comp0[(size_t)k] + j)] = (uint16_t)k;
        }
        int* info = &pk.slot_info[pk.slot_info.size() - 2];
        info[0] = std::max(info[0], N);
        info[1] = fill == 0 ? 1 : 0;  // (a second class in the slot clears it)
        fill += N;
    }
    pk.slots = (int)(pk.lanes.size() / 64);
    return pk;
}

int LoopModels::from_arrays(int K, const int* Ns_, int M_, const double* const* pis, const double* const* As, const double* const* Bs)
{
    M = M_;
    Ns.assign(Ns_, Ns_ + K);
    return models_from_arrays(K, Ns_, M_, pis, As, Bs, models, ms);
}

int LoopModels::load_checked(const char* who, const char* const* files, unsigned n)
{
    if (load(files, n)) return 1;
    for (const Hmm& h : models) Ns.push_back(h.N);
    return segment_check_shape(who, (int)n, Ns.data());
}

int LoopModels::logs(const char* const* files)
{
    lflats.resize(models.size());
    for (size_t k = 0; k < models.size(); ++k)
        if (log_model(models[k], lflats[k])) return files ? e2vq_set_error("%s: %s", files[k], std::string(e2vq_last_error()).c_str()) : 1;
    return 0;
}

// the models go to <out_dir>/<class>.hmm: none of them may be an input model
int model_out_paths(const char* who, const char* out_dir, const LoopModels& fm, const char* const* model_filenames, unsigned num_models,
                    std::vector<std::string>& out_paths)
{
    out_paths.clear();
    for (int k = 0; k < fm.K(); ++k) {
        out_paths.push_back(std::string(out_dir) + "/" + fm.names[(size_t)k] + ".hmm");
        char *a = realpath(out_paths.back().c_str(), nullptr);
        bool same = false;
        for (unsigned m = 0; a && m < num_models && !same; ++m) {
            char* b = realpath(model_filenames[m], nullptr);
            same = b && strcmp(a, b) == 0;
            free(b);
        }
        free(a);
        if (same) return e2vq_set_error("%s: %s would overwrite an input model (choose another output directory)", who, out_paths.back().c_str());
    }
    return 0;
}

int loop_check_args(const char* who, int K, const int* Ns, const double* const* pis, const double* const* As, const double* const* Bs,
                    bool rest)
{
    if (K < 1) return e2vq_set_error("%s: %d models (at least 1)", who, K);
    if (!Ns || !pis || !As || !Bs || !rest) return e2vq_set_error("%s: bad arguments", who);
    return 0;
}

std::vector<double> loop_log_params(const LoopModels& lm, const SegPacking& pk)
{
    const size_t sumN = (size_t)pk.sumN, a_words = (size_t)pk.a_words, M = (size_t)lm.M;
    std::vector<double> params(sumN + a_words + sumN * M);
    for (size_t k = 0; k < lm.ms.size(); ++k) {
        const std::vector<double>& lflat = lm.lflats[k];
        const size_t N = (size_t)lm.ms[k]->N;
        std::copy(lflat.begin(), lflat.begin() + N, params.begin() + pk.comp0[k]);
        std::copy(lflat.begin() + N, lflat.begin() + N + N * N, params.begin() + sumN + pk.a_at[k]);
        std::copy(lflat.begin() + N + N * N, lflat.end(), params.begin() + sumN + a_words + (size_t)pk.comp0[k] * M);
    }
    return params;
}

int loop_body_looped(const char* env_name, int slots, bool* looped)
{
    const char* body = getenv(env_name);
    if (body && *body && strcmp(body, "resident") != 0 && strcmp(body, "looped") != 0)
        return e2vq_set_error("%s=%s: resident or looped", env_name, body);
    *looped = slots > e2hmm::SEG_MAX_WAVES || (body && strcmp(body, "looped") == 0);
    return 0;
}

int opt_in_body(const char* env_name, LoopBody* body)
{
    const char* v = getenv(env_name);
    *body = LoopBody::Resident;
    if (!v || !*v || strcmp(v, "resident") == 0) return 0;
    if (strcmp(v, "looped") == 0) *body = LoopBody::Looped;
    else if (strcmp(v, "auto") == 0) *body = LoopBody::Auto;
    else return e2vq_set_error("%s=%s: auto, resident or looped", env_name, v);
    return 0;
}

int posteriors_body(LoopBody* body) { return opt_in_body("ECOZ2_HMM_POSTERIOR_BODY", body); }
int segment_trans_body(LoopBody* body) { return opt_in_body("ECOZ2_HMM_SEGMENT_TRANS_BODY", body); }
int trans_fb_body(LoopBody* body) { return opt_in_body("ECOZ2_HMM_TRANS_FB_BODY", body); }

bool runs_looped(LoopBody body, int slots)
{
    return body == LoopBody::Looped || (body == LoopBody::Auto && slots > e2hmm::SEG_MAX_WAVES);
}

int body_waves(bool looped, int slots) { return looped ? std::min(slots, (int)e2hmm::SEG_MAX_WAVES) : slots; }

e2hmm::SegPlanDev loop_shape(const SegPacking& pk, int K, int M)
{
    e2hmm::SegPlanDev shape{};
    shape.K = K, shape.M = M, shape.sumN = pk.sumN, shape.slots = pk.slots, shape.a_words = pk.a_words;
    return shape;
}

int ClassLoopDev::upload(const SegPacking& pk, const std::vector<double>& host_params, int K, int M, hipStream_t st)
{
    if (params.upload(host_params.data(), host_params.size(), st) || lanes.upload(pk.lanes.data(), pk.lanes.size(), st) ||
        slot_info.upload(pk.slot_info.data(), pk.slot_info.size(), st) || comp0.upload(pk.comp0.data(), pk.comp0.size(), st) ||
        comp_cls.upload(pk.comp_cls.data(), pk.comp_cls.size(), st))
        return 1;
    bytes = (i64)host_params.size() * 8 + (i64)pk.lanes.size() * (i64)sizeof(e2hmm::SegLaneDev) + (i64)pk.slot_info.size() * 4 +
            (i64)K * 4 + (i64)pk.sumN * 2;
    pl = e2hmm::SegPlanDev{K, M, pk.sumN, pk.slots, pk.a_words, lanes.get(), slot_info.get(), params.get(), comp_cls.get(), comp0.get()};
    return 0;
}

// ---- what hmm_trans_train.cpp shares with the passes below (hmm_host.h) ---------------------------------------------------------
// where only the resident layout exists: a packing of more than SEG_MAX_WAVES slots is refused (host only)
int check_resident(const char* who, int slots, const char* what_has)
{
    if (slots > e2hmm::SEG_MAX_WAVES)
        return e2vq_set_error("%s: the classes take %d wave-slots of 64 lanes (at most %d: %s no looped body)", who, slots,
                              e2hmm::SEG_MAX_WAVES, what_has);
    return 0;
}

int check_body_slots(const char* who, const SegPacking& pk, int K, LoopBody body, const char* resident_has, const char* looped_of,
                     size_t looped_lds, bool classes)
{
    if (!runs_looped(body, pk.slots)) return check_resident(who, pk.slots, resident_has);
    if (looped_lds <= e2hmm::SEG_LDS_BYTES) return 0;
    if (!classes)
        return e2vq_set_error("%s: %d wave-slots and %d states take %zu bytes of LDS in the looped body of %s (at most %zu)", who,
                              pk.slots, pk.sumN, looped_lds, looped_of, (size_t)e2hmm::SEG_LDS_BYTES);
    return e2vq_set_error("%s: %d wave-slots, %d states and %d classes take %zu bytes of LDS in the looped body of %s (at most %zu)",
                          who, pk.slots, pk.sumN, K, looped_lds, looped_of, (size_t)e2hmm::SEG_LDS_BYTES);
}

// the mandatory LDS of hmm_segment_trans_looped.hip (147 712 bytes at K = sum N = 4096)
int trans_check_slots(const char* who, int K, const int* Ns, LoopBody body)
{
    const SegPacking pk = pack_slots(std::vector<int>(Ns, Ns + K));
    const e2hmm::SegPlanDev shape = loop_shape(pk, K);
    return check_body_slots(who, pk, K, body, "the class-transition decoder has", "the class-transition decoder",
                            e2hmm::segment_trans_looped_lds_bytes(shape, false, false));
}

std::vector<double> trans_transposed(int K, const double* lt)
{
    std::vector<double> ltT((size_t)K * K);
    for (int f = 0; f < K; ++f)
        for (int k = 0; k < K; ++k) ltT[(size_t)k * K + f] = lt[(size_t)f * K + k];
    return ltT;
}

int ForwardTable::reserve(const char* prefix, int sumN, int waves, int extra, const i64* h_offs, int S)
{
    const i64 row = 8 * ((i64)sumN + waves + extra);
    chunks = plan_chunks("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", row, h_offs, S, &max_frames);
    if (!(d_ah.reserve((size_t)max_frames * sumN) || d_c.reserve((size_t)max_frames * waves) ||
          (extra && d_x.reserve((size_t)max_frames * extra))))
        return 0;
    const std::string why = e2vq_last_error();
    return e2vq_set_error("%s: no room for the forward table of %lld frames x %d states (%lld bytes; "
                          "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES bounds it by whole streams): %s",
                          prefix, (long long)max_frames, sumN, (long long)(max_frames * row), why.c_str());
}

std::string frames_csv_path(const std::string& dir, const char* input_filename)
{
    return dir + "/" + e2vq_io::basename_noext(input_filename) + ".csv";
}

int frames_csv_distinct(const std::string& dir, const char* const* input_filenames, int num_inputs)
{
    for (int f = 0; f < num_inputs && !dir.empty(); ++f)
        for (int g = 0; g < f; ++g)
            if (input_filenames[f] && input_filenames[g] && frames_csv_path(dir, input_filenames[g]) == frames_csv_path(dir, input_filenames[f]))
                return e2vq_set_error("%s and %s would both write %s", input_filenames[g], input_filenames[f],
                                      frames_csv_path(dir, input_filenames[f]).c_str());
    return 0;
}

// log_model's refusal, without the logarithms: a negative, NaN or infinite parameter (then no NaN can arise on the device)
int posteriors_check_params(const Hmm& h)
{
    const std::vector<double>* parts[3] = {&h.pi, &h.A, &h.B};
    const char* names[3] = {"pi", "A", "B"};
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < parts[k]->size(); ++i) {
            const double x = (*parts[k])[i];
            if (!(x >= 0.0) || !std::isfinite(x))
                return e2vq_set_error("HMM parameter %s[%zu] = %g: not a finite non-negative number", names[k], i, x);
        }
    return 0;
}

// the leading dimension of a class's A in the sum-product passes
int posteriors_a_ld(int N) { return N | 1; }  // (odd: see hmm_posterior.hip)

int trans_check_lt(const char* who, int K, const double* lt)
{
    for (int f = 0; f < K; ++f)
        for (int k = 0; k < K; ++k) {
            const double v = lt[(size_t)f * K + k];
            if (std::isnan(v) || v > 0.0)
                return e2vq_set_error("%s: lt[%d][%d] = %g: the logarithm of a price, at most 0 (-inf forbids the succession)", who, f, k, v);
        }
    return 0;
}

// w[f][k] = exp(lt[f][k]) (-inf: 0.0), then its transpose: each walk of the sum-product kernels reads consecutive words
std::vector<double> trans_prices(int K, const double* lt)
{
    std::vector<double> w((size_t)2 * K * K);
    for (int f = 0; f < K; ++f)
        for (int k = 0; k < K; ++k) w[(size_t)f * K + k] = w[(size_t)K * K + (size_t)k * K + f] = exp(lt[(size_t)f * K + k]);
    return w;
}

// pi of every class | A of every class, row i at i (N | 1) | B of every class (pk: the packing with posteriors_a_ld)
std::vector<double> trans_params(const LoopModels& lm, const SegPacking& pk)
{
    const int K = lm.K(), M = lm.M, sumN = pk.sumN, a_words = pk.a_words;
    std::vector<double> params((size_t)sumN + (size_t)a_words + (size_t)sumN * M, 0.0);
    for (int k = 0; k < K; ++k) {
        const Hmm& h = *lm.ms[(size_t)k];
        const int N = h.N, ld = posteriors_a_ld(N), c0 = pk.comp0[(size_t)k];
        for (int j = 0; j < N; ++j) {
            params[(size_t)(c0 + j)] = h.pi[(size_t)j];
            std::copy(h.A.begin() + (size_t)j * N, h.A.begin() + (size_t)(j + 1) * N,
                      params.begin() + sumN + pk.a_at[(size_t)k] + (size_t)j * ld);
        }
        std::copy(h.B.begin(), h.B.end(), params.begin() + sumN + a_words + (size_t)c0 * M);
    }
    return params;
}

// the slot check of `hmm segment --posteriors` and of its streamed form (hmm_host.h; body: what posteriors_body gave): the
// mandatory LDS of hmm_posterior_looped.hip
int posteriors_check_slots(const char* who, int K, const int* Ns, LoopBody body)
{
    const SegPacking pk = pack_slots(std::vector<int>(Ns, Ns + K), posteriors_a_ld);
    const e2hmm::SegPlanDev shape = loop_shape(pk, K);
    return check_body_slots(who, pk, K, body, "the posteriors have", "the posteriors", e2hmm::posteriors_looped_lds_bytes(shape, false),
                            /*classes=*/false);
}

namespace {

thread_local float g_segment_kernel_ms = -1.f;        // e2vq_hmm_segment_last_kernel_ms
thread_local float g_posteriors_kernel_ms = -1.f;     // e2vq_hmm_segment_posteriors_last_kernel_ms
thread_local float g_segment_trans_kernel_ms = -1.f;  // e2vq_hmm_segment_trans_last_kernel_ms
thread_local float g_trans_posteriors_kernel_ms = -1.f;  // e2vq_hmm_segment_trans_posteriors_last_kernel_ms

struct SegOut {  // host arrays, any may be null; per frame: cls, state, entered, gbest; per stream: log_prob, status
    uint16_t* cls = nullptr;
    uint16_t* state = nullptr;
    uint8_t* entered = nullptr;
    double* gbest = nullptr;
    double* log_prob = nullptr;
    int* status = nullptr;
};

// What the two Viterbi decoders of the class loop leave on the device: per frame cls / state / entered / score (gbest, or
// exit_score under class-to-class prices); per stream logp / status / qlast.
struct SegResultsDev {
    DeviceBuffer<double> logp, score;
    DeviceBuffer<int> status, qlast;
    DeviceBuffer<unsigned short> cls, state;
    DeviceBuffer<unsigned char> entered;
    int reserve(i64 frames, int S)
    {
        return logp.reserve((size_t)S) || status.reserve((size_t)S) || qlast.reserve((size_t)S) || score.reserve((size_t)frames) ||
               cls.reserve((size_t)frames) || state.reserve((size_t)frames) || entered.reserve((size_t)frames);
    }
    // enqueues the copies of what `out` asks for (the caller synchronises)
    int download(const SegOut& out, i64 frames, int S, hipStream_t st) const
    {
        if (frames > 0) {
            if (out.cls) HIPCHK(hipMemcpyAsync(out.cls, cls.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
            if (out.state) HIPCHK(hipMemcpyAsync(out.state, state.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
            if (out.entered) HIPCHK(hipMemcpyAsync(out.entered, entered.get(), (size_t)frames, hipMemcpyDeviceToHost, st));
            if (out.gbest) HIPCHK(hipMemcpyAsync(out.gbest, score.get(), (size_t)frames * 8, hipMemcpyDeviceToHost, st));
        }
        if (S > 0) {
            if (out.log_prob) HIPCHK(hipMemcpyAsync(out.log_prob, logp.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
            if (out.status) HIPCHK(hipMemcpyAsync(out.status, status.get(), (size_t)S * 4, hipMemcpyDeviceToHost, st));
        }
        return 0;
    }
};

// ---- hmm segment: one Viterbi pass through the class loop of all models ------------------------------------
// The joint Viterbi of S device-resident streams (h_offs: their S + 1 offsets, on the host) under the class loop of the
// models (already checked by segment_check_shape; all of one M; with their logarithms), on the current device and the
// stream st.
int segment_device(const LoopModels& lm, const unsigned short* d_sym, const i64* h_offs, int S, double ln_switch, hipStream_t st,
                   const SegOut& out)
{
    const SegPacking pk = pack_slots(lm.Ns);
    const int sumN = pk.sumN, slots = pk.slots;
    const std::vector<double> params = loop_log_params(lm, pk);
    // the body: resident where the packing fits a workgroup's waves, unless ECOZ2_HMM_SEGMENT_BODY=looped
    bool looped = false;
    if (loop_body_looped("ECOZ2_HMM_SEGMENT_BODY", slots, &looped)) return 1;

    ClassLoopDev loop;
    SegResultsDev res;
    DeviceBuffer<int> d_gsel;
    DeviceBuffer<unsigned short> d_psi;
    DeviceBuffer<i64> d_offs;
    const i64 frames = h_offs[S];
    if (loop.upload(pk, params, lm.K(), lm.M, st) || d_offs.upload(h_offs, (size_t)S + 1, st) || res.reserve(frames, S)) return 1;
    const e2hmm::SegPlanDev& pl = loop.pl;
    // launches of whole streams whose psi (2 sumN bytes a frame) and g (4 bytes a frame) stay within the budget
    const i64 row = 2 * (i64)sumN + 4;
    i64 max_frames = 0;
    const auto chunks = plan_chunks("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", row, h_offs, S, &max_frames);
    if (d_psi.reserve((size_t)max_frames * sumN) || d_gsel.reserve((size_t)max_frames)) {
        const std::string why = e2vq_last_error();
        return e2vq_set_error("hmm segment: no room for the back-pointer table of %lld frames x %d states (%lld bytes; "
                              "ECOZ2_HMM_SEGMENT_CHUNK_BYTES bounds it by whole streams): %s",
                              (long long)max_frames, sumN, (long long)(max_frames * row), why.c_str());
    }
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes psi only after the previous chunk's backtrack has read it)
    for (const auto& c : chunks) {
        const int s0 = c.first, n = c.second - c.first;
        if (e2hmm::launch_segment(pl, looped, d_sym, d_offs.get() + s0, n, h_offs[s0], ln_switch, d_psi.get(), d_gsel.get(), res.score.get(),
                                  res.logp.get() + s0, res.qlast.get() + s0, res.status.get() + s0, st))
            return e2vq_set_error("hmm segment: %d wave-slots of %d states cannot be launched", slots, sumN);
        HIPCHK(hipGetLastError());
        e2hmm::launch_segment_backtrack(pl, d_offs.get() + s0, n, h_offs[s0], d_psi.get(), d_gsel.get(), res.qlast.get() + s0,
                                        res.status.get() + s0, res.cls.get(), res.state.get(), res.entered.get(), res.score.get(), st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    if (res.download(out, frames, S, st)) return 1;
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    return timer.elapsed_ms(&g_segment_kernel_ms);
}

// ---- hmm segment --posteriors: forward-backward through the same class loop -------------------------------
struct PostOut {  // host arrays, any may be null; post: K doubles a frame; per stream: log_prob, status
    double* post = nullptr;
    double* log_prob = nullptr;
    int* status = nullptr;
};

// The smoothed class posteriors of S device-resident streams (h_offs: their S + 1 offsets, on the host) under the class
// loop of the models (already checked by segment_check_shape and posteriors_check_slots; all of one M), on the current
// device and the stream st, by the body that posteriors_body gave.
int posteriors_device(const LoopModels& lm, const unsigned short* d_sym, const i64* h_offs, int S, double ln_switch, hipStream_t st,
                      const PostOut& out, LoopBody body)
{
    const int K = lm.K(), M = lm.M;
    const SegPacking pk = pack_slots(lm.Ns, posteriors_a_ld);
    const int sumN = pk.sumN, a_words = pk.a_words, slots = pk.slots;
    const double sw = exp(ln_switch);  // (-inf: 0.0)
    const bool looped = runs_looped(body, slots);
    // pi of every class | e = sw pi | A of every class, row i at i (N | 1) | B of every class
    std::vector<double> params((size_t)2 * sumN + (size_t)a_words + (size_t)sumN * M, 0.0);
    for (int k = 0; k < K; ++k) {
        const Hmm& h = *lm.ms[(size_t)k];
        const int N = h.N, ld = posteriors_a_ld(N), c0 = pk.comp0[(size_t)k];
        for (int j = 0; j < N; ++j) {
            params[(size_t)(c0 + j)] = h.pi[(size_t)j];
            params[(size_t)(sumN + c0 + j)] = sw * h.pi[(size_t)j];
            std::copy(h.A.begin() + (size_t)j * N, h.A.begin() + (size_t)(j + 1) * N,
                      params.begin() + 2 * sumN + pk.a_at[(size_t)k] + (size_t)j * ld);
        }
        std::copy(h.B.begin(), h.B.end(), params.begin() + 2 * sumN + a_words + (size_t)c0 * M);
    }
    ClassLoopDev loop;
    Scores sc;  // P(O) of each stream
    DeviceBuffer<double> d_post;
    ForwardTable ft;
    DeviceBuffer<i64> d_offs;
    const i64 frames = h_offs[S];
    if (loop.upload(pk, params, K, M, st) || d_offs.upload(h_offs, (size_t)S + 1, st) || sc.reserve((size_t)S) ||
        d_post.reserve((size_t)frames * K) || ft.reserve("hmm segment --posteriors", sumN, body_waves(looped, slots), 0, h_offs, S))
        return 1;
    const e2hmm::SegPlanDev& pl = loop.pl;
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes the tables only after the previous chunk's backward pass has read them)
    for (const auto& c : ft.chunks) {
        const int s0 = c.first, n = c.second - c.first;
        const auto launch = looped ? e2hmm::launch_loop_posteriors_looped : e2hmm::launch_loop_posteriors;
        if (launch(pl, d_sym, d_offs.get() + s0, n, h_offs[s0], sw, ft.d_ah.get(), ft.d_c.get(), d_post.get(), sc.d_mant.get() + s0,
                   sc.d_exp.get() + s0, sc.d_status.get() + s0, st))
            return e2vq_set_error("hmm segment --posteriors: %d wave-slots of %d states cannot be launched", slots, sumN);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    if (frames > 0 && out.post) HIPCHK(hipMemcpyAsync(out.post, d_post.get(), (size_t)frames * K * 8, hipMemcpyDeviceToHost, st));
    if (sc.download((size_t)S, st)) return 1;
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    if (timer.elapsed_ms(&g_posteriors_kernel_ms)) return 1;
    sc.get_all((size_t)S, out.status, out.log_prob);
    return 0;
}

// ---- hmm segment --class-transitions ----------------------------------------------------------------------
// segment_device under the K x K prices lt (row: the class left); out.gbest receives exit_score.  Already checked:
// segment_check_shape, trans_check_slots (with the same body), trans_check_lt.
int segment_trans_device(const LoopModels& lm, const unsigned short* d_sym, const i64* h_offs, int S, const double* lt, hipStream_t st,
                         const SegOut& out, LoopBody body)
{
    const int K = lm.K();
    const SegPacking pk = pack_slots(lm.Ns);
    const int sumN = pk.sumN, slots = pk.slots;
    const std::vector<double> params = loop_log_params(lm, pk), ltT = trans_transposed(K, lt);

    ClassLoopDev loop;
    SegResultsDev res;
    DeviceBuffer<double> d_ltT, d_Es;
    DeviceBuffer<unsigned short> d_psi, d_src, d_xs;
    DeviceBuffer<i64> d_offs;
    const i64 frames = h_offs[S];
    if (loop.upload(pk, params, K, lm.M, st) || d_ltT.upload(ltT.data(), ltT.size(), st) || d_offs.upload(h_offs, (size_t)S + 1, st) ||
        res.reserve(frames, S))
        return 1;
    const e2hmm::SegPlanDev& pl = loop.pl;
    // launches of whole streams whose tables stay within the budget: psi (2 sumN bytes a frame), src and x (2 K each), E (8 K)
    const i64 row = 2 * (i64)sumN + 12 * (i64)K;
    i64 max_frames = 0;
    const auto chunks = plan_chunks("ECOZ2_HMM_SEGMENT_CHUNK_BYTES", row, h_offs, S, &max_frames);
    if (d_psi.reserve((size_t)max_frames * sumN) || d_src.reserve((size_t)max_frames * K) || d_xs.reserve((size_t)max_frames * K) ||
        d_Es.reserve((size_t)max_frames * K)) {
        const std::string why = e2vq_last_error();
        return e2vq_set_error("hmm segment --class-transitions: no room for the back-pointer tables of %lld frames x (%d states, %d "
                              "classes) (%lld bytes; ECOZ2_HMM_SEGMENT_CHUNK_BYTES bounds them by whole streams): %s",
                              (long long)max_frames, sumN, K, (long long)(max_frames * row), why.c_str());
    }
    // (both bodies write the same tables: the backtrack below serves either)
    const auto launch = runs_looped(body, slots) ? e2hmm::launch_segment_trans_looped : e2hmm::launch_segment_trans;
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes the tables only after the previous chunk's backtrack has read them)
    for (const auto& c : chunks) {
        const int s0 = c.first, n = c.second - c.first;
        if (launch(pl, d_sym, d_offs.get() + s0, n, h_offs[s0], d_ltT.get(), d_psi.get(), d_src.get(), d_xs.get(), d_Es.get(),
                   res.logp.get() + s0, res.qlast.get() + s0, res.status.get() + s0, st))
            return e2vq_set_error("hmm segment --class-transitions: %d wave-slots of %d states cannot be launched", slots, sumN);
        HIPCHK(hipGetLastError());
        e2hmm::launch_segment_trans_backtrack(pl, d_offs.get() + s0, n, h_offs[s0], d_psi.get(), d_src.get(), d_xs.get(), d_Es.get(),
                                              res.qlast.get() + s0, res.status.get() + s0, res.cls.get(), res.state.get(), res.entered.get(),
                                              res.score.get(), st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    if (res.download(out, frames, S, st)) return 1;
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    return timer.elapsed_ms(&g_segment_trans_kernel_ms);
}

// ---- hmm segment --class-transitions --grammar-posteriors --------------------------------------------------
// the slot check of the pass (body: what trans_fb_body gave): the mandatory LDS of hmm_posterior_trans_looped.hip
// (99 328 bytes at K = sum N = 4096)
int trans_posteriors_check_slots(const char* who, int K, const int* Ns, LoopBody body)
{
    const SegPacking pk = pack_slots(std::vector<int>(Ns, Ns + K), posteriors_a_ld);
    const e2hmm::SegPlanDev shape = loop_shape(pk, K);
    return check_body_slots(who, pk, K, body, "the posteriors under class-to-class prices have", "the posteriors under class-to-class prices",
                            e2hmm::posteriors_trans_looped_lds_bytes(shape, false, false));
}

// posteriors_device under the K x K prices lt (row: the class left).  Already checked: segment_check_shape,
// trans_posteriors_check_slots (with the same body), trans_check_lt (and the models' parameters: finite and non-negative).
int trans_posteriors_device(const LoopModels& lm, const unsigned short* d_sym, const i64* h_offs, int S, const double* lt, hipStream_t st,
                            const PostOut& out, LoopBody body)
{
    const int K = lm.K(), M = lm.M;
    const SegPacking pk = pack_slots(lm.Ns, posteriors_a_ld);
    const int sumN = pk.sumN, slots = pk.slots;
    const bool looped = runs_looped(body, slots);
    const std::vector<double> w = trans_prices(K, lt), params = trans_params(lm, pk);
    ClassLoopDev loop;
    Scores sc;  // P(O) of each stream
    DeviceBuffer<double> d_post, d_w;
    ForwardTable ft;  // (the class masses live in LDS only: the kernel stores nothing more per frame than 4.8.7's)
    DeviceBuffer<i64> d_offs;
    const i64 frames = h_offs[S];
    if (loop.upload(pk, params, K, M, st) || d_w.upload(w.data(), w.size(), st) || d_offs.upload(h_offs, (size_t)S + 1, st) ||
        sc.reserve((size_t)S) || d_post.reserve((size_t)frames * K) ||
        ft.reserve("hmm segment --grammar-posteriors", sumN, body_waves(looped, slots), 0, h_offs, S))
        return 1;
    const e2hmm::SegPlanDev& pl = loop.pl;
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes the tables only after the previous chunk's backward pass has read them)
    for (const auto& c : ft.chunks) {
        const int s0 = c.first, n = c.second - c.first;
        const auto launch = looped ? e2hmm::launch_loop_posteriors_trans_looped : e2hmm::launch_loop_posteriors_trans;
        if (launch(pl, d_sym, d_offs.get() + s0, n, h_offs[s0], d_w.get(), ft.d_ah.get(), ft.d_c.get(), d_post.get(), sc.d_mant.get() + s0,
                   sc.d_exp.get() + s0, sc.d_status.get() + s0, st))
            return e2vq_set_error("hmm segment --grammar-posteriors: %d wave-slots of %d states cannot be launched", slots, sumN);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    if (frames > 0 && out.post) HIPCHK(hipMemcpyAsync(out.post, d_post.get(), (size_t)frames * K * 8, hipMemcpyDeviceToHost, st));
    if (sc.download((size_t)S, st)) return 1;
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    if (timer.elapsed_ms(&g_trans_posteriors_kernel_ms)) return 1;
    sc.get_all((size_t)S, out.status, out.log_prob);
    return 0;
}

// CSV and stdout block of one segmented input from the per-frame outputs (host only).  post (T rows of K; may be null: every
// byte as without it): two more CSV columns and a p= field per segment, and with frames_csv the per-frame table.  lt (K x K;
// may be null: ln_switch for every pair): the price of the succession that starts a segment (4.8.8; gbest is then exit_score).
int segment_report(const char* who, const char* name, int64_t T, int K, const char* const* class_names, int W_ms, int O_ms,
                   const uint16_t* cls, const uint8_t* entered, const double* gbest, double log_prob, double ln_switch,
                   const double* post, const char* csv_filename, const char* frames_csv, const double* lt = nullptr)
{
    FlushStdout flush_on_return;
    if (!name || K < 1 || !class_names || T < 0 || (T > 0 && (!cls || !entered || !gbest))) return e2vq_set_error("%s: bad arguments", who);
    if (T > 0 && !entered[0]) return e2vq_set_error("%s: frame 0 does not start a segment", who);
    for (int64_t t = 0; t < T; ++t)
        if (cls[t] >= K) return e2vq_set_error("%s: frame %lld names a model outside [0, %d)", who, (long long)t, K);
    struct Seg {
        int64_t b, e;
        double lp, mean, min;
    };
    std::vector<Seg> segs;
    for (int64_t b = 0; b < T;) {
        int64_t e = b + 1;
        while (e < T && !entered[e]) ++e;
        // (gbest[e] of an entered frame e is the path's own cumulative score at e - 1)
        const double hi = e == T ? log_prob : gbest[e];
        const double lo = b == 0 ? 0.0 : gbest[b] + (lt ? lt[(size_t)cls[b - 1] * K + cls[b]] : ln_switch);
        Seg g{b, e, hi - lo, 0.0, 0.0};
        if (post) {  // the class's posterior over the segment's frames: a serial sum in frame order, then one division
            const double* col = post + cls[b];
            double sum = 0.0, least = col[(size_t)b * K];
            for (int64_t t = b; t < e; ++t) {
                const double v = col[(size_t)t * K];
                sum = sum + v;
                if (v < least) least = v;
            }
            g.mean = sum / (double)(e - b);
            g.min = least;
        }
        segs.push_back(g);
        b = e;
    }
    auto begin_s = [&](int64_t b) { return (double)(b * O_ms) / 1000.0; };
    // (the end of the analysis window of the segment's last frame)
    auto end_s = [&](int64_t e) { return (double)((e - 1) * O_ms + W_ms) / 1000.0; };
    if (csv_filename && *csv_filename) {
        std::string doc = "segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame";
        doc += post ? ",posterior,min_posterior\n" : "\n";
        for (size_t i = 0; i < segs.size(); ++i) {
            const Seg& g = segs[i];
            doc += std::to_string(i) + "," + std::to_string(g.b) + "," + std::to_string(g.e) + "," + fmt_17g(begin_s(g.b)) + "," +
                   fmt_17g(end_s(g.e)) + "," + class_names[cls[g.b]] + "," + fmt_17g(g.lp) + "," + fmt_17g(g.lp / (double)(g.e - g.b));
            if (post) doc += "," + fmt_17g(g.mean) + "," + fmt_17g(g.min);
            doc += "\n";
        }
        if (write_file(csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    const bool frames = post && frames_csv && *frames_csv;
    if (frames) {
        std::string doc = "frame,begin_s,class";
        for (int k = 0; k < K; ++k) doc += std::string(",") + class_names[k];
        doc += "\n";
        for (int64_t t = 0; t < T; ++t) {
            doc += std::to_string(t) + "," + fmt_17g(begin_s(t)) + "," + class_names[cls[t]];
            for (int k = 0; k < K; ++k) doc += "," + fmt_17g(post[(size_t)t * K + k]);
            doc += "\n";
        }
        if (write_file(frames_csv, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    printf("%s: T=%lld  segments=%zu  (switch penalty %g)\n", name, (long long)T, segs.size(), ln_switch);
    std::vector<int64_t> count((size_t)K, 0);
    for (int64_t t = 0; t < T; ++t) ++count[cls[t]];
    for (int k = 0; k < K; ++k) printf("  '%s': %lld\n", class_names[k], (long long)count[(size_t)k]);
    printf("  segments:\n");
    for (const Seg& g : segs) {
        printf("    %.3f - %.3f %s", begin_s(g.b), end_s(g.e), class_names[cls[g.b]]);
        if (post) printf(" p=%.3f", g.mean);
        printf("\n");
    }
    if (csv_filename && *csv_filename) printf("  %s saved\n", csv_filename);
    if (frames) printf("  %s saved\n", frames_csv);
    return 0;
}

// `hmm segment` over whole recordings, in its four forms: every input (.wav: lpc -> quantize -> segment; .prd: quantize ->
// segment; .seq: segment) under the models.  transitions_csv: null under the one ln_switch; else the file of the class-to-class
// prices of `--class-transitions` (empty: refused), whose values plus ln_switch are the effective prices.  posteriors:
// `--posteriors`, or under a transitions file `--grammar-posteriors`.  read_body: the reader of the variable that chooses the
// body of the form (null: the form has none).  The symbols of an input are staged once; the posteriors run on the same device
// buffer, under the same effective prices.
int segment_files(const char* who, const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                  const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                  const char* transitions_csv, int (*read_body)(LoopBody*), const char* csv_dir_or_file, bool posteriors,
                  const char* frames_dir)
{
    FlushStdout flush_on_return;
    LoopModels lm;
    const bool trans = transitions_csv != nullptr;
    if (files_given(who, model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
    if (trans && !*transitions_csv) return e2vq_set_error("%s: no class-transitions file", who);
    if (segment_check_switch(who, ln_switch) || window_ms_ok(who, W_ms, O_ms) || lm.load_checked(who, model_filenames, num_models)) return 1;
    const int K = lm.K();
    // (--grammar-posteriors reads its own variable, never the decoder's: the decode of the same input follows that one choice,
    // runs_looped with its value, so that what the posteriors take the decoder takes too)
    LoopBody body = LoopBody::Resident;
    if (read_body && read_body(&body)) return 1;
    if (trans ? trans_check_slots(who, K, lm.Ns.data(), body) || (posteriors && trans_posteriors_check_slots(who, K, lm.Ns.data(), body)) ||
                    check_names(who, K, lm.names.data())
              : posteriors && posteriors_check_slots(who, K, lm.Ns.data(), body))
        return 1;
    std::vector<double> lt;
    if (trans && transitions_read(transitions_csv, K, lm.names.data(), lt)) return 1;
    for (double& v : lt) v = v + ln_switch;  // the effective price
    if (lm.logs(model_filenames)) return 1;
    const std::string fdir = posteriors && frames_dir ? frames_dir : "";
    if (frames_csv_distinct(fdir, input_filenames, num_inputs)) return 1;
    auto run = [&](const SymInput& in, int64_t T, const unsigned short* d_sym, hipStream_t st) -> int {
        const i64 offs[2] = {0, T};
        const size_t n = (size_t)std::max<int64_t>(T, 1);
        std::vector<uint16_t> cls(n);
        std::vector<uint8_t> entered(n);
        std::vector<double> gbest(n), post;  // (gbest: exit_score under a transitions file)
        double lp = 0.0;
        int status = 0;
        SegOut out;
        out.cls = cls.data(), out.entered = entered.data(), out.gbest = gbest.data(), out.log_prob = &lp, out.status = &status;
        if (trans ? segment_trans_device(lm, d_sym, offs, 1, lt.data(), st, out, body) : segment_device(lm, d_sym, offs, 1, ln_switch, st, out))
            return 1;
        if (status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d", in.path.c_str(), lm.M);
        if (posteriors) {
            post.resize(n * (size_t)K);
            PostOut po;
            po.post = post.data();
            if (trans ? trans_posteriors_device(lm, d_sym, offs, 1, lt.data(), st, po, body)
                      : posteriors_device(lm, d_sym, offs, 1, ln_switch, st, po, body))
                return 1;
        }
        const std::string fcsv = fdir.empty() ? "" : frames_csv_path(fdir, in.path.c_str());
        return segment_report(who, in.path.c_str(), T, K, lm.names.data(), W_ms, O_ms, cls.data(), entered.data(), gbest.data(), lp,
                              ln_switch, posteriors ? post.data() : nullptr, in.csv.empty() ? nullptr : in.csv.c_str(),
                              fcsv.empty() ? nullptr : fcsv.c_str(), trans ? lt.data() : nullptr);
    };
    return run_on_files(who, lm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, run);
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

// ---- hmm segment --------------------------------------------------------------------------------------
extern "C" int e2vq_hmm_segment_last_kernel_ms(float* ms)
{
    return last_kernel_ms("e2vq_hmm_segment_last_kernel_ms", g_segment_kernel_ms, ms);
}

// the most likely path of each of S streams through the class loop of K models sharing M.  One device.
extern "C" int e2vq_hmm_segment(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                const double* const* Bs, const void* sym, const int64_t* offs, int S, double ln_switch,
                                uint16_t* cls, uint16_t* state, uint8_t* entered, double* gbest, double* log_prob, int* status,
                                int sym_on_device)
{
    const char* who = "e2vq_hmm_segment";
    LoopModels lm;
    DevSeqs seqs;
    if (loop_check_args(who, K, Ns, pis, As, Bs, syms_given(sym, offs, S)) || segment_check_shape(who, K, Ns) ||
        segment_check_switch(who, ln_switch))
        return 1;
    // (segment_check_shape has passed every N, and M is one: the models can fail here only before any logarithm does)
    if (lm.from_arrays(K, Ns, M, pis, As, Bs) || lm.logs() || seqs.open(device, sym, offs, S, sym_on_device != 0)) return 1;
    const SegOut out{cls, state, entered, gbest, log_prob, status};
    return segment_device(lm, seqs.sym, (const i64*)offs, S, ln_switch, seqs.st.s, out);
}

extern "C" int e2vq_hmm_segment_report(const char* name, int64_t T, int K, const char* const* class_names, int W_ms, int O_ms,
                                       const uint16_t* cls, const uint8_t* entered, const double* gbest, double log_prob,
                                       double ln_switch, const char* csv_filename)
{
    return segment_report("e2vq_hmm_segment_report", name, T, K, class_names, W_ms, O_ms, cls, entered, gbest, log_prob, ln_switch,
                          nullptr, csv_filename, nullptr);
}

extern "C" int e2vq_hmm_segment_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                      const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                                      const char* csv_dir_or_file)
{
    return segment_files("e2vq_hmm_segment_files", model_filenames, num_models, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms,
                         ln_switch, nullptr, nullptr, csv_dir_or_file, false, nullptr);
}


// ---- hmm segment --posteriors -------------------------------------------------------------------------
extern "C" int e2vq_hmm_segment_posteriors_last_kernel_ms(float* ms)
{
    return last_kernel_ms("e2vq_hmm_segment_posteriors_last_kernel_ms", g_posteriors_kernel_ms, ms);
}

// P(class at frame t | the whole stream) of each of S streams under the class loop of K models sharing M.  One device.
extern "C" int e2vq_hmm_segment_posteriors(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                           const double* const* Bs, const void* sym, const int64_t* offs, int S, double ln_switch,
                                           double* post, double* log_prob, int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_segment_posteriors";
    LoopModels lm;
    DevSeqs seqs;
    LoopBody body = LoopBody::Resident;
    if (loop_check_args(who, K, Ns, pis, As, Bs, syms_given(sym, offs, S)) || segment_check_shape(who, K, Ns) ||
        segment_check_switch(who, ln_switch) || posteriors_body(&body) || posteriors_check_slots(who, K, Ns, body) ||
        lm.from_arrays(K, Ns, M, pis, As, Bs))
        return 1;
    for (const Hmm& h : lm.models)
        if (posteriors_check_params(h)) return 1;
    if (seqs.open(device, sym, offs, S, sym_on_device != 0)) return 1;
    const PostOut out{post, log_prob, status};
    return posteriors_device(lm, seqs.sym, (const i64*)offs, S, ln_switch, seqs.st.s, out, body);
}

extern "C" int e2vq_hmm_segment_report_posteriors(const char* name, int64_t T, int K, const char* const* class_names, int W_ms,
                                                  int O_ms, const uint16_t* cls, const uint8_t* entered, const double* gbest,
                                                  double log_prob, double ln_switch, const double* post, const char* csv_filename,
                                                  const char* frames_csv_filename)
{
    if (T > 0 && !post) return e2vq_set_error("e2vq_hmm_segment_report_posteriors: bad arguments");
    const double none = 0.0;  // (T = 0: no row is read)
    return segment_report("e2vq_hmm_segment_report_posteriors", name, T, K, class_names, W_ms, O_ms, cls, entered, gbest, log_prob,
                          ln_switch, post ? post : &none, csv_filename, frames_csv_filename);
}

extern "C" int e2vq_hmm_segment_files_posteriors(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                                 const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                                 double ln_switch, const char* csv_dir_or_file, const char* frames_dir)
{
    return segment_files("e2vq_hmm_segment_files_posteriors", model_filenames, num_models, cb_filename, input_filenames, num_inputs, P,
                         W_ms, O_ms, ln_switch, nullptr, posteriors_body, csv_dir_or_file, true,
                         frames_dir && *frames_dir ? frames_dir : nullptr);
}

// ---- hmm segment --class-transitions ----------------------------------------------------------------------
extern "C" int e2vq_hmm_segment_trans_last_kernel_ms(float* ms)
{
    return last_kernel_ms("e2vq_hmm_segment_trans_last_kernel_ms", g_segment_trans_kernel_ms, ms);
}

extern "C" int e2vq_hmm_segment_trans(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                      const double* const* Bs, const void* sym, const int64_t* offs, int S, const double* lt,
                                      uint16_t* cls, uint16_t* state, uint8_t* entered, double* exit_score, double* log_prob,
                                      int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_segment_trans";
    LoopModels lm;
    DevSeqs seqs;
    LoopBody body = LoopBody::Resident;
    if (loop_check_args(who, K, Ns, pis, As, Bs, lt && syms_given(sym, offs, S)) || segment_check_shape(who, K, Ns) ||
        trans_check_lt(who, K, lt) || segment_trans_body(&body) || trans_check_slots(who, K, Ns, body))
        return 1;
    if (lm.from_arrays(K, Ns, M, pis, As, Bs) || lm.logs() || seqs.open(device, sym, offs, S, sym_on_device != 0)) return 1;
    const SegOut out{cls, state, entered, exit_score, log_prob, status};
    return segment_trans_device(lm, seqs.sym, (const i64*)offs, S, lt, seqs.st.s, out, body);
}

extern "C" int e2vq_hmm_segment_trans_report(const char* name, int64_t T, int K, const char* const* class_names, int W_ms, int O_ms,
                                             const uint16_t* cls, const uint8_t* entered, const double* exit_score, double log_prob,
                                             double ln_switch, const double* lt, const char* csv_filename)
{
    if (!lt) return e2vq_set_error("e2vq_hmm_segment_trans_report: bad arguments");
    return segment_report("e2vq_hmm_segment_trans_report", name, T, K, class_names, W_ms, O_ms, cls, entered, exit_score, log_prob,
                          ln_switch, nullptr, csv_filename, nullptr, lt);
}

extern "C" int e2vq_hmm_segment_trans_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                            const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                            double ln_switch, const char* transitions_csv, const char* csv_dir_or_file)
{
    return segment_files("e2vq_hmm_segment_trans_files", model_filenames, num_models, cb_filename, input_filenames, num_inputs, P, W_ms,
                         O_ms, ln_switch, transitions_csv ? transitions_csv : "", segment_trans_body, csv_dir_or_file, false, nullptr);
}

// ---- hmm segment --class-transitions --grammar-posteriors --------------------------------------------------
extern "C" int e2vq_hmm_segment_trans_posteriors_last_kernel_ms(float* ms)
{
    return last_kernel_ms("e2vq_hmm_segment_trans_posteriors_last_kernel_ms", g_trans_posteriors_kernel_ms, ms);
}

// P(class at frame t | the whole stream) of each of S streams under the class loop of K models and the K x K prices lt
extern "C" int e2vq_hmm_segment_trans_posteriors(int device, int K, const int* Ns, int M, const double* const* pis,
                                                 const double* const* As, const double* const* Bs, const void* sym, const int64_t* offs,
                                                 int S, const double* lt, double* post, double* log_prob, int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_segment_trans_posteriors";
    LoopModels lm;
    DevSeqs seqs;
    LoopBody body = LoopBody::Resident;
    if (loop_check_args(who, K, Ns, pis, As, Bs, lt && syms_given(sym, offs, S)) || segment_check_shape(who, K, Ns) ||
        trans_check_lt(who, K, lt) || trans_fb_body(&body) || trans_posteriors_check_slots(who, K, Ns, body) ||
        lm.from_arrays(K, Ns, M, pis, As, Bs))
        return 1;
    for (const Hmm& h : lm.models)
        if (posteriors_check_params(h)) return 1;
    if (seqs.open(device, sym, offs, S, sym_on_device != 0)) return 1;
    const PostOut out{post, log_prob, status};
    return trans_posteriors_device(lm, seqs.sym, (const i64*)offs, S, lt, seqs.st.s, out, body);
}

extern "C" int e2vq_hmm_segment_trans_files_posteriors(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                                       const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                                       double ln_switch, const char* transitions_csv, const char* csv_dir_or_file,
                                                       const char* frames_dir)
{
    return segment_files("e2vq_hmm_segment_trans_files_posteriors", model_filenames, num_models, cb_filename, input_filenames, num_inputs,
                         P, W_ms, O_ms, ln_switch, transitions_csv ? transitions_csv : "", trans_fb_body, csv_dir_or_file, true,
                         frames_dir && *frames_dir ? frames_dir : nullptr);
}
