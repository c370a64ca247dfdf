// hmm_loop_train.cpp -- Baum-Welch for the class models under the class loop (`hmm learn --loop`, e2vq_hmm_loop_estep,
// e2vq_hmm_train_loop): pi, A and B of every class re-estimated from whole unlabelled streams under the loop
// and the prices `hmm segment --class-transitions` decodes, and on request the matrix with them, over the kernel of
// hmm_loop_estep.hip.  The host takes exp of the prices, chooses the LDS layout and the routes of the two count tables (all
// before any HIP call), keeps the device state over the iterations, takes the logarithm of the (mantissa, exponent) pairs, sums
// ln P over the streams in stream order, zeroes the blocks of the frozen classes, runs the M-steps and decides when to stop.
// The checks, the packing, the parameter block, the prices and the forward table are hmm_class_loop.cpp's, the M-step of the models
// hmm_embed.hip's, that of the matrix hmm_trans_train.cpp's, the file of the matrix hmm_transitions.cpp's, the input stage
// hmm_input.cpp's (hmm_host.h).
#include "hmm_host.h"

namespace e2hmm_host {
namespace {

thread_local float g_loop_estep_kernel_ms = -1.f;  // e2vq_hmm_loop_estep_last_kernel_ms

constexpr int LOOP_MAX_ESTEPS = 1000;  // the safety cap of the other trainers (hmm_train.cpp: MAX_ESTEPS)

inline i64 trans_acc_words(int K) { return 2 * (i64)K * K + 2; }

// What the host decides about a call before the device is touched: the packing, the classes' places in the count and M-step
// blocks, the LDS layout and the routes of the AN and C tables (ECOZ2_HMM_LOOP_EM_AN, ECOZ2_HMM_LOOP_EM_C: lds or global;
// unset: LDS when the table fits behind the mandatory terms, AN first).  gram: the call forms the grammar counts.
struct LoopEmPlan {
    SegPacking pk;
    std::vector<e2hmm::EmbedClassDev> classes;
    std::vector<i64> acc_at;  // [K + 1]
    i64 dense_words = 0, max_P = 0;
    int max_N = 0;
    bool gram = false, an_lds = false, c_lds = false, a_lds = false, w_lds = false;
};

int loop_em_plan(const char* who, const std::vector<int>& Ns, int M, bool gram, LoopEmPlan& lp)
{
    const int K = (int)Ns.size();
    lp.gram = gram;
    lp.pk = pack_slots(Ns, posteriors_a_ld);
    if (check_resident(who, lp.pk.slots, "the E-step of the class models under the loop has")) return 1;
    lp.acc_at.assign((size_t)K + 1, 0);
    for (int k = 0; k < K; ++k) {
        const int N = Ns[(size_t)k];
        lp.classes.push_back(e2hmm::EmbedClassDev{N, lp.pk.a_at[(size_t)k], lp.acc_at[(size_t)k], lp.dense_words});
        lp.acc_at[(size_t)k + 1] = lp.acc_at[(size_t)k] + e2hmm::acc_words(N, M);
        const i64 P = (i64)N + (i64)N * N + (i64)N * M;
        lp.dense_words += P;
        lp.max_P = std::max(lp.max_P, P);
        lp.max_N = std::max(lp.max_N, N);
    }
    bool an_forced = false, c_forced = false;
    if (embed_route("ECOZ2_HMM_LOOP_EM_AN", &an_forced, &lp.an_lds) || embed_route("ECOZ2_HMM_LOOP_EM_C", &c_forced, &lp.c_lds)) return 1;
    const e2hmm::SegPlanDev shape = loop_shape(lp.pk, K, M);
    e2hmm::loop_estep_layout(shape, gram, an_forced, c_forced, &lp.an_lds, &lp.c_lds, &lp.a_lds, &lp.w_lds);
    const size_t lds = e2hmm::loop_estep_lds_bytes(shape, lp.an_lds, lp.c_lds, lp.a_lds, lp.w_lds);
    if (lds > e2hmm::SEG_LDS_BYTES)
        return e2vq_set_error("%s: %d classes of %d states with the AN table in %s and the class-to-class table in %s take %zu bytes of "
                              "LDS (at most %zu)", who, K, lp.pk.sumN, lp.an_lds ? "LDS" : "global memory",
                              lp.c_lds ? "LDS" : "global memory", lds, (size_t)e2hmm::SEG_LDS_BYTES);
    return 0;
}

// The device side of a planned call: the tables, the scratch and the accumulators, kept over the iterations of a training.
struct LoopEmDev {
    ClassLoopDev loop;
    Scores sc;  // P(O | loop) of each stream
    ForwardTable ft;  // 4.8.13's row and m_t of every class (ft.d_x, K doubles a frame), bounded by whole streams in the same way
    DeviceBuffer<double> d_w, d_dense;
    DeviceBuffer<i64> d_offs, d_acc, d_acc_t;
    DeviceBuffer<e2hmm::EmbedClassDev> d_classes;
    std::vector<double> params, w, dense;
    std::vector<i64> acc_t;  // the grammar counts of the last E-step: 2 K^2 + 2 words (gram)
    KernelTimer timer;

    int setup(const char* who, const LoopEmPlan& lp, const LoopModels& lm, const i64* h_offs, int S, hipStream_t st)
    {
        const int K = lm.K();
        params = trans_params(lm, lp.pk);
        return loop.upload(lp.pk, params, K, lm.M, st) || d_classes.upload(lp.classes.data(), lp.classes.size(), st) ||
               d_offs.upload(h_offs, (size_t)S + 1, st) || sc.reserve((size_t)S) || d_acc.reserve((size_t)lp.acc_at.back()) ||
               d_acc_t.reserve((size_t)trans_acc_words(K)) || d_w.reserve((size_t)2 * K * K) || timer.create() ||
               ft.reserve(who, lp.pk.sumN, lp.pk.slots, K, h_offs, S);
    }
    // One E-step under the models lm and the effective prices lt: the counts of all streams in d_acc (from zero, AD summed),
    // with lp.gram the grammar counts in acc_t (from zero), P and status of every stream in sc's host mirrors.  Waits for the
    // stream.
    int estep(const char* who, const LoopEmPlan& lp, const LoopModels& lm, const double* lt, const unsigned short* d_sym, const i64* h_offs,
              int S, hipStream_t st)
    {
        const int K = loop.pl.K;
        const size_t words_t = (size_t)trans_acc_words(K);
        params = trans_params(lm, lp.pk);
        w = trans_prices(K, lt);
        if (loop.params.upload(params.data(), params.size(), st) || d_w.upload(w.data(), w.size(), st)) return 1;
        loop.pl.params = loop.params.get();
        HIPCHK(hipMemsetAsync(d_acc.get(), 0, (size_t)lp.acc_at.back() * 8, st));
        if (lp.gram) HIPCHK(hipMemsetAsync(d_acc_t.get(), 0, words_t * 8, st));
        HIPCHK(hipEventRecord(timer.start.e, st));
        // (one stream: a chunk's forward pass writes the tables only after the previous chunk's backward pass has read them)
        for (const auto& c : ft.chunks) {
            const int s0 = c.first, n = c.second - c.first;
            if (e2hmm::launch_loop_estep(loop.pl, d_classes.get(), lp.an_lds, lp.c_lds, lp.a_lds, lp.w_lds, d_sym, d_offs.get() + s0, n,
                                         h_offs[s0], d_w.get(), ft.d_ah.get(), ft.d_c.get(), ft.d_x.get(), d_acc.get(),
                                         lp.gram ? d_acc_t.get() : nullptr, sc.d_mant.get() + s0, sc.d_exp.get() + s0,
                                         sc.d_status.get() + s0, st))
                return e2vq_set_error("%s: %d wave-slots of %d states cannot be launched", who, lp.pk.slots, lp.pk.sumN);
            HIPCHK(hipGetLastError());
        }
        e2hmm::launch_embed_rowsum(d_classes.get(), K, lp.max_N, d_acc.get(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(timer.stop.e, st));
        if (lp.gram) {
            acc_t.resize(words_t);
            HIPCHK(hipMemcpyAsync(acc_t.data(), d_acc_t.get(), words_t * 8, hipMemcpyDeviceToHost, st));
        }
        if (sc.download((size_t)S, st)) return 1;
        HIPCHK(hipStreamSynchronize(st));
        return timer.elapsed_ms(&g_loop_estep_kernel_ms);
    }
    // M-step from d_acc: the models re-estimated in place (on the host, through the device); the block of a frozen class is
    // zeroed first, so that class keeps every byte.  Waits for the stream.
    int mstep(const LoopEmPlan& lp, LoopModels& lm, const uint8_t* frozen, double epsilon, hipStream_t st)
    {
        const int K = lm.K();
        for (int k = 0; frozen && k < K; ++k)
            if (frozen[k])
                HIPCHK(hipMemsetAsync(d_acc.get() + lp.acc_at[(size_t)k], 0, (size_t)(lp.acc_at[(size_t)k + 1] - lp.acc_at[(size_t)k]) * 8, st));
        dense.resize((size_t)lp.dense_words);
        for (int k = 0; k < K; ++k) lm.models[(size_t)k].pack(dense.data() + lp.classes[(size_t)k].param_at);
        if (d_dense.upload(dense.data(), dense.size(), st)) return 1;
        e2hmm::launch_reestimate_embedded(d_classes.get(), K, lm.M, lp.max_P, lp.max_N, d_acc.get(), epsilon, d_dense.get(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dense.data(), d_dense.get(), dense.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < K; ++k) lm.models[(size_t)k].unpack(dense.data() + lp.classes[(size_t)k].param_at);
        return 0;
    }
};

struct LoopIteration {
    double L;
    int used, skipped;
};

// The loop of the other trainers over this E-step: per iteration one E-step over all streams under lm and ln_p + ln_switch
// and L = the sum of ln P over the status-0 streams in stream order; a stopping iteration gets no M-step.  on_estep (may be
// empty) sees every E-step's result before the decision.  lm and ln_p are the caller's copies: where no stream has status 0
// after the first E-step, the call fails before either is written.
int loop_train(const char* who, const LoopEmPlan& lp, LoopEmDev& dev, LoopModels& lm, double* ln_p, double ln_switch, const uint8_t* frozen,
               double alpha, double epsilon, const unsigned short* d_sym, const i64* h_offs, int S, hipStream_t st, double val_auto,
               int max_iterations, std::vector<LoopIteration>& hist,
               const std::function<void(int, const LoopIteration&, const Scores&)>& on_estep)
{
    const int K = lm.K();
    std::vector<double> eff((size_t)K * K);
    double Lprev = 0.0;
    hist.clear();
    for (int it = 0;; ++it) {
        if ((max_iterations >= 0 && it >= max_iterations) || it >= LOOP_MAX_ESTEPS) break;
        for (size_t i = 0; i < eff.size(); ++i) eff[i] = ln_p[i] + ln_switch;  // the effective price, as --class-transitions forms it
        if (dev.estep(who, lp, lm, eff.data(), d_sym, h_offs, S, st)) return 1;
        LoopIteration e{0.0, 0, 0};
        for (int s = 0; s < S; ++s) {
            if (dev.sc.ok((size_t)s)) {
                e.L = e.L + dev.sc.log_prob((size_t)s);
                ++e.used;
            } else {
                ++e.skipped;
            }
        }
        if (on_estep) on_estep(it, e, dev.sc);
        if (it == 0 && e.used == 0)
            return e2vq_set_error("%s: no stream can be explained by the class loop under the models and the prices (all %d skipped)", who, S);
        hist.push_back(e);
        if (it > 0 && e.L - Lprev <= val_auto) break;
        if (dev.mstep(lp, lm, frozen, epsilon, st)) return 1;
        if (lp.gram) trans_mstep(K, dev.acc_t.data(), alpha, ln_p);
        Lprev = e.L;
    }
    return 0;
}

// the first checks of the array-level entry points: the arguments, the shapes, the prices, the slots, the models
int loop_em_check_args(const char* who, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                       const double* const* Bs, const void* sym, const int64_t* offs, int S, const double* lt, bool rest, bool gram,
                       LoopModels& lm, LoopEmPlan& lp)
{
    if (loop_check_args(who, K, Ns, pis, As, Bs, lt && rest && syms_given(sym, offs, S)) || segment_check_shape(who, K, Ns) ||
        trans_check_lt(who, K, lt) || loop_em_plan(who, std::vector<int>(Ns, Ns + K), M, gram, lp) ||
        lm.from_arrays(K, Ns, M, pis, As, Bs))
        return 1;
    for (const Hmm& h : lm.models)
        if (posteriors_check_params(h)) return 1;
    return check_offsets(offs, S);
}

int check_epsilon(const char* who, double epsilon)
{
    if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return e2vq_set_error("%s: epsilon = %g: a finite number, at least 0", who, epsilon);
    return 0;
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

extern "C" int e2vq_hmm_loop_estep_last_kernel_ms(float* ms)
{
    return last_kernel_ms("e2vq_hmm_loop_estep_last_kernel_ms", g_loop_estep_kernel_ms, ms);
}

extern "C" int e2vq_hmm_loop_estep(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                   const double* const* Bs, const void* sym, const int64_t* offs, int S, const double* lt,
                                   int64_t* const* acc, int64_t* acc_trans, double* log_prob, int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_loop_estep";
    LoopModels lm;
    LoopEmPlan lp;
    if (loop_em_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, lt, acc != nullptr, acc_trans != nullptr, lm, lp)) return 1;
    for (int k = 0; k < K; ++k)
        if (!acc[k]) return e2vq_set_error("%s: bad arguments", who);
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    LoopEmDev dev;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0) || dev.setup(who, lp, lm, (const i64*)offs, S, seqs.st.s) ||
        dev.estep(who, lp, lm, lt, seqs.sym, (const i64*)offs, S, seqs.st.s))
        return 1;
    for (int k = 0; k < K; ++k)
        HIPCHK(hipMemcpyAsync(acc[k], dev.d_acc.get() + lp.acc_at[(size_t)k], (size_t)(lp.acc_at[(size_t)k + 1] - lp.acc_at[(size_t)k]) * 8,
                              hipMemcpyDeviceToHost, seqs.st.s));
    HIPCHK(hipStreamSynchronize(seqs.st.s));
    if (acc_trans)
        for (size_t i = 0; i < dev.acc_t.size(); ++i) acc_trans[i] += dev.acc_t[i];
    dev.sc.get_all((size_t)S, status, log_prob);
    return 0;
}

extern "C" int e2vq_hmm_train_loop(int device, int K, const int* Ns, int M, double* const* pis, double* const* As, double* const* Bs,
                                   const void* sym, const int64_t* offs, int S, double* ln_p, double ln_switch, int train_transitions,
                                   const uint8_t* frozen, double alpha, double epsilon, double val_auto, int max_iterations,
                                   double* sum_log_prob, int cap, int* num_esteps, void (*callback)(char* variable, double value),
                                   int sym_on_device)
{
    const char* who = "e2vq_hmm_train_loop";
    LoopModels lm;
    LoopEmPlan lp;
    if (loop_em_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, ln_p, !(cap > 0 && !sum_log_prob), train_transitions != 0, lm, lp) ||
        segment_check_switch(who, ln_switch) || trans_check_alpha(who, alpha) || check_epsilon(who, epsilon))
        return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    LoopEmDev dev;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    std::vector<LoopIteration> hist;
    std::vector<double> p(ln_p, ln_p + (size_t)K * K);
    static char var[] = "sum_log_prob";
    auto on_estep = [&](int, const LoopIteration& e, const Scores&) {
        if (callback) callback(var, e.L);
    };
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0) || dev.setup(who, lp, lm, (const i64*)offs, S, seqs.st.s) ||
        loop_train(who, lp, dev, lm, p.data(), ln_switch, frozen, alpha, epsilon, seqs.sym, (const i64*)offs, S, seqs.st.s, val_auto,
                   max_iterations, hist, on_estep))
        return 1;
    for (int k = 0; k < K; ++k) model_to_arrays(lm.models[(size_t)k], pis[k], As[k], Bs[k]);
    if (train_transitions) std::copy(p.begin(), p.end(), ln_p);
    for (size_t i = 0; i < hist.size() && (int)i < cap; ++i) sum_log_prob[i] = hist[i].L;
    if (num_esteps) *num_esteps = (int)hist.size();
    return 0;
}

extern "C" int e2vq_hmm_learn_loop_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                         const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                                         const char* transitions_csv, int train_transitions, const char* const* frozen_classes,
                                         int num_frozen, double alpha, double epsilon, double val_auto, int max_iterations,
                                         const char* out_dir, void (*callback)(char* variable, double value))
{
    const char* who = "e2vq_hmm_learn_loop_files";
    FlushStdout flush_on_return;
    LoopModels lm;
    LoopEmPlan lp;
    if (files_given(who, model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
    if (!out_dir || !*out_dir) return e2vq_set_error("%s: no output directory", who);
    if (num_frozen < 0 || (num_frozen > 0 && !frozen_classes)) return e2vq_set_error("%s: bad arguments", who);
    if (segment_check_switch(who, ln_switch) || trans_check_alpha(who, alpha) || check_epsilon(who, epsilon) ||
        window_ms_ok(who, W_ms, O_ms) || lm.load_checked(who, model_filenames, num_models))
        return 1;
    const int K = lm.K();
    if (loop_em_plan(who, lm.Ns, lm.M, train_transitions != 0, lp) || check_names(who, K, lm.names.data())) return 1;
    for (unsigned k = 0; k < num_models; ++k)
        if (posteriors_check_params(lm.models[k])) return e2vq_set_error("%s: %s", model_filenames[k], std::string(e2vq_last_error()).c_str());
    std::vector<uint8_t> frozen((size_t)K, 0);
    for (int i = 0; i < num_frozen; ++i) {
        int k = 0;
        while (k < K && (!frozen_classes[i] || strcmp(frozen_classes[i], lm.names[(size_t)k]) != 0)) ++k;
        if (k == K) return e2vq_set_error("%s: --freeze %s: no model has this class", who, frozen_classes[i] ? frozen_classes[i] : "(null)");
        frozen[(size_t)k] = 1;
    }
    std::vector<std::string> out_paths;
    if (model_out_paths(who, out_dir, lm, model_filenames, num_models, out_paths)) return 1;
    // the start: the file's matrix, or zeros (the effective prices are then the one ln_switch)
    std::vector<double> ln_p((size_t)K * K, 0.0);
    if (transitions_csv && *transitions_csv && transitions_read(transitions_csv, K, lm.names.data(), ln_p)) return 1;
    SymInputs si;
    if (sym_inputs_check(who, lm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, nullptr, si)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    DeviceBuffer<unsigned short> d_all;
    LoopEmDev dev;
    std::vector<i64> offs(1, 0);  // (before the stage: its stream copies from them)
    SymStage stg;
    if (require_device(device) || stg.open(device, si)) return 1;
    if (stg.gather(who, si, P, W_ms, O_ms, d_all, offs)) return 1;
    if (dev.setup(who, lp, lm, offs.data(), num_inputs, stg.st.s)) return 1;
    const bool verbose = getenv("ECOZ2_VQ_QUIET") == nullptr;
    const int n_frozen = (int)std::count(frozen.begin(), frozen.end(), 1);
    static char var[] = "sum_log_prob";
    printf("\nHMM learn --loop: %d class(es)  M=%d  #streams = %d  frames = %lld\n", K, lm.M, num_inputs, (long long)offs.back());
    printf("  switch penalty=%g  transitions=%s%s  frozen=%d  alpha=%g  epsilon=%g  val_auto=%g  max_iterations=%d\n", ln_switch,
           transitions_csv && *transitions_csv ? transitions_csv : "(zeros)", train_transitions ? " (trained)" : "", n_frozen, alpha, epsilon,
           val_auto, max_iterations);
    std::vector<LoopIteration> hist;
    std::vector<int> last_status((size_t)num_inputs, 0);
    auto on_estep = [&](int it, const LoopIteration& e, const Scores& sc) {
        // a stream is named whenever its status changes: skipped from the start, lost after an M-step, or used again
        for (int f = 0; f < num_inputs; ++f) {
            const int stf = sc.status.get()[f];
            if (stf == last_status[(size_t)f]) continue;
            last_status[(size_t)f] = stf;
            fprintf(stderr, "%s: it=%d: %s\n", si.inputs[(size_t)f].path.c_str(), it,
                    stf == 0   ? "used again"
                    : stf == 2 ? "skipped: a symbol outside the models' alphabet"
                               : "skipped: no path of probability > 0 through the class loop");
        }
        if (verbose)
            printf("  it=%d  sum log(P) = %.10g%s\n", it, e.L,
                   e.skipped ? (" (" + std::to_string(e.skipped) + " stream(s) skipped)").c_str() : "");
        if (callback) callback(var, e.L);
    };
    if (loop_train(who, lp, dev, lm, ln_p.data(), ln_switch, frozen.data(), alpha, epsilon, d_all.get(), offs.data(), num_inputs, stg.st.s,
                   val_auto, max_iterations, hist, on_estep))
        return 1;
    for (int k = 0; k < K; ++k)
        if (hmm_save(out_paths[(size_t)k], lm.models[(size_t)k])) return 1;
    const std::string t_path = std::string(out_dir) + "/transitions.csv";
    if (train_transitions && e2vq_hmm_transitions_write(t_path.c_str(), K, lm.names.data(), ln_p.data())) return 1;
    std::string csv = "iteration,sum_log_prob,streams_used,streams_skipped\n";
    for (size_t i = 0; i < hist.size(); ++i)
        csv += std::to_string(i) + "," + fmt_17g(hist[i].L) + "," + std::to_string(hist[i].used) + "," + std::to_string(hist[i].skipped) + "\n";
    const std::string csv_path = std::string(out_dir) + "/loop.csv";
    if (write_file(csv_path, std::vector<unsigned char>(csv.begin(), csv.end()))) return 1;
    printf("%zu E-step(s); %d model(s) saved in %s%s; %s saved\n", hist.size(), K, out_dir,
           train_transitions ? (", " + t_path + " saved").c_str() : "", csv_path.c_str());
    return 0;
}
