// hmm_embed.cpp -- embedded (transcript-constrained) Baum-Welch on the GPU (`hmm learn --embedded`, e2vq_hmm_embedded_estep,
// e2vq_hmm_train_embedded): the class models re-estimated from whole streams and the order of their units,
// over the kernels of hmm_embed.hip.  The host adds the accumulator and M-step places and the AN table to hmm_transcript.cpp's
// plan (all before any HIP call), takes the logarithm of the (mantissa, exponent) pairs, sums ln P over the streams in stream
// order, decides when to stop, and writes the models and the report.  The checks, the transcripts of the label files, the plan
// and the parameter block are hmm_transcript.cpp's, the models hmm_class_loop.cpp's, the input stage hmm_input.cpp's (hmm_host.h).
#include "hmm_host.h"

namespace e2hmm_host {
namespace {

thread_local float g_embed_kernel_ms = -1.f;  // e2vq_hmm_embedded_last_kernel_ms

constexpr int EMBED_MAX_ESTEPS = 1000;  // the safety cap of the other trainers (hmm_train.cpp: MAX_ESTEPS)

// What the host decides about a call before the device is touched: the plan of the forward-backward pass with EMBED_FIRST, the
// classes' places in the count and M-step blocks, and the LDS layout.
struct EmbedPlan : EStepPlan {
    std::vector<i64> acc_at;  // [K + 1]
    i64 dense_words = 0, max_P = 0;
    int max_N = 0;
    bool an_lds = false;
    struct LoopLds {  // of a launch of the looped body
        bool a_lds = false, an_lds = false;
    };
    std::vector<LoopLds> loop_lds;  // per chunk
};

int embed_plan(const char* who, int K, const int* Ns, int M, const i64* offs, int S, const int32_t* units, const i64* unit_offs,
               const uint8_t* optional, double ln_switch, EmbedPlan& ep)
{
    LoopBody body = LoopBody::Resident;
    if (embed_body(&body)) return 1;
    if (estep_plan(who, K, Ns, M, offs, S, units, unit_offs, optional, ln_switch, "the embedded E-step has no looped body", true, body, ep))
        return 1;
    ep.acc_at.assign((size_t)K + 1, 0);
    for (int k = 0; k < K; ++k) {
        const int N = Ns[k];
        ep.classes[(size_t)k].acc_at = ep.acc_at[(size_t)k], ep.classes[(size_t)k].param_at = ep.dense_words;
        ep.acc_at[(size_t)k + 1] = ep.acc_at[(size_t)k] + e2hmm::acc_words(N, M);
        const i64 P = (i64)N + (i64)N * N + (i64)N * M;
        ep.dense_words += P;
        ep.max_P = std::max(ep.max_P, P);
        ep.max_N = std::max(ep.max_N, N);
    }
    // the LDS layout: A when it fits, then the AN table when it fits as well; either route may be forced
    bool fan = false;
    if (embed_route("ECOZ2_HMM_EMBED_AN", &fan, &ep.an_lds)) return 1;
    const int aw = ep.cls.a_words;
    const bool a_said = ep.a_lds, an_said = ep.an_lds;  // what the variables force
    // the launches of the looped body: each by its own largest shapes
    ep.loop_lds.resize(ep.chunks.size());
    for (size_t i = 0; i < ep.chunks.size(); ++i) {
        const EStepPlan::Shape& g = ep.shapes[i];
        if (!g.looped) continue;
        EmbedPlan::LoopLds& ll = ep.loop_lds[i];
        auto bytes = [&](bool a, bool an) { return e2hmm::embed_looped_lds_bytes(g.max_L, g.max_slots, g.max_sumN, aw, a, an); };
        ll.a_lds = ep.a_forced ? a_said : bytes(true, fan && an_said) <= e2hmm::SEG_LDS_BYTES;
        ll.an_lds = fan ? an_said : bytes(ll.a_lds, true) <= e2hmm::SEG_LDS_BYTES;
        if (bytes(ll.a_lds, ll.an_lds) > e2hmm::SEG_LDS_BYTES)
            return e2vq_set_error("%s: streams %d to %d: %d units of sum N = %d states in %d wave-slots, A in %s and the AN table in %s take "
                                  "%zu bytes of LDS (at most %zu)", who, ep.chunks[i].first, ep.chunks[i].second - 1, g.max_L, g.max_sumN,
                                  g.max_slots, ll.a_lds ? "LDS" : "global memory", ll.an_lds ? "LDS" : "global memory",
                                  bytes(ll.a_lds, ll.an_lds), e2hmm::SEG_LDS_BYTES);
    }
    // the launches of the resident body: one layout for all of them, by the most units of their streams
    if (!ep.a_forced) ep.a_lds = e2hmm::embed_lds_bytes(ep.max_L, aw, true, fan && ep.an_lds) <= e2hmm::SEG_LDS_BYTES;
    if (!fan) ep.an_lds = e2hmm::embed_lds_bytes(ep.max_L, aw, ep.a_lds, true) <= e2hmm::SEG_LDS_BYTES;
    const size_t lds = e2hmm::embed_lds_bytes(ep.max_L, aw, ep.a_lds, ep.an_lds);
    const bool resident_runs = S == 0 || std::count(ep.looped.begin(), ep.looped.end(), 0) > 0;
    if (lds > e2hmm::SEG_LDS_BYTES && resident_runs)
        return e2vq_set_error("%s: %d units, A in %s and the AN table in %s take %zu bytes of LDS (at most %zu)", who, ep.max_L,
                              ep.a_lds ? "LDS" : "global memory", ep.an_lds ? "LDS" : "global memory", lds, e2hmm::SEG_LDS_BYTES);
    return 0;
}

// The device side of a planned call: the tables, the scratch and the accumulators, kept over the iterations of a training.
struct EmbedDev {
    EStepDev pd;
    DeviceBuffer<i64> d_acc;
    DeviceBuffer<double> d_params, d_dense;
    Scores sc;  // P(O, transcript) of each stream
    std::vector<double> params, dense;
    KernelTimer timer;

    int setup(const char* who, const EmbedPlan& ep, const i64* h_offs, int S, hipStream_t st)
    {
        return pd.upload(ep, h_offs, S, st) || d_acc.reserve((size_t)ep.acc_at.back()) || sc.reserve((size_t)S) || timer.create() ||
               pd.scratch(who, ep);
    }
    // One E-step under the models: the counts of all streams in d_acc (zeroed first), P and status of every stream in sc's
    // host mirrors.  Waits for the stream.
    int estep(const char* who, const EmbedPlan& ep, const LoopModels& lm, double ln_switch, const unsigned short* d_sym, const i64* h_offs,
              hipStream_t st)
    {
        const int K = lm.K(), S = (int)ep.ap.streams.size();
        params = embed_params(lm, ep.cls, exp(ln_switch));
        if (d_params.upload(params.data(), params.size(), st)) return 1;
        HIPCHK(hipMemsetAsync(d_acc.get(), 0, (size_t)ep.acc_at.back() * 8, st));
        HIPCHK(hipEventRecord(timer.start.e, st));
        // (one stream: a chunk's forward pass writes the scratch only after the previous chunk's backward pass has read it)
        for (size_t i = 0; i < ep.chunks.size(); ++i) {
            const int s0 = ep.chunks[i].first, n = ep.chunks[i].second - s0;
            const EStepPlan::Shape& g = ep.shapes[i];
            if (g.looped) {
                e2hmm::EmbedPlanDev pl = pd.plan(ep, s0, d_params.get());
                pl.max_L = g.max_L;
                if (e2hmm::launch_embed_fb_looped(pl, ep.loop_lds[i].a_lds, ep.loop_lds[i].an_lds, g.max_slots, g.max_sumN, d_sym,
                                                  pd.offs.get() + s0, n, h_offs[s0], ep.row_words, pd.scr.get(), d_acc.get(),
                                                  sc.d_mant.get() + s0, sc.d_exp.get() + s0, sc.d_status.get() + s0, st))
                    return e2vq_set_error("%s: %d units of sum N = %d states in %d wave-slots cannot be launched", who, g.max_L, g.max_sumN,
                                          g.max_slots);
            } else if (e2hmm::launch_embed_fb(pd.plan(ep, s0, d_params.get()), ep.a_lds, ep.an_lds, ep.max_slots, d_sym, pd.offs.get() + s0,
                                              n, h_offs[s0], ep.row_words, pd.scr.get(), d_acc.get(), sc.d_mant.get() + s0,
                                              sc.d_exp.get() + s0, sc.d_status.get() + s0, st)) {
                return e2vq_set_error("%s: %d units in %d wave-slots cannot be launched", who, ep.max_L, ep.max_slots);
            }
            HIPCHK(hipGetLastError());
        }
        e2hmm::launch_embed_rowsum(pd.classes.get(), K, ep.max_N, d_acc.get(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(timer.stop.e, st));
        if (sc.download((size_t)S, st)) return 1;
        HIPCHK(hipStreamSynchronize(st));
        return timer.elapsed_ms(&g_embed_kernel_ms);
    }
    // M-step from d_acc: the models re-estimated in place (on the host, through the device).  Waits for the stream.
    int mstep(const EmbedPlan& ep, LoopModels& lm, double epsilon, hipStream_t st)
    {
        const int K = lm.K();
        dense.resize((size_t)ep.dense_words);
        for (int k = 0; k < K; ++k) lm.models[(size_t)k].pack(dense.data() + ep.classes[(size_t)k].param_at);
        if (d_dense.upload(dense.data(), dense.size(), st)) return 1;
        e2hmm::launch_reestimate_embedded(pd.classes.get(), K, lm.M, ep.max_P, ep.max_N, d_acc.get(), epsilon, d_dense.get(), st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dense.data(), d_dense.get(), dense.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < K; ++k) lm.models[(size_t)k].unpack(dense.data() + ep.classes[(size_t)k].param_at);
        return 0;
    }
};

struct EmbedIteration {
    double L;
    int used, skipped;
};

// The loop of the other trainers over the embedded E-step: per iteration one E-step over all streams and L = the sum of
// ln P over the status-0 streams in stream order; a stopping iteration gets no M-step.  on_estep (may be empty) sees every
// E-step's result before the decision.
int embed_train(const char* who, const EmbedPlan& ep, EmbedDev& dev, LoopModels& lm, double ln_switch, const unsigned short* d_sym,
                const i64* h_offs, hipStream_t st, double epsilon, double val_auto, int max_iterations, std::vector<EmbedIteration>& hist,
                const std::function<void(int, const EmbedIteration&, const Scores&)>& on_estep)
{
    const int S = (int)ep.ap.streams.size();
    double Lprev = 0.0;
    hist.clear();
    for (int it = 0;; ++it) {
        if ((max_iterations >= 0 && it >= max_iterations) || it >= EMBED_MAX_ESTEPS) break;
        if (dev.estep(who, ep, lm, ln_switch, d_sym, h_offs, st)) return 1;
        EmbedIteration e{0.0, 0, 0};
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
            return e2vq_set_error("%s: no stream can be explained by its transcript under the models (all %d skipped)", who, S);
        hist.push_back(e);
        if (it > 0 && e.L - Lprev <= val_auto) break;
        if (dev.mstep(ep, lm, epsilon, st)) return 1;
        Lprev = e.L;
    }
    return 0;
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

extern "C" int e2vq_hmm_embedded_last_kernel_ms(float* ms) { return last_kernel_ms("e2vq_hmm_embedded_last_kernel_ms", g_embed_kernel_ms, ms); }

extern "C" int e2vq_hmm_embedded_estep(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                       const double* const* Bs, const void* sym, const int64_t* offs, int S, const int32_t* units,
                                       const int64_t* unit_offs, const uint8_t* optional, double ln_switch, int64_t* const* acc,
                                       double* log_prob, int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_embedded_estep";
    LoopModels lm;
    if (transcript_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, units, unit_offs, lm)) return 1;
    if (!acc) return e2vq_set_error("%s: bad arguments", who);
    for (int k = 0; k < K; ++k)
        if (!acc[k]) return e2vq_set_error("%s: bad arguments", who);
    EmbedPlan ep;
    if (embed_plan(who, K, Ns, M, (const i64*)offs, S, units, (const i64*)unit_offs, optional, ln_switch, ep)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    EmbedDev dev;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0) || dev.setup(who, ep, (const i64*)offs, S, seqs.st.s) ||
        dev.estep(who, ep, lm, ln_switch, seqs.sym, (const i64*)offs, seqs.st.s))
        return 1;
    for (int k = 0; k < K; ++k)
        HIPCHK(hipMemcpyAsync(acc[k], dev.d_acc.get() + ep.acc_at[(size_t)k], (size_t)(ep.acc_at[(size_t)k + 1] - ep.acc_at[(size_t)k]) * 8,
                              hipMemcpyDeviceToHost, seqs.st.s));
    HIPCHK(hipStreamSynchronize(seqs.st.s));
    for (int s = 0; s < S; ++s) dev.sc.get((size_t)s, nullptr, nullptr, status ? status + s : nullptr, log_prob ? log_prob + s : nullptr);
    return 0;
}

extern "C" int e2vq_hmm_train_embedded(int device, int K, const int* Ns, int M, double* const* pis, double* const* As, double* const* Bs,
                                       const void* sym, const int64_t* offs, int S, const int32_t* units, const int64_t* unit_offs,
                                       const uint8_t* optional, double ln_switch, double epsilon, double val_auto, int max_iterations,
                                       double* sum_log_prob, int cap, int* num_esteps, int sym_on_device)
{
    const char* who = "e2vq_hmm_train_embedded";
    LoopModels lm;
    if (transcript_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, units, unit_offs, lm)) return 1;
    if (cap > 0 && !sum_log_prob) return e2vq_set_error("%s: bad arguments", who);
    EmbedPlan ep;
    if (embed_plan(who, K, Ns, M, (const i64*)offs, S, units, (const i64*)unit_offs, optional, ln_switch, ep)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    EmbedDev dev;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    std::vector<EmbedIteration> hist;
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0) || dev.setup(who, ep, (const i64*)offs, S, seqs.st.s) ||
        embed_train(who, ep, dev, lm, ln_switch, seqs.sym, (const i64*)offs, seqs.st.s, epsilon, val_auto, max_iterations, hist, nullptr))
        return 1;
    for (int k = 0; k < K; ++k) model_to_arrays(lm.models[(size_t)k], pis[k], As[k], Bs[k]);
    for (size_t i = 0; i < hist.size() && (int)i < cap; ++i) sum_log_prob[i] = hist[i].L;
    if (num_esteps) *num_esteps = (int)hist.size();
    return 0;
}

extern "C" int e2vq_hmm_learn_embedded_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                             const char* const* input_filenames, const char* const* label_filenames, int num_inputs,
                                             int P, int W_ms, int O_ms, double ln_switch, const char* filler_class, double hmm_epsilon,
                                             double val_auto, int max_iterations, const char* out_dir,
                                             void (*callback)(char* variable, double value))
{
    const char* who = "e2vq_hmm_learn_embedded_files";
    FlushStdout flush_on_return;
    LoopModels fm;
    if (files_given(who, model_filenames, num_models, input_filenames && label_filenames && num_inputs >= 1)) return 1;
    if (!out_dir || !*out_dir) return e2vq_set_error("%s: no output directory", who);
    if (window_ms_ok(who, W_ms, O_ms) || fm.load_checked(who, model_filenames, num_models)) return 1;
    const int K = fm.K();
    if (check_names(who, K, fm.names.data())) return 1;
    Transcripts tr;
    if (tr.set_filler(who, fm, filler_class)) return 1;
    if (fm.logs(model_filenames)) return 1;
    std::vector<std::string> out_paths;
    if (model_out_paths(who, out_dir, fm, model_filenames, num_models, out_paths)) return 1;
    SymInputs si;
    if (sym_inputs_check(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, nullptr, si)) return 1;
    for (int f = 0; f < num_inputs; ++f) {
        if (tr.add_labels(who, fm, label_filenames[f])) return 1;
        // (with the frame count known so far: a .wav may still lose frames, which only shrinks the tables)
        const i64 offs1[2] = {0, si.inputs[(size_t)f].T}, uoffs1[2] = {0, tr.L(f)};
        EmbedPlan ep1;
        if (embed_plan(who, K, fm.Ns.data(), fm.M, offs1, 1, tr.u(f), uoffs1, tr.o(f), ln_switch, ep1))
            return e2vq_set_error("%s: %s", label_filenames[f], std::string(e2vq_last_error()).c_str());
    }
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    DeviceBuffer<unsigned short> d_all;
    EmbedDev dev;
    EmbedPlan ep;  // (before the stage, as the offsets: its stream copies from them)
    std::vector<i64> offs(1, 0);
    SymStage stg;
    if (require_device(device) || stg.open(device, si)) return 1;
    if (stg.gather(who, si, P, W_ms, O_ms, d_all, offs)) return 1;
    if (embed_plan(who, K, fm.Ns.data(), fm.M, offs.data(), num_inputs, tr.units.data(), tr.unit_offs.data(), tr.optional.data(), ln_switch, ep)) return 1;
    if (dev.setup(who, ep, offs.data(), num_inputs, stg.st.s)) return 1;
    const bool verbose = getenv("ECOZ2_VQ_QUIET") == nullptr;
    static char var[] = "sum_log_prob";
    printf("\nHMM learn --embedded: %d class(es)  M=%d  #streams = %d  #units = %lld  frames = %lld\n", K, fm.M, num_inputs,
           (long long)tr.unit_offs.back(), (long long)offs.back());
    printf("  switch penalty=%g  filler=%s  epsilon=%g  val_auto=%g  max_iterations=%d\n", ln_switch, tr.filler >= 0 ? fm.names[(size_t)tr.filler] : "(none)",
           hmm_epsilon, val_auto, max_iterations);
    std::vector<EmbedIteration> hist;
    std::vector<int> last_status((size_t)num_inputs, 0);
    auto on_estep = [&](int it, const EmbedIteration& e, const Scores& sc) {
        // a stream is named whenever its status changes: skipped from the start, lost after an M-step, or used again
        for (int f = 0; f < num_inputs; ++f) {
            const int stf = sc.status.get()[f];
            if (stf == last_status[(size_t)f]) continue;
            last_status[(size_t)f] = stf;
            fprintf(stderr, "%s: it=%d: %s\n", si.inputs[(size_t)f].path.c_str(), it,
                    stf == 0   ? "used again"
                    : stf == 2 ? "skipped: a symbol outside the models' alphabet"
                               : "skipped: no path of probability > 0 through its transcript");
        }
        if (verbose)
            printf("  it=%d  sum log(P) = %.10g%s\n", it, e.L,
                   e.skipped ? (" (" + std::to_string(e.skipped) + " stream(s) skipped)").c_str() : "");
        if (callback) callback(var, e.L);
    };
    if (embed_train(who, ep, dev, fm, ln_switch, d_all.get(), offs.data(), stg.st.s, hmm_epsilon, val_auto, max_iterations, hist, on_estep))
        return 1;
    for (int k = 0; k < K; ++k)
        if (hmm_save(out_paths[(size_t)k], fm.models[(size_t)k])) return 1;
    std::string csv = "iteration,sum_log_prob,streams_used,streams_skipped\n";
    for (size_t i = 0; i < hist.size(); ++i)
        csv += std::to_string(i) + "," + fmt_17g(hist[i].L) + "," + std::to_string(hist[i].used) + "," + std::to_string(hist[i].skipped) + "\n";
    const std::string csv_path = std::string(out_dir) + "/embedded.csv";
    if (write_file(csv_path, std::vector<unsigned char>(csv.begin(), csv.end()))) return 1;
    printf("%zu E-step(s); %d model(s) saved in %s; %s saved\n", hist.size(), K, out_dir, csv_path.c_str());
    return 0;
}
