// hmm_trans_train.cpp -- Baum-Welch for the matrix of class-to-class prices (`hmm transitions --em`,
// e2vq_hmm_transitions_estep, e2vq_hmm_train_transitions): the grammar of the class loop re-estimated from
// whole unlabelled streams, over the kernel of hmm_trans_estep.hip or, above 16 wave-slots or on request
// (ECOZ2_HMM_TRANS_FB_BODY), its looped body hmm_trans_estep_looped.hip.  The host takes exp of the prices, chooses the LDS layout
// and the route of the count table (all before any HIP call), takes the logarithm of the (mantissa, exponent) pairs, sums
// ln P over the streams in stream order, forms the M-step (K^2 values) and decides when to stop.  The checks, the packing, the
// parameter block, the prices, the choice of the body with its slot check and the forward table are hmm_class_loop.cpp's, the
// file of the matrix hmm_transitions.cpp's, the input stage hmm_input.cpp's (hmm_host.h).
#include "hmm_host.h"
#include "vq_fixed.h"

namespace e2hmm_host {

// ---- what hmm_loop_train.cpp shares (hmm_host.h) ----------------------------------------------------------------------------
int trans_check_alpha(const char* who, double alpha)
{
    if (!(alpha >= 0.0) || !std::isfinite(alpha)) return e2vq_set_error("%s: alpha = %g: a finite number, at least 0", who, alpha);
    return 0;
}

// The M-step of 4.8.14 (host; K^2 values): row f of ln_p from the counts.  A -inf entry stays; a row without mass keeps its bytes.
void trans_mstep(int K, const i64* acc, double alpha, double* ln_p)
{
    for (int f = 0; f < K; ++f) {
        const i64* row = acc + (size_t)f * K * 2;
        double* lp = ln_p + (size_t)f * K;
        i64 hi = 0, lo = 0;
        int n = 0;
        for (int k = 0; k < K; ++k) {
            hi += row[2 * k];
            lo += row[2 * k + 1];
            n += lp[k] != -INFINITY;
        }
        const double den = e2vq::unfix(hi, lo, e2hmm::ACC_SHIFT) + alpha * (double)n;
        if (!(den > 0.0)) continue;
        for (int k = 0; k < K; ++k)
            if (lp[k] != -INFINITY) lp[k] = log((e2vq::unfix(row[2 * k], row[2 * k + 1], e2hmm::ACC_SHIFT) + alpha) / den);
    }
}

namespace {

thread_local float g_trans_estep_kernel_ms = -1.f;  // e2vq_hmm_transitions_estep_last_kernel_ms

constexpr int TRANS_MAX_ESTEPS = 1000;  // the safety cap of the other trainers (hmm_train.cpp: MAX_ESTEPS)

inline i64 trans_acc_words(int K) { return 2 * (i64)K * K + 2; }

// What the host decides about a call before the device is touched: the packing, the LDS layout and the route of the C table
// (ECOZ2_HMM_TRANS_EM_C: lds or global; unset: LDS when the table fits next to the mandatory terms).
struct TransPlan {
    SegPacking pk;
    bool looped = false;  // the body of every E-step of the call (ECOZ2_HMM_TRANS_FB_BODY, read once)
    int waves = 0;        // of a workgroup: each stores its copy of c_t
    bool c_lds = false, a_lds = false, w_lds = false;
};

// body: what trans_fb_body gave; the slot check holds it against the mandatory LDS of hmm_trans_estep_looped.hip (DESIGN.md
// 4.8.14: 132 096 bytes at K = sum N = 4096).
int trans_plan(const char* who, const std::vector<int>& Ns, int M, LoopBody body, TransPlan& tp)
{
    const int K = (int)Ns.size();
    tp.pk = pack_slots(Ns, posteriors_a_ld);
    tp.looped = runs_looped(body, tp.pk.slots);
    tp.waves = body_waves(tp.looped, tp.pk.slots);
    const e2hmm::SegPlanDev shape = loop_shape(tp.pk, K, M);
    if (check_body_slots(who, tp.pk, K, body, "the E-step of the class transitions has", "the E-step of the class transitions",
                         e2hmm::trans_estep_looped_lds_bytes(shape, false, false, false)))
        return 1;
    // (the two bodies' formulas and decision orders have one signature)
    const auto lds_bytes = tp.looped ? e2hmm::trans_estep_looped_lds_bytes : e2hmm::trans_estep_lds_bytes;
    const auto layout = tp.looped ? e2hmm::trans_estep_looped_layout : e2hmm::trans_estep_layout;
    bool forced = false;
    if (embed_route("ECOZ2_HMM_TRANS_EM_C", &forced, &tp.c_lds)) return 1;
    layout(shape, forced, &tp.c_lds, &tp.a_lds, &tp.w_lds);
    const size_t lds = lds_bytes(shape, tp.c_lds, tp.a_lds, tp.w_lds);
    if (lds > e2hmm::SEG_LDS_BYTES)
        return e2vq_set_error("%s: %d classes of %d states with the count table in LDS take %zu bytes of LDS (at most %zu)", who, K,
                              tp.pk.sumN, lds, (size_t)e2hmm::SEG_LDS_BYTES);
    return 0;
}

// The device side of a planned call: the tables, the scratch and the accumulator, kept over the iterations of a training.
struct TransDev {
    ClassLoopDev loop;
    Scores sc;  // P(O | loop) of each stream
    ForwardTable ft;  // 4.8.13's, bounded by whole streams in the same way
    DeviceBuffer<double> d_w;
    DeviceBuffer<i64> d_offs, d_acc;
    std::vector<double> params, w;
    std::vector<i64> acc;  // the counts of the last E-step: 2 K^2 + 2 words
    KernelTimer timer;

    int setup(const char* who, const TransPlan& tp, const LoopModels& lm, const i64* h_offs, int S, hipStream_t st)
    {
        const int K = lm.K();
        params = trans_params(lm, tp.pk);
        return loop.upload(tp.pk, params, K, lm.M, st) || d_offs.upload(h_offs, (size_t)S + 1, st) || sc.reserve((size_t)S) ||
               d_acc.reserve((size_t)trans_acc_words(K)) || d_w.reserve((size_t)2 * K * K) || timer.create() ||
               ft.reserve(who, tp.pk.sumN, tp.waves, 0, h_offs, S);
    }
    // One E-step under the effective prices lt: the counts of all streams in `acc` (from zero), P and status of every stream
    // in sc's host mirrors.  Waits for the stream.
    int estep(const char* who, const TransPlan& tp, const double* lt, const unsigned short* d_sym, const i64* h_offs, int S,
              hipStream_t st)
    {
        const int K = loop.pl.K;
        const size_t words = (size_t)trans_acc_words(K);
        w = trans_prices(K, lt);
        if (d_w.upload(w.data(), w.size(), st)) return 1;
        HIPCHK(hipMemsetAsync(d_acc.get(), 0, words * 8, st));
        HIPCHK(hipEventRecord(timer.start.e, st));
        // (one stream: a chunk's forward pass writes the tables only after the previous chunk's backward pass has read them)
        for (const auto& c : ft.chunks) {
            const int s0 = c.first, n = c.second - c.first;
            const auto launch = tp.looped ? e2hmm::launch_trans_estep_looped : e2hmm::launch_trans_estep;
            if (launch(loop.pl, tp.c_lds, tp.a_lds, tp.w_lds, d_sym, d_offs.get() + s0, n, h_offs[s0], d_w.get(), ft.d_ah.get(), ft.d_c.get(),
                       d_acc.get(), sc.d_mant.get() + s0, sc.d_exp.get() + s0, sc.d_status.get() + s0, st))
                return e2vq_set_error("%s: %d wave-slots of %d states cannot be launched", who, tp.pk.slots, tp.pk.sumN);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(timer.stop.e, st));
        acc.resize(words);
        HIPCHK(hipMemcpyAsync(acc.data(), d_acc.get(), words * 8, hipMemcpyDeviceToHost, st));
        if (sc.download((size_t)S, st)) return 1;
        HIPCHK(hipStreamSynchronize(st));
        return timer.elapsed_ms(&g_trans_estep_kernel_ms);
    }
};

struct TransIteration {
    double L;
    int used, skipped;
};

// The loop of the other trainers over this E-step: per iteration one E-step over all streams under ln_p + ln_switch and L =
// the sum of ln P over the status-0 streams in stream order; a stopping iteration gets no M-step.  on_estep (may be empty)
// sees every E-step's result before the decision.  Where no stream has status 0 after the first E-step, ln_p is as it came.
int trans_train(const char* who, const TransPlan& tp, TransDev& dev, double* ln_p, double ln_switch, double alpha,
                const unsigned short* d_sym, const i64* h_offs, int S, hipStream_t st, double val_auto, int max_iterations,
                std::vector<TransIteration>& hist, const std::function<void(int, const TransIteration&, const Scores&)>& on_estep)
{
    const int K = dev.loop.pl.K;
    std::vector<double> eff((size_t)K * K);
    double Lprev = 0.0;
    hist.clear();
    for (int it = 0;; ++it) {
        if ((max_iterations >= 0 && it >= max_iterations) || it >= TRANS_MAX_ESTEPS) break;
        for (size_t i = 0; i < eff.size(); ++i) eff[i] = ln_p[i] + ln_switch;  // the effective price, as --class-transitions forms it
        if (dev.estep(who, tp, eff.data(), d_sym, h_offs, S, st)) return 1;
        TransIteration e{0.0, 0, 0};
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
        trans_mstep(K, dev.acc.data(), alpha, ln_p);
        Lprev = e.L;
    }
    return 0;
}

// the first checks of the array-level entry points: the arguments, the shapes, the prices, the slots, the models
int trans_check_args(const char* who, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                     const double* const* Bs, const void* sym, const int64_t* offs, int S, const double* lt, bool rest, LoopModels& lm,
                     TransPlan& tp)
{
    LoopBody body = LoopBody::Resident;  // (read once a call: a training keeps it over its E-steps)
    if (loop_check_args(who, K, Ns, pis, As, Bs, lt && rest && syms_given(sym, offs, S)) || segment_check_shape(who, K, Ns) ||
        trans_check_lt(who, K, lt) || trans_fb_body(&body) || trans_plan(who, std::vector<int>(Ns, Ns + K), M, body, tp) ||
        lm.from_arrays(K, Ns, M, pis, As, Bs))
        return 1;
    for (const Hmm& h : lm.models)
        if (posteriors_check_params(h)) return 1;
    return check_offsets(offs, S);
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

extern "C" int64_t e2vq_hmm_transitions_acc_words(int K) { return K < 1 ? 0 : (int64_t)trans_acc_words(K); }

extern "C" int e2vq_hmm_transitions_estep_last_kernel_ms(float* ms)
{
    return last_kernel_ms("e2vq_hmm_transitions_estep_last_kernel_ms", g_trans_estep_kernel_ms, ms);
}

extern "C" int e2vq_hmm_transitions_estep(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                          const double* const* Bs, const void* sym, const int64_t* offs, int S, const double* lt,
                                          int64_t* acc, double* log_prob, int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_transitions_estep";
    LoopModels lm;
    TransPlan tp;
    if (trans_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, lt, acc != nullptr, lm, tp)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    TransDev dev;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0) || dev.setup(who, tp, lm, (const i64*)offs, S, seqs.st.s) ||
        dev.estep(who, tp, lt, seqs.sym, (const i64*)offs, S, seqs.st.s))
        return 1;
    for (size_t i = 0; i < dev.acc.size(); ++i) acc[i] += dev.acc[i];
    dev.sc.get_all((size_t)S, status, log_prob);
    return 0;
}

extern "C" int e2vq_hmm_train_transitions(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                          const double* const* Bs, const void* sym, const int64_t* offs, int S, double* ln_p,
                                          double ln_switch, double alpha, double val_auto, int max_iterations, double* sum_log_prob,
                                          int cap, int* num_esteps, void (*callback)(char* variable, double value), int sym_on_device)
{
    const char* who = "e2vq_hmm_train_transitions";
    LoopModels lm;
    TransPlan tp;
    if (trans_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, ln_p, !(cap > 0 && !sum_log_prob), lm, tp) ||
        segment_check_switch(who, ln_switch) || trans_check_alpha(who, alpha))
        return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    TransDev dev;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    std::vector<TransIteration> hist;
    std::vector<double> p(ln_p, ln_p + (size_t)K * K);
    static char var[] = "sum_log_prob";
    auto on_estep = [&](int, const TransIteration& e, const Scores&) {
        if (callback) callback(var, e.L);
    };
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0) || dev.setup(who, tp, lm, (const i64*)offs, S, seqs.st.s) ||
        trans_train(who, tp, dev, p.data(), ln_switch, alpha, seqs.sym, (const i64*)offs, S, seqs.st.s, val_auto, max_iterations, hist,
                    on_estep))
        return 1;
    std::copy(p.begin(), p.end(), ln_p);
    for (size_t i = 0; i < hist.size() && (int)i < cap; ++i) sum_log_prob[i] = hist[i].L;
    if (num_esteps) *num_esteps = (int)hist.size();
    return 0;
}

extern "C" int e2vq_hmm_learn_transitions_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                                const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                                double ln_switch, const char* init_csv, double alpha, double val_auto,
                                                int max_iterations, const char* out_csv)
{
    const char* who = "e2vq_hmm_learn_transitions_files";
    FlushStdout flush_on_return;
    LoopModels lm;
    TransPlan tp;
    if (files_given(who, model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
    if (!out_csv || !*out_csv) return e2vq_set_error("%s: no output file", who);
    if (segment_check_switch(who, ln_switch) || trans_check_alpha(who, alpha) || window_ms_ok(who, W_ms, O_ms) ||
        lm.load_checked(who, model_filenames, num_models))
        return 1;
    const int K = lm.K();
    LoopBody body = LoopBody::Resident;  // (read once, before the first E-step)
    if (trans_fb_body(&body) || trans_plan(who, lm.Ns, lm.M, body, tp) || check_names(who, K, lm.names.data())) return 1;
    for (unsigned k = 0; k < num_models; ++k)
        if (posteriors_check_params(lm.models[k])) return e2vq_set_error("%s: %s", model_filenames[k], std::string(e2vq_last_error()).c_str());
    // the start: the file's matrix, or every succession as likely as any other
    std::vector<double> ln_p((size_t)K * K, log(1.0 / K));
    if (init_csv && *init_csv && transitions_read(init_csv, K, lm.names.data(), ln_p)) return 1;
    SymInputs si;
    if (sym_inputs_check(who, lm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, nullptr, si)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    DeviceBuffer<unsigned short> d_all;
    TransDev dev;
    std::vector<i64> offs(1, 0);  // (before the stage: its stream copies from them)
    SymStage stg;
    if (require_device(device) || stg.open(device, si)) return 1;
    if (stg.gather(who, si, P, W_ms, O_ms, d_all, offs)) return 1;
    if (dev.setup(who, tp, lm, offs.data(), num_inputs, stg.st.s)) return 1;
    const bool verbose = getenv("ECOZ2_VQ_QUIET") == nullptr;
    printf("\nHMM transitions --em: %d class(es)  M=%d  #streams = %d  frames = %lld\n", K, lm.M, num_inputs, (long long)offs.back());
    printf("  switch penalty=%g  init=%s  alpha=%g  val_auto=%g  max_iterations=%d\n", ln_switch, init_csv && *init_csv ? init_csv : "(uniform)",
           alpha, val_auto, max_iterations);
    std::vector<TransIteration> hist;
    std::vector<int> last_status((size_t)num_inputs, 0);
    auto on_estep = [&](int it, const TransIteration& e, const Scores& sc) {
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
    };
    if (trans_train(who, tp, dev, ln_p.data(), ln_switch, alpha, d_all.get(), offs.data(), num_inputs, stg.st.s, val_auto, max_iterations,
                    hist, on_estep))
        return 1;
    if (e2vq_hmm_transitions_write(out_csv, K, lm.names.data(), ln_p.data())) return 1;
    std::string csv = "iteration,sum_log_prob,streams_used,streams_skipped\n";
    for (size_t i = 0; i < hist.size(); ++i)
        csv += std::to_string(i) + "," + fmt_17g(hist[i].L) + "," + std::to_string(hist[i].used) + "," + std::to_string(hist[i].skipped) + "\n";
    const std::string csv_path = std::string(out_csv) + ".em.csv";
    if (write_file(csv_path, std::vector<unsigned char>(csv.begin(), csv.end()))) return 1;
    printf("%zu E-step(s); %s saved (alpha %g, %d classes); %s saved\n", hist.size(), out_csv, alpha, K, csv_path.c_str());
    return 0;
}
