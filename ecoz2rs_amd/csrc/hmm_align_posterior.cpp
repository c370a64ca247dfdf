// hmm_align_posterior.cpp -- how sure the alignment is (`hmm align --posteriors`, e2vq_hmm_align_posteriors):
// per unit and frame the posterior that the unit holds the frame, per unit the probability that a path visits it and the mean
// and spread of the frame it is entered at, over the kernels of hmm_align_posterior.hip (the resident body) and
// hmm_align_posterior_looped.hip (the looped body, which ECOZ2_HMM_ALIGN_POSTERIOR_BODY opts into).  The host adds the body, the
// places of the occupancies and each launch's LDS layout to hmm_transcript.cpp's plan of the embedded forward-backward pass (all
// before any HIP call), takes the logarithm of the (mantissa, exponent) pairs and the unit moments, and writes the reports.
// The checks, the transcripts of the label files, the plan, the parameter block and the reports' common parts are
// hmm_transcript.cpp's (hmm_host.h).
#include "hmm_host.h"

namespace e2hmm_host {
namespace {

thread_local float g_align_post_kernel_ms = -1.f;  // e2vq_hmm_align_posteriors_last_kernel_ms

// What the host decides about a call before the device is touched: the plan of the forward-backward pass, whether A goes to
// LDS (the resident launches share one layout, a launch of the looped body has its own), and where each stream's occupancies
// begin.
struct PostPlan : EStepPlan {
    std::vector<i64> occ_at;        // [S + 1]
    std::vector<uint8_t> loop_a_lds;  // per chunk: A in LDS, of a launch of the looped body
};

int post_plan(const char* who, int K, const int* Ns, int M, const i64* offs, int S, const int32_t* units, const i64* unit_offs,
              const uint8_t* optional, double ln_switch, PostPlan& pp)
{
    // ECOZ2_HMM_ALIGN_POSTERIOR_BODY: unset or "resident" keeps every stream resident and every refusal as it was
    LoopBody body = LoopBody::Resident;
    if (align_post_body(&body)) return 1;
    if (estep_plan(who, K, Ns, M, offs, S, units, unit_offs, optional, ln_switch, "the alignment posteriors have a resident body only", false,
                   body, pp, /*looped_unit_bytes=*/3 * sizeof(double)))
        return 1;
    pp.occ_at.assign((size_t)S + 1, 0);
    for (int s = 0; s < S; ++s) pp.occ_at[(size_t)s + 1] = pp.occ_at[(size_t)s] + (offs[s + 1] - offs[s]) * pp.ap.streams[(size_t)s].L;
    // A in LDS when it fits; ECOZ2_HMM_EMBED_A = lds | global forces either, as in the E-step
    const int aw = pp.cls.a_words;
    // the launches of the looped body: each by its own largest shapes
    const bool a_said = pp.a_lds;  // what the variable forces
    pp.loop_a_lds.assign(pp.chunks.size(), 0);
    for (size_t i = 0; i < pp.chunks.size(); ++i) {
        const EStepPlan::Shape& g = pp.shapes[i];
        if (!g.looped) continue;
        auto bytes = [&](bool a) { return e2hmm::align_post_looped_lds_bytes(g.max_L, g.max_slots, g.max_sumN, aw, a); };
        const bool a = pp.a_forced ? a_said : bytes(true) <= e2hmm::SEG_LDS_BYTES;
        pp.loop_a_lds[i] = a ? 1 : 0;
        if (bytes(a) > e2hmm::SEG_LDS_BYTES)
            return e2vq_set_error("%s: streams %d to %d: %d units of sum N = %d states in %d wave-slots and A in %s take %zu bytes of LDS "
                                  "(at most %zu)", who, pp.chunks[i].first, pp.chunks[i].second - 1, g.max_L, g.max_sumN, g.max_slots,
                                  a ? "LDS" : "global memory", bytes(a), e2hmm::SEG_LDS_BYTES);
    }
    // the launches of the resident body: one layout for all of them, by the most units of their streams
    if (!pp.a_forced) pp.a_lds = e2hmm::align_post_lds_bytes(pp.max_L, aw, true) <= e2hmm::SEG_LDS_BYTES;
    const size_t lds = e2hmm::align_post_lds_bytes(pp.max_L, aw, pp.a_lds);
    const bool resident_runs = S == 0 || std::count(pp.looped.begin(), pp.looped.end(), 0) > 0;
    if (lds > e2hmm::SEG_LDS_BYTES && resident_runs)
        return e2vq_set_error("%s: %d units and A in %s take %zu bytes of LDS (at most %zu)", who, pp.max_L, pp.a_lds ? "LDS" : "global memory",
                              lds, e2hmm::SEG_LDS_BYTES);
    return 0;
}

// every ref[l] of every stream in [0, T) (ref may be null; a stream without frames reads none)
int post_check_ref(const char* who, const i64* offs, int S, const i64* unit_offs, const int64_t* ref)
{
    for (int s = 0; s < S && ref; ++s) {
        const i64 T = offs[s + 1] - offs[s];
        for (i64 x = unit_offs[s]; x < unit_offs[s + 1] && T > 0; ++x)
            if (ref[x] < 0 || ref[x] >= T)
                return e2vq_set_error("%s: stream %d, unit %lld: ref = %lld outside [0, %lld)", who, s, (long long)(x - unit_offs[s]),
                                      (long long)ref[x], (long long)T);
    }
    return 0;
}

struct PostOut {  // host arrays, any may be null; occ: sum T L; post_path: per frame; w0 .. w2: per unit; the rest per stream
    double* occ = nullptr;
    double* post_path = nullptr;
    double* w0 = nullptr;
    double* w1 = nullptr;
    double* w2 = nullptr;
    double* log_prob = nullptr;
    int* status = nullptr;
};

// The posteriors of S device-resident streams (h_offs: their S + 1 offsets, on the host) as planned by post_plan, on the
// current device and the stream st.  path_unit / ref: host arrays or null.  Waits for the stream.
int post_device(const char* who, const PostPlan& pp, const LoopModels& lm, const unsigned short* d_sym, const i64* h_offs, int S,
                const i64* unit_offs, double ln_switch, const uint16_t* path_unit, const int64_t* ref, hipStream_t st, const PostOut& out)
{
    const i64 frames = h_offs[S], nunits = unit_offs[S], nocc = out.occ ? pp.occ_at[(size_t)S] : 0;
    const std::vector<double> params = embed_params(lm, pp.cls, exp(ln_switch));
    EStepDev pd;
    DeviceBuffer<unsigned short> d_path;
    DeviceBuffer<i64> d_occ_at, d_ref;
    DeviceBuffer<double> d_params, d_occ, d_post, d_w;
    Scores sc;
    KernelTimer timer;
    if (pd.upload(pp, h_offs, S, st) || d_occ_at.upload(pp.occ_at.data(), pp.occ_at.size(), st) ||
        d_params.upload(params.data(), params.size(), st) || (path_unit && frames > 0 && d_path.upload(path_unit, (size_t)frames, st)) ||
        (ref && nunits > 0 && d_ref.upload((const i64*)ref, (size_t)nunits, st)) || d_post.reserve((size_t)std::max<i64>(frames, 1)) ||
        d_w.reserve((size_t)std::max<i64>(3 * nunits, 1)) || (nocc > 0 && d_occ.reserve((size_t)nocc)) || sc.reserve((size_t)S) ||
        timer.create() || pd.scratch(who, pp))
        return 1;
    // (+0.0 everywhere: what a stream of status != 0 and a frame without a unit keep)
    HIPCHK(hipMemsetAsync(d_post.get(), 0, (size_t)std::max<i64>(frames, 1) * 8, st));
    HIPCHK(hipMemsetAsync(d_w.get(), 0, (size_t)std::max<i64>(3 * nunits, 1) * 8, st));
    if (nocc > 0) HIPCHK(hipMemsetAsync(d_occ.get(), 0, (size_t)nocc * 8, st));
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes the scratch only after the previous chunk's backward pass has read it)
    for (size_t i = 0; i < pp.chunks.size(); ++i) {
        const int s0 = pp.chunks[i].first, n = pp.chunks[i].second - s0;
        const EStepPlan::Shape& g = pp.shapes[i];
        const e2hmm::AlignPostDev po{path_unit && frames > 0 ? d_path.get() : nullptr, ref && nunits > 0 ? d_ref.get() : nullptr,
                                     d_occ_at.get() + s0, nocc > 0 ? d_occ.get() : nullptr, d_post.get(), d_w.get(), nunits};
        if (g.looped) {
            e2hmm::EmbedPlanDev pl = pd.plan(pp, s0, d_params.get());
            pl.max_L = g.max_L;
            if (e2hmm::launch_align_posteriors_looped(pl, pp.loop_a_lds[i] != 0, g.max_slots, g.max_sumN, d_sym, pd.offs.get() + s0, n,
                                                      h_offs[s0], pp.row_words, pd.scr.get(), po, sc.d_mant.get() + s0,
                                                      sc.d_exp.get() + s0, sc.d_status.get() + s0, st))
                return e2vq_set_error("%s: %d units of sum N = %d states in %d wave-slots cannot be launched", who, g.max_L, g.max_sumN,
                                      g.max_slots);
        } else if (e2hmm::launch_align_posteriors(pd.plan(pp, s0, d_params.get()), pp.a_lds, pp.max_slots, d_sym, pd.offs.get() + s0, n,
                                                  h_offs[s0], pp.row_words, pd.scr.get(), po, sc.d_mant.get() + s0, sc.d_exp.get() + s0,
                                                  sc.d_status.get() + s0, st)) {
            return e2vq_set_error("%s: %d units in %d wave-slots cannot be launched", who, pp.max_L, pp.max_slots);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    if (sc.download((size_t)S, st)) return 1;
    if (out.occ && nocc > 0) HIPCHK(hipMemcpyAsync(out.occ, d_occ.get(), (size_t)nocc * 8, hipMemcpyDeviceToHost, st));
    if (out.post_path && frames > 0) HIPCHK(hipMemcpyAsync(out.post_path, d_post.get(), (size_t)frames * 8, hipMemcpyDeviceToHost, st));
    double* const w[3] = {out.w0, out.w1, out.w2};
    for (int i = 0; i < 3; ++i)
        if (w[i] && nunits > 0) HIPCHK(hipMemcpyAsync(w[i], d_w.get() + (size_t)i * nunits, (size_t)nunits * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (timer.elapsed_ms(&g_align_post_kernel_ms)) return 1;
    sc.get_all((size_t)S, out.status, out.log_prob);
    return 0;
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

extern "C" int e2vq_hmm_align_posteriors_last_kernel_ms(float* ms)
{
    return last_kernel_ms("e2vq_hmm_align_posteriors_last_kernel_ms", g_align_post_kernel_ms, ms);
}

extern "C" int e2vq_hmm_align_posteriors(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                         const double* const* Bs, const void* sym, const int64_t* offs, int S, const int32_t* units,
                                         const int64_t* unit_offs, const uint8_t* optional, double ln_switch, const uint16_t* path_unit,
                                         const int64_t* ref, double* occ, double* post_path, double* w0, double* w1, double* w2,
                                         double* log_prob, int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_align_posteriors";
    LoopModels lm;
    if (transcript_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, units, unit_offs, lm)) return 1;
    PostPlan pp;
    if (post_plan(who, K, Ns, M, (const i64*)offs, S, units, (const i64*)unit_offs, optional, ln_switch, pp) ||
        post_check_ref(who, (const i64*)offs, S, (const i64*)unit_offs, ref))
        return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    DevSeqs seqs;
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0)) return 1;
    PostOut out;
    out.occ = occ, out.post_path = post_path, out.w0 = w0, out.w1 = w1, out.w2 = w2, out.log_prob = log_prob, out.status = status;
    return post_device(who, pp, lm, seqs.sym, (const i64*)offs, S, (const i64*)unit_offs, ln_switch, path_unit, ref, seqs.st.s, out);
}

extern "C" int e2vq_hmm_align_unit_moments(int64_t n, const double* w0, const double* w1, const double* w2, const int64_t* ref,
                                           double* present, double* begin_mean, double* begin_sd)
{
    if (n < 0 || (n > 0 && (!w0 || !w1 || !w2))) return e2vq_set_error("e2vq_hmm_align_unit_moments: bad arguments");
    for (int64_t i = 0; i < n; ++i) {
        if (present) present[i] = w0[i];
        double mean = NAN, sd = NAN;
        if (w0[i] > 0.0) {
            const double q = w1[i] / w0[i];
            mean = (double)(ref ? ref[i] : 0) + q;
            const double v = w2[i] / w0[i] - q * q;
            sd = sqrt(v > 0.0 ? v : 0.0);
        }
        if (begin_mean) begin_mean[i] = mean;
        if (begin_sd) begin_sd[i] = sd;
    }
    return 0;
}

extern "C" int e2vq_hmm_align_report_posteriors(const char* name, int64_t T, int K, const char* const* class_names, int W_ms, int O_ms,
                                                int L, const int32_t* units, const uint8_t* optional, const int64_t* begin,
                                                const int64_t* end, const double* score, double log_prob, double ln_switch,
                                                const uint16_t* path_unit, const double* post_path, const double* w0, const double* w1,
                                                const double* w2, const int64_t* ref, const char* csv_filename,
                                                const char* frames_csv_filename)
{
    const char* who = "e2vq_hmm_align_report_posteriors";
    FlushStdout flush_on_return;
    const bool frames = frames_csv_filename && *frames_csv_filename;
    const int skipped = align_report_check(who, name, T, K, class_names, L, units, optional, begin, end, score,
                                           (T <= 0 || post_path) && w0 && w1 && w2);
    if (skipped < 0) return 1;
    if (frames && T > 0 && !path_unit) return e2vq_set_error("%s: the per-frame table needs the path's units", who);
    for (int64_t t = 0; t < T && frames; ++t)
        if (path_unit[t] != 0xFFFF && path_unit[t] >= L) return e2vq_set_error("%s: frame %lld names a unit outside [0, %d)", who, (long long)t, L);
    std::vector<double> present((size_t)L), bmean((size_t)L), bsd((size_t)L), mean((size_t)L, 0.0), least((size_t)L, 0.0);
    if (e2vq_hmm_align_unit_moments(L, w0, w1, w2, ref, present.data(), bmean.data(), bsd.data())) return 1;
    for (int l = 0; l < L; ++l) {  // the path's posterior over the unit's frames: a serial sum in frame order, then one division
        if (begin[l] < 0) continue;
        double sum = 0.0, mn = post_path[begin[l]];
        for (int64_t t = begin[l]; t < end[l]; ++t) {
            const double v = post_path[t];
            sum = sum + v;
            if (v < mn) mn = v;
        }
        mean[(size_t)l] = sum / (double)(end[l] - begin[l]);
        least[(size_t)l] = mn;
    }
    if (csv_filename && *csv_filename) {
        std::string doc = "unit,class,begin_frame,end_frame,begin_s,end_s,score,posterior,min_posterior,p_present,begin_mean_frame,begin_sd_frames\n";
        for (int l = 0; l < L; ++l) {
            if (begin[l] < 0) continue;
            doc += std::to_string(l) + "," + class_names[units[l]] + "," + std::to_string(begin[l]) + "," + std::to_string(end[l]) + "," +
                   fmt_17g(align_time_s(begin[l], O_ms)) + "," + fmt_17g(align_time_s(end[l] - 1, O_ms, W_ms)) + "," +
                   fmt_17g(align_unit_score(score, begin, end, l, ln_switch)) + "," + fmt_17g(mean[(size_t)l]) + "," + fmt_17g(least[(size_t)l]) + "," + fmt_17g(present[(size_t)l]) + "," + fmt_17g(bmean[(size_t)l]) + "," +
                   fmt_17g(bsd[(size_t)l]) + "\n";
        }
        if (write_file(csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    if (frames) {
        std::string doc = "frame,begin_s,unit,class,posterior\n";
        for (int64_t t = 0; t < T; ++t) {
            const bool named = path_unit[t] != 0xFFFF;
            doc += std::to_string(t) + "," + fmt_17g(align_time_s(t, O_ms)) + "," + (named ? std::to_string(path_unit[t]) : std::string("-1")) + "," +
                   (named ? class_names[units[path_unit[t]]] : "") + "," + fmt_17g(post_path[t]) + "\n";
        }
        if (write_file(frames_csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    align_report_head(name, T, K, class_names, L, units, begin, end, skipped, log_prob, ln_switch);
    for (int l = 0; l < L; ++l) {
        if (begin[l] >= 0) printf("    %.3f - %.3f %s p=%.3f\n", align_time_s(begin[l], O_ms), align_time_s(end[l] - 1, O_ms, W_ms), class_names[units[l]],
                   mean[(size_t)l]);
        else printf("    (passed over) %s p_present=%.3f\n", class_names[units[l]], present[(size_t)l]);
    }
    if (csv_filename && *csv_filename) printf("  %s saved\n", csv_filename);
    if (frames) printf("  %s saved\n", frames_csv_filename);
    return 0;
}

extern "C" int e2vq_hmm_align_files_posteriors(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                               const char* const* input_filenames, const char* const* label_filenames, int num_inputs,
                                               int P, int W_ms, int O_ms, double ln_switch, const char* filler_class,
                                               const char* csv_dir_or_file, const char* frames_dir)
{
    const char* who = "e2vq_hmm_align_files_posteriors";
    FlushStdout flush_on_return;
    LoopModels fm;
    if (files_given(who, model_filenames, num_models, input_filenames && label_filenames && num_inputs >= 1) ||
        window_ms_ok(who, W_ms, O_ms) || fm.load_checked(who, model_filenames, num_models))
        return 1;
    const int K = fm.K();
    const std::vector<int>& Ns = fm.Ns;
    Transcripts tr;
    if (tr.set_filler(who, fm, filler_class)) return 1;
    if (fm.logs(model_filenames)) return 1;
    const std::string fdir = frames_dir && *frames_dir ? frames_dir : "";
    if (frames_csv_distinct(fdir, input_filenames, num_inputs)) return 1;
    SymInputs si;
    if (sym_inputs_check(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, si)) return 1;
    for (int f = 0; f < num_inputs; ++f) {
        if (tr.add_labels(who, fm, label_filenames[f])) return 1;
        // (with the frame count known so far: a .wav may still lose frames, which only shrinks the tables)
        const i64 offs[2] = {0, si.inputs[(size_t)f].T}, uoffs[2] = {0, tr.L(f)};
        AlignPlan ap;
        PostPlan pp;
        if (align_plan(who, K, Ns.data(), offs, 1, tr.u(f), uoffs, tr.o(f), ln_switch, ap) ||
            post_plan(who, K, Ns.data(), fm.M, offs, 1, tr.u(f), uoffs, tr.o(f), ln_switch, pp))
            return e2vq_set_error("%s: %s", label_filenames[f], std::string(e2vq_last_error()).c_str());
    }
    std::vector<const double*> pis, As, Bs;
    for (int k = 0; k < K; ++k) pis.push_back(fm.ms[(size_t)k]->pi.data()), As.push_back(fm.ms[(size_t)k]->A.data()), Bs.push_back(fm.ms[(size_t)k]->B.data());
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    SymStage stg;
    if (require_device(device) || stg.open(device, si)) return 1;
    for (int f = 0; f < num_inputs; ++f) {
        const SymInput& in = si.inputs[(size_t)f];
        const int32_t* u = tr.u(f);
        const uint8_t* o = tr.o(f);
        const int L = (int)tr.L(f);
        int64_t T = 0;
        if (stg.input(in, si, P, W_ms, O_ms, &T)) return 1;  // (the symbols of the input, staged once: both decoders read them)
        const int64_t offs[2] = {0, T}, uoffs[2] = {0, (int64_t)L};
        const size_t n = (size_t)std::max<int64_t>(T, 1);
        std::vector<uint16_t> path(n);
        std::vector<double> score(n), post(n), w0((size_t)L), w1((size_t)L), w2((size_t)L);
        std::vector<int64_t> begin((size_t)L), end((size_t)L), ref((size_t)L);
        double lp = 0.0;
        int status = 0, pstatus = 0;
        if (e2vq_hmm_align(device, K, Ns.data(), fm.M, pis.data(), As.data(), Bs.data(), stg.d_sym.get(), offs, 1, u, uoffs, o,
                           ln_switch, path.data(), nullptr, nullptr, score.data(), begin.data(), end.data(), &lp, &status, 1))
            return 1;
        if (status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d", in.path.c_str(), fm.M);
        if (status == 1)
            return e2vq_set_error("%s: %lld frames cannot be aligned to the %zu units of %s (no path of probability > 0)", in.path.c_str(),
                                  (long long)T, (size_t)L, label_filenames[f]);
        for (int l = 0; l < L; ++l) ref[(size_t)l] = begin[(size_t)l] < 0 ? 0 : begin[(size_t)l];
        PostPlan pp;
        if (post_plan(who, K, Ns.data(), fm.M, (const i64*)offs, 1, u, (const i64*)uoffs, o, ln_switch, pp)) return 1;
        PostOut out;
        out.post_path = post.data(), out.w0 = w0.data(), out.w1 = w1.data(), out.w2 = w2.data(), out.status = &pstatus;
        if (post_device(who, pp, fm, stg.d_sym.get(), (const i64*)offs, 1, (const i64*)uoffs, ln_switch, path.data(), ref.data(), stg.st.s, out))
            return 1;
        // (a path of log-probability > -inf whose linear products underflow to 0 leaves status 1 here: every posterior is 0.0)
        if (pstatus != 0) fprintf(stderr, "%s: the posteriors are all 0: the scaled forward pass found no mass (status %d)\n", in.path.c_str(), pstatus);
        const std::string fcsv = fdir.empty() ? "" : frames_csv_path(fdir, in.path.c_str());
        if (e2vq_hmm_align_report_posteriors(in.path.c_str(), T, K, fm.names.data(), W_ms, O_ms, L, u, o, begin.data(), end.data(),
                                             score.data(), lp, ln_switch, path.data(), post.data(), w0.data(), w1.data(), w2.data(),
                                             ref.data(), in.csv.empty() ? nullptr : in.csv.c_str(), fcsv.empty() ? nullptr : fcsv.c_str()))
            return 1;
    }
    return 0;
}
