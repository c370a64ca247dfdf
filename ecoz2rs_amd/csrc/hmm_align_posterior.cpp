// hmm_align_posterior.cpp -- how sure the alignment is (`hmm align --posteriors`, e2vq_hmm_align_posteriors):
// per unit and frame the posterior that the unit holds the frame, per unit the probability that a path visits it and the mean
// and spread of the frame it is entered at, over the kernel of hmm_align_posterior.hip.  The host checks the transcripts and
// packs each stream's units into wave-slots with hmm_align.cpp's align_plan (all before any HIP call), adds the three flags and
// the parameter block of the embedded E-step (copied from hmm_embed.cpp, which keeps its own), cuts the launches by the scratch
// budget, takes the logarithm of the (mantissa, exponent) pairs and the unit moments, and writes the reports.
#include "hmm_host.h"

namespace e2hmm_host {
namespace {

thread_local float g_align_post_kernel_ms = -1.f;  // e2vq_hmm_align_posteriors_last_kernel_ms

int post_a_ld(int N) { return N | 1; }  // (odd: see hmm_embed.hip)

// What the host decides about a call before the device is touched: align_plan's packing of every stream with the three flags
// of the E-step, the classes' A at the padded leading dimension, the LDS layout and the launches.
struct PostPlan {
    AlignPlan ap;
    SegPacking cls;
    std::vector<e2hmm::EmbedClassDev> classes;
    std::vector<uint16_t> row_cls;
    std::vector<i64> occ_at;  // [S + 1]
    i64 row_words = 0, max_frames = 0;
    int max_L = 0, max_slots = 0;
    bool a_lds = false;
    std::vector<std::pair<int, int>> chunks;
};

int post_plan(const char* who, int K, const int* Ns, const i64* offs, int S, const int32_t* units, const i64* unit_offs,
              const uint8_t* optional, double ln_switch, PostPlan& pp)
{
    if (align_plan(who, K, Ns, offs, S, units, unit_offs, optional, ln_switch, pp.ap, /*embedded=*/true)) return 1;
    int max_sumN = 0;
    pp.occ_at.assign((size_t)S + 1, 0);
    for (int s = 0; s < S; ++s) {
        e2hmm::AlignStreamDev& sd = pp.ap.streams[(size_t)s];
        if (sd.slots > e2hmm::SEG_MAX_WAVES)
            return e2vq_set_error("%s: stream %d: the units take %d wave-slots of 64 lanes (at most %d: the alignment posteriors have a "
                                  "resident body only)", who, s, sd.slots, e2hmm::SEG_MAX_WAVES);
        pp.max_L = std::max(pp.max_L, sd.L);
        pp.max_slots = std::max(pp.max_slots, sd.slots);
        max_sumN = std::max(max_sumN, sd.sumN);
        pp.occ_at[(size_t)s + 1] = pp.occ_at[(size_t)s] + (offs[s + 1] - offs[s]) * sd.L;
        const uint8_t* opt = optional ? optional + unit_offs[s] : nullptr;
        for (int x = 0; x < sd.slots * 64; ++x) {
            e2hmm::AlignLaneDev& al = pp.ap.lanes[(size_t)sd.lane_at + (size_t)x];
            if (al.unit < 0) continue;
            const int l = al.unit;
            al.flags |= (l + 1 < sd.L ? e2hmm::EMBED_SUCC : 0) | (l + 2 < sd.L && opt && opt[l + 1] ? e2hmm::EMBED_SUCC2 : 0);
        }
    }
    pp.cls = pack_slots(std::vector<int>(Ns, Ns + K), post_a_ld);
    pp.row_cls = pp.cls.comp_cls;
    for (int k = 0; k < K; ++k) pp.classes.push_back(e2hmm::EmbedClassDev{Ns[k], pp.cls.a_at[(size_t)k], 0, 0});
    // A in LDS when it fits; ECOZ2_HMM_EMBED_A = lds | global forces either, as in the E-step
    const char* v = getenv("ECOZ2_HMM_EMBED_A");
    const bool forced = v && *v;
    if (forced && strcmp(v, "lds") != 0 && strcmp(v, "global") != 0) return e2vq_set_error("ECOZ2_HMM_EMBED_A=%s: lds or global", v);
    const int aw = pp.cls.a_words;
    pp.a_lds = forced ? strcmp(v, "lds") == 0 : e2hmm::align_post_lds_bytes(pp.max_L, aw, true) <= e2hmm::SEG_LDS_BYTES;
    const size_t lds = e2hmm::align_post_lds_bytes(pp.max_L, aw, pp.a_lds);
    if (lds > e2hmm::SEG_LDS_BYTES)
        return e2vq_set_error("%s: %d units and A in %s take %zu bytes of LDS (at most %zu)", who, pp.max_L, pp.a_lds ? "LDS" : "global memory",
                              lds, e2hmm::SEG_LDS_BYTES);
    // launches of whole streams whose scratch stays within the budget, counted as the E-step counts it
    pp.row_words = 2 * (i64)max_sumN + e2hmm::SEG_MAX_WAVES;
    pp.chunks = plan_chunks("ECOZ2_HMM_EMBED_CHUNK_BYTES", 8 * pp.row_words, offs, S, &pp.max_frames);
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

// pi of every class | e = sw pi | A of every class, row i at i (N | 1) | B of every class (hmm_embed.cpp's embed_params)
std::vector<double> post_params(const LoopModels& lm, const SegPacking& pk, double sw)
{
    const int sumN = pk.sumN, M = lm.M;
    std::vector<double> params((size_t)2 * sumN + (size_t)pk.a_words + (size_t)sumN * M, 0.0);
    for (int k = 0; k < lm.K(); ++k) {
        const Hmm& h = *lm.ms[(size_t)k];
        const int N = h.N, ld = post_a_ld(N), c0 = pk.comp0[(size_t)k];
        for (int j = 0; j < N; ++j) {
            params[(size_t)(c0 + j)] = h.pi[(size_t)j];
            params[(size_t)(sumN + c0 + j)] = sw * h.pi[(size_t)j];
            std::copy(h.A.begin() + (size_t)j * N, h.A.begin() + (size_t)(j + 1) * N,
                      params.begin() + 2 * sumN + pk.a_at[(size_t)k] + (size_t)j * ld);
        }
        std::copy(h.B.begin(), h.B.end(), params.begin() + 2 * sumN + pk.a_words + (size_t)c0 * M);
    }
    return params;
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
    const AlignPlan& ap = pp.ap;
    const i64 frames = h_offs[S], nunits = unit_offs[S], nocc = out.occ ? pp.occ_at[(size_t)S] : 0;
    const std::vector<double> params = post_params(lm, pp.cls, exp(ln_switch));
    DeviceBuffer<e2hmm::AlignLaneDev> d_lanes;
    DeviceBuffer<e2hmm::AlignStreamDev> d_streams;
    DeviceBuffer<int> d_info;
    DeviceBuffer<e2hmm::EmbedClassDev> d_classes;
    DeviceBuffer<unsigned short> d_row_cls, d_path;
    DeviceBuffer<i64> d_offs, d_occ_at, d_ref;
    DeviceBuffer<double> d_params, d_scr, d_occ, d_post, d_w;
    Scores sc;
    KernelTimer timer;
    if (d_lanes.upload(ap.lanes.data(), ap.lanes.size(), st) || d_streams.upload(ap.streams.data(), ap.streams.size(), st) ||
        d_info.upload(ap.slot_info.data(), ap.slot_info.size(), st) || d_classes.upload(pp.classes.data(), pp.classes.size(), st) ||
        d_row_cls.upload(pp.row_cls.data(), pp.row_cls.size(), st) || d_offs.upload(h_offs, (size_t)S + 1, st) ||
        d_occ_at.upload(pp.occ_at.data(), pp.occ_at.size(), st) || d_params.upload(params.data(), params.size(), st) ||
        (path_unit && frames > 0 && d_path.upload(path_unit, (size_t)frames, st)) ||
        (ref && nunits > 0 && d_ref.upload((const i64*)ref, (size_t)nunits, st)) || d_post.reserve((size_t)std::max<i64>(frames, 1)) ||
        d_w.reserve((size_t)std::max<i64>(3 * nunits, 1)) || (nocc > 0 && d_occ.reserve((size_t)nocc)) || sc.reserve((size_t)S) ||
        timer.create())
        return 1;
    if (d_scr.reserve((size_t)std::max<i64>(pp.max_frames * pp.row_words, 1))) {
        const std::string why = e2vq_last_error();
        return e2vq_set_error("%s: no room for the forward tables of %lld frames x %lld doubles (ECOZ2_HMM_EMBED_CHUNK_BYTES bounds "
                              "them by whole streams): %s", who, (long long)pp.max_frames, (long long)pp.row_words, why.c_str());
    }
    // (+0.0 everywhere: what a stream of status != 0 and a frame without a unit keep)
    HIPCHK(hipMemsetAsync(d_post.get(), 0, (size_t)std::max<i64>(frames, 1) * 8, st));
    HIPCHK(hipMemsetAsync(d_w.get(), 0, (size_t)std::max<i64>(3 * nunits, 1) * 8, st));
    if (nocc > 0) HIPCHK(hipMemsetAsync(d_occ.get(), 0, (size_t)nocc * 8, st));
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes the scratch only after the previous chunk's backward pass has read it)
    for (const auto& c : pp.chunks) {
        const int s0 = c.first, n = c.second - c.first;
        const e2hmm::EmbedPlanDev pl{lm.K(), lm.M, pp.cls.sumN, pp.cls.a_words, pp.max_L, d_streams.get() + s0, d_lanes.get(),
                                     d_info.get(), d_params.get(), d_classes.get(), d_row_cls.get()};
        const e2hmm::AlignPostDev po{path_unit && frames > 0 ? d_path.get() : nullptr, ref && nunits > 0 ? d_ref.get() : nullptr,
                                     d_occ_at.get() + s0, nocc > 0 ? d_occ.get() : nullptr, d_post.get(), d_w.get(), nunits};
        if (e2hmm::launch_align_posteriors(pl, pp.a_lds, pp.max_slots, d_sym, d_offs.get() + s0, n, h_offs[s0], pp.row_words, d_scr.get(),
                                           po, sc.d_mant.get() + s0, sc.d_exp.get() + s0, sc.d_status.get() + s0, st))
            return e2vq_set_error("%s: %d units in %d wave-slots cannot be launched", who, pp.max_L, pp.max_slots);
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
    for (int s = 0; s < S; ++s) sc.get((size_t)s, nullptr, nullptr, out.status ? out.status + s : nullptr, out.log_prob ? out.log_prob + s : nullptr);
    return 0;
}

// the first checks of the array-level entry point, in e2vq_hmm_embedded_estep's order
int post_check(const char* who, int K, const int* Ns, int M, const double* const* pis, const double* const* As, const double* const* Bs,
               const void* sym, const int64_t* offs, int S, const int32_t* units, const int64_t* unit_offs, LoopModels& lm)
{
    return loop_check_args(who, K, Ns, pis, As, Bs, offs && unit_offs && (S <= 0 || units) && syms_given(sym, offs, S)) ||
           segment_check_shape(who, K, Ns) || lm.from_arrays(K, Ns, M, pis, As, Bs) || lm.logs() || check_offsets(offs, S);
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
    if (post_check(who, K, Ns, M, pis, As, Bs, sym, offs, S, units, unit_offs, lm)) return 1;
    PostPlan pp;
    if (post_plan(who, K, Ns, (const i64*)offs, S, units, (const i64*)unit_offs, optional, ln_switch, pp) ||
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
    if (!name || K < 1 || !class_names || T < 0 || L < 1 || !units || !begin || !end || (T > 0 && (!score || !post_path)) || !w0 || !w1 || !w2)
        return e2vq_set_error("%s: bad arguments", who);
    const bool frames = frames_csv_filename && *frames_csv_filename;
    if (frames && T > 0 && !path_unit) return e2vq_set_error("%s: the per-frame table needs the path's units", who);
    int skipped = 0;
    for (int l = 0; l < L; ++l) {
        if (units[l] < 0 || units[l] >= K) return e2vq_set_error("%s: unit %d names a model outside [0, %d)", who, l, K);
        if (begin[l] < 0) {
            skipped += optional && optional[l] ? 1 : 0;
            continue;
        }
        if (begin[l] >= end[l] || end[l] > T) return e2vq_set_error("%s: unit %d spans [%lld, %lld) of %lld frames", who, l, (long long)begin[l], (long long)end[l], (long long)T);
    }
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
    auto begin_s = [&](int64_t b) { return (double)(b * O_ms) / 1000.0; };
    // (the end of the analysis window of the unit's last frame)
    auto end_s = [&](int64_t e) { return (double)((e - 1) * O_ms + W_ms) / 1000.0; };
    auto unit_score = [&](int l) { return score[end[l] - 1] - (begin[l] == 0 ? 0.0 : score[begin[l] - 1] + ln_switch); };
    if (csv_filename && *csv_filename) {
        std::string doc = "unit,class,begin_frame,end_frame,begin_s,end_s,score,posterior,min_posterior,p_present,begin_mean_frame,begin_sd_frames\n";
        for (int l = 0; l < L; ++l) {
            if (begin[l] < 0) continue;
            doc += std::to_string(l) + "," + class_names[units[l]] + "," + std::to_string(begin[l]) + "," + std::to_string(end[l]) + "," +
                   fmt_17g(begin_s(begin[l])) + "," + fmt_17g(end_s(end[l])) + "," + fmt_17g(unit_score(l)) + "," + fmt_17g(mean[(size_t)l]) +
                   "," + fmt_17g(least[(size_t)l]) + "," + fmt_17g(present[(size_t)l]) + "," + fmt_17g(bmean[(size_t)l]) + "," +
                   fmt_17g(bsd[(size_t)l]) + "\n";
        }
        if (write_file(csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    if (frames) {
        std::string doc = "frame,begin_s,unit,class,posterior\n";
        for (int64_t t = 0; t < T; ++t) {
            const bool named = path_unit[t] != 0xFFFF;
            doc += std::to_string(t) + "," + fmt_17g(begin_s(t)) + "," + (named ? std::to_string(path_unit[t]) : std::string("-1")) + "," +
                   (named ? class_names[units[path_unit[t]]] : "") + "," + fmt_17g(post_path[t]) + "\n";
        }
        if (write_file(frames_csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    printf("%s: T=%lld  units=%d  optional units passed over=%d  log_prob=%g  (switch penalty %g)\n", name, (long long)T, L, skipped, log_prob,
           ln_switch);
    std::vector<int64_t> count((size_t)K, 0);
    for (int l = 0; l < L; ++l)
        if (begin[l] >= 0) count[(size_t)units[l]] += end[l] - begin[l];
    for (int k = 0; k < K; ++k) printf("  '%s': %lld\n", class_names[k], (long long)count[(size_t)k]);
    printf("  units:\n");
    for (int l = 0; l < L; ++l) {
        if (begin[l] >= 0) printf("    %.3f - %.3f %s p=%.3f\n", begin_s(begin[l]), end_s(end[l]), class_names[units[l]], mean[(size_t)l]);
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
    auto class_of = [&](const std::string& name) {
        int k = 0;
        while (k < K && name != fm.names[(size_t)k]) ++k;
        return k < K ? k : -1;
    };
    int filler = -1;
    if (filler_class && *filler_class && (filler = class_of(filler_class)) < 0)
        return e2vq_set_error("%s: the filler '%s' is no model's class", who, filler_class);
    if (fm.logs(model_filenames)) return 1;
    const std::string fdir = frames_dir && *frames_dir ? frames_dir : "";
    auto frames_csv = [&](const char* path) { return fdir + "/" + e2vq_io::basename_noext(path) + ".csv"; };
    for (int f = 0; f < num_inputs && !fdir.empty(); ++f)
        for (int g = 0; g < f; ++g)
            if (input_filenames[f] && input_filenames[g] && frames_csv(input_filenames[g]) == frames_csv(input_filenames[f]))
                return e2vq_set_error("%s and %s would both write %s", input_filenames[g], input_filenames[f], frames_csv(input_filenames[f]).c_str());
    SymInputs si;
    if (sym_inputs_check(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, si)) return 1;
    // the transcripts: the labels of file i in their order, the filler around and between them (as e2vq_hmm_align_files)
    std::vector<std::vector<int32_t>> units((size_t)num_inputs);
    std::vector<std::vector<uint8_t>> optional((size_t)num_inputs);
    for (int f = 0; f < num_inputs; ++f) {
        const char* path = label_filenames[f];
        if (!path) return e2vq_set_error("%s: NULL file name", who);
        std::vector<LabelRow> rows;
        if (read_label_file(path, rows)) return 1;
        if (rows.empty()) return e2vq_set_error("%s: no labelled units", path);
        std::vector<int32_t>& u = units[(size_t)f];
        std::vector<uint8_t>& o = optional[(size_t)f];
        auto fill = [&] {
            if (filler >= 0) u.push_back(filler), o.push_back(1);
        };
        fill();
        for (const LabelRow& r : rows) {
            const int k = class_of(r.label);
            if (k < 0) return e2vq_set_error("%s:%zu: '%s' is no model's class", path, r.line, r.label.c_str());
            u.push_back(k), o.push_back(0);
            fill();
        }
        // (with the frame count known so far: a .wav may still lose frames, which only shrinks the tables)
        const i64 offs[2] = {0, si.inputs[(size_t)f].T}, uoffs[2] = {0, (i64)u.size()};
        AlignPlan ap;
        PostPlan pp;
        if (align_plan(who, K, Ns.data(), offs, 1, u.data(), uoffs, o.data(), ln_switch, ap) ||
            post_plan(who, K, Ns.data(), offs, 1, u.data(), uoffs, o.data(), ln_switch, pp))
            return e2vq_set_error("%s: %s", path, std::string(e2vq_last_error()).c_str());
    }
    std::vector<const double*> pis, As, Bs;
    for (int k = 0; k < K; ++k) pis.push_back(fm.ms[(size_t)k]->pi.data()), As.push_back(fm.ms[(size_t)k]->A.data()), Bs.push_back(fm.ms[(size_t)k]->B.data());
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    SymStage stg;
    if (require_device(device) || stg.open(device, si)) return 1;
    for (int f = 0; f < num_inputs; ++f) {
        const SymInput& in = si.inputs[(size_t)f];
        const std::vector<int32_t>& u = units[(size_t)f];
        const std::vector<uint8_t>& o = optional[(size_t)f];
        const int L = (int)u.size();
        int64_t T = 0;
        if (stg.input(in, si, P, W_ms, O_ms, &T)) return 1;  // (the symbols of the input, staged once: both decoders read them)
        const int64_t offs[2] = {0, T}, uoffs[2] = {0, (int64_t)L};
        const size_t n = (size_t)std::max<int64_t>(T, 1);
        std::vector<uint16_t> path(n);
        std::vector<double> score(n), post(n), w0((size_t)L), w1((size_t)L), w2((size_t)L);
        std::vector<int64_t> begin((size_t)L), end((size_t)L), ref((size_t)L);
        double lp = 0.0;
        int status = 0, pstatus = 0;
        if (e2vq_hmm_align(device, K, Ns.data(), fm.M, pis.data(), As.data(), Bs.data(), stg.d_sym.get(), offs, 1, u.data(), uoffs, o.data(),
                           ln_switch, path.data(), nullptr, nullptr, score.data(), begin.data(), end.data(), &lp, &status, 1))
            return 1;
        if (status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d", in.path.c_str(), fm.M);
        if (status == 1)
            return e2vq_set_error("%s: %lld frames cannot be aligned to the %zu units of %s (no path of probability > 0)", in.path.c_str(),
                                  (long long)T, u.size(), label_filenames[f]);
        for (int l = 0; l < L; ++l) ref[(size_t)l] = begin[(size_t)l] < 0 ? 0 : begin[(size_t)l];
        PostPlan pp;
        if (post_plan(who, K, Ns.data(), (const i64*)offs, 1, u.data(), (const i64*)uoffs, o.data(), ln_switch, pp)) return 1;
        PostOut out;
        out.post_path = post.data(), out.w0 = w0.data(), out.w1 = w1.data(), out.w2 = w2.data(), out.status = &pstatus;
        if (post_device(who, pp, fm, stg.d_sym.get(), (const i64*)offs, 1, (const i64*)uoffs, ln_switch, path.data(), ref.data(), stg.st.s, out))
            return 1;
        // (a path of log-probability > -inf whose linear products underflow to 0 leaves status 1 here: every posterior is 0.0)
        if (pstatus != 0) fprintf(stderr, "%s: the posteriors are all 0: the scaled forward pass found no mass (status %d)\n", in.path.c_str(), pstatus);
        const std::string fcsv = fdir.empty() ? "" : frames_csv(in.path.c_str());
        if (e2vq_hmm_align_report_posteriors(in.path.c_str(), T, K, fm.names.data(), W_ms, O_ms, L, u.data(), o.data(), begin.data(), end.data(),
                                             score.data(), lp, ln_switch, path.data(), post.data(), w0.data(), w1.data(), w2.data(),
                                             ref.data(), in.csv.empty() ? nullptr : in.csv.c_str(), fcsv.empty() ? nullptr : fcsv.c_str()))
            return 1;
    }
    return 0;
}
