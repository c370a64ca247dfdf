// hmm_align.cpp -- forced alignment on the GPU (`hmm align`, e2vq_hmm_align): the most likely path of a
// symbol stream through the units of its transcript, in their order, over the kernels of hmm_align.hip.  The host checks
// runs the launches align_plan cut, replays the decoded path for its per-frame score, and writes the reports.  The checks,
// the transcripts of the label files and align_plan are hmm_transcript.cpp's, models, packing and the parameter block
// hmm_class_loop.cpp's, the input stage hmm_input.cpp's (hmm_host.h).
#include "hmm_host.h"

namespace e2hmm_host {
namespace {

thread_local float g_align_kernel_ms = -1.f;  // e2vq_hmm_align_last_kernel_ms

struct AlignOut {  // host arrays, any may be null; per frame: unit, state, entered, score; per unit: begin, end; per stream: the rest
    uint16_t* unit = nullptr;
    uint16_t* state = nullptr;
    uint8_t* entered = nullptr;
    double* score = nullptr;
    int64_t* begin = nullptr;
    int64_t* end = nullptr;
    double* log_prob = nullptr;
    int* status = nullptr;
};

// the path's own cumulative score, frame by frame, from the decoded path: one addition per term in the device's order
void align_replay(const LoopModels& lm, const uint16_t* sym, i64 T, const int32_t* units, const uint8_t* opt, double ln_switch,
                  const uint16_t* unit, const uint16_t* state, const uint8_t* entered, double* score)
{
    const int M = lm.M;
    for (i64 t = 0; t < T; ++t) {
        const int l = unit[t], j = state[t], k = units[l];
        const size_t N = (size_t)lm.Ns[(size_t)k];
        const double* lf = lm.lflats[(size_t)k].data();
        const double lpi = lf[j], lB = lf[N + N * N + (size_t)j * M + sym[t]];
        if (t == 0) score[0] = unit_is_initial(l, opt) ? lpi + lB : -INFINITY;
        else if (entered[t]) score[t] = ((score[t - 1] + ln_switch) + lpi) + lB;
        else score[t] = (score[t - 1] + lf[N + (size_t)state[t - 1] * N + j]) + lB;
    }
}

// The alignment of S device-resident streams (h_offs: their S + 1 offsets, on the host) to their transcripts under the
// models (all of one M, with their logarithms), as planned by align_plan, on the current device and the stream st.
int align_device(const char* who, const AlignPlan& ap, const LoopModels& lm, const unsigned short* d_sym, const i64* h_offs, int S,
                 const int32_t* units, const i64* unit_offs, const uint8_t* optional, double ln_switch, hipStream_t st, const AlignOut& out)
{
    const int M = lm.M, sumN = ap.cls.sumN, a_words = ap.cls.a_words;
    const std::vector<double> params = loop_log_params(lm, ap.cls);
    const i64 frames = h_offs[S], nunits = unit_offs[S];
    DeviceBuffer<double> d_params, d_logp;
    DeviceBuffer<e2hmm::AlignLaneDev> d_lanes;
    DeviceBuffer<e2hmm::AlignStreamDev> d_streams;
    DeviceBuffer<int> d_info, d_comp0, d_status, d_qlast;
    DeviceBuffer<unsigned short> d_comp_unit, d_unit, d_state;
    DeviceBuffer<unsigned char> d_entered, d_tab;
    DeviceBuffer<i64> d_offs, d_begin, d_end;
    if (d_params.upload(params.data(), params.size(), st) || d_lanes.upload(ap.lanes.data(), ap.lanes.size(), st) ||
        d_streams.upload(ap.streams.data(), ap.streams.size(), st) || d_info.upload(ap.slot_info.data(), ap.slot_info.size(), st) ||
        d_comp0.upload(ap.unit_comp0.data(), ap.unit_comp0.size(), st) || d_comp_unit.upload(ap.comp_unit.data(), ap.comp_unit.size(), st) ||
        d_offs.upload(h_offs, (size_t)S + 1, st) || d_logp.reserve((size_t)S) || d_status.reserve((size_t)S) || d_qlast.reserve((size_t)S) ||
        d_unit.reserve((size_t)frames) || d_state.reserve((size_t)frames) || d_entered.reserve((size_t)frames) ||
        d_begin.reserve((size_t)nunits) || d_end.reserve((size_t)nunits))
        return 1;
    if (d_tab.reserve((size_t)ap.max_bytes)) {
        const std::string why = e2vq_last_error();
        return e2vq_set_error("%s: no room for the back-pointer tables of %lld bytes (ECOZ2_HMM_ALIGN_TABLE_BYTES bounds them by whole "
                              "streams): %s", who, (long long)ap.max_bytes, why.c_str());
    }
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a launch's forward pass writes the tables only after the previous launch's backtrack has read them)
    for (const AlignPlan::Launch& g : ap.launches) {
        const int s0 = g.s0, n = g.s1 - g.s0;
        const e2hmm::AlignPlanDev pl{M, sumN, a_words, g.max_L, g.max_sumN, d_streams.get() + s0, d_lanes.get(), d_info.get(),
                                     d_params.get(), d_comp_unit.get(), d_comp0.get()};
        if (e2hmm::launch_align(pl, g.looped, g.waves, d_sym, d_offs.get() + s0, n, ln_switch, d_tab.get(), d_logp.get() + s0,
                                d_qlast.get() + s0, d_status.get() + s0, st))
            return e2vq_set_error("%s: %d units of sum N = %d states cannot be launched", who, g.max_L, g.max_sumN);
        HIPCHK(hipGetLastError());
        e2hmm::launch_align_backtrack(pl, d_offs.get() + s0, n, d_tab.get(), d_qlast.get() + s0, d_status.get() + s0, d_unit.get(),
                                      d_state.get(), d_entered.get(), d_begin.get(), d_end.get(), st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    // the path comes to the host whatever the caller asks for: the score is replayed from it
    const size_t nf = (size_t)std::max<i64>(frames, 1);
    std::vector<uint16_t> h_unit(nf), h_state(nf), h_sym(nf);
    std::vector<uint8_t> h_entered(nf);
    std::vector<double> h_logp((size_t)S), h_score(nf);
    std::vector<int> h_status((size_t)S);
    if (frames > 0) {
        HIPCHK(hipMemcpyAsync(h_unit.data(), d_unit.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_state.data(), d_state.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_entered.data(), d_entered.get(), (size_t)frames, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_sym.data(), d_sym, (size_t)frames * 2, hipMemcpyDeviceToHost, st));
    }
    if (nunits > 0) {
        if (out.begin) HIPCHK(hipMemcpyAsync(out.begin, d_begin.get(), (size_t)nunits * 8, hipMemcpyDeviceToHost, st));
        if (out.end) HIPCHK(hipMemcpyAsync(out.end, d_end.get(), (size_t)nunits * 8, hipMemcpyDeviceToHost, st));
    }
    if (S > 0) {
        HIPCHK(hipMemcpyAsync(h_logp.data(), d_logp.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_status.data(), d_status.get(), (size_t)S * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    if (timer.elapsed_ms(&g_align_kernel_ms)) return 1;
    for (int s = 0; s < S; ++s) {
        const i64 a = h_offs[s], T = h_offs[s + 1] - a;
        if (T < 1) continue;
        double* sc = h_score.data() + a;
        if (h_status[(size_t)s] == 2) {
            std::fill(sc, sc + T, -INFINITY);
            sc[0] = 0.0;
            continue;
        }
        align_replay(lm, h_sym.data() + a, T, units + unit_offs[s], optional ? optional + unit_offs[s] : nullptr, ln_switch,
                     h_unit.data() + a, h_state.data() + a, h_entered.data() + a, sc);
        if (memcmp(&sc[T - 1], &h_logp[(size_t)s], 8) != 0)
            return e2vq_set_error("%s: internal error: stream %d: the replayed path scores %.17g, the device found %.17g", who, s, sc[T - 1],
                                  h_logp[(size_t)s]);
    }
    if (frames > 0) {
        if (out.unit) std::copy(h_unit.begin(), h_unit.begin() + frames, out.unit);
        if (out.state) std::copy(h_state.begin(), h_state.begin() + frames, out.state);
        if (out.entered) std::copy(h_entered.begin(), h_entered.begin() + frames, out.entered);
        if (out.score) std::copy(h_score.begin(), h_score.begin() + frames, out.score);
    }
    if (out.log_prob) std::copy(h_logp.begin(), h_logp.end(), out.log_prob);
    if (out.status) std::copy(h_status.begin(), h_status.end(), out.status);
    return 0;
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

extern "C" int e2vq_hmm_align_last_kernel_ms(float* ms) { return last_kernel_ms("e2vq_hmm_align_last_kernel_ms", g_align_kernel_ms, ms); }

extern "C" int e2vq_hmm_align(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                              const double* const* Bs, const void* sym, const int64_t* offs, int S, const int32_t* units,
                              const int64_t* unit_offs, const uint8_t* optional, double ln_switch, uint16_t* unit, uint16_t* state,
                              uint8_t* entered, double* score, int64_t* begin, int64_t* end, double* log_prob, int* status,
                              int sym_on_device)
{
    const char* who = "e2vq_hmm_align";
    LoopModels lm;
    if (transcript_check_args(who, K, Ns, M, pis, As, Bs, sym, offs, S, units, unit_offs, lm)) return 1;
    AlignPlan ap;
    if (align_plan(who, K, Ns, (const i64*)offs, S, units, (const i64*)unit_offs, optional, ln_switch, ap)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    if (require_device(device)) return 1;
    DevSeqs seqs;
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0)) return 1;
    const AlignOut out{unit, state, entered, score, begin, end, log_prob, status};
    return align_device(who, ap, lm, seqs.sym, (const i64*)offs, S, units, (const i64*)unit_offs, optional, ln_switch, seqs.st.s, out);
}

extern "C" int e2vq_hmm_align_report(const char* name, int64_t T, int K, const char* const* class_names, int W_ms, int O_ms, int L,
                                     const int32_t* units, const uint8_t* optional, const int64_t* begin, const int64_t* end,
                                     const double* score, double log_prob, double ln_switch, const char* csv_filename)
{
    const char* who = "e2vq_hmm_align_report";
    FlushStdout flush_on_return;
    const int skipped = align_report_check(who, name, T, K, class_names, L, units, optional, begin, end, score, true);
    if (skipped < 0) return 1;
    if (csv_filename && *csv_filename) {
        std::string doc = "unit,class,begin_frame,end_frame,begin_s,end_s,score\n";
        for (int l = 0; l < L; ++l) {
            if (begin[l] < 0) continue;
            doc += std::to_string(l) + "," + class_names[units[l]] + "," + std::to_string(begin[l]) + "," + std::to_string(end[l]) + "," +
                   fmt_17g(align_time_s(begin[l], O_ms)) + "," + fmt_17g(align_time_s(end[l] - 1, O_ms, W_ms)) + "," +
                   fmt_17g(align_unit_score(score, begin, end, l, ln_switch)) + "\n";
        }
        if (write_file(csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    align_report_head(name, T, K, class_names, L, units, begin, end, skipped, log_prob, ln_switch);
    for (int l = 0; l < L; ++l)
        if (begin[l] >= 0) printf("    %.3f - %.3f %s\n", align_time_s(begin[l], O_ms), align_time_s(end[l] - 1, O_ms, W_ms), class_names[units[l]]);
    if (csv_filename && *csv_filename) printf("  %s saved\n", csv_filename);
    return 0;
}

extern "C" int e2vq_hmm_align_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                    const char* const* input_filenames, const char* const* label_filenames, int num_inputs, int P,
                                    int W_ms, int O_ms, double ln_switch, const char* filler_class, const char* csv_dir_or_file)
{
    const char* who = "e2vq_hmm_align_files";
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
    SymInputs si;
    if (sym_inputs_check(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, si)) return 1;
    for (int f = 0; f < num_inputs; ++f) {
        if (tr.add_labels(who, fm, label_filenames[f])) return 1;
        // (with the frame count known so far: a .wav may still lose frames, which only shrinks the tables)
        const i64 offs[2] = {0, si.inputs[(size_t)f].T}, uoffs[2] = {0, tr.L(f)};
        AlignPlan ap;
        if (align_plan(who, K, Ns.data(), offs, 1, tr.u(f), uoffs, tr.o(f), ln_switch, ap))
            return e2vq_set_error("%s: %s", label_filenames[f], std::string(e2vq_last_error()).c_str());
    }
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    SymStage stg;
    if (require_device(device) || stg.open(device, si)) return 1;
    for (int f = 0; f < num_inputs; ++f) {
        const SymInput& in = si.inputs[(size_t)f];
        const int32_t* u = tr.u(f);
        const uint8_t* o = tr.o(f);
        const size_t L = (size_t)tr.L(f);
        int64_t T = 0;
        if (stg.input(in, si, P, W_ms, O_ms, &T)) return 1;
        const i64 offs[2] = {0, T}, uoffs[2] = {0, (i64)L};
        AlignPlan ap;
        if (align_plan(who, K, Ns.data(), offs, 1, u, uoffs, o, ln_switch, ap)) return 1;
        std::vector<double> score((size_t)std::max<int64_t>(T, 1));
        std::vector<int64_t> begin(L), end(L);
        double lp = 0.0;
        int status = 0;
        AlignOut out;
        out.score = score.data(), out.begin = begin.data(), out.end = end.data(), out.log_prob = &lp, out.status = &status;
        if (align_device(who, ap, fm, stg.d_sym.get(), offs, 1, u, uoffs, o, ln_switch, stg.st.s, out)) return 1;
        if (status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d", in.path.c_str(), fm.M);
        if (status == 1)
            return e2vq_set_error("%s: %lld frames cannot be aligned to the %zu units of %s (no path of probability > 0)", in.path.c_str(),
                                  (long long)T, L, label_filenames[f]);
        if (e2vq_hmm_align_report(in.path.c_str(), T, K, fm.names.data(), W_ms, O_ms, (int)L, u, o, begin.data(),
                                  end.data(), score.data(), lp, ln_switch, in.csv.empty() ? nullptr : in.csv.c_str()))
            return 1;
    }
    return 0;
}
