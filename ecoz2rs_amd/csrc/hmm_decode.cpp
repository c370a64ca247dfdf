// hmm_decode.cpp -- decoding under single models on the GPU: Viterbi under one model (`seq show -P / -Q --hmm`,
// e2vq_hmm_viterbi) and the models over the windows of whole recordings (`hmm scan`, 4.8.5), over the
// kernels of hmm_viterbi.hip and hmm_scan.hip; and the cut of a decoder's launches by a table budget, which the class loop
// (hmm_class_loop.cpp) shares.
#include "hmm_host.h"

namespace e2hmm_host {

std::vector<std::pair<int, int>> plan_chunks(const char* env, i64 row, const i64* hoffs, int S, i64* max_frames)
{
    const i64 budget = env_bytes(env, (i64)256 << 20);
    std::vector<std::pair<int, int>> chunks;
    *max_frames = 0;
    for (int s0 = 0; s0 < S;) {
        int s1 = s0 + 1;
        while (s1 < S && (hoffs[s1 + 1] - hoffs[s0]) * row <= budget) ++s1;
        chunks.emplace_back(s0, s1);
        *max_frames = std::max(*max_frames, hoffs[s1] - hoffs[s0]);
        s0 = s1;
    }
    return chunks;
}

namespace {

// Viterbi of S device-resident sequences (hoffs: the S+1 offsets on the host, to cut the launches) under the model
// whose logarithms `lflat` holds; path (may be null: no psi, no backtrack) receives hoffs[S] states
int viterbi_device(int N, int M, const std::vector<double>& lflat, const unsigned short* d_sym, const i64* d_offs,
                   const i64* hoffs, int S, hipStream_t st, uint16_t* path, double* logp, int* status)
{
    DeviceBuffer<double> d_model, d_logp;
    DeviceBuffer<int> d_status, d_qlast;
    DeviceBuffer<unsigned short> d_psi, d_path;
    if (d_model.upload(lflat.data(), lflat.size(), st)) return 1;
    HIPCHK(hipStreamSynchronize(st));  // (`lflat` may go)
    const double* base = d_model.get();
    const ModelDev lm{N, M, base, base + N, base + N + (size_t)N * N};
    if (d_logp.reserve((size_t)S) || d_status.reserve((size_t)S)) return 1;
    if (!path) {
        e2hmm::launch_viterbi(lm, d_sym, d_offs, S, 0, nullptr, d_logp.get(), nullptr, d_status.get(), st);
        HIPCHK(hipGetLastError());
    } else {
        i64 max_syms = 0;  // (psi: 2 N bytes a frame)
        const auto chunks = plan_chunks("ECOZ2_HMM_VITERBI_CHUNK_BYTES", 2 * (i64)N, hoffs, S, &max_syms);
        if (d_psi.reserve((size_t)max_syms * N) || d_path.reserve((size_t)hoffs[S]) || d_qlast.reserve((size_t)S)) return 1;
        // (one stream: a chunk's forward pass writes psi only after the previous chunk's backtrack has read it)
        for (const auto& c : chunks) {
            const int s0 = c.first, n = c.second - c.first;
            e2hmm::launch_viterbi(lm, d_sym, d_offs + s0, n, hoffs[s0], d_psi.get(), d_logp.get() + s0, d_qlast.get() + s0,
                                  d_status.get() + s0, st);
            HIPCHK(hipGetLastError());
            e2hmm::launch_backtrack(N, d_offs + s0, n, hoffs[s0], d_psi.get(), d_qlast.get() + s0, d_status.get() + s0,
                                    d_path.get(), st);
            HIPCHK(hipGetLastError());
        }
        if (hoffs[S] > 0) HIPCHK(hipMemcpyAsync(path, d_path.get(), (size_t)hoffs[S] * 2, hipMemcpyDeviceToHost, st));
    }
    if (S > 0) {
        HIPCHK(hipMemcpyAsync(logp, d_logp.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(status, d_status.get(), (size_t)S * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// values of one sequence as `seq show` prints its symbols: all of them when `full` or L <= 30, else the first 10,
// ", ..., " and the last 10
template <typename V>
void print_abbreviated(const V* v, size_t len, bool full)
{
    if (full || len <= 30) {
        for (size_t t = 0; t < len; ++t) printf("%s%u", t ? ", " : "", (unsigned)v[t]);
    } else {
        for (size_t t = 0; t < 10; ++t) printf("%s%u", t ? ", " : "", (unsigned)v[t]);
        printf(", ..., ");
        for (size_t t = len - 10; t < len; ++t) printf("%s%u", t > len - 10 ? ", " : "", (unsigned)v[t]);
    }
}

// ---- hmm scan: the trained models over the windows of whole recordings ------------------------------------
// windows of `window` frames every `hop` frames: stream s of T_s symbols has (T_s - window) / hop + 1 of them when
// T_s >= window, else none (a trailing incomplete window is dropped); win_offs: S + 1 entries
void scan_window_offsets(const i64* offs, int S, i64 window, i64 hop, i64* win_offs)
{
    win_offs[0] = 0;
    for (int s = 0; s < S; ++s) {
        const i64 T = offs[s + 1] - offs[s];
        win_offs[s + 1] = win_offs[s] + (T >= window ? (T - window) / hop + 1 : 0);
    }
}

int scan_check_geometry(const char* who, i64 window, i64 hop)
{
    if (window < 1) return e2vq_set_error("%s: window of %lld frames (at least 1)", who, (long long)window);
    if (window > (1 << 30)) return e2vq_set_error("%s: window of %lld frames (at most 2^30)", who, (long long)window);
    if (hop < 1) return e2vq_set_error("%s: hop of %lld frames (at least 1)", who, (long long)hop);
    return 0;
}

// windows to a wave: floor(64 / N) where that is at least 3 (N <= SCAN_PACK_MAX_N), else one -- two windows to a wave measured
// between 1.4 % faster (N = 22) and 3 % slower (N = 28, 32) than one (DESIGN.md 4.8.5's table).
// ECOZ2_HMM_SCAN_PACK=0 scores one window per wave at every N, =1 packs floor(64 / N) at every N <= 32 (the other arms of
// tools/hmm_scan_bench.py and of the tests; the bits are the same)
constexpr int SCAN_PACK_MAX_N = 21;
int scan_pack_width_in_use(int N)
{
    const char* v = getenv("ECOZ2_HMM_SCAN_PACK");
    if (v && *v) return atoi(v) == 0 || N > 32 ? 1 : e2hmm::WAVE_N / N;
    return N <= SCAN_PACK_MAX_N ? e2hmm::WAVE_N / N : 1;
}

// rounds of (waves x G) windows a k_hmm_scan workgroup takes from one staging of A and the symbols
// (ECOZ2_HMM_SCAN_ROUNDS, 1 .. 64; changes no bit)
int scan_rounds()
{
    const int r = e2vq_env_int("ECOZ2_HMM_SCAN_ROUNDS", 4);
    return r < 1 ? 1 : (r > 64 ? 64 : r);
}

thread_local float g_scan_kernel_ms = -1.f;  // e2vq_hmm_scan_last_kernel_ms

struct ScanOut {  // any may be null; matrices W x K, the others W
    double* mant = nullptr;
    int64_t* exp2 = nullptr;
    int* status = nullptr;
    double* log_probs = nullptr;
    int* best = nullptr;
    double* best_log_prob = nullptr;
    int* second = nullptr;
    double* second_log_prob = nullptr;
    bool matrix() const { return mant || exp2 || status || log_probs; }
    bool top() const { return best || best_log_prob || second || second_log_prob; }
};

// Scores every window of the S device-resident streams (h_offs: their S + 1 offsets, on the host) under the models, on the
// current device and the stream st.  Models of one N <= 64 go into one k_hmm_scan launch over runs of at most
// waves x G x rounds windows whose span fits the staging area; models of more states through k_hmm_scan_wg; then
// k_scan_top2.  One copy back: two results per window, and the W x K matrix only when `out` asks for it.
int scan_device(const std::vector<const Hmm*>& ms, const unsigned short* d_sym, const i64* h_offs, int S, i64 window, i64 hop,
                hipStream_t st, const ScanOut& out)
{
    const int K = (int)ms.size();
    std::vector<i64> win_offs((size_t)S + 1);
    scan_window_offsets(h_offs, S, window, hop, win_offs.data());
    const i64 W = win_offs[(size_t)S];
    if (W == 0) return 0;
    if (W > (i64)INT32_MAX - 64 || W * K > ((i64)1 << 40)) return e2vq_set_error("hmm scan: %lld windows x %d models", (long long)W, K);
    std::vector<e2hmm::ScanWin> wins((size_t)W);
    for (int s = 0; s < S; ++s)
        for (i64 i = 0, n = win_offs[(size_t)s + 1] - win_offs[(size_t)s]; i < n; ++i)
            wins[(size_t)(win_offs[(size_t)s] + i)] = e2hmm::ScanWin{s, (int)window, i * hop};
    // runs of at most `cap` windows, stream by stream
    auto make_runs = [&](i64 cap, std::vector<e2hmm::ScanRun>& runs) {
        for (int s = 0; s < S; ++s)
            for (i64 w = win_offs[(size_t)s]; w < win_offs[(size_t)s + 1]; w += cap)
                runs.push_back(e2hmm::ScanRun{(int)w, (int)std::min<i64>(cap, win_offs[(size_t)s + 1] - w)});
    };
    std::map<int, std::vector<int>> by_N;  // models of N <= 64 states, by N
    std::vector<int> big;                  // the others
    int big_N = 0;
    for (int k = 0; k < K; ++k) {
        if (ms[(size_t)k]->N > e2hmm::WAVE_N) {
            big.push_back(k);
            big_N = std::max(big_N, ms[(size_t)k]->N);
        } else {
            by_N[ms[(size_t)k]->N].push_back(k);
        }
    }
    struct Launch {
        int N, G, span_lds, ks_at, nk, runs_at, nruns;
    };
    std::vector<Launch> launches;
    std::vector<int> ks;
    std::vector<e2hmm::ScanRun> runs;
    const int rounds = scan_rounds();
    for (const auto& kv : by_N) {
        const int N = kv.first, G = scan_pack_width_in_use(N);
        i64 cap = (i64)e2hmm::scan_waves() * G * rounds;
        // (a window longer than the staging area is read from global memory; shorter ones: as many as fit)
        if (window <= e2hmm::SCAN_SPAN_CAP) cap = std::min<i64>(cap, (e2hmm::SCAN_SPAN_CAP - window) / hop + 1);
        // the longest span among the runs this launch makes: a run lies in one stream, so (count - 1) hop + window is at most
        // that stream's length, whatever the hop
        i64 span = 0;
        for (int s = 0; s < S; ++s)
            if (const i64 n = win_offs[(size_t)s + 1] - win_offs[(size_t)s]) span = std::max(span, (std::min(cap, n) - 1) * hop + window);
        Launch l{N, G, (int)(span <= e2hmm::SCAN_SPAN_CAP ? span : 0), (int)ks.size(), (int)kv.second.size(), (int)runs.size(), 0};
        ks.insert(ks.end(), kv.second.begin(), kv.second.end());
        make_runs(cap, runs);
        l.nruns = (int)runs.size() - l.runs_at;
        launches.push_back(l);
    }
    const int big_at = (int)ks.size();
    ks.insert(ks.end(), big.begin(), big.end());

    DevModels dm;
    if (dm.upload(ms, st)) return 1;
    DeviceBuffer<e2hmm::ScanWin> d_wins;
    DeviceBuffer<e2hmm::ScanRun> d_runs;
    DeviceBuffer<int> d_ks, d_top;
    DeviceBuffer<i64> d_offs, d_texp;
    DeviceBuffer<double> d_tmant;
    Scores sc;  // the W x K matrix
    const size_t n = (size_t)W * K;
    if (d_wins.upload(wins.data(), wins.size(), st) || d_runs.upload(runs.data(), runs.size(), st) ||
        d_ks.upload(ks.data(), ks.size(), st) || d_offs.upload(h_offs, (size_t)S + 1, st) || sc.reserve(n) ||
        d_top.reserve((size_t)2 * W) || d_tmant.reserve((size_t)2 * W) || d_texp.reserve((size_t)2 * W))
        return 1;
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    for (const Launch& l : launches) {
        if (e2hmm::launch_scan(dm.table.get(), d_ks.get() + l.ks_at, l.nk, K, l.N, l.G, d_wins.get(), d_runs.get() + l.runs_at, l.nruns,
                               l.span_lds, d_sym, d_offs.get(), sc.d_mant.get(), sc.d_exp.get(), sc.d_status.get(), st))
            return e2vq_set_error("hmm scan: %d runs of N=%d, G=%d over a staged span of %d symbols cannot be launched", l.nruns, l.N,
                                  l.G, l.span_lds);
        HIPCHK(hipGetLastError());
    }
    if (!big.empty()) {
        if (e2hmm::launch_scan_wg(dm.table.get(), d_ks.get() + big_at, (int)big.size(), K, big_N, d_wins.get(), W, d_sym, d_offs.get(),
                                  sc.d_mant.get(), sc.d_exp.get(), sc.d_status.get(), st))
            return e2vq_set_error("hmm scan: %lld windows under models of up to %d states cannot be launched", (long long)W, big_N);
        HIPCHK(hipGetLastError());
    }
    e2hmm::launch_scan_top2(sc.d_mant.get(), sc.d_exp.get(), sc.d_status.get(), W, K, d_top.get(), d_tmant.get(), d_texp.get(), st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(timer.stop.e, st));
    std::vector<int> top;
    std::vector<double> tmant;
    std::vector<i64> texp;
    if (out.top()) {
        top.resize((size_t)2 * W);
        tmant.resize((size_t)2 * W);
        texp.resize((size_t)2 * W);
        HIPCHK(hipMemcpyAsync(top.data(), d_top.get(), top.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(tmant.data(), d_tmant.get(), tmant.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(texp.data(), d_texp.get(), texp.size() * 8, hipMemcpyDeviceToHost, st));
    }
    if (out.matrix() && sc.download(n, st)) return 1;
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    if (timer.elapsed_ms(&g_scan_kernel_ms)) return 1;
    if (out.top())
        for (i64 w = 0; w < W; ++w) {
            const size_t a = (size_t)2 * w, b = a + 1;
            if (out.best) out.best[w] = top[a];
            if (out.second) out.second[w] = top[b];
            if (out.best_log_prob) out.best_log_prob[w] = log_prob(tmant[a], texp[a]);
            if (out.second_log_prob) out.second_log_prob[w] = log_prob(tmant[b], texp[b]);
        }
    if (out.matrix())
        for (size_t i = 0; i < n; ++i)
            sc.get(i, out.mant ? out.mant + i : nullptr, out.exp2 ? out.exp2 + i : nullptr, out.status ? out.status + i : nullptr,
                   out.log_probs ? out.log_probs + i : nullptr);
    return 0;
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

// `seq show [-P] [-Q] --hmm <model>` (the reference's commented `ecoz2_seq_show_files`, src/ecoz2_lib/mod.rs:169-177,
// with --full and -L of `seq show` on top).  Every file is loaded first; the sequences whose M is the model's then go
// through one forward scoring call (with_prob) and one Viterbi call (gen_q_opt), and the report follows, file by file.
extern "C" int e2vq_seq_show_files(int with_prob, int gen_q_opt, int no_sequence, const char* hmm_filename,
                                   const char* const* sequence_filenames, int num_sequences, int full, int only_length)
{
    FlushStdout flush_on_return;
    if (num_sequences < 0 || (num_sequences > 0 && !sequence_filenames)) return e2vq_set_error("e2vq_seq_show_files: bad arguments");
    const bool model = with_prob || gen_q_opt;
    Hmm h;
    std::vector<double> lflat;
    if (model) {
        if (!hmm_filename || !*hmm_filename) return e2vq_set_error("-P / -Q need a model (--hmm)");
        if (hmm_load(hmm_filename, h)) return 1;
        if (log_model(h, lflat)) return 1;
        if (require_device(env_device())) return 1;
    }
    struct File {
        bool ok = false;
        std::string cls;
        int M = 0;
        std::vector<uint16_t> sym;
        int batch = -1;  // index among the sequences decoded / scored
    };
    std::vector<File> fs((size_t)num_sequences);
    std::vector<uint16_t> sym;
    std::vector<i64> offs(1, 0);
    for (int i = 0; i < num_sequences; ++i) {
        File& f = fs[(size_t)i];
        char cls[96];
        int64_t T;
        if (e2vq_seq_info(sequence_filenames[i], cls, &f.M, &T)) continue;
        f.sym.resize((size_t)T);
        if (T > 0 && e2vq_seq_read(sequence_filenames[i], f.sym.data(), T)) continue;
        f.ok = true;
        f.cls = cls;
        if (model && f.M == h.M) {
            f.batch = (int)offs.size() - 1;
            sym.insert(sym.end(), f.sym.begin(), f.sym.end());
            offs.push_back((i64)sym.size());
        }
    }
    const int S = (int)offs.size() - 1;
    Scores lp;
    std::vector<double> vlp((size_t)S);
    std::vector<int> vst((size_t)S);
    std::vector<uint16_t> path(sym.size());
    if (model && S > 0) {
        DevSeqs seqs;
        if (seqs.upload(sym.data(), offs.data(), S)) return 1;
        if (with_prob && score_device({&h}, seqs.sym, seqs.d_offs.get(), S, seqs.st.s, lp)) return 1;
        if (gen_q_opt && viterbi_device(h.N, h.M, lflat, seqs.sym, seqs.d_offs.get(), offs.data(), S, seqs.st.s, path.data(), vlp.data(), vst.data()))
            return 1;
    }
    for (int i = 0; i < num_sequences; ++i) {
        const File& f = fs[(size_t)i];
        if (!f.ok) {
            printf("%s: Not a sequence\n", sequence_filenames[i]);
            continue;
        }
        const size_t len = f.sym.size();
        if (!no_sequence) {
            if (only_length) {
                printf("%zu\n", len);
            } else {
                printf("<%s(M=%d,L=%zu): ", f.cls.c_str(), f.M, len);
                print_abbreviated(f.sym.data(), len, full != 0);
                printf(">\n");
            }
        }
        if (!model) continue;
        if (f.batch < 0) {
            printf("  codebook size M=%d differs from the model's M=%d: no log_prob, no q_opt\n", f.M, h.M);
            continue;
        }
        const size_t b = (size_t)f.batch;
        if (with_prob) printf("  log_prob = %.17g\n", lp.log_prob(b));
        if (gen_q_opt) {
            if (vst[b] != 2) {
                printf("  q_opt = ");
                print_abbreviated(path.data() + offs[b], len, full != 0);
                printf("\n");
            }
            printf("  q_opt_log_prob = %.17g\n", vlp[b]);
        }
        for (size_t t = 0; t < len; ++t)
            if ((int)f.sym[t] >= h.M) {
                printf("  note: symbol %u at t = %zu is outside the model's alphabet (M = %d)\n", (unsigned)f.sym[t], t, h.M);
                break;
            }
    }
    return 0;
}

// fn ecoz2_seq_show_files(with_prob, gen_q_opt, show_sequence, hmm_filename, sequence_filenames, num_sequences)
//                                                      src/ecoz2_lib/mod.rs:169-177 (commented out in the reference)
// The third argument is the reference caller's `no_sequence` (its wrapper, :518-523, passes it there), not the
// declaration's `show_sequence`: nonzero leaves the symbol line out.
extern "C" int ecoz2_seq_show_files(int with_prob, int gen_q_opt, int no_sequence, const char* hmm_filename,
                                    const char* const* sequence_filenames, int num_sequences)
{
    return e2vq_seq_show_files(with_prob, gen_q_opt, no_sequence, hmm_filename, sequence_filenames, num_sequences, 0, 0);
}

// Viterbi decoding of S host sequences under one model: ln P*, status and (path non-null) Q*
extern "C" int e2vq_hmm_viterbi(int device, int N, int M, const double* pi, const double* A, const double* B,
                                const uint16_t* sym, const int64_t* offs, int S, uint16_t* path, double* log_prob,
                                int* status)
{
    Hmm h;
    std::vector<double> lflat;
    if (model_from_arrays(N, M, pi, A, B, h) || log_model(h, lflat) || check_offsets(offs, S)) return 1;
    if (!log_prob || !status) return e2vq_set_error("e2vq_hmm_viterbi: log_prob and status are required");
    if (require_device(device)) return 1;
    DevSeqs seqs;
    if (seqs.upload(sym, (const i64*)offs, S)) return 1;
    return viterbi_device(N, M, lflat, seqs.sym, seqs.d_offs.get(), (const i64*)offs, S, seqs.st.s, path, log_prob, status);
}

// ---- hmm scan -----------------------------------------------------------------------------------------
// window count of every stream (host only): win_offs[S + 1]
extern "C" int e2vq_hmm_scan_windows(const int64_t* offs, int S, int64_t window_frames, int64_t hop_frames, int64_t* win_offs)
{
    if (scan_check_geometry("e2vq_hmm_scan_windows", window_frames, hop_frames)) return 1;
    if (!win_offs) return e2vq_set_error("e2vq_hmm_scan_windows: bad arguments");
    if (check_offsets(offs, S)) return 1;
    scan_window_offsets((const i64*)offs, S, window_frames, hop_frames, (i64*)win_offs);
    return 0;
}

extern "C" int e2vq_hmm_scan_last_kernel_ms(float* ms) { return last_kernel_ms("e2vq_hmm_scan_last_kernel_ms", g_scan_kernel_ms, ms); }

// every window of S streams under K models sharing M: each result is e2vq_hmm_score's for the window's symbols, bit for bit
extern "C" int e2vq_hmm_scan(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                             const double* const* Bs, const void* sym, const int64_t* offs, int S, int64_t window_frames,
                             int64_t hop_frames, int64_t* win_offs, double* mant, int64_t* exp2, int* status, double* log_probs,
                             int* best, double* best_log_prob, int* second, double* second_log_prob, int sym_on_device)
{
    if (scan_check_geometry("e2vq_hmm_scan", window_frames, hop_frames)) return 1;
    if (loop_check_args("e2vq_hmm_scan", K, Ns, pis, As, Bs, syms_given(sym, offs, S))) return 1;
    for (int k = 0; k < K; ++k)
        if (Ns[k] < 1 || Ns[k] > e2hmm::MAX_N)
            return e2vq_set_error("e2vq_hmm_scan: model %d has N=%d states (1 .. %d)", k, Ns[k], e2hmm::MAX_N);
    std::vector<Hmm> models;
    std::vector<const Hmm*> ms;
    if (models_from_arrays(K, Ns, M, pis, As, Bs, models, ms) || check_offsets(offs, S)) return 1;
    std::vector<i64> wo((size_t)S + 1);
    scan_window_offsets((const i64*)offs, S, window_frames, hop_frames, wo.data());
    if (win_offs) memcpy(win_offs, wo.data(), wo.size() * 8);
    if (require_device(device)) return 1;
    DevSeqs seqs;
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0)) return 1;
    ScanOut out;
    out.mant = mant, out.exp2 = exp2, out.status = status, out.log_probs = log_probs;
    out.best = best, out.best_log_prob = best_log_prob, out.second = second, out.second_log_prob = second_log_prob;
    return scan_device(ms, seqs.sym, (const i64*)offs, S, window_frames, hop_frames, seqs.st.s, out);
}

// CSV and stdout block of one scanned input from its two results per window (host only)
extern "C" int e2vq_hmm_scan_report(const char* name, int64_t T, int K, const char* const* class_names, int64_t W,
                                    int64_t window_frames, int64_t hop_frames, int W_ms, int O_ms, const int* best,
                                    const double* best_log_prob, const int* second, const double* second_log_prob,
                                    double min_margin, const char* csv_filename)
{
    FlushStdout flush_on_return;
    if (!name || K < 1 || !class_names || W < 0 || (W > 0 && (!best || !best_log_prob || !second || !second_log_prob)))
        return e2vq_set_error("e2vq_hmm_scan_report: bad arguments");
    if (scan_check_geometry("e2vq_hmm_scan_report", window_frames, hop_frames)) return 1;
    for (int64_t w = 0; w < W; ++w)
        if (best[w] < 0 || best[w] >= K || second[w] < -1 || second[w] >= K)
            return e2vq_set_error("e2vq_hmm_scan_report: window %lld names a model outside [0, %d)", (long long)w, K);
    auto begin_s = [&](int64_t w) { return (double)(w * hop_frames * O_ms) / 1000.0; };
    // (the end of the analysis window of the window's last frame)
    auto end_s = [&](int64_t w) { return (double)((w * hop_frames + window_frames - 1) * O_ms + W_ms) / 1000.0; };
    if (csv_filename && *csv_filename) {
        std::string doc = "window,begin_frame,end_frame,begin_s,end_s,class,log_prob,second_class,second_log_prob\n";
        for (int64_t w = 0; w < W; ++w) {
            const bool has1 = best_log_prob[w] > -INFINITY, has2 = second[w] >= 0 && second_log_prob[w] > -INFINITY;
            doc += std::to_string(w) + "," + std::to_string(w * hop_frames) + "," + std::to_string(w * hop_frames + window_frames) + "," +
                   fmt_17g(begin_s(w)) + "," + fmt_17g(end_s(w)) + "," + (has1 ? class_names[best[w]] : "") + "," +
                   fmt_17g(best_log_prob[w]) + "," + (has2 ? class_names[second[w]] : "") + "," +
                   fmt_17g(second[w] >= 0 ? second_log_prob[w] : -INFINITY) + "\n";
        }
        if (write_file(csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    printf("%s: T=%lld  windows=%lld  (window %lld frames, hop %lld)\n", name, (long long)T, (long long)W, (long long)window_frames,
           (long long)hop_frames);
    std::vector<int64_t> won((size_t)K, 0);
    int64_t none = 0;
    for (int64_t w = 0; w < W; ++w) {
        if (best_log_prob[w] > -INFINITY) ++won[(size_t)best[w]];
        else ++none;
    }
    for (int k = 0; k < K; ++k) printf("  '%s': %lld\n", class_names[k], (long long)won[(size_t)k]);
    if (none) printf("  (no model can emit the window): %lld\n", (long long)none);
    printf("  runs (margin >= %g):\n", min_margin);
    // maximal runs of consecutive windows won by one class with margin >= min_margin (a window no model can emit wins nothing)
    auto winner = [&](int64_t w) -> int {
        if (!(best_log_prob[w] > -INFINITY)) return -1;
        const double second_lp = second[w] >= 0 ? second_log_prob[w] : -INFINITY;
        return best_log_prob[w] - second_lp >= min_margin ? best[w] : -1;
    };
    for (int64_t w = 0; w < W;) {
        const int c = winner(w);
        int64_t e = w + 1;
        while (e < W && winner(e) == c) ++e;
        if (c >= 0) printf("    %.3f - %.3f %s\n", begin_s(w), end_s(e - 1), class_names[c]);
        w = e;
    }
    if (csv_filename && *csv_filename) printf("  %s saved\n", csv_filename);
    return 0;
}

// `hmm scan`: every input (.wav: lpc -> quantize -> scan; .prd: quantize -> scan; .seq: scan) under the models
extern "C" int e2vq_hmm_scan_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                   const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                   int64_t window_frames, int64_t hop_frames, double min_margin, const char* csv_dir_or_file)
{
    FlushStdout flush_on_return;
    if (files_given("e2vq_hmm_scan_files", model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
    if (scan_check_geometry("e2vq_hmm_scan_files", window_frames, hop_frames) || window_ms_ok("e2vq_hmm_scan_files", W_ms, O_ms)) return 1;
    FilesModels fm;
    if (fm.load(model_filenames, num_models)) return 1;
    auto run = [&](const SymInput& in, int64_t T, const unsigned short* d_sym, hipStream_t st) -> int {
        const i64 offs[2] = {0, T};
        i64 wo[2];
        scan_window_offsets(offs, 1, window_frames, hop_frames, wo);
        const size_t W = (size_t)wo[1];
        std::vector<int> best(W), second(W);
        std::vector<double> lp1(W), lp2(W);
        ScanOut out;
        out.best = best.data(), out.best_log_prob = lp1.data(), out.second = second.data(), out.second_log_prob = lp2.data();
        if (scan_device(fm.ms, d_sym, offs, 1, window_frames, hop_frames, st, out)) return 1;
        HIPCHK(hipStreamSynchronize(st));  // (the host buffers of this input are locals)
        return e2vq_hmm_scan_report(in.path.c_str(), T, (int)num_models, fm.names.data(), (int64_t)W, window_frames, hop_frames, W_ms, O_ms,
                                    best.data(), lp1.data(), second.data(), lp2.data(), min_margin, in.csv.empty() ? nullptr : in.csv.c_str());
    };
    return run_on_files("e2vq_hmm_scan_files", fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, run);
}
