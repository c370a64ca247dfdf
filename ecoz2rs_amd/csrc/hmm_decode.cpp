// hmm_decode.cpp -- decoding on the GPU: Viterbi under one model (`seq show -P / -Q --hmm`, e2vq_hmm_viterbi; DESIGN.md
// 4.8.1), the models over the windows of whole recordings (`hmm scan`, 4.8.5), the joint Viterbi through the class
// loop of all models (`hmm segment`, 4.8.6) and the class posteriors under that loop (`--posteriors`, 4.8.7), with the
// stage that turns a .wav / .prd / .seq input into device symbols; over the kernels of hmm_viterbi.hip, hmm_scan.hip,
// hmm_segment.hip and hmm_posterior.hip; and the same loop under a matrix of class-to-class prices (`hmm segment
// --class-transitions`, 4.8.8, hmm_segment_trans.hip) with the estimator of that matrix (`hmm transitions`).
#include "hmm_host.h"

#include <functional>

namespace e2hmm_host {
namespace {

// The launches of a decoder whose table takes `row` bytes a frame: whole sequences [s0, s1) up to the budget of the
// environment variable `env` (default 256 MiB), a longer sequence alone; *max_frames: the most frames of a launch
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
        const i64 span = (std::min<i64>(cap, W) - 1) * hop + window;
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
    DeviceBuffer<int> d_ks, d_st, d_top;
    DeviceBuffer<i64> d_offs, d_exp, d_texp;
    DeviceBuffer<double> d_mant, d_tmant;
    const size_t n = (size_t)W * K;
    if (d_wins.upload(wins.data(), wins.size(), st) || d_runs.upload(runs.data(), runs.size(), st) ||
        d_ks.upload(ks.data(), ks.size(), st) || d_offs.upload(h_offs, (size_t)S + 1, st) || d_mant.reserve(n) || d_exp.reserve(n) ||
        d_st.reserve(n) || d_top.reserve((size_t)2 * W) || d_tmant.reserve((size_t)2 * W) || d_texp.reserve((size_t)2 * W))
        return 1;
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    for (const Launch& l : launches) {
        e2hmm::launch_scan(dm.table.get(), d_ks.get() + l.ks_at, l.nk, K, l.N, l.G, d_wins.get(), d_runs.get() + l.runs_at, l.nruns,
                           l.span_lds, d_sym, d_offs.get(), d_mant.get(), d_exp.get(), d_st.get(), st);
        HIPCHK(hipGetLastError());
    }
    if (!big.empty()) {
        e2hmm::launch_scan_wg(dm.table.get(), d_ks.get() + big_at, (int)big.size(), K, big_N, d_wins.get(), W, d_sym, d_offs.get(),
                              d_mant.get(), d_exp.get(), d_st.get(), st);
        HIPCHK(hipGetLastError());
    }
    e2hmm::launch_scan_top2(d_mant.get(), d_exp.get(), d_st.get(), W, K, d_top.get(), d_tmant.get(), d_texp.get(), st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(timer.stop.e, st));
    std::vector<int> top, stat;
    std::vector<double> tmant, mant;
    std::vector<i64> texp, ex;
    if (out.top()) {
        top.resize((size_t)2 * W);
        tmant.resize((size_t)2 * W);
        texp.resize((size_t)2 * W);
        HIPCHK(hipMemcpyAsync(top.data(), d_top.get(), top.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(tmant.data(), d_tmant.get(), tmant.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(texp.data(), d_texp.get(), texp.size() * 8, hipMemcpyDeviceToHost, st));
    }
    if (out.matrix()) {
        mant.resize(n);
        ex.resize(n);
        stat.resize(n);
        HIPCHK(hipMemcpyAsync(mant.data(), d_mant.get(), n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ex.data(), d_exp.get(), n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stat.data(), d_st.get(), n * 4, hipMemcpyDeviceToHost, st));
    }
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
        for (size_t i = 0; i < n; ++i) {
            if (out.mant) out.mant[i] = mant[i];
            if (out.exp2) out.exp2[i] = ex[i];
            if (out.status) out.status[i] = stat[i];
            if (out.log_probs) out.log_probs[i] = stat[i] == 0 ? log_prob(mant[i], ex[i]) : -INFINITY;
        }
    return 0;
}

// ---- hmm segment: one Viterbi pass through the class loop of all models ------------------------------------
thread_local float g_segment_kernel_ms = -1.f;  // e2vq_hmm_segment_last_kernel_ms

}  // namespace

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

namespace {

struct SegOut {  // host arrays, any may be null; per frame: cls, state, entered, gbest; per stream: log_prob, status
    uint16_t* cls = nullptr;
    uint16_t* state = nullptr;
    uint8_t* entered = nullptr;
    double* gbest = nullptr;
    double* log_prob = nullptr;
    int* status = nullptr;
};

}  // namespace

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

namespace {

// The joint Viterbi of S device-resident streams (h_offs: their S + 1 offsets, on the host) under the class loop of the
// models (already checked by segment_check_shape; all of one M; lflats: log_model of each), on the current device and the
// stream st.
int segment_device(const std::vector<const Hmm*>& ms, const std::vector<std::vector<double>>& lflats, const unsigned short* d_sym, const i64* h_offs, int S, double ln_switch,
                   hipStream_t st, const SegOut& out)
{
    const int K = (int)ms.size(), M = ms[0]->M;
    std::vector<int> Ns;
    for (const Hmm* h : ms) Ns.push_back(h->N);
    const SegPacking pk = pack_slots(Ns, [](int N) { return N; });
    const int sumN = pk.sumN, a_words = pk.a_words, slots = pk.slots;
    const std::vector<int>& comp0 = pk.comp0;
    const std::vector<int>& a_at = pk.a_at;
    const std::vector<int>& slot_info = pk.slot_info;
    const std::vector<e2hmm::SegLaneDev>& lanes = pk.lanes;
    const std::vector<uint16_t>& comp_cls = pk.comp_cls;
    // logarithms: lpi of every class | lA of every class | lB of every class
    std::vector<double> params((size_t)sumN + (size_t)a_words + (size_t)sumN * M);
    for (int k = 0; k < K; ++k) {
        const std::vector<double>& lflat = lflats[(size_t)k];
        const size_t N = (size_t)ms[(size_t)k]->N;
        std::copy(lflat.begin(), lflat.begin() + N, params.begin() + comp0[(size_t)k]);
        std::copy(lflat.begin() + N, lflat.begin() + N + N * N, params.begin() + sumN + a_at[(size_t)k]);
        std::copy(lflat.begin() + N + N * N, lflat.end(), params.begin() + sumN + a_words + (size_t)comp0[(size_t)k] * M);
    }
    // the body: resident where the packing fits a workgroup's waves, unless ECOZ2_HMM_SEGMENT_BODY=looped
    const char* body = getenv("ECOZ2_HMM_SEGMENT_BODY");
    if (body && *body && strcmp(body, "resident") != 0 && strcmp(body, "looped") != 0)
        return e2vq_set_error("ECOZ2_HMM_SEGMENT_BODY=%s: resident or looped", body);
    const bool looped = slots > e2hmm::SEG_MAX_WAVES || (body && strcmp(body, "looped") == 0);

    DeviceBuffer<double> d_params, d_logp, d_gbest;
    DeviceBuffer<e2hmm::SegLaneDev> d_lanes;
    DeviceBuffer<int> d_info, d_comp0, d_status, d_qlast, d_gsel;
    DeviceBuffer<unsigned short> d_comp_cls, d_psi, d_cls, d_state;
    DeviceBuffer<unsigned char> d_entered;
    DeviceBuffer<i64> d_offs;
    const i64 frames = h_offs[S];
    if (d_params.upload(params.data(), params.size(), st) || d_lanes.upload(lanes.data(), lanes.size(), st) ||
        d_info.upload(slot_info.data(), slot_info.size(), st) || d_comp0.upload(comp0.data(), comp0.size(), st) ||
        d_comp_cls.upload(comp_cls.data(), comp_cls.size(), st) || d_offs.upload(h_offs, (size_t)S + 1, st) ||
        d_logp.reserve((size_t)S) || d_status.reserve((size_t)S) || d_qlast.reserve((size_t)S) || d_gbest.reserve((size_t)frames) ||
        d_cls.reserve((size_t)frames) || d_state.reserve((size_t)frames) || d_entered.reserve((size_t)frames))
        return 1;
    const e2hmm::SegPlanDev pl{K, M, sumN, slots, a_words, d_lanes.get(), d_info.get(), d_params.get(), d_comp_cls.get(), d_comp0.get()};
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
        if (e2hmm::launch_segment(pl, looped, d_sym, d_offs.get() + s0, n, h_offs[s0], ln_switch, d_psi.get(), d_gsel.get(), d_gbest.get(),
                                  d_logp.get() + s0, d_qlast.get() + s0, d_status.get() + s0, st))
            return e2vq_set_error("hmm segment: %d wave-slots of %d states cannot be launched", slots, sumN);
        HIPCHK(hipGetLastError());
        e2hmm::launch_segment_backtrack(pl, d_offs.get() + s0, n, h_offs[s0], d_psi.get(), d_gsel.get(), d_qlast.get() + s0,
                                        d_status.get() + s0, d_cls.get(), d_state.get(), d_entered.get(), d_gbest.get(), st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    if (frames > 0) {
        if (out.cls) HIPCHK(hipMemcpyAsync(out.cls, d_cls.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
        if (out.state) HIPCHK(hipMemcpyAsync(out.state, d_state.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
        if (out.entered) HIPCHK(hipMemcpyAsync(out.entered, d_entered.get(), (size_t)frames, hipMemcpyDeviceToHost, st));
        if (out.gbest) HIPCHK(hipMemcpyAsync(out.gbest, d_gbest.get(), (size_t)frames * 8, hipMemcpyDeviceToHost, st));
    }
    if (S > 0) {
        if (out.log_prob) HIPCHK(hipMemcpyAsync(out.log_prob, d_logp.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        if (out.status) HIPCHK(hipMemcpyAsync(out.status, d_status.get(), (size_t)S * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    if (timer.elapsed_ms(&g_segment_kernel_ms)) return 1;
    return 0;
}

// ---- hmm segment --posteriors: forward-backward through the same class loop -------------------------------
thread_local float g_posteriors_kernel_ms = -1.f;  // e2vq_hmm_segment_posteriors_last_kernel_ms

int posteriors_a_ld(int N) { return N | 1; }  // (odd: see hmm_posterior.hip)

// only the resident layout exists: a packing of more than SEG_MAX_WAVES slots is refused (host only)
int posteriors_check_slots(const char* who, int K, const int* Ns)
{
    const int slots = pack_slots(std::vector<int>(Ns, Ns + K), posteriors_a_ld).slots;
    if (slots > e2hmm::SEG_MAX_WAVES)
        return e2vq_set_error("%s: the classes take %d wave-slots of 64 lanes (at most %d: the posteriors have no looped body)", who,
                              slots, e2hmm::SEG_MAX_WAVES);
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

struct PostOut {  // host arrays, any may be null; post: K doubles a frame; per stream: log_prob, status
    double* post = nullptr;
    double* log_prob = nullptr;
    int* status = nullptr;
};

// The smoothed class posteriors of S device-resident streams (h_offs: their S + 1 offsets, on the host) under the class
// loop of the models (already checked by segment_check_shape and posteriors_check_slots; all of one M), on the current
// device and the stream st.
int posteriors_device(const std::vector<const Hmm*>& ms, const unsigned short* d_sym, const i64* h_offs, int S, double ln_switch,
                      hipStream_t st, const PostOut& out)
{
    const int K = (int)ms.size(), M = ms[0]->M;
    std::vector<int> Ns;
    for (const Hmm* h : ms) Ns.push_back(h->N);
    const SegPacking pk = pack_slots(Ns, posteriors_a_ld);
    const int sumN = pk.sumN, a_words = pk.a_words, slots = pk.slots;
    const double sw = exp(ln_switch);  // (-inf: 0.0)
    // pi of every class | e = sw pi | A of every class, row i at i (N | 1) | B of every class
    std::vector<double> params((size_t)2 * sumN + (size_t)a_words + (size_t)sumN * M, 0.0);
    for (int k = 0; k < K; ++k) {
        const Hmm& h = *ms[(size_t)k];
        const int N = h.N, ld = posteriors_a_ld(N), c0 = pk.comp0[(size_t)k];
        for (int j = 0; j < N; ++j) {
            params[(size_t)(c0 + j)] = h.pi[(size_t)j];
            params[(size_t)(sumN + c0 + j)] = sw * h.pi[(size_t)j];
            std::copy(h.A.begin() + (size_t)j * N, h.A.begin() + (size_t)(j + 1) * N,
                      params.begin() + 2 * sumN + pk.a_at[(size_t)k] + (size_t)j * ld);
        }
        std::copy(h.B.begin(), h.B.end(), params.begin() + 2 * sumN + a_words + (size_t)c0 * M);
    }
    DeviceBuffer<double> d_params, d_mant, d_post, d_ah, d_c;
    DeviceBuffer<e2hmm::SegLaneDev> d_lanes;
    DeviceBuffer<int> d_info, d_comp0, d_status;
    DeviceBuffer<unsigned short> d_comp_cls;
    DeviceBuffer<i64> d_offs, d_exp;
    const i64 frames = h_offs[S];
    if (d_params.upload(params.data(), params.size(), st) || d_lanes.upload(pk.lanes.data(), pk.lanes.size(), st) ||
        d_info.upload(pk.slot_info.data(), pk.slot_info.size(), st) || d_comp0.upload(pk.comp0.data(), pk.comp0.size(), st) ||
        d_comp_cls.upload(pk.comp_cls.data(), pk.comp_cls.size(), st) || d_offs.upload(h_offs, (size_t)S + 1, st) ||
        d_mant.reserve((size_t)S) || d_exp.reserve((size_t)S) || d_status.reserve((size_t)S) || d_post.reserve((size_t)frames * K))
        return 1;
    const e2hmm::SegPlanDev pl{K, M, sumN, slots, a_words, d_lanes.get(), d_info.get(), d_params.get(), d_comp_cls.get(), d_comp0.get()};
    // launches of whole streams whose ah (8 sumN bytes a frame) and c (8 bytes a frame and wave) stay within the budget
    const i64 row = 8 * ((i64)sumN + slots);
    i64 max_frames = 0;
    const auto chunks = plan_chunks("ECOZ2_HMM_POSTERIOR_CHUNK_BYTES", row, h_offs, S, &max_frames);
    if (d_ah.reserve((size_t)max_frames * sumN) || d_c.reserve((size_t)max_frames * slots)) {
        const std::string why = e2vq_last_error();
        return e2vq_set_error("hmm segment --posteriors: no room for the forward table of %lld frames x %d states (%lld bytes; "
                              "ECOZ2_HMM_POSTERIOR_CHUNK_BYTES bounds it by whole streams): %s",
                              (long long)max_frames, sumN, (long long)(max_frames * row), why.c_str());
    }
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes the tables only after the previous chunk's backward pass has read them)
    for (const auto& c : chunks) {
        const int s0 = c.first, n = c.second - c.first;
        if (e2hmm::launch_loop_posteriors(pl, d_sym, d_offs.get() + s0, n, h_offs[s0], sw, d_ah.get(), d_c.get(), d_post.get(),
                                          d_mant.get() + s0, d_exp.get() + s0, d_status.get() + s0, st))
            return e2vq_set_error("hmm segment --posteriors: %d wave-slots of %d states cannot be launched", slots, sumN);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    std::vector<double> mant((size_t)S);
    std::vector<i64> ex((size_t)S);
    std::vector<int> stat((size_t)S);
    if (frames > 0 && out.post) HIPCHK(hipMemcpyAsync(out.post, d_post.get(), (size_t)frames * K * 8, hipMemcpyDeviceToHost, st));
    if (S > 0) {
        HIPCHK(hipMemcpyAsync(mant.data(), d_mant.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ex.data(), d_exp.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stat.data(), d_status.get(), (size_t)S * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    if (timer.elapsed_ms(&g_posteriors_kernel_ms)) return 1;
    for (int s = 0; s < S; ++s) {
        if (out.log_prob) out.log_prob[s] = stat[(size_t)s] == 0 ? log_prob(mant[(size_t)s], ex[(size_t)s]) : -INFINITY;
        if (out.status) out.status[s] = stat[(size_t)s];
    }
    return 0;
}

}  // namespace

// ---- input -> device symbols: the stage `hmm scan` and `hmm segment` share (its structs: hmm_host.h) --------------------------

// the checks of the inputs against the models' M and the codebook, and the codebook itself: host only, no file written
int sym_inputs_check(const char* who, int M, const char* cb_filename, const char* const* input_filenames, int num_inputs,
                            int P, int W_ms, int O_ms, const char* csv_dir_or_file, SymInputs& si)
{
    si.have_cb = cb_filename && *cb_filename;
    if (si.have_cb) {
        char cls[96];
        if (e2vq_cbook_info(cb_filename, cls, &si.cbP, &si.cbM)) return 1;
        if (si.cbM != M) return e2vq_set_error("%s: codebook has M=%d but the models have M=%d", cb_filename, si.cbM, M);
    }
    const bool have_cb = si.have_cb;
    const int cbP = si.cbP;
    std::vector<SymInput>& inputs = si.inputs;
    inputs.assign((size_t)num_inputs, SymInput());
    const std::string csv = csv_dir_or_file ? csv_dir_or_file : "";
    const bool csv_is_file = num_inputs == 1 && ends_with(csv, ".csv");
    for (int f = 0; f < num_inputs; ++f) {
        SymInput& in = inputs[(size_t)f];
        if (!input_filenames[f]) return e2vq_set_error("%s: NULL file name", who);
        in.path = input_filenames[f];
        char cls[96];
        if (ends_with(in.path, ".seq")) {
            in.kind = 2;
            int m;
            if (e2vq_seq_info(in.path.c_str(), cls, &m, &in.T)) return 1;
            if (m != M) return e2vq_set_error("%s: codebook size %d differs from the models' %d", in.path.c_str(), m, M);
        } else if (ends_with(in.path, ".prd")) {
            in.kind = 1;
            int p;
            if (e2vq_prd_info(in.path.c_str(), cls, &p, &in.T)) return 1;
            if (have_cb && p != cbP)
                return e2vq_set_error("%s: prediction order %d differs from the codebook's %d", in.path.c_str(), p, cbP);
            si.need_cb = true;
        } else if (ends_with(in.path, ".wav")) {
            in.kind = 0;
            if (e2vq_wav_info(in.path.c_str(), &in.sample_rate, &in.samples, nullptr)) return 1;
            if (have_cb && P != cbP) return e2vq_set_error("%s: prediction order -P %d differs from the codebook's %d", in.path.c_str(), P, cbP);
            int win, off;
            if (e2vq_lpc_frame_count(in.samples, in.sample_rate, W_ms, O_ms, &win, &off, &in.T)) return 1;
            if (in.T < 0) return e2vq_set_error("%s: signal too short (%lld samples, window %d)", in.path.c_str(), (long long)in.samples, win);
            si.need_cb = true;
        } else {
            return e2vq_set_error("%s: not a .wav, .prd or .seq file", in.path.c_str());
        }
        if (!csv.empty()) in.csv = csv_is_file ? csv : csv + "/" + e2vq_io::basename_noext(in.path.c_str()) + ".csv";
        for (int g = 0; g < f && !in.csv.empty(); ++g)
            if (inputs[(size_t)g].csv == in.csv) return e2vq_set_error("%s and %s would both write %s", inputs[(size_t)g].path.c_str(), in.path.c_str(), in.csv.c_str());
    }
    if (si.need_cb && !have_cb) return e2vq_set_error("%s: signals and predictors need a codebook", who);
    if (si.need_cb) {
        si.refl.resize((size_t)si.cbM * (cbP + 1));
        if (e2vq_cbook_read(cb_filename, si.refl.data(), si.cbM)) return 1;
    }
    return 0;
}

// one input to symbols in stg.d_sym (read and uploaded once; frames and symbols stay on the device): *T_out of them
int sym_input_to_device(const SymInput& in, const SymInputs& si, SymStage& stg, e2vq_session* vq, int device, int P, int W_ms,
                               int O_ms, hipStream_t st, int64_t* T_out)
{
    const int cbP = si.cbP, NC = cbP + 1;
    int64_t T = in.T;
    std::vector<uint16_t> h_sym;
    std::vector<double> h_frames;
    if (in.kind == 2) {
        h_sym.resize((size_t)std::max<int64_t>(T, 1));
        if (T > 0 && e2vq_seq_read(in.path.c_str(), h_sym.data(), T)) return 1;
        if (stg.d_sym.upload(h_sym.data(), (size_t)T, st)) return 1;
        HIPCHK(hipStreamSynchronize(st));  // (`h_sym` is a local)
    } else {
        if (stg.d_frames.reserve((size_t)std::max<int64_t>(T, 1) * NC) || stg.d_sym.reserve((size_t)T + 64)) return 1;
        if (in.kind == 1) {
            h_frames.resize((size_t)std::max<int64_t>(T, 1) * NC);
            bool fin = true;
            if (T > 0 && e2vq_io::prd_read_range_mt(in.path.c_str(), cbP, 0, T, h_frames.data(), e2vq_io::io_threads(), &fin)) return 1;
            if (!fin) return e2vq_set_error("%s: contains NaN or infinite values", in.path.c_str());
            if (T > 0) HIPCHK(hipMemcpyAsync(stg.d_frames.get(), h_frames.data(), (size_t)T * NC * 8, hipMemcpyHostToDevice, st));
        } else {
            std::vector<int32_t> samples((size_t)std::max<int64_t>(in.samples, 1));
            if (e2vq_wav_read(in.path.c_str(), samples.data(), in.samples)) return 1;
            if (stg.d_status.reserve((size_t)std::max<int64_t>(T, 1))) return 1;
            int64_t T2 = 0;
            if (T > 0 && e2vq_lpc_analyze(device, P, W_ms, O_ms, samples.data(), in.samples, in.sample_rate, stg.d_frames.get(),
                                          stg.d_status.get(), T, &T2, 1))
                return 1;
            std::vector<int32_t> fst((size_t)T);
            if (T > 0) HIPCHK(hipMemcpyAsync(fst.data(), stg.d_status.get(), (size_t)T * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            int64_t good = 0;
            for (int64_t t = 0; t < T; ++t) good += fst[(size_t)t] == 0;
            if (good != T) {
                // frames whose Levinson recursion failed are left out, as `ecoz2 lpc` leaves them out of the .prd: the rest
                // makes one round trip through the host (the only place where the frames leave the device)
                h_frames.resize((size_t)T * NC);
                HIPCHK(hipMemcpy(h_frames.data(), stg.d_frames.get(), (size_t)T * NC * 8, hipMemcpyDeviceToHost));
                int64_t o = 0;
                for (int64_t t = 0; t < T; ++t)
                    if (fst[(size_t)t] == 0) memmove(h_frames.data() + (size_t)(o++) * NC, h_frames.data() + (size_t)t * NC, (size_t)NC * 8);
                printf("%s: %lld frames left out: Levinson status != 0 (later frame times are early by their offsets)\n",
                       in.path.c_str(), (long long)(T - good));
                T = good;
                if (T > 0) HIPCHK(hipMemcpyAsync(stg.d_frames.get(), h_frames.data(), (size_t)T * NC * 8, hipMemcpyHostToDevice, st));
            }
        }
        if (T > 0 && e2vq_quantize_device(vq, stg.d_frames.get(), T, stg.d_sym.get(), nullptr)) return 1;
        HIPCHK(hipStreamSynchronize(st));  // (`h_frames` is a local)
    }
    *T_out = T;
    return 0;
}

namespace {

// What `hmm scan` and `hmm segment` do once the command's own checks have passed (`who`: the entry point): the check of
// the inputs and the codebook against M, still on the host alone; then one device, stream and quantize session, and
// for every input its symbols on the device followed by the command's work on them, run(input, T, d_sym, stream).
int run_on_files(const char* who, int M, const char* cb_filename, const char* const* input_filenames, int num_inputs, int P, int W_ms,
                 int O_ms, const char* csv_dir_or_file,
                 const std::function<int(const SymInput&, int64_t, const unsigned short*, hipStream_t)>& run)
{
    SymInputs si;
    if (sym_inputs_check(who, M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, si)) return 1;
    // ---- the device from here on --------------------------------------------------------------------------------
    const int device = env_device();
    if (require_device(device)) return 1;
    SymStage stg;
    Stream st;
    if (st.create()) return 1;
    VqSessionHolder vq;
    if (si.need_cb) {
        if (e2vq_session_create(device, si.cbP, &vq.s) || e2vq_set_stream(vq.s, (void*)st.s) || e2vq_set_codebook(vq.s, si.refl.data(), si.cbM))
            return 1;
    }
    for (const SymInput& in : si.inputs) {
        int64_t T = 0;
        if (sym_input_to_device(in, si, stg, vq.s, device, P, W_ms, O_ms, st.s, &T)) return 1;
        if (run(in, T, stg.d_sym.get(), st.s)) return 1;
    }
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

extern "C" int e2vq_hmm_scan_last_kernel_ms(float* ms)
{
    if (!ms) return e2vq_set_error("e2vq_hmm_scan_last_kernel_ms: bad arguments");
    *ms = g_scan_kernel_ms;
    return 0;
}

// every window of S streams under K models sharing M: each result is e2vq_hmm_score's for the window's symbols, bit for bit
extern "C" int e2vq_hmm_scan(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                             const double* const* Bs, const void* sym, const int64_t* offs, int S, int64_t window_frames,
                             int64_t hop_frames, int64_t* win_offs, double* mant, int64_t* exp2, int* status, double* log_probs,
                             int* best, double* best_log_prob, int* second, double* second_log_prob, int sym_on_device)
{
    if (scan_check_geometry("e2vq_hmm_scan", window_frames, hop_frames)) return 1;
    if (K < 1) return e2vq_set_error("e2vq_hmm_scan: %d models (at least 1)", K);
    if (!Ns || !pis || !As || !Bs || S < 0 || (!sym && S > 0 && offs && offs[S] > 0)) return e2vq_set_error("e2vq_hmm_scan: bad arguments");
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
    if (!model_filenames || num_models < 1) return e2vq_set_error("e2vq_hmm_scan_files: no models");
    if (!input_filenames || num_inputs < 1) return e2vq_set_error("e2vq_hmm_scan_files: no inputs");
    if (scan_check_geometry("e2vq_hmm_scan_files", window_frames, hop_frames)) return 1;
    if (W_ms < 1 || O_ms < 1) return e2vq_set_error("e2vq_hmm_scan_files: window %d ms / offset %d ms", W_ms, O_ms);
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

// ---- hmm segment --------------------------------------------------------------------------------------
extern "C" int e2vq_hmm_segment_last_kernel_ms(float* ms)
{
    if (!ms) return e2vq_set_error("e2vq_hmm_segment_last_kernel_ms: bad arguments");
    *ms = g_segment_kernel_ms;
    return 0;
}

// the most likely path of each of S streams through the class loop of K models sharing M.  One device.
extern "C" int e2vq_hmm_segment(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                const double* const* Bs, const void* sym, const int64_t* offs, int S, double ln_switch,
                                uint16_t* cls, uint16_t* state, uint8_t* entered, double* gbest, double* log_prob, int* status,
                                int sym_on_device)
{
    if (K < 1) return e2vq_set_error("e2vq_hmm_segment: %d models (at least 1)", K);
    if (!Ns || !pis || !As || !Bs || S < 0 || (!sym && S > 0 && offs && offs[S] > 0)) return e2vq_set_error("e2vq_hmm_segment: bad arguments");
    if (segment_check_shape("e2vq_hmm_segment", K, Ns) || segment_check_switch("e2vq_hmm_segment", ln_switch)) return 1;
    std::vector<Hmm> models;
    std::vector<const Hmm*> ms;
    std::vector<std::vector<double>> lflats((size_t)K);
    // (segment_check_shape has passed every N, and M is one: the models can fail here only before any logarithm does)
    if (models_from_arrays(K, Ns, M, pis, As, Bs, models, ms)) return 1;
    for (int k = 0; k < K; ++k)
        if (log_model(models[(size_t)k], lflats[(size_t)k])) return 1;
    if (check_offsets(offs, S) || require_device(device)) return 1;
    DevSeqs seqs;
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0)) return 1;
    SegOut out;
    out.cls = cls, out.state = state, out.entered = entered, out.gbest = gbest, out.log_prob = log_prob, out.status = status;
    return segment_device(ms, lflats, seqs.sym, (const i64*)offs, S, ln_switch, seqs.st.s, out);
}

namespace {

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

// `hmm segment` with and without --posteriors: every input (.wav: lpc -> quantize -> segment; .prd: quantize -> segment;
// .seq: segment) under the models.  The symbols of an input are staged once; the posteriors run on the same device buffer.
int segment_files(const char* who, const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                  const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                  const char* csv_dir_or_file, bool posteriors, const char* frames_dir)
{
    FlushStdout flush_on_return;
    if (!model_filenames || num_models < 1) return e2vq_set_error("%s: no models", who);
    if (!input_filenames || num_inputs < 1) return e2vq_set_error("%s: no inputs", who);
    if (segment_check_switch(who, ln_switch)) return 1;
    if (W_ms < 1 || O_ms < 1) return e2vq_set_error("%s: window %d ms / offset %d ms", who, W_ms, O_ms);
    FilesModels fm;
    if (fm.load(model_filenames, num_models)) return 1;
    std::vector<int> Ns;
    for (const Hmm& h : fm.models) Ns.push_back(h.N);
    if (segment_check_shape(who, (int)num_models, Ns.data())) return 1;
    if (posteriors && posteriors_check_slots(who, (int)num_models, Ns.data())) return 1;
    std::vector<std::vector<double>> lflats((size_t)num_models);
    for (unsigned k = 0; k < num_models; ++k)
        if (log_model(fm.models[k], lflats[k])) return e2vq_set_error("%s: %s", model_filenames[k], std::string(e2vq_last_error()).c_str());
    const std::string fdir = posteriors && frames_dir ? frames_dir : "";
    auto frames_csv = [&](const char* path) { return fdir + "/" + e2vq_io::basename_noext(path) + ".csv"; };
    for (int f = 0; f < num_inputs && !fdir.empty(); ++f)
        for (int g = 0; g < f; ++g)
            if (input_filenames[f] && input_filenames[g] && frames_csv(input_filenames[g]) == frames_csv(input_filenames[f]))
                return e2vq_set_error("%s and %s would both write %s", input_filenames[g], input_filenames[f], frames_csv(input_filenames[f]).c_str());
    const int K = (int)num_models;
    auto run = [&](const SymInput& in, int64_t T, const unsigned short* d_sym, hipStream_t st) -> int {
        const i64 offs[2] = {0, T};
        const size_t n = (size_t)std::max<int64_t>(T, 1);
        std::vector<uint16_t> cls(n);
        std::vector<uint8_t> entered(n);
        std::vector<double> gbest(n), post;
        double lp = 0.0;
        int status = 0;
        SegOut out;
        out.cls = cls.data(), out.entered = entered.data(), out.gbest = gbest.data(), out.log_prob = &lp, out.status = &status;
        if (segment_device(fm.ms, lflats, d_sym, offs, 1, ln_switch, st, out)) return 1;
        if (status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d", in.path.c_str(), fm.M);
        if (posteriors) {
            post.resize(n * (size_t)K);
            PostOut po;
            po.post = post.data();
            if (posteriors_device(fm.ms, d_sym, offs, 1, ln_switch, st, po)) return 1;
        }
        const std::string fcsv = fdir.empty() ? "" : frames_csv(in.path.c_str());
        return segment_report(who, in.path.c_str(), T, K, fm.names.data(), W_ms, O_ms, cls.data(), entered.data(), gbest.data(), lp,
                              ln_switch, posteriors ? post.data() : nullptr, in.csv.empty() ? nullptr : in.csv.c_str(),
                              fcsv.empty() ? nullptr : fcsv.c_str());
    };
    return run_on_files(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, run);
}

}  // namespace

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
                         ln_switch, csv_dir_or_file, false, nullptr);
}

// ---- hmm segment --posteriors -------------------------------------------------------------------------
extern "C" int e2vq_hmm_segment_posteriors_last_kernel_ms(float* ms)
{
    if (!ms) return e2vq_set_error("e2vq_hmm_segment_posteriors_last_kernel_ms: bad arguments");
    *ms = g_posteriors_kernel_ms;
    return 0;
}

// P(class at frame t | the whole stream) of each of S streams under the class loop of K models sharing M.  One device.
extern "C" int e2vq_hmm_segment_posteriors(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                           const double* const* Bs, const void* sym, const int64_t* offs, int S, double ln_switch,
                                           double* post, double* log_prob, int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_segment_posteriors";
    if (K < 1) return e2vq_set_error("%s: %d models (at least 1)", who, K);
    if (!Ns || !pis || !As || !Bs || S < 0 || (!sym && S > 0 && offs && offs[S] > 0)) return e2vq_set_error("%s: bad arguments", who);
    if (segment_check_shape(who, K, Ns) || segment_check_switch(who, ln_switch) || posteriors_check_slots(who, K, Ns)) return 1;
    std::vector<Hmm> models;
    std::vector<const Hmm*> ms;
    if (models_from_arrays(K, Ns, M, pis, As, Bs, models, ms)) return 1;
    for (const Hmm& h : models)
        if (posteriors_check_params(h)) return 1;
    if (check_offsets(offs, S) || require_device(device)) return 1;
    DevSeqs seqs;
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0)) return 1;
    PostOut out;
    out.post = post, out.log_prob = log_prob, out.status = status;
    return posteriors_device(ms, seqs.sym, (const i64*)offs, S, ln_switch, seqs.st.s, out);
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
                         W_ms, O_ms, ln_switch, csv_dir_or_file, true, frames_dir && *frames_dir ? frames_dir : nullptr);
}

// ---- hmm segment --class-transitions ----------------------------------------------------------------------
namespace {

thread_local float g_segment_trans_kernel_ms = -1.f;  // e2vq_hmm_segment_trans_last_kernel_ms

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

// only the resident layout exists: a packing of more than SEG_MAX_WAVES slots is refused (host only)
int trans_check_slots(const char* who, int K, const int* Ns)
{
    const int slots = pack_slots(std::vector<int>(Ns, Ns + K), [](int N) { return N; }).slots;
    if (slots > e2hmm::SEG_MAX_WAVES)
        return e2vq_set_error("%s: the classes take %d wave-slots of 64 lanes (at most %d: the class-transition decoder has no looped body)",
                              who, slots, e2hmm::SEG_MAX_WAVES);
    return 0;
}

// segment_device under the K x K prices lt (row: the class left); out.gbest receives exit_score.  Already checked:
// segment_check_shape, trans_check_slots, trans_check_lt.
int segment_trans_device(const std::vector<const Hmm*>& ms, const std::vector<std::vector<double>>& lflats, const unsigned short* d_sym,
                         const i64* h_offs, int S, const double* lt, hipStream_t st, const SegOut& out)
{
    const int K = (int)ms.size(), M = ms[0]->M;
    std::vector<int> Ns;
    for (const Hmm* h : ms) Ns.push_back(h->N);
    const SegPacking pk = pack_slots(Ns, [](int N) { return N; });
    const int sumN = pk.sumN, a_words = pk.a_words, slots = pk.slots;
    // logarithms: lpi of every class | lA of every class | lB of every class
    std::vector<double> params((size_t)sumN + (size_t)a_words + (size_t)sumN * M);
    for (int k = 0; k < K; ++k) {
        const std::vector<double>& lflat = lflats[(size_t)k];
        const size_t N = (size_t)ms[(size_t)k]->N;
        std::copy(lflat.begin(), lflat.begin() + N, params.begin() + pk.comp0[(size_t)k]);
        std::copy(lflat.begin() + N, lflat.begin() + N + N * N, params.begin() + sumN + pk.a_at[(size_t)k]);
        std::copy(lflat.begin() + N + N * N, lflat.end(), params.begin() + sumN + a_words + (size_t)pk.comp0[(size_t)k] * M);
    }
    std::vector<double> ltT((size_t)K * K);  // a lane of class k walks its sources along consecutive words
    for (int f = 0; f < K; ++f)
        for (int k = 0; k < K; ++k) ltT[(size_t)k * K + f] = lt[(size_t)f * K + k];

    DeviceBuffer<double> d_params, d_ltT, d_logp, d_exit, d_Es;
    DeviceBuffer<e2hmm::SegLaneDev> d_lanes;
    DeviceBuffer<int> d_info, d_comp0, d_status, d_qlast;
    DeviceBuffer<unsigned short> d_comp_cls, d_psi, d_src, d_xs, d_cls, d_state;
    DeviceBuffer<unsigned char> d_entered;
    DeviceBuffer<i64> d_offs;
    const i64 frames = h_offs[S];
    if (d_params.upload(params.data(), params.size(), st) || d_ltT.upload(ltT.data(), ltT.size(), st) ||
        d_lanes.upload(pk.lanes.data(), pk.lanes.size(), st) || d_info.upload(pk.slot_info.data(), pk.slot_info.size(), st) ||
        d_comp0.upload(pk.comp0.data(), pk.comp0.size(), st) || d_comp_cls.upload(pk.comp_cls.data(), pk.comp_cls.size(), st) ||
        d_offs.upload(h_offs, (size_t)S + 1, st) || d_logp.reserve((size_t)S) || d_status.reserve((size_t)S) ||
        d_qlast.reserve((size_t)S) || d_exit.reserve((size_t)frames) || d_cls.reserve((size_t)frames) ||
        d_state.reserve((size_t)frames) || d_entered.reserve((size_t)frames))
        return 1;
    const e2hmm::SegPlanDev pl{K, M, sumN, slots, a_words, d_lanes.get(), d_info.get(), d_params.get(), d_comp_cls.get(), d_comp0.get()};
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
    KernelTimer timer;
    if (timer.create()) return 1;
    HIPCHK(hipEventRecord(timer.start.e, st));
    // (one stream: a chunk's forward pass writes the tables only after the previous chunk's backtrack has read them)
    for (const auto& c : chunks) {
        const int s0 = c.first, n = c.second - c.first;
        if (e2hmm::launch_segment_trans(pl, d_sym, d_offs.get() + s0, n, h_offs[s0], d_ltT.get(), d_psi.get(), d_src.get(), d_xs.get(),
                                        d_Es.get(), d_logp.get() + s0, d_qlast.get() + s0, d_status.get() + s0, st))
            return e2vq_set_error("hmm segment --class-transitions: %d wave-slots of %d states cannot be launched", slots, sumN);
        HIPCHK(hipGetLastError());
        e2hmm::launch_segment_trans_backtrack(pl, d_offs.get() + s0, n, h_offs[s0], d_psi.get(), d_src.get(), d_xs.get(), d_Es.get(),
                                              d_qlast.get() + s0, d_status.get() + s0, d_cls.get(), d_state.get(), d_entered.get(),
                                              d_exit.get(), st);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(timer.stop.e, st));
    if (frames > 0) {
        if (out.cls) HIPCHK(hipMemcpyAsync(out.cls, d_cls.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
        if (out.state) HIPCHK(hipMemcpyAsync(out.state, d_state.get(), (size_t)frames * 2, hipMemcpyDeviceToHost, st));
        if (out.entered) HIPCHK(hipMemcpyAsync(out.entered, d_entered.get(), (size_t)frames, hipMemcpyDeviceToHost, st));
        if (out.gbest) HIPCHK(hipMemcpyAsync(out.gbest, d_exit.get(), (size_t)frames * 8, hipMemcpyDeviceToHost, st));
    }
    if (S > 0) {
        if (out.log_prob) HIPCHK(hipMemcpyAsync(out.log_prob, d_logp.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        if (out.status) HIPCHK(hipMemcpyAsync(out.status, d_status.get(), (size_t)S * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // (the one synchronisation; the host tables above are locals)
    if (timer.elapsed_ms(&g_segment_trans_kernel_ms)) return 1;
    return 0;
}

// ---- the transitions file: "class,<name_1>,...,<name_K>", then one line "<from>,v_1,...,v_K" per class ------------------
std::vector<std::string> split_on(const std::string& s, char sep)
{
    std::vector<std::string> out(1);
    for (char ch : s) {
        if (ch == sep) out.emplace_back();
        else out.back() += ch;
    }
    return out;
}

// the lines of a text file without their line ends; a last line without one counts, trailing empty lines do not
int read_lines(const char* path, std::vector<std::string>& lines)
{
    std::vector<unsigned char> bytes;
    if (read_file(path, bytes)) return 1;
    lines = split_on(std::string(bytes.begin(), bytes.end()), '\n');
    for (std::string& l : lines)
        if (!l.empty() && l.back() == '\r') l.pop_back();
    while (!lines.empty() && lines.back().empty()) lines.pop_back();
    return 0;
}

// the file's matrix in the order of `names` (the models' classes): lt[f * K + k], each value <= 0 or -inf
int transitions_read(const char* path, int K, const char* const* names, std::vector<double>& lt)
{
    std::vector<std::string> lines;
    if (read_lines(path, lines)) return 1;
    if (lines.empty()) return e2vq_set_error("%s: empty: no header 'class,<name>,...'", path);
    auto index_of = [&](const std::string& name) {
        for (int k = 0; k < K; ++k)
            if (name == names[k]) return k;
        return -1;
    };
    const std::vector<std::string> head = split_on(lines[0], ',');
    if (head[0] != "class") return e2vq_set_error("%s:1: the header starts with '%s', not 'class'", path, head[0].c_str());
    if ((int)head.size() != K + 1) return e2vq_set_error("%s:1: %zu class names for %d models", path, head.size() - 1, K);
    std::vector<int> col((size_t)K), seen_col((size_t)K, 0), seen_row((size_t)K, 0);
    for (int c = 0; c < K; ++c) {
        const int k = index_of(head[(size_t)c + 1]);
        if (k < 0) return e2vq_set_error("%s:1: '%s' is no model's class", path, head[(size_t)c + 1].c_str());
        if (seen_col[(size_t)k]++) return e2vq_set_error("%s:1: class '%s' is named twice", path, names[k]);
        col[(size_t)c] = k;
    }
    if ((int)lines.size() != K + 1) return e2vq_set_error("%s:%zu: %zu rows for %d models", path, lines.size(), lines.size() - 1, K);
    lt.assign((size_t)K * K, 0.0);
    for (int r = 0; r < K; ++r) {
        const int line = r + 2;
        const std::vector<std::string> cells = split_on(lines[(size_t)r + 1], ',');
        if ((int)cells.size() != K + 1) return e2vq_set_error("%s:%d: %zu fields, not %d", path, line, cells.size(), K + 1);
        const int f = index_of(cells[0]);
        if (f < 0) return e2vq_set_error("%s:%d: '%s' is no model's class", path, line, cells[0].c_str());
        if (seen_row[(size_t)f]++) return e2vq_set_error("%s:%d: class '%s' has a second row", path, line, names[f]);
        for (int c = 0; c < K; ++c) {
            const std::string& cell = cells[(size_t)c + 1];
            char* end = nullptr;
            const double v = strtod(cell.c_str(), &end);
            if (cell.empty() || *end) return e2vq_set_error("%s:%d: '%s' is not a number", path, line, cell.c_str());
            if (std::isnan(v) || v > 0.0)
                return e2vq_set_error("%s:%d: %s -> %s = %g: the logarithm of a price, at most 0 or -inf", path, line, names[f],
                                      names[col[(size_t)c]], v);
            lt[(size_t)f * K + col[(size_t)c]] = v;
        }
    }
    return 0;
}

int transitions_write(const char* path, int K, const char* const* names, const double* lt)
{
    std::string doc = "class";
    for (int k = 0; k < K; ++k) doc += std::string(",") + names[k];
    doc += "\n";
    for (int f = 0; f < K; ++f) {
        doc += names[f];
        for (int k = 0; k < K; ++k) doc += "," + fmt_17g(lt[(size_t)f * K + k]);
        doc += "\n";
    }
    return write_file(path, std::vector<unsigned char>(doc.begin(), doc.end()));
}

int check_names(const char* who, int K, const char* const* names)
{
    if (K < 1 || !names) return e2vq_set_error("%s: bad arguments", who);
    for (int k = 0; k < K; ++k) {
        if (!names[k] || !*names[k] || strpbrk(names[k], ",\t\r\n")) return e2vq_set_error("%s: class name %d cannot head a column", who, k);
        for (int g = 0; g < k; ++g)
            if (strcmp(names[g], names[k]) == 0) return e2vq_set_error("%s: two models of the class '%s'", who, names[k]);
    }
    return 0;
}

// ln((c[f][k] + alpha) / (sum_k' c[f][k'] + alpha K)) from the bigram counts c (K x K)
int transitions_from_counts(const char* who, int K, const std::vector<int64_t>& c, double alpha, const char* const* names, double* lt)
{
    if (!(alpha >= 0.0) || !std::isfinite(alpha)) return e2vq_set_error("%s: alpha = %g: a finite number, at least 0", who, alpha);
    for (int f = 0; f < K; ++f) {
        int64_t n = 0;
        for (int k = 0; k < K; ++k) n += c[(size_t)f * K + k];
        const double den = (double)n + alpha * (double)K;
        if (!(den > 0.0)) {
            if (names) return e2vq_set_error("%s: nothing follows class '%s' in the inputs: its row is undefined at alpha = 0", who, names[f]);
            return e2vq_set_error("%s: nothing follows class %d in the inputs: its row is undefined at alpha = 0", who, f);
        }
        for (int k = 0; k < K; ++k) {
            const double num = (double)c[(size_t)f * K + k] + alpha;
            lt[(size_t)f * K + k] = num > 0.0 ? log(num / den) : -INFINITY;
        }
    }
    return 0;
}

}  // namespace

// the labelled units of one file in their order (hmm_host.h): what `hmm transitions` counts and `hmm align` aligns to
int e2hmm_host::read_label_file(const char* path, std::vector<LabelRow>& rows)
{
    std::vector<std::string> lines;
    if (read_lines(path, lines)) return 1;
    // the first line that is no '#' comment is the header: a segment CSV (column `class`) or a tab-separated selection table
    size_t h = 0;
    while (h < lines.size() && (lines[h].empty() || lines[h][0] == '#')) ++h;
    if (h == lines.size()) return e2vq_set_error("%s: no header", path);
    const bool table = lines[h].find('\t') != std::string::npos;
    const std::vector<std::string> head = split_on(lines[h], table ? '\t' : ',');
    auto column = [&](const char* name) { return (int)(std::find(head.begin(), head.end(), name) - head.begin()); };
    const int ncol = (int)head.size();
    const int c_label = column(table ? "Type" : "class"), c_time = table ? column("Begin Time (s)") : -1;
    if (c_label == ncol || c_time == ncol)
        return e2vq_set_error("%s:%zu: neither a segment CSV (column 'class') nor a selection table (tab-separated, 'Begin Time (s)' and 'Type')",
                              path, h + 1);
    std::vector<std::pair<double, LabelRow>> timed;  // (begin time or row number, label)
    for (size_t l = h + 1; l < lines.size(); ++l) {
        if (lines[l].empty() || lines[l][0] == '#') continue;
        const std::vector<std::string> cells = split_on(lines[l], table ? '\t' : ',');
        if ((int)cells.size() != ncol) return e2vq_set_error("%s:%zu: %zu fields, not %d", path, l + 1, cells.size(), ncol);
        double at = (double)timed.size();
        if (table) {
            char* end = nullptr;
            at = strtod(cells[(size_t)c_time].c_str(), &end);
            if (cells[(size_t)c_time].empty() || *end || std::isnan(at))
                return e2vq_set_error("%s:%zu: begin time '%s' is not a number", path, l + 1, cells[(size_t)c_time].c_str());
        }
        timed.emplace_back(at, LabelRow{cells[(size_t)c_label], l + 1});
    }
    std::stable_sort(timed.begin(), timed.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    rows.clear();
    for (auto& r : timed) rows.push_back(std::move(r.second));
    return 0;
}

extern "C" int e2vq_hmm_segment_trans_last_kernel_ms(float* ms)
{
    if (!ms) return e2vq_set_error("e2vq_hmm_segment_trans_last_kernel_ms: bad arguments");
    *ms = g_segment_trans_kernel_ms;
    return 0;
}

extern "C" int e2vq_hmm_segment_trans(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                                      const double* const* Bs, const void* sym, const int64_t* offs, int S, const double* lt,
                                      uint16_t* cls, uint16_t* state, uint8_t* entered, double* exit_score, double* log_prob,
                                      int* status, int sym_on_device)
{
    const char* who = "e2vq_hmm_segment_trans";
    if (K < 1) return e2vq_set_error("%s: %d models (at least 1)", who, K);
    if (!Ns || !pis || !As || !Bs || !lt || S < 0 || (!sym && S > 0 && offs && offs[S] > 0)) return e2vq_set_error("%s: bad arguments", who);
    if (segment_check_shape(who, K, Ns) || trans_check_lt(who, K, lt) || trans_check_slots(who, K, Ns)) return 1;
    std::vector<Hmm> models;
    std::vector<const Hmm*> ms;
    std::vector<std::vector<double>> lflats((size_t)K);
    if (models_from_arrays(K, Ns, M, pis, As, Bs, models, ms)) return 1;
    for (int k = 0; k < K; ++k)
        if (log_model(models[(size_t)k], lflats[(size_t)k])) return 1;
    if (check_offsets(offs, S) || require_device(device)) return 1;
    DevSeqs seqs;
    if (seqs.symbols(sym, (size_t)offs[S], sym_on_device != 0)) return 1;
    SegOut out;
    out.cls = cls, out.state = state, out.entered = entered, out.gbest = exit_score, out.log_prob = log_prob, out.status = status;
    return segment_trans_device(ms, lflats, seqs.sym, (const i64*)offs, S, lt, seqs.st.s, out);
}

extern "C" int e2vq_hmm_segment_trans_report(const char* name, int64_t T, int K, const char* const* class_names, int W_ms, int O_ms,
                                             const uint16_t* cls, const uint8_t* entered, const double* exit_score, double log_prob,
                                             double ln_switch, const double* lt, const char* csv_filename)
{
    if (!lt) return e2vq_set_error("e2vq_hmm_segment_trans_report: bad arguments");
    return segment_report("e2vq_hmm_segment_trans_report", name, T, K, class_names, W_ms, O_ms, cls, entered, exit_score, log_prob,
                          ln_switch, nullptr, csv_filename, nullptr, lt);
}

extern "C" int e2vq_hmm_transitions_read(const char* filename, int K, const char* const* class_names, double* lt)
{
    if (!filename || !lt) return e2vq_set_error("e2vq_hmm_transitions_read: bad arguments");
    if (check_names("e2vq_hmm_transitions_read", K, class_names)) return 1;
    std::vector<double> m;
    if (transitions_read(filename, K, class_names, m)) return 1;
    std::copy(m.begin(), m.end(), lt);
    return 0;
}

extern "C" int e2vq_hmm_transitions_write(const char* filename, int K, const char* const* class_names, const double* lt)
{
    if (!filename || !lt) return e2vq_set_error("e2vq_hmm_transitions_write: bad arguments");
    if (check_names("e2vq_hmm_transitions_write", K, class_names)) return 1;
    return transitions_write(filename, K, class_names, lt);
}

extern "C" int e2vq_hmm_segment_trans_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                            const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                            double ln_switch, const char* transitions_csv, const char* csv_dir_or_file)
{
    const char* who = "e2vq_hmm_segment_trans_files";
    FlushStdout flush_on_return;
    if (!model_filenames || num_models < 1) return e2vq_set_error("%s: no models", who);
    if (!input_filenames || num_inputs < 1) return e2vq_set_error("%s: no inputs", who);
    if (!transitions_csv || !*transitions_csv) return e2vq_set_error("%s: no class-transitions file", who);
    if (segment_check_switch(who, ln_switch)) return 1;
    if (W_ms < 1 || O_ms < 1) return e2vq_set_error("%s: window %d ms / offset %d ms", who, W_ms, O_ms);
    FilesModels fm;
    if (fm.load(model_filenames, num_models)) return 1;
    const int K = (int)num_models;
    std::vector<int> Ns;
    for (const Hmm& h : fm.models) Ns.push_back(h.N);
    if (segment_check_shape(who, K, Ns.data()) || trans_check_slots(who, K, Ns.data())) return 1;
    if (check_names(who, K, fm.names.data())) return 1;
    std::vector<double> lt;
    if (transitions_read(transitions_csv, K, fm.names.data(), lt)) return 1;
    for (double& v : lt) v = v + ln_switch;  // the effective price
    std::vector<std::vector<double>> lflats((size_t)num_models);
    for (unsigned k = 0; k < num_models; ++k)
        if (log_model(fm.models[k], lflats[k])) return e2vq_set_error("%s: %s", model_filenames[k], std::string(e2vq_last_error()).c_str());
    auto run = [&](const SymInput& in, int64_t T, const unsigned short* d_sym, hipStream_t st) -> int {
        const i64 offs[2] = {0, T};
        const size_t n = (size_t)std::max<int64_t>(T, 1);
        std::vector<uint16_t> cls(n);
        std::vector<uint8_t> entered(n);
        std::vector<double> exit_score(n);
        double lp = 0.0;
        int status = 0;
        SegOut out;
        out.cls = cls.data(), out.entered = entered.data(), out.gbest = exit_score.data(), out.log_prob = &lp, out.status = &status;
        if (segment_trans_device(fm.ms, lflats, d_sym, offs, 1, lt.data(), st, out)) return 1;
        if (status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d", in.path.c_str(), fm.M);
        return segment_report(who, in.path.c_str(), T, K, fm.names.data(), W_ms, O_ms, cls.data(), entered.data(), exit_score.data(), lp,
                              ln_switch, nullptr, in.csv.empty() ? nullptr : in.csv.c_str(), nullptr, lt.data());
    };
    return run_on_files(who, fm.M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, run);
}

// ---- hmm transitions: the matrix from labelled successions (host only) ---------------------------------------------------
extern "C" int e2vq_hmm_class_transitions(const int32_t* labels, const int64_t* offs, int S, int K, double alpha, double* lt)
{
    const char* who = "e2vq_hmm_class_transitions";
    if (K < 1 || S < 0 || !offs || !lt || (S > 0 && offs[S] > 0 && !labels)) return e2vq_set_error("%s: bad arguments", who);
    if (check_offsets(offs, S)) return 1;
    std::vector<int64_t> c((size_t)K * K, 0);
    for (int s = 0; s < S; ++s)
        for (int64_t t = offs[s]; t < offs[s + 1]; ++t) {
            if (labels[t] < 0 || labels[t] >= K) return e2vq_set_error("%s: label %d at %lld is outside [0, %d)", who, labels[t], (long long)t, K);
            if (t > offs[s]) ++c[(size_t)labels[t - 1] * K + labels[t]];
        }
    return transitions_from_counts(who, K, c, alpha, nullptr, lt);
}

extern "C" int e2vq_hmm_transitions_files(const char* const* model_filenames, unsigned num_models, const char* const* input_filenames,
                                          int num_inputs, double alpha, const char* out_csv)
{
    const char* who = "e2vq_hmm_transitions_files";
    FlushStdout flush_on_return;
    if (!model_filenames || num_models < 1) return e2vq_set_error("%s: no models", who);
    if (!input_filenames || num_inputs < 1) return e2vq_set_error("%s: no inputs", who);
    if (!out_csv || !*out_csv) return e2vq_set_error("%s: no output file", who);
    std::vector<std::string> names;
    for (unsigned k = 0; k < num_models; ++k) {
        char cls[96];
        int N, M;
        if (e2vq_hmm_info(model_filenames[k], cls, &N, &M)) return 1;
        names.push_back(cls);
    }
    const int K = (int)num_models;
    std::vector<const char*> pn;
    for (const std::string& s : names) pn.push_back(s.c_str());
    if (check_names(who, K, pn.data())) return 1;
    std::vector<int64_t> c((size_t)K * K, 0);
    int64_t pairs = 0, skipped = 0;
    for (int i = 0; i < num_inputs; ++i) {
        const char* path = input_filenames[i];
        if (!path) return e2vq_set_error("%s: NULL file name", who);
        std::vector<LabelRow> rows;
        if (read_label_file(path, rows)) return 1;
        int prev = -1;  // (a label that is no model's class is left out: its neighbours follow one another)
        for (const auto& r : rows) {
            int k = 0;
            while (k < K && r.label != names[(size_t)k]) ++k;
            if (k == K) {
                ++skipped;
                continue;
            }
            if (prev >= 0) {
                ++c[(size_t)prev * K + k];
                ++pairs;
            }
            prev = k;
        }
    }
    std::vector<double> lt((size_t)K * K);
    if (transitions_from_counts(who, K, c, alpha, pn.data(), lt.data())) return 1;
    if (transitions_write(out_csv, K, pn.data(), lt.data())) return 1;
    printf("%d inputs: %lld successions counted, %lld labels skipped (no model's class)\n", num_inputs, (long long)pairs, (long long)skipped);
    printf("%s saved (alpha %g, %d classes)\n", out_csv, alpha, K);
    return 0;
}
