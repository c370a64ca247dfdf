// hmm_host.cpp -- host side of the HMM consumers of the VQ path: the reference's FFI symbols
// ecoz2_set_random_seed / ecoz2_hmm_learn / ecoz2_hmm_classify / ecoz2_hmm_classify_predictors / ecoz2_hmm_show
// (/root/reference/src/ecoz2_lib/mod.rs:75,134-167) over the kernels of hmm_device.hip.  The host loads files,
// draws the initial model, sequences the launches, takes the logarithm of the (mantissa, exponent) pairs the
// kernels return and the stopping decision, and prints the report; every sum over states, time or sequences that
// defines a model or a score runs on the GPU (no CPU fallback: without a HIP device the entry points fail).
// Definitions (file layout, generator, scaled Baum-Welch with exact fixed-point sums, stopping rule): this repo's
// own -- the reference's C bodies are absent -- written down in oracle/hmm_oracle.h and DESIGN.md.
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
#include <time.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>
#include <string>
#include <thread>
#include <vector>

using namespace e2hip;
using namespace e2host;
using e2hmm::ModelDev;
typedef long long i64;

namespace {

// ---- generator: ecoz2_set_random_seed (oracle: e2h_set_random_seed / splitmix64) ---------------------------
uint64_t g_rng = 0x9E3779B97F4A7C15ull;

uint64_t rng_next()
{
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- model ----------------------------------------------------------------------------------------------------
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
};

// uniform draws in (0, 1] divided by their sequential sum
void random_row(double* row, int n)
{
    double s = 0.0;
    for (int k = 0; k < n; ++k) {
        row[k] = (double)((rng_next() >> 11) + 1) * 0x1.0p-53;
        s = s + row[k];
    }
    for (int k = 0; k < n; ++k) row[k] = row[k] / s;
}

// model types of `hmm learn -t` (src/hmm/mod.rs:49-55): 0 random, 1 uniform, 2 cascade-2, 3 cascade-3 (random B)
int hmm_init(Hmm& h, int type)
{
    const int N = h.N, M = h.M;
    if (type == 0) {
        random_row(h.pi.data(), N);
        for (int i = 0; i < N; ++i) random_row(&h.A[(size_t)i * N], N);
        for (int j = 0; j < N; ++j) random_row(&h.B[(size_t)j * M], M);
    } else if (type == 1) {
        for (int i = 0; i < N; ++i) h.pi[i] = 1.0 / (double)N;
        for (int i = 0; i < N * N; ++i) h.A[i] = 1.0 / (double)N;
        for (size_t k = 0; k < (size_t)N * M; ++k) h.B[k] = 1.0 / (double)M;
    } else if (type == 2 || type == 3) {
        const int width = type == 2 ? 2 : 3;
        for (int i = 0; i < N; ++i) h.pi[i] = i == 0 ? 1.0 : 0.0;
        for (int i = 0; i < N; ++i) {
            const int reach = std::min(N - i, width);
            for (int j = 0; j < N; ++j) h.A[(size_t)i * N + j] = (j >= i && j < i + reach) ? 1.0 / (double)reach : 0.0;
        }
        for (int j = 0; j < N; ++j) random_row(&h.B[(size_t)j * M], M);
    } else {
        return e2vq_set_error("model type %d not in 0..3", type);
    }
    return 0;
}

// .hmm: 16-byte ident "<hmm>", 96-byte class name (src/utl/mod.rs:19-20), u32 N, u32 M, pi, A, B as LE f64
int hmm_save(const std::string& path, const Hmm& h)
{
    std::vector<unsigned char> b(16 + 96 + 8, 0);
    memcpy(b.data(), "<hmm>", 5);
    memcpy(b.data() + 16, h.class_name.data(), std::min<size_t>(h.class_name.size(), 95));
    for (int k = 0; k < 4; ++k) {
        b[112 + k] = (unsigned char)((uint32_t)h.N >> (8 * k));
        b[116 + k] = (unsigned char)((uint32_t)h.M >> (8 * k));
    }
    auto put = [&](const std::vector<double>& v) {
        const unsigned char* p = (const unsigned char*)v.data();
        b.insert(b.end(), p, p + v.size() * 8);  // little-endian host (as the other writers of this library)
    };
    put(h.pi);
    put(h.A);
    put(h.B);
    return write_file(path, b);
}

int hmm_load(const char* path, Hmm& h)
{
    std::vector<unsigned char> raw;
    if (read_file(path, raw)) return 1;
    if (raw.size() < 120 || strncmp((const char*)raw.data(), "<hmm>", 5) != 0) return e2vq_set_error("%s: Not an HMM model", path);
    char cls[97] = {0};
    memcpy(cls, raw.data() + 16, 96);
    h.class_name = cls;
    uint32_t n = 0, m = 0;
    for (int k = 0; k < 4; ++k) {
        n |= (uint32_t)raw[112 + k] << (8 * k);
        m |= (uint32_t)raw[116 + k] << (8 * k);
    }
    if (n < 1 || n > (uint32_t)e2hmm::MAX_N || m < 1 || m > 65536) return e2vq_set_error("%s: implausible N=%u M=%u", path, n, m);
    const size_t need = 120 + ((size_t)n + (size_t)n * n + (size_t)n * m) * 8;
    if (raw.size() != need) return e2vq_set_error("%s: %zu bytes, expected %zu for N=%u M=%u", path, raw.size(), need, n, m);
    h.resize((int)n, (int)m);
    const unsigned char* p = raw.data() + 120;
    memcpy(h.pi.data(), p, h.pi.size() * 8);
    memcpy(h.A.data(), p + h.pi.size() * 8, h.A.size() * 8);
    memcpy(h.B.data(), p + (h.pi.size() + h.A.size()) * 8, h.B.size() * 8);
    return 0;
}

// natural log of mant * 2^exp2 (oracle: e2h_log_prob)
double log_prob(double mant, i64 exp2)
{
    if (!(mant > 0.0)) return -INFINITY;
    return log(mant) + (double)exp2 * M_LN2;
}

// ---- sequences ---------------------------------------------------------------------------------------------------
struct SeqSet {
    std::vector<std::string> files, classes;
    std::vector<uint16_t> sym;  // concatenated
    std::vector<i64> offs;      // S + 1
    int M = -1;                 // codebook size (all equal, unless loaded with mixed_M)
    std::vector<int> Ms;        // each file's codebook size
    int S() const { return (int)files.size(); }
};

// mixed_M: files of different codebook sizes are accepted (ss.M is then the first file's)
int load_sequences(const char* const* files, unsigned n, SeqSet& ss, bool mixed_M = false)
{
    ss.offs.assign(1, 0);
    for (unsigned i = 0; i < n; ++i) {
        char cls[96];
        int M;
        int64_t T;
        if (e2vq_seq_info(files[i], cls, &M, &T)) return 1;
        if (ss.M < 0) ss.M = M;
        if (M != ss.M && !mixed_M)
            return e2vq_set_error("%s: codebook size %d differs from the first sequence's %d", files[i], M, ss.M);
        const size_t at = ss.sym.size();
        ss.sym.resize(at + (size_t)T);
        if (T > 0 && e2vq_seq_read(files[i], ss.sym.data() + at, T)) return 1;
        ss.files.push_back(files[i]);
        ss.classes.push_back(cls);
        ss.Ms.push_back(M);
        ss.offs.push_back((i64)ss.sym.size());
    }
    return 0;
}

// ---- device-side model set ----------------------------------------------------------------------------------------
struct DevModels {
    DeviceBuffer<double> params;   // all pi | A | B, model after model
    DeviceBuffer<ModelDev> table;
    std::vector<ModelDev> host;
    int maxN = 0;
    int upload(const std::vector<const Hmm*>& ms, hipStream_t st)
    {
        size_t total = 0;
        std::vector<size_t> at;
        for (const Hmm* h : ms) {
            at.push_back(total);
            total += h->params();
        }
        std::vector<double> flat(total);
        for (size_t k = 0; k < ms.size(); ++k) ms[k]->pack(flat.data() + at[k]);
        if (params.upload(flat.data(), flat.size(), st)) return 1;
        HIPCHK(hipStreamSynchronize(st));  // `flat` is a local
        host.clear();
        maxN = 0;
        for (size_t k = 0; k < ms.size(); ++k) {
            const double* base = params.get() + at[k];
            host.push_back(ModelDev{ms[k]->N, ms[k]->M, base, base + ms[k]->N, base + ms[k]->N + (size_t)ms[k]->N * ms[k]->N});
            maxN = std::max(maxN, ms[k]->N);
        }
        if (table.upload(host.data(), host.size(), st)) return 1;
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
};

// scores of S device-resident sequences under K models: log_probs[s * K + k] (natural log; -inf when the model cannot
// emit the sequence or a symbol is outside its alphabet)
int score_device(const std::vector<const Hmm*>& ms, const unsigned short* d_sym, const i64* d_offs, int S, hipStream_t st,
                 std::vector<double>& log_probs, std::vector<double>* mant_out = nullptr, std::vector<i64>* exp_out = nullptr,
                 std::vector<int>* status_out = nullptr)
{
    const int K = (int)ms.size();
    DevModels dm;
    if (dm.upload(ms, st)) return 1;
    DeviceBuffer<double> d_mant;
    DeviceBuffer<i64> d_exp;
    DeviceBuffer<int> d_st;
    const size_t n = (size_t)S * K;
    if (d_mant.reserve(n) || d_exp.reserve(n) || d_st.reserve(n)) return 1;
    e2hmm::launch_score(dm.table.get(), K, dm.maxN, d_sym, d_offs, S, d_mant.get(), d_exp.get(), d_st.get(), st);
    HIPCHK(hipGetLastError());
    std::vector<double> mant(n);
    std::vector<i64> ex(n);
    std::vector<int> stat(n);
    if (n) {
        HIPCHK(hipMemcpyAsync(mant.data(), d_mant.get(), n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ex.data(), d_exp.get(), n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stat.data(), d_st.get(), n * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    log_probs.resize(n);
    for (size_t i = 0; i < n; ++i) log_probs[i] = stat[i] == 0 ? log_prob(mant[i], ex[i]) : -INFINITY;
    if (mant_out) *mant_out = mant;
    if (exp_out) *exp_out = ex;
    if (status_out) *status_out = stat;
    return 0;
}

// ---- Baum-Welch driver over device-resident sequences -----------------------------------------------------------
struct Trainer {
    int N, M, S;
    i64 total;
    hipStream_t st;
    DeviceBuffer<double> d_params, d_alpha, d_c, d_mant;
    DeviceBuffer<i64> d_acc, d_exp, d_scratch;
    DeviceBuffer<int> d_status;
    std::vector<double> mant;
    std::vector<i64> ex;
    std::vector<int> stat;
    ModelDev md{};
    i64 W = 0;

    int setup(const Hmm& h, int S_, i64 total_, hipStream_t st_)
    {
        N = h.N; M = h.M; S = S_; total = total_; st = st_;
        W = e2hmm::acc_words(N, M);
        std::vector<double> flat(h.params());
        h.pack(flat.data());
        if (d_params.upload(flat.data(), flat.size(), st)) return 1;
        HIPCHK(hipStreamSynchronize(st));
        double* base = d_params.get();
        md = ModelDev{N, M, base, base + N, base + N + (size_t)N * N};
        if (d_alpha.reserve((size_t)total * N) || d_c.reserve((size_t)total) || d_acc.reserve((size_t)W) || d_mant.reserve((size_t)S) ||
            d_exp.reserve((size_t)S) || d_status.reserve((size_t)S))
            return 1;
        if (e2hmm::fb_scratch_words(N) > 0 && d_scratch.reserve((size_t)e2hmm::fb_scratch_words(N))) return 1;
        mant.resize((size_t)S);
        ex.resize((size_t)S);
        stat.resize((size_t)S);
        return 0;
    }
    // E-step, the device part: expected counts of this trainer's sequences into d_acc, P(O) of each into mant / ex / stat.
    // acc_out (optional): the count words copied to the host (several workers: summed there and handed back)
    int estep_counts(const unsigned short* d_sym, const i64* d_offs, std::vector<i64>* acc_out = nullptr)
    {
        HIPCHK(hipMemsetAsync(d_acc.get(), 0, (size_t)W * 8, st));
        e2hmm::launch_fb(md, d_sym, d_offs, S, d_alpha.get(), d_c.get(), d_acc.get(), d_mant.get(), d_exp.get(), d_status.get(), st, d_scratch.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(mant.data(), d_mant.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(ex.data(), d_exp.get(), (size_t)S * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stat.data(), d_status.get(), (size_t)S * 4, hipMemcpyDeviceToHost, st));
        if (acc_out) {
            acc_out->resize((size_t)W);
            HIPCHK(hipMemcpyAsync(acc_out->data(), d_acc.get(), (size_t)W * 8, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    int acc_upload(const std::vector<i64>& acc)
    {
        HIPCHK(hipMemcpyAsync(d_acc.get(), acc.data(), (size_t)W * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    // E-step: expected counts into d_acc; returns L = sequential sum of log P over the used sequences
    int estep(const unsigned short* d_sym, const i64* d_offs, double* L, i64* used, i64* skipped)
    {
        if (estep_counts(d_sym, d_offs)) return 1;
        double sum = 0.0;
        i64 u = 0;
        for (int s = 0; s < S; ++s)
            if (stat[(size_t)s] == 0) {
                sum = sum + log_prob(mant[(size_t)s], ex[(size_t)s]);
                ++u;
            }
        *L = sum;
        if (used) *used = u;
        if (skipped) *skipped = S - u;
        return 0;
    }
    int mstep(double epsilon)
    {
        double* base = d_params.get();
        e2hmm::launch_reestimate(N, M, d_acc.get(), epsilon, base, base + N, base + N + (size_t)N * N, st);
        HIPCHK(hipGetLastError());
        return 0;
    }
    int download(Hmm& h)
    {
        std::vector<double> flat(h.params());
        HIPCHK(hipMemcpyAsync(flat.data(), d_params.get(), flat.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        h.unpack(flat.data());
        return 0;
    }
};

// ---- Viterbi ---------------------------------------------------------------------------------------
// lpi | lA | lB: the C library's log of every parameter, log 0 = -inf.  A negative, NaN or infinite parameter is refused
// (no +inf can then enter a sum, so no NaN can arise on the device).
int log_model(const Hmm& h, std::vector<double>& flat)
{
    flat.clear();
    flat.reserve(h.pi.size() + h.A.size() + h.B.size());
    const std::vector<double>* parts[3] = {&h.pi, &h.A, &h.B};
    const char* names[3] = {"pi", "A", "B"};
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < parts[k]->size(); ++i) {
            const double x = (*parts[k])[i];
            if (!(x >= 0.0) || !std::isfinite(x))
                return e2vq_set_error("HMM parameter %s[%zu] = %g: not a finite non-negative number", names[k], i, x);
            flat.push_back(x == 0.0 ? -INFINITY : log(x));
        }
    return 0;
}

// psi bytes per launch: whole sequences up to ECOZ2_HMM_VITERBI_CHUNK_BYTES (default 256 MiB); a longer sequence alone
i64 viterbi_chunk_bytes()
{
    const char* v = getenv("ECOZ2_HMM_VITERBI_CHUNK_BYTES");
    const i64 b = v && *v ? atoll(v) : (i64)256 << 20;
    return std::max<i64>(b, 1);
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
        const i64 budget = viterbi_chunk_bytes(), row = 2 * (i64)N;
        std::vector<std::pair<int, int>> chunks;
        i64 max_syms = 0;
        for (int s0 = 0; s0 < S;) {
            int s1 = s0 + 1;
            while (s1 < S && (hoffs[s1 + 1] - hoffs[s0]) * row <= budget) ++s1;
            chunks.emplace_back(s0, s1);
            max_syms = std::max(max_syms, hoffs[s1] - hoffs[s0]);
            s0 = s1;
        }
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

// S + 1 offsets that start at 0 and never decrease (the kernels index the symbols with them)
int check_offsets(const int64_t* offs, int S)
{
    if (S < 0 || !offs) return e2vq_set_error("bad sequence count %d or offsets", S);
    if (offs[0] != 0) return e2vq_set_error("offs[0] = %lld, expected 0", (long long)offs[0]);
    for (int s = 0; s < S; ++s)
        if (offs[s + 1] < offs[s]) return e2vq_set_error("offs[%d] = %lld < offs[%d] = %lld", s + 1, (long long)offs[s + 1], s, (long long)offs[s]);
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

typedef void (*hmm_learn_callback_t)(char* variable, double value);
constexpr int MAX_ESTEPS = 1000;  // safety cap, same in the oracle (val_auto <= 0 with no iteration limit would never stop)

// the report line of one E-step of hmm learn
void print_iteration(int it, double L, i64 skipped)
{
    printf("  it=%d  sum log(P) = %.10g%s\n", it, L,
           skipped ? (" (" + std::to_string(skipped) + " sequence(s) the model cannot emit were skipped)").c_str() : "");
}

// the training loop of oracle/hmm_oracle.h (e2h_learn): returns the number of E-steps through *n_esteps
// The same loop with the sequences dealt to `workers` devices (independent sequences; the expected counts
// are exact int64 limb sums, so their sum over the workers -- taken on the host here: acc_words(N, M) words, 50 KB at
// N = 6, M = 1024 -- is the count of a single worker bit for bit).  Every worker then runs the M-step on the summed
// counts: identical parameters everywhere, no broadcast.  L is summed on the host over all sequences in sequence order.
int train_sharded(Hmm& h, const SeqSet& ss, double epsilon, double val_auto, int max_iterations,
                  hmm_learn_callback_t callback, std::vector<double>& hist, bool verbose, int workers)
{
    struct Worker {
        int device = 0;
        i64 s0 = 0, s1 = 0;
        DeviceBuffer<unsigned short> d_sym;
        DeviceBuffer<i64> d_offs;
        Trainer tr;
        std::vector<i64> acc;
        Stream st;  // (after the buffers: see Stream)
    };
    const int ndev = device_count();
    if (!ndev) return 1;
    std::vector<Worker> ws((size_t)workers);
    if (run_workers(workers, [&](int w) -> int {
            Worker& k = ws[(size_t)w];
            k.device = worker_device(env_device(), w, ndev);
            split_range(ss.S(), workers, w, &k.s0, &k.s1);
            if (require_device(k.device) || k.st.create()) return 1;
            const i64 a = ss.offs[(size_t)k.s0], b = ss.offs[(size_t)k.s1];
            std::vector<i64> offs;
            for (i64 i = k.s0; i <= k.s1; ++i) offs.push_back(ss.offs[(size_t)i] - a);
            if (k.d_sym.upload(ss.sym.data() + a, (size_t)(b - a), k.st.s) || k.d_offs.upload(offs.data(), offs.size(), k.st.s)) return 1;
            HIPCHK(hipStreamSynchronize(k.st.s));  // (`offs` is a local)
            return k.tr.setup(h, (int)(k.s1 - k.s0), b - a, k.st.s);
        }))
        return 1;
    static char var[] = "sum_log_prob";
    int it = 0;
    double Lprev = 0.0;
    hist.clear();
    std::vector<i64> total;
    for (;;) {
        if ((max_iterations >= 0 && it >= max_iterations) || it >= MAX_ESTEPS) break;
        if (run_workers(workers, [&](int w) -> int {
                Worker& k = ws[(size_t)w];
                HIPCHK(hipSetDevice(k.device));
                return k.tr.estep_counts(k.d_sym.get(), k.d_offs.get(), &k.acc);
            }))
            return 1;
        total.assign(ws[0].acc.size(), 0);
        double L = 0.0;
        i64 skipped = 0;
        for (const Worker& k : ws) {
            for (size_t i = 0; i < total.size(); ++i) total[i] = (i64)((unsigned long long)total[i] + (unsigned long long)k.acc[i]);
            for (int q = 0; q < k.s1 - k.s0; ++q) {
                if (k.tr.stat[(size_t)q] == 0)
                    L = L + log_prob(k.tr.mant[(size_t)q], k.tr.ex[(size_t)q]);
                else
                    ++skipped;
            }
        }
        hist.push_back(L);
        if (verbose) print_iteration(it, L, skipped);
        if (callback) callback(var, L);
        if (it > 0 && L - Lprev <= val_auto) {
            ++it;
            break;
        }
        if (run_workers(workers, [&](int w) -> int {
                Worker& k = ws[(size_t)w];
                HIPCHK(hipSetDevice(k.device));
                if (k.tr.acc_upload(total)) return 1;
                if (k.tr.mstep(epsilon)) return 1;
                HIPCHK(hipStreamSynchronize(k.st.s));
                return 0;
            }))
            return 1;
        Lprev = L;
        ++it;
    }
    HIPCHK(hipSetDevice(ws[0].device));
    return ws[0].tr.download(h);
}

int train(Hmm& h, const SeqSet& ss, double epsilon, double val_auto, int max_iterations, hmm_learn_callback_t callback,
          std::vector<double>& hist, bool verbose)
{
    const int workers = std::min(env_workers(), std::max(1, ss.S()));
    if (workers > 1) return train_sharded(h, ss, epsilon, val_auto, max_iterations, callback, hist, verbose, workers);
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<i64> d_offs;
    Trainer tr;
    Stream st;
    if (st.create()) return 1;
    if (d_sym.upload(ss.sym.data(), ss.sym.size(), st.s) || d_offs.upload(ss.offs.data(), ss.offs.size(), st.s)) return 1;
    if (tr.setup(h, ss.S(), (i64)ss.sym.size(), st.s)) return 1;
    static char var[] = "sum_log_prob";
    int it = 0;
    double Lprev = 0.0;
    hist.clear();
    for (;;) {
        if ((max_iterations >= 0 && it >= max_iterations) || it >= MAX_ESTEPS) break;
        double L;
        i64 used, skipped;
        if (tr.estep(d_sym.get(), d_offs.get(), &L, &used, &skipped)) return 1;
        hist.push_back(L);
        if (verbose) print_iteration(it, L, skipped);
        if (callback) callback(var, L);
        if (it > 0 && L - Lprev <= val_auto) {
            ++it;
            break;
        }
        if (tr.mstep(epsilon)) return 1;
        Lprev = L;
        ++it;
    }
    return tr.download(h);
}

std::string fmt_g(double v)
{
    char b[64];
    snprintf(b, sizeof b, "%g", v);
    return b;
}

// data/hmms/N<N>__M<M>_t<type>__a<val_auto>[_I<max_iterations>]/<class>.hmm (CHANGELOG.md:460) and the training measure per
// iteration beside it as <class>.csv (CHANGELOG.md:288 "generates csv with hmm training measure"); *path: the model's file
int save_learned(const Hmm& h, int model_type, double val_auto, int max_iterations, const std::vector<double>& hist,
                 std::string* path)
{
    std::string dir = std::string(out_root()) + "/data/hmms/N" + std::to_string(h.N) + "__M" + std::to_string(h.M) + "_t" +
                      std::to_string(model_type) + "__a" + fmt_g(val_auto);
    if (max_iterations >= 0) dir += "_I" + std::to_string(max_iterations);
    *path = dir + "/" + h.class_name + ".hmm";
    if (hmm_save(*path, h)) return 1;
    std::string csv = "# class=" + h.class_name + " N=" + std::to_string(h.N) + " M=" + std::to_string(h.M) + "\nI,sum_log_prob\n";
    for (size_t i = 0; i < hist.size(); ++i) {
        char b[64];
        snprintf(b, sizeof b, "%zu,%.17g\n", i, hist[i]);
        csv += b;
    }
    return write_file(dir + "/" + h.class_name + ".csv", std::vector<unsigned char>(csv.begin(), csv.end()));
}

// ECOZ2_HMM_LEARN_BATCH_BYTES: the budget of one training batch (default 4 GiB)
i64 learn_batch_bytes()
{
    const char* v = getenv("ECOZ2_HMM_LEARN_BATCH_BYTES");
    const i64 b = v && *v ? atoll(v) : (i64)4 << 30;
    return std::max<i64>(b, 1);
}

// ---- many models at once: a grid of (N, M) points, or every class of one (N, M) ------------------
// The sequences a batch's models train on: host symbols and S + 1 offsets from 0.  Each model trains on a range of them;
// the models of different N of one class and M share theirs, the classes of `--all-classes` have disjoint ones.
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
    BatchSeqs(std::vector<std::pair<int, int>> ranges, const SeqStore& ss) : offs(1, 0)
    {
        std::sort(ranges.begin(), ranges.end());
        for (const auto& r : ranges) {
            if (!merged.empty() && r.first <= merged.back().second)
                merged.back().second = std::max(merged.back().second, r.second);
            else
                merged.push_back(r);
        }
        for (const auto& r : merged) {
            run_at.push_back((int)offs.size() - 1);
            for (int s = r.first; s < r.second; ++s) offs.push_back(offs.back() + (ss.offs[s + 1] - ss.offs[s]));
        }
    }
    int local(int s) const  // batch index of the store's sequence s (one of a range given)
    {
        const auto it = std::upper_bound(merged.begin(), merged.end(), std::make_pair(s, INT32_MAX));
        const size_t q = (size_t)(it - merged.begin()) - 1;
        return run_at[q] + (s - merged[q].first);
    }
    // d_sym: offs.back() symbols.  A run goes up in pieces of 128 KB: the store is pageable caller memory, and a copy of
    // megabytes from it makes the runtime pin the pages first, at a cost that varies from call to call; pieces of this
    // size go through the runtime's staging buffer instead (docs/HISTORY.md, "one batched HMM trainer")
    int upload_symbols(const SeqStore& ss, unsigned short* d_sym, hipStream_t st) const
    {
        constexpr i64 PIECE = 65536;
        for (size_t q = 0; q < merged.size(); ++q) {
            const i64 a = ss.offs[merged[q].first], b = ss.offs[merged[q].second];
            for (i64 c = a; c < b; c += PIECE)
                HIPCHK(hipMemcpyAsync(d_sym + offs[(size_t)run_at[q]] + (c - a), ss.sym + c, (size_t)std::min(PIECE, b - c) * 2,
                                      hipMemcpyHostToDevice, st));
        }
        return 0;
    }
};

// One model of a grid, trained exactly as `train` trains it alone on the store's sequences [s_lo, s_hi)
struct GridJob {
    Hmm h;                     // in: the initial model; out: the trained one
    int s_lo = 0, s_hi = 0;    // its sequences (s_lo < s_hi)
    std::vector<double> hist;  // out: sum ln P per E-step
    std::vector<i64> skipped;  // out: sequences skipped per E-step
    int S() const { return s_hi - s_lo; }
};

i64 grid_T(const GridJob& j, const SeqStore& ss) { return ss.offs[j.s_hi] - ss.offs[j.s_lo]; }

// device bytes a model takes in a grid batch besides its symbols: alpha^ and c over its symbols, and its accumulators
i64 grid_model_bytes(const GridJob& j, const SeqStore& ss)
{
    return (grid_T(j, ss) * ((i64)j.h.N + 1) + e2hmm::acc_words(j.h.N, j.h.M)) * 8;
}

// K models of any (N, M) trained together on the current device.  The models' sequence ranges are merged into disjoint
// runs and uploaded once.  Per iteration: one memset of the accumulators, one k_hmm_fb_grid launch per distinct N <= 64
// and one launch_fb per active model above, one copy of the per-sequence P(O) of every model back, one sync, each model's
// L summed on the host in sequence order, and one M-step launch pair over the models that go on.  A model that stops
// leaves the launches; its parameters on the device are not touched again.
int train_grid_batch(GridJob* const* jobs, int K, const SeqStore& ss, double epsilon, double val_auto, int max_iterations)
{
    std::vector<std::pair<int, int>> ranges;
    for (int k = 0; k < K; ++k) ranges.emplace_back(jobs[k]->s_lo, jobs[k]->s_hi);
    const BatchSeqs seqs(std::move(ranges), ss);
    const std::vector<i64>& offs = seqs.offs;
    std::vector<e2hmm::GridModelDev> g((size_t)K);
    i64 n_alpha = 0, n_c = 0, n_acc = 0, n_par = 0;
    int n_res = 0, max_blocks = 0, big_N = 0;
    for (int k = 0; k < K; ++k) {
        const Hmm& h = jobs[k]->h;
        e2hmm::GridModelDev& m = g[(size_t)k];
        m.s_lo = seqs.local(jobs[k]->s_lo);
        m.s_hi = m.s_lo + jobs[k]->S();
        const i64 T = offs[(size_t)m.s_hi] - offs[(size_t)m.s_lo];
        m.alpha_at = n_alpha;
        n_alpha += T * h.N;
        m.c_at = n_c;
        n_c += T;
        m.res_at = n_res;
        n_res += jobs[k]->S();
        m.acc_at = n_acc;
        n_acc += e2hmm::acc_words(h.N, h.M);
        m.param_at = n_par;
        n_par += (i64)h.params();
        if (h.N <= e2hmm::WAVE_N)
            max_blocks += e2hmm::fb_class_workgroups(jobs[k]->S());
        else
            big_N = std::max(big_N, h.N);
    }
    std::vector<double> flat((size_t)n_par);
    for (int k = 0; k < K; ++k) jobs[k]->h.pack(flat.data() + g[(size_t)k].param_at);
    DeviceBuffer<double> d_params, d_alpha, d_c, d_mant;
    DeviceBuffer<i64> d_acc, d_exp, d_offs, d_scratch;
    DeviceBuffer<int> d_status, d_blocks, d_active;
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<e2hmm::GridModelDev> d_models;
    Stream st;  // (after the buffers: see Stream)
    if (st.create()) return 1;
    if (d_sym.reserve((size_t)offs.back()) || d_params.upload(flat.data(), flat.size(), st.s) ||
        d_offs.upload(offs.data(), offs.size(), st.s) || d_alpha.reserve((size_t)n_alpha) || d_c.reserve((size_t)n_c) ||
        d_acc.reserve((size_t)n_acc) || d_mant.reserve((size_t)n_res) || d_exp.reserve((size_t)n_res) ||
        d_status.reserve((size_t)n_res) || d_blocks.reserve((size_t)max_blocks * 3) || d_active.reserve((size_t)K))
        return 1;
    if (big_N && d_scratch.reserve((size_t)e2hmm::fb_scratch_words(big_N))) return 1;
    if (seqs.upload_symbols(ss, d_sym.get(), st.s)) return 1;
    for (int k = 0; k < K; ++k) {
        e2hmm::GridModelDev& m = g[(size_t)k];
        const double* q = d_params.get() + m.param_at;
        const int N = jobs[k]->h.N, M = jobs[k]->h.M;
        m.md = ModelDev{N, M, q, q + N, q + N + (size_t)N * N};
    }
    if (d_models.upload(g.data(), g.size(), st.s)) return 1;
    HIPCHK(hipStreamSynchronize(st.s));  // (`flat`, `offs`, `g` are locals; the copies are done)
    std::vector<double> mant((size_t)n_res);
    std::vector<i64> ex((size_t)n_res);
    std::vector<int> stat((size_t)n_res), blocks, estep_list, mstep_list;
    std::map<int, std::vector<int>> by_N;  // the active models of each N <= 64
    std::vector<char> active((size_t)K, 1);
    std::vector<double> Lprev((size_t)K, 0.0);
    for (int k = 0; k < K; ++k) {
        jobs[k]->hist.clear();
        jobs[k]->skipped.clear();
    }
    // (host vectors copied to the device below are rewritten only after the stream synchronisation that follows the copy)
    for (int it = 0;; ++it) {
        if ((max_iterations >= 0 && it >= max_iterations) || it >= MAX_ESTEPS) break;
        estep_list.clear();
        for (int k = 0; k < K; ++k)
            if (active[(size_t)k]) estep_list.push_back(k);
        if (estep_list.empty()) break;
        HIPCHK(hipMemsetAsync(d_acc.get(), 0, (size_t)n_acc * 8, st.s));
        by_N.clear();
        for (int k : estep_list)
            if (g[(size_t)k].md.N <= e2hmm::WAVE_N) by_N[g[(size_t)k].md.N].push_back(k);
        if (!by_N.empty()) {
            blocks.clear();
            for (const auto& kv : by_N)
                for (int k : kv.second) {
                    const int nb = e2hmm::fb_class_workgroups(jobs[k]->S());
                    for (int b = 0; b < nb; ++b) blocks.insert(blocks.end(), {k, b, nb});
                }
            HIPCHK(hipMemcpyAsync(d_blocks.get(), blocks.data(), blocks.size() * 4, hipMemcpyHostToDevice, st.s));
            int at = 0;  // one launch per N: each sized by its own LDS (4 N^2 words a workgroup)
            for (const auto& kv : by_N) {
                int nb = 0;
                for (int k : kv.second) nb += e2hmm::fb_class_workgroups(jobs[k]->S());
                e2hmm::launch_fb_grid(d_models.get(), kv.first, d_blocks.get() + 3 * at, nb, d_sym.get(), d_offs.get(), d_alpha.get(),
                                      d_c.get(), d_acc.get(), d_mant.get(), d_exp.get(), d_status.get(), st.s);
                HIPCHK(hipGetLastError());
                at += nb;
            }
        }
        for (int k : estep_list) {
            const e2hmm::GridModelDev& m = g[(size_t)k];
            if (m.md.N <= e2hmm::WAVE_N) continue;
            const i64 o = offs[(size_t)m.s_lo];
            e2hmm::launch_fb(m.md, d_sym.get(), d_offs.get() + m.s_lo, jobs[k]->S(), d_alpha.get() + (m.alpha_at - o * m.md.N),
                             d_c.get() + (m.c_at - o), d_acc.get() + m.acc_at, d_mant.get() + m.res_at, d_exp.get() + m.res_at,
                             d_status.get() + m.res_at, st.s, d_scratch.get());
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(mant.data(), d_mant.get(), (size_t)n_res * 8, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(ex.data(), d_exp.get(), (size_t)n_res * 8, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(stat.data(), d_status.get(), (size_t)n_res * 4, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipStreamSynchronize(st.s));
        mstep_list.clear();
        i64 max_P = 0;
        int max_N = 0;
        for (int k : estep_list) {
            const e2hmm::GridModelDev& m = g[(size_t)k];
            double L = 0.0;
            i64 skipped = 0;
            for (i64 r = m.res_at; r < m.res_at + jobs[k]->S(); ++r) {
                if (stat[(size_t)r] == 0)
                    L = L + log_prob(mant[(size_t)r], ex[(size_t)r]);
                else
                    ++skipped;
            }
            jobs[k]->hist.push_back(L);
            jobs[k]->skipped.push_back(skipped);
            if (it > 0 && L - Lprev[(size_t)k] <= val_auto) {
                active[(size_t)k] = 0;
            } else {
                mstep_list.push_back(k);
                Lprev[(size_t)k] = L;
                max_P = std::max(max_P, (i64)jobs[k]->h.params());
                max_N = std::max(max_N, m.md.N);
            }
        }
        if (!mstep_list.empty()) {
            HIPCHK(hipMemcpyAsync(d_active.get(), mstep_list.data(), mstep_list.size() * 4, hipMemcpyHostToDevice, st.s));
            e2hmm::launch_reestimate_grid(d_models.get(), d_active.get(), (int)mstep_list.size(), max_P, max_N, d_acc.get(), epsilon,
                                          d_params.get(), st.s);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipMemcpyAsync(flat.data(), d_params.get(), flat.size() * 8, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    for (int k = 0; k < K; ++k) jobs[k]->h.unpack(flat.data() + g[(size_t)k].param_at);
    return 0;
}

// every model of a grid: dealt to `workers` workers in contiguous ranges of the grid order balanced by grid_model_bytes,
// worker w on device (dev0 + w) % device count; each worker packs its models greedily, in order, into batches of at most
// learn_batch_bytes() (a larger model alone), counting a sequence range's symbols once per batch, and trains them one
// batch after the other.  Models are independent, so neither the dealing nor the batching changes a bit of any result.
int train_grid(std::vector<GridJob>& jobs, const SeqStore& ss, double epsilon, double val_auto, int max_iterations, int workers,
               int dev0)
{
    const int K = (int)jobs.size();
    workers = std::max(1, std::min(workers, K));
    const int ndev = device_count();
    if (!ndev) return 1;
    std::vector<i64> prefix(1, 0);
    for (const GridJob& j : jobs) prefix.push_back(prefix.back() + grid_model_bytes(j, ss));
    std::vector<int> bound((size_t)workers + 1, K);
    bound[0] = 0;
    for (int w = 1; w < workers; ++w) {
        int c = bound[(size_t)w - 1];
        while (c < K && prefix[(size_t)c] * workers < prefix[(size_t)K] * w) ++c;
        bound[(size_t)w] = c;
    }
    const i64 budget = learn_batch_bytes();
    return run_workers(workers, [&](int w) -> int {
        const int lo = bound[(size_t)w], hi = bound[(size_t)w + 1];
        if (lo >= hi) return 0;
        if (require_device(worker_device(dev0, w, ndev))) return 1;
        for (int c0 = lo; c0 < hi;) {
            std::vector<GridJob*> batch;
            std::vector<std::pair<int, int>> ranges;  // (the sequence ranges whose symbols the batch already counts)
            i64 bytes = 0;
            int c1 = c0;
            while (c1 < hi) {
                const GridJob& j = jobs[(size_t)c1];
                const bool seen = std::find(ranges.begin(), ranges.end(), std::make_pair(j.s_lo, j.s_hi)) != ranges.end();
                const i64 more = grid_model_bytes(j, ss) + (seen ? 0 : grid_T(j, ss) * 2);
                if (c1 > c0 && bytes + more > budget) break;
                bytes += more;
                if (!seen) ranges.emplace_back(j.s_lo, j.s_hi);
                batch.push_back(&jobs[(size_t)c1++]);
            }
            if (train_grid_batch(batch.data(), (int)batch.size(), ss, epsilon, val_auto, max_iterations)) return 1;
            c0 = c1;
        }
        return 0;
    });
}

// What `hmm learn --all-classes` and `hmm learn --grid` do once their checks have passed: one model per (N, M, class)
// -- the N of n_list in its order; the M of the sequences' headers, ascending; the classes present at that M in byte
// order of their names -- each trained on the files of its class and M in list order, all models in one batched
// training.  Every model starts from the generator state of entry (the draw a fresh seeded call would make; after the
// last model the generator is where that call leaves it) and gets byte for byte what ecoz2_hmm_learn writes and prints
// for its files alone; files are written only once every model has trained.
int learn_models(const SeqSet& ss, const std::vector<int>& n_list, int model_type, double hmm_epsilon, double val_auto,
                 int max_iterations, hmm_learn_callback_t callback)
{
    // (std::map: M ascending; std::string's order is the bytes', as strcmp's)
    std::map<int, std::map<std::string, std::vector<int>>> by_M;
    for (int i = 0; i < ss.S(); ++i) by_M[ss.Ms[(size_t)i]][ss.classes[(size_t)i]].push_back(i);
    // the store: each (M, class)'s symbols contiguous, in list order, groups in grid order
    struct Group {
        std::string name;
        int M, s_lo, s_hi;
        i64 max_T;
    };
    std::vector<uint16_t> sym;
    std::vector<i64> offs(1, 0);
    std::vector<Group> groups;
    for (const auto& mv : by_M)
        for (const auto& kv : mv.second) {
            Group gr{kv.first, mv.first, (int)offs.size() - 1, 0, 0};
            for (int i : kv.second) {
                const i64 a = ss.offs[(size_t)i], b = ss.offs[(size_t)i + 1];
                sym.insert(sym.end(), ss.sym.begin() + a, ss.sym.begin() + b);
                offs.push_back((i64)sym.size());
                gr.max_T = std::max(gr.max_T, b - a);
            }
            gr.s_hi = (int)offs.size() - 1;
            groups.push_back(gr);
        }
    std::vector<GridJob> jobs;
    std::vector<const Group*> job_group;
    const uint64_t rng0 = g_rng;
    for (int N : n_list)
        for (const Group& gr : groups) {
            GridJob j;
            j.h.class_name = gr.name;
            j.h.resize(N, gr.M);
            j.s_lo = gr.s_lo;
            j.s_hi = gr.s_hi;
            g_rng = rng0;
            if (hmm_init(j.h, model_type)) return 1;
            jobs.push_back(std::move(j));
            job_group.push_back(&gr);
        }
    SeqStore store;
    store.sym = sym.data();
    store.offs = offs.data();
    if (train_grid(jobs, store, hmm_epsilon, val_auto, max_iterations, env_workers(), env_device())) return 1;
    const bool verbose = getenv("ECOZ2_VQ_QUIET") == nullptr;
    static char var[] = "sum_log_prob";
    for (size_t k = 0; k < jobs.size(); ++k) {
        const GridJob& j = jobs[k];
        printf("\nHMM learn: class '%s'  N=%d M=%d type=%d  #sequences = %d  max_T=%lld\n", j.h.class_name.c_str(), j.h.N, j.h.M,
               model_type, j.S(), (long long)job_group[k]->max_T);
        printf("  epsilon=%g  val_auto=%g  max_iterations=%d\n", hmm_epsilon, val_auto, max_iterations);
        for (size_t i = 0; i < j.hist.size(); ++i) {
            if (verbose) print_iteration((int)i, j.hist[i], j.skipped[i]);
            if (callback) callback(var, j.hist[i]);
        }
        std::string path;
        if (save_learned(j.h, model_type, val_auto, max_iterations, j.hist, &path)) return 1;
        printf("%zu E-step(s); model saved: %s\n", j.hist.size(), path.c_str());
    }
    return 0;
}

// classification report shared by ecoz2_hmm_classify / ecoz2_hmm_classify_predictors
// what a report says in figures (hmm classify --grid sums them up): the cases that had a model of their class, and
// C12nResults::last_accuracy / last_avg_accuracy
struct ReportFigures {
    size_t classified = 0;
    float accuracy = 0.f, avg_accuracy = 0.f;
};

int classify_report(const std::vector<Hmm>& models, const std::vector<std::string>& case_files,
                    const std::vector<std::string>& case_classes, const std::vector<double>& log_probs, int M,
                    bool show_ranked, const char* c12n_filename, ReportFigures* figures = nullptr)
{
    const size_t K = models.size();
    std::vector<std::string> names;
    for (const Hmm& h : models) names.push_back(h.class_name);
    C12nResults c12n(names);
    std::string csv;
    size_t classified = 0;
    for (size_t s = 0; s < case_files.size(); ++s) {
        const auto it = std::find(names.begin(), names.end(), case_classes[s]);
        if (it == names.end()) continue;  // no model of that class
        const size_t class_id = (size_t)(it - names.begin());
        std::vector<double> probs(log_probs.begin() + (ptrdiff_t)(s * K), log_probs.begin() + (ptrdiff_t)((s + 1) * K));
        c12n.add_case(class_id, case_classes[s], probs, show_ranked,
                      [&] { return std::string("\n") + case_files[s] + ": '" + case_classes[s] + "'"; });
        // rank of the true class, from 1 (CHANGELOG.md:273-284)
        std::vector<std::pair<size_t, double>> ranked;
        for (size_t k = 0; k < K; ++k) ranked.emplace_back(k, probs[k]);
        std::stable_sort(ranked.begin(), ranked.end(), [](const auto& a, const auto& b) { return a.second < b.second; });
        size_t rank = 0;
        for (size_t i = 0; i < K; ++i)
            if (ranked[K - 1 - i].first == class_id) rank = i + 1;
        csv += case_files[s] + "," + case_classes[s] + "," + (rank == 1 ? "*" : "!") + "," + std::to_string(rank) + "\n";
        ++classified;
    }
    printf("\n");
    if (c12n.report_results(names, "", /*c_report=*/true)) return 1;
    if (figures) *figures = ReportFigures{classified, c12n.last_accuracy, c12n.last_avg_accuracy};
    if (c12n_filename && *c12n_filename) {
        std::string doc = "# num_models=" + std::to_string(K) + "  M=" + std::to_string(M) + "  num_seqs=" + std::to_string(classified) +
                          "\nseq_filename,seq_class_name,correct,rank\n" + csv;
        if (write_file(c12n_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
        printf("%s saved\n", c12n_filename);
    }
    return 0;
}

int load_models(const char* const* files, unsigned n, std::vector<Hmm>& models)
{
    models.resize(n);
    for (unsigned i = 0; i < n; ++i)
        if (hmm_load(files[i], models[i])) return 1;
    return 0;
}

// ---- scoring at every point of a grid at once -------------------------------------------------------------
// One model of a grid scoring: scored exactly as k_hmm_score scores it on the store's sequences [s_lo, s_hi); out[s - s_lo]
struct ScoreJob {
    const Hmm* h = nullptr;
    int s_lo = 0, s_hi = 0;
    double* log_prob = nullptr;  // ln P, -inf unless the status is 0
    double* mant = nullptr;      // (the three below may be null)
    int64_t* exp2 = nullptr;
    int* status = nullptr;
    int S() const { return s_hi - s_lo; }
};

// models to a wave: score_pack_width(N), the widths that measured faster than one model per wave (DESIGN.md 4.8.4's
// table).  ECOZ2_HMM_SCORE_PACK=0 scores one model per wave at every N, =1 packs floor(64 / N) at every N <= 32 (the
// benchmark's other arms; the bits are the same)
int score_pack_width_in_use(int N)
{
    const char* v = getenv("ECOZ2_HMM_SCORE_PACK");
    if (v && *v) return atoi(v) == 0 || N > 32 ? 1 : e2hmm::WAVE_N / N;
    return e2hmm::score_pack_width(N);
}

// K jobs of any (N, M) scored together on the current device.  The jobs' sequence ranges are merged into disjoint runs
// and uploaded once.  Consecutive jobs of one (N, M, range) form groups: for N <= 64 a group is cut into packs of
// score_pack_width_in_use(N) models, and all packs of one N go into one k_hmm_score_grid launch; a group of N > 64 goes
// through launch_score (k_hmm_score_wg).  Every launch is enqueued before the one copy back and synchronisation.
int score_grid_batch(const ScoreJob* jobs, int K, const SeqStore& ss)
{
    std::vector<std::pair<int, int>> ranges;
    for (int k = 0; k < K; ++k) ranges.emplace_back(jobs[k].s_lo, jobs[k].s_hi);
    const BatchSeqs seqs(std::move(ranges), ss);
    const std::vector<i64>& offs = seqs.offs;
    // parameters, model table, result slots
    std::vector<e2hmm::ScoreModelDev> table((size_t)K);
    std::vector<i64> param_at((size_t)K), res_at((size_t)K), res_stride((size_t)K, 1);
    i64 n_par = 0, n_res = 0;
    for (int k = 0; k < K; ++k) {
        param_at[(size_t)k] = n_par;
        n_par += (i64)jobs[k].h->params();
    }
    struct Big {  // a group of N > 64: the models [k0, k0 + count) through launch_score, results at [s * count + i]
        int k0, count, s_lo, S;
        i64 base;
    };
    std::vector<Big> bigs;
    std::vector<e2hmm::ScorePackDev> packs;
    std::map<int, std::vector<int>> blocks_by_N;  // N <= 64 -> (pack, workgroup) pairs
    std::map<int, int> width_of_N;
    for (int k0 = 0; k0 < K;) {
        const ScoreJob& a = jobs[k0];
        int k1 = k0 + 1;
        while (k1 < K && jobs[k1].h->N == a.h->N && jobs[k1].h->M == a.h->M && jobs[k1].s_lo == a.s_lo && jobs[k1].s_hi == a.s_hi) ++k1;
        const int N = a.h->N, S = a.S(), lo = seqs.local(a.s_lo);
        if (N > e2hmm::WAVE_N) {
            bigs.push_back(Big{k0, k1 - k0, lo, S, n_res});
            for (int k = k0; k < k1; ++k) {
                res_at[(size_t)k] = n_res + (k - k0);
                res_stride[(size_t)k] = k1 - k0;
            }
            n_res += (i64)S * (k1 - k0);
        } else {
            const int G = width_of_N.emplace(N, score_pack_width_in_use(N)).first->second;
            std::vector<int>& blocks = blocks_by_N[N];
            for (int p0 = k0; p0 < k1; p0 += G) {
                const int count = std::min(G, k1 - p0);
                for (int b = 0; b < e2hmm::score_grid_workgroups(S); ++b) blocks.insert(blocks.end(), {(int)packs.size(), b});
                packs.push_back(e2hmm::ScorePackDev{p0, count, lo, lo + S});
                for (int k = p0; k < p0 + count; ++k) {
                    res_at[(size_t)k] = n_res;
                    n_res += S;
                }
            }
        }
        k0 = k1;
    }
    std::vector<double> flat((size_t)n_par);
    for (int k = 0; k < K; ++k) jobs[k].h->pack(flat.data() + param_at[(size_t)k]);
    std::vector<int> blocks;
    for (const auto& kv : blocks_by_N) blocks.insert(blocks.end(), kv.second.begin(), kv.second.end());
    DeviceBuffer<double> d_params, d_mant;
    DeviceBuffer<i64> d_exp, d_offs;
    DeviceBuffer<int> d_status, d_blocks;
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<e2hmm::ScoreModelDev> d_table;
    DeviceBuffer<e2hmm::ScorePackDev> d_packs;
    DeviceBuffer<ModelDev> d_big;
    Stream st;  // (after the buffers: see Stream)
    if (st.create()) return 1;
    if (d_sym.reserve((size_t)offs.back()) || d_params.upload(flat.data(), flat.size(), st.s) || d_offs.upload(offs.data(), offs.size(), st.s) ||
        d_mant.reserve((size_t)n_res) || d_exp.reserve((size_t)n_res) || d_status.reserve((size_t)n_res) ||
        d_blocks.upload(blocks.data(), blocks.size(), st.s) || d_packs.upload(packs.data(), packs.size(), st.s))
        return 1;
    if (seqs.upload_symbols(ss, d_sym.get(), st.s)) return 1;
    std::vector<ModelDev> big_table;
    for (int k = 0; k < K; ++k) {
        const double* q = d_params.get() + param_at[(size_t)k];
        const int N = jobs[k].h->N, M = jobs[k].h->M;
        table[(size_t)k] = e2hmm::ScoreModelDev{ModelDev{N, M, q, q + N, q + N + (size_t)N * N}, res_at[(size_t)k]};
        big_table.push_back(table[(size_t)k].md);
    }
    if (d_table.upload(table.data(), table.size(), st.s)) return 1;
    if (!bigs.empty() && d_big.upload(big_table.data(), big_table.size(), st.s)) return 1;
    int at = 0;  // one launch per N: each sized by its own LDS (N^2 G doubles a workgroup)
    for (const auto& kv : blocks_by_N) {
        const int nb = (int)(kv.second.size() / 2);
        e2hmm::launch_score_grid(d_table.get(), d_packs.get(), kv.first, width_of_N[kv.first], d_blocks.get() + 2 * at, nb, d_sym.get(),
                                 d_offs.get(), d_mant.get(), d_exp.get(), d_status.get(), st.s);
        HIPCHK(hipGetLastError());
        at += nb;
    }
    for (const Big& g : bigs) {
        e2hmm::launch_score(d_big.get() + g.k0, g.count, jobs[g.k0].h->N, d_sym.get(), d_offs.get() + g.s_lo, g.S, d_mant.get() + g.base,
                            d_exp.get() + g.base, d_status.get() + g.base, st.s);
        HIPCHK(hipGetLastError());
    }
    std::vector<double> mant((size_t)n_res);
    std::vector<i64> ex((size_t)n_res);
    std::vector<int> stat((size_t)n_res);
    if (n_res) {
        HIPCHK(hipMemcpyAsync(mant.data(), d_mant.get(), (size_t)n_res * 8, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(ex.data(), d_exp.get(), (size_t)n_res * 8, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(stat.data(), d_status.get(), (size_t)n_res * 4, hipMemcpyDeviceToHost, st.s));
    }
    HIPCHK(hipStreamSynchronize(st.s));  // (the one synchronisation; the host vectors above are locals)
    for (int k = 0; k < K; ++k) {
        const ScoreJob& j = jobs[k];
        for (int q = 0; q < j.S(); ++q) {
            const size_t r = (size_t)(res_at[(size_t)k] + q * res_stride[(size_t)k]);
            j.log_prob[q] = stat[r] == 0 ? log_prob(mant[r], ex[r]) : -INFINITY;
            if (j.mant) j.mant[q] = mant[r];
            if (j.exp2) j.exp2[q] = ex[r];
            if (j.status) j.status[q] = stat[r];
        }
    }
    return 0;
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

std::string fmt_17g(double v)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

bool ends_with(const std::string& s, const char* ext)
{
    const size_t n = strlen(ext);
    return s.size() >= n && s.compare(s.size() - n, n, ext) == 0;
}

// ---- hmm segment: one Viterbi pass through the class loop of all models ------------------------------------
thread_local float g_segment_kernel_ms = -1.f;  // e2vq_hmm_segment_last_kernel_ms

// psi and g bytes per launch: whole streams up to ECOZ2_HMM_SEGMENT_CHUNK_BYTES (default 256 MiB); a longer stream alone
i64 segment_chunk_bytes()
{
    const char* v = getenv("ECOZ2_HMM_SEGMENT_CHUNK_BYTES");
    const i64 b = v && *v ? atoll(v) : (i64)256 << 20;
    return std::max<i64>(b, 1);
}

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

struct SegOut {  // host arrays, any may be null; per frame: cls, state, entered, gbest; per stream: log_prob, status
    uint16_t* cls = nullptr;
    uint16_t* state = nullptr;
    uint8_t* entered = nullptr;
    double* gbest = nullptr;
    double* log_prob = nullptr;
    int* status = nullptr;
};

// The joint Viterbi of S device-resident streams (h_offs: their S + 1 offsets, on the host) under the class loop of the
// models (already checked by segment_check_shape; all of one M; lflats: log_model of each), on the current device and the
// stream st.
int segment_device(const std::vector<const Hmm*>& ms, const std::vector<std::vector<double>>& lflats, const unsigned short* d_sym, const i64* h_offs, int S, double ln_switch,
                   hipStream_t st, const SegOut& out)
{
    const int K = (int)ms.size(), M = ms[0]->M;
    // logarithms: lpi of every class | lA of every class | lB of every class
    int sumN = 0, a_words = 0;
    std::vector<int> comp0((size_t)K), a_at((size_t)K);
    for (int k = 0; k < K; ++k) {
        comp0[(size_t)k] = sumN;
        a_at[(size_t)k] = a_words;
        sumN += ms[(size_t)k]->N;
        a_words += ms[(size_t)k]->N * ms[(size_t)k]->N;
    }
    std::vector<double> params((size_t)sumN + (size_t)a_words + (size_t)sumN * M);
    for (int k = 0; k < K; ++k) {
        const std::vector<double>& lflat = lflats[(size_t)k];
        const size_t N = (size_t)ms[(size_t)k]->N;
        std::copy(lflat.begin(), lflat.begin() + N, params.begin() + comp0[(size_t)k]);
        std::copy(lflat.begin() + N, lflat.begin() + N + N * N, params.begin() + sumN + a_at[(size_t)k]);
        std::copy(lflat.begin() + N + N * N, lflat.end(), params.begin() + sumN + a_words + (size_t)comp0[(size_t)k] * M);
    }
    // the packing: class after class, a class that does not fit the current slot opens the next
    std::vector<e2hmm::SegLaneDev> lanes;
    std::vector<int> slot_info;
    std::vector<uint16_t> comp_cls((size_t)sumN);
    int fill = 64;  // lanes taken of the current slot (64: none is open)
    for (int k = 0; k < K; ++k) {
        const int N = ms[(size_t)k]->N;
        if (fill + N > 64) {
            const int l0 = (int)lanes.size();
            lanes.resize((size_t)l0 + 64);
            for (int l = 0; l < 64; ++l) lanes[(size_t)(l0 + l)] = e2hmm::SegLaneDev{-1, 0, 0, l, 0, 0};
            slot_info.push_back(0);
            slot_info.push_back(0);
            fill = 0;
        }
        const size_t l0 = lanes.size() - 64;
        for (int j = 0; j < N; ++j) {
            lanes[l0 + (size_t)(fill + j)] = e2hmm::SegLaneDev{k, j, N, fill, comp0[(size_t)k] + j, a_at[(size_t)k]};
            comp_cls[(size_t)(comp0[(size_t)k] + j)] = (uint16_t)k;
        }
        int* info = &slot_info[slot_info.size() - 2];
        info[0] = std::max(info[0], N);
        info[1] = fill == 0 ? 1 : 0;  // (a second class in the slot clears it)
        fill += N;
    }
    const int slots = (int)(lanes.size() / 64);
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
    const i64 budget = segment_chunk_bytes(), row = 2 * (i64)sumN + 4;
    std::vector<std::pair<int, int>> chunks;
    i64 max_frames = 0;
    for (int s0 = 0; s0 < S;) {
        int s1 = s0 + 1;
        while (s1 < S && (h_offs[s1 + 1] - h_offs[s0]) * row <= budget) ++s1;
        chunks.emplace_back(s0, s1);
        max_frames = std::max(max_frames, h_offs[s1] - h_offs[s0]);
        s0 = s1;
    }
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

}  // namespace

// ==========================================================================================
// the reference's FFI symbols
// ==========================================================================================

// fn ecoz2_set_random_seed(seed: c_long) -> c_ulong    src/ecoz2_lib/mod.rs:75; negative = time based (src/hmm/mod.rs:73-76)
extern "C" unsigned long ecoz2_set_random_seed(long seed)
{
    const uint64_t s = seed < 0 ? (uint64_t)time(nullptr) : (uint64_t)seed;
    g_rng = s;
    return (unsigned long)s;
}

// fn ecoz2_hmm_learn(N, model_type, sequence_filenames, num_sequences, hmm_epsilon, val_auto, max_iterations, use_par,
//                    callback: extern "C" fn(*mut c_char, c_double))                     src/ecoz2_lib/mod.rs:134-145
// use_par is accepted and ignored (the E-step always runs one wavefront per sequence on the GPU).
extern "C" int ecoz2_hmm_learn(int N, int model_type, const char* const* sequence_filenames, unsigned num_sequences,
                               double hmm_epsilon, double val_auto, int max_iterations, int use_par,
                               hmm_learn_callback_t callback)
{
    FlushStdout flush_on_return;
    (void)use_par;
    if (!sequence_filenames || num_sequences < 1) return e2vq_set_error("ecoz2_hmm_learn: no sequences");
    if (N < 1 || N > e2hmm::MAX_N) return e2vq_set_error("number of states %d not in [1, %d]", N, e2hmm::MAX_N);
    if (require_device(env_device())) return 1;
    SeqSet ss;
    if (load_sequences(sequence_filenames, num_sequences, ss)) return 1;
    // the name of the trained model is taken from the first training sequence (CHANGELOG.md:174-176)
    for (int i = 1; i < ss.S(); ++i)
        if (ss.classes[(size_t)i] != ss.classes[0])
            return e2vq_set_error("conformity error: class_name: %s != %s", ss.classes[0].c_str(), ss.classes[(size_t)i].c_str());
    for (uint16_t v : ss.sym)
        if ((int)v >= ss.M) return e2vq_set_error("symbol %u outside the codebook size %d", v, ss.M);
    i64 maxT = 0;
    for (int i = 0; i < ss.S(); ++i) maxT = std::max(maxT, ss.offs[(size_t)i + 1] - ss.offs[(size_t)i]);
    Hmm h;
    h.class_name = ss.classes[0];
    h.resize(N, ss.M);
    if (hmm_init(h, model_type)) return 1;
    printf("\nHMM learn: class '%s'  N=%d M=%d type=%d  #sequences = %d  max_T=%lld\n", h.class_name.c_str(), N, ss.M,
           model_type, ss.S(), (long long)maxT);
    printf("  epsilon=%g  val_auto=%g  max_iterations=%d\n", hmm_epsilon, val_auto, max_iterations);
    std::vector<double> hist;
    if (train(h, ss, hmm_epsilon, val_auto, max_iterations, callback, hist, getenv("ECOZ2_VQ_QUIET") == nullptr)) return 1;
    std::string path;
    if (save_learned(h, model_type, val_auto, max_iterations, hist, &path)) return 1;
    printf("%zu E-step(s); model saved: %s\n", hist.size(), path.c_str());
    return 0;
}

// `hmm learn --all-classes`: learn_models over one N, after this entry point's own checks (all before
// any HIP call).  Unlike the grid, sequences of different codebook sizes are refused.
extern "C" int e2vq_hmm_learn_classes(int N, int model_type, const char* const* sequence_filenames, unsigned num_sequences,
                                      double hmm_epsilon, double val_auto, int max_iterations, hmm_learn_callback_t callback)
{
    FlushStdout flush_on_return;
    if (!sequence_filenames || num_sequences < 1) return e2vq_set_error("e2vq_hmm_learn_classes: no sequences");
    if (N < 1 || N > e2hmm::MAX_N) return e2vq_set_error("number of states %d not in [1, %d]", N, e2hmm::MAX_N);
    if (model_type < 0 || model_type > 3) return e2vq_set_error("model type %d not in 0..3", model_type);
    SeqSet ss;
    if (load_sequences(sequence_filenames, num_sequences, ss)) return 1;
    for (uint16_t v : ss.sym)
        if ((int)v >= ss.M) return e2vq_set_error("symbol %u outside the codebook size %d", v, ss.M);
    return learn_models(ss, {N}, model_type, hmm_epsilon, val_auto, max_iterations, callback);
}

// `hmm learn --grid`: learn_models over the N given, ascending, after this entry point's own checks
// (all before any HIP call).  Each model gets what e2vq_hmm_learn_classes(N, ...) of the files of its M gives its class.
extern "C" int e2vq_hmm_learn_grid(const int* Ns, int num_N, int model_type, const char* const* sequence_filenames,
                                   unsigned num_sequences, double hmm_epsilon, double val_auto, int max_iterations,
                                   hmm_learn_callback_t callback)
{
    FlushStdout flush_on_return;
    if (!sequence_filenames || num_sequences < 1) return e2vq_set_error("e2vq_hmm_learn_grid: no sequences");
    if (!Ns || num_N < 1) return e2vq_set_error("e2vq_hmm_learn_grid: no number of states given");
    std::vector<int> n_list(Ns, Ns + num_N);
    std::sort(n_list.begin(), n_list.end());
    for (size_t i = 0; i < n_list.size(); ++i) {
        if (n_list[i] < 1 || n_list[i] > e2hmm::MAX_N) return e2vq_set_error("number of states %d not in [1, %d]", n_list[i], e2hmm::MAX_N);
        if (i > 0 && n_list[i] == n_list[i - 1]) return e2vq_set_error("number of states %d given more than once", n_list[i]);
    }
    if (model_type < 0 || model_type > 3) return e2vq_set_error("model type %d not in 0..3", model_type);
    SeqSet ss;
    if (load_sequences(sequence_filenames, num_sequences, ss, /*mixed_M=*/true)) return 1;
    for (int i = 0; i < ss.S(); ++i)
        for (i64 t = ss.offs[(size_t)i]; t < ss.offs[(size_t)i + 1]; ++t)
            if ((int)ss.sym[(size_t)t] >= ss.Ms[(size_t)i])
                return e2vq_set_error("%s: symbol %u outside the codebook size %d", ss.files[(size_t)i].c_str(), ss.sym[(size_t)t],
                                      ss.Ms[(size_t)i]);
    return learn_models(ss, n_list, model_type, hmm_epsilon, val_auto, max_iterations, callback);
}

// fn ecoz2_hmm_classify(model_filenames, num_models, sequence_filenames, num_sequences, show_ranked,
//                       classification_filename)                                       src/ecoz2_lib/mod.rs:147-154
extern "C" int ecoz2_hmm_classify(const char* const* model_filenames, unsigned num_models,
                                  const char* const* sequence_filenames, unsigned num_sequences, int show_ranked,
                                  const char* classification_filename)
{
    FlushStdout flush_on_return;
    if (!model_filenames || num_models < 1 || !sequence_filenames) return e2vq_set_error("ecoz2_hmm_classify: bad arguments");
    if (require_device(env_device())) return 1;
    std::vector<Hmm> models;
    if (load_models(model_filenames, num_models, models)) return 1;
    SeqSet ss;
    if (load_sequences(sequence_filenames, num_sequences, ss)) return 1;
    std::vector<const Hmm*> ms;
    for (const Hmm& h : models) ms.push_back(&h);
    // ECOZ2_VQ_GPUS workers, each scoring a contiguous share of the sequences under every model (independent: the
    // scores are the single worker's bit for bit)
    const int workers = std::min(env_workers(), std::max(1, ss.S())), ndev = device_count();
    if (!ndev) return 1;
    const size_t K = ms.size();
    std::vector<double> lp((size_t)ss.S() * K);
    if (run_workers(workers, [&](int w) -> int {
            i64 s0, s1;
            split_range(ss.S(), workers, w, &s0, &s1);
            if (require_device(worker_device(env_device(), w, ndev))) return 1;
            const i64 a = ss.offs[(size_t)s0], b = ss.offs[(size_t)s1];
            std::vector<i64> offs;
            for (i64 i = s0; i <= s1; ++i) offs.push_back(ss.offs[(size_t)i] - a);
            DeviceBuffer<unsigned short> d_sym;
            DeviceBuffer<i64> d_offs;
            Stream st;
            if (st.create()) return 1;
            if (d_sym.upload(ss.sym.data() + a, (size_t)(b - a), st.s) || d_offs.upload(offs.data(), offs.size(), st.s)) return 1;
            std::vector<double> part;
            if (score_device(ms, d_sym.get(), d_offs.get(), (int)(s1 - s0), st.s, part)) return 1;
            std::copy(part.begin(), part.end(), lp.begin() + (ptrdiff_t)((size_t)s0 * K));
            return 0;
        }))
        return 1;
    return classify_report(models, ss.files, ss.classes, lp, ss.M < 0 ? models[0].M : ss.M, show_ranked != 0,
                           classification_filename);
}

// `hmm classify --grid`: a grid point is an (N, M) for which a model is given -- N ascending, then M
// ascending; its models are the given .hmm files of that header in list order, its sequences the given .seq files of
// that M in list order.  Every sequence is scored under every model of every point in one batch; then each point gets
// the line "grid point: N=<n> M=<m>" followed byte for byte by what ecoz2_hmm_classify prints for its lists (and, with
// classification_dir, that call's CSV as <dir>/N<n>__M<m>.csv), and a summary block (and CSV) closes the output.  All the
// checks run before any HIP call, and files are written only once everything is scored.
extern "C" int e2vq_hmm_classify_grid(const char* const* model_filenames, unsigned num_models,
                                      const char* const* sequence_filenames, unsigned num_sequences, int show_ranked,
                                      const char* classification_dir, const char* summary_filename)
{
    FlushStdout flush_on_return;
    if (!model_filenames || num_models < 1) return e2vq_set_error("e2vq_hmm_classify_grid: no models");
    if (!sequence_filenames || num_sequences < 1) return e2vq_set_error("e2vq_hmm_classify_grid: no sequences");
    std::vector<Hmm> models;
    if (load_models(model_filenames, num_models, models)) return 1;
    SeqSet ss;
    if (load_sequences(sequence_filenames, num_sequences, ss, /*mixed_M=*/true)) return 1;
    std::map<std::pair<int, int>, std::vector<int>> by_point;  // (std::map: N ascending, then M ascending)
    for (int k = 0; k < (int)models.size(); ++k) by_point[{models[(size_t)k].N, models[(size_t)k].M}].push_back(k);
    std::map<int, std::vector<int>> by_M;
    for (int i = 0; i < ss.S(); ++i) by_M[ss.Ms[(size_t)i]].push_back(i);
    for (const auto& pv : by_point) {
        const int N = pv.first.first, M = pv.first.second;
        for (size_t a = 0; a < pv.second.size(); ++a)
            for (size_t b = a + 1; b < pv.second.size(); ++b)
                if (models[(size_t)pv.second[a]].class_name == models[(size_t)pv.second[b]].class_name)
                    return e2vq_set_error("grid point N=%d M=%d: class '%s' has more than one model (%s, %s)", N, M,
                                          models[(size_t)pv.second[a]].class_name.c_str(), model_filenames[pv.second[a]],
                                          model_filenames[pv.second[b]]);
        if (!by_M.count(M)) return e2vq_set_error("grid point N=%d M=%d: no sequence with codebook size %d among the given ones", N, M, M);
    }
    for (const auto& mv : by_M) {
        bool found = false;
        for (const auto& pv : by_point) found = found || pv.first.second == mv.first;
        if (!found)
            return e2vq_set_error("%s: no model with codebook size %d among the given ones", ss.files[(size_t)mv.second[0]].c_str(), mv.first);
    }
    // the store: each M's sequences contiguous, in list order
    struct MRange {
        int s_lo = 0, s_hi = 0;
    };
    std::vector<uint16_t> sym;
    std::vector<i64> offs(1, 0);
    std::map<int, MRange> range_of_M;
    for (const auto& mv : by_M) {
        MRange r;
        r.s_lo = (int)offs.size() - 1;
        for (int i : mv.second) {
            sym.insert(sym.end(), ss.sym.begin() + ss.offs[(size_t)i], ss.sym.begin() + ss.offs[(size_t)i + 1]);
            offs.push_back((i64)sym.size());
        }
        r.s_hi = (int)offs.size() - 1;
        range_of_M[mv.first] = r;
    }
    SeqStore store;
    store.sym = sym.data();
    store.offs = offs.data();
    // model k's ln P of its point's sequences, in the point's sequence order
    std::vector<std::vector<double>> lp(models.size());
    std::vector<ScoreJob> jobs;
    for (const auto& pv : by_point)
        for (int k : pv.second) {
            const MRange r = range_of_M[pv.first.second];
            lp[(size_t)k].assign((size_t)(r.s_hi - r.s_lo), 0.0);
            ScoreJob j;
            j.h = &models[(size_t)k];
            j.s_lo = r.s_lo;
            j.s_hi = r.s_hi;
            j.log_prob = lp[(size_t)k].data();
            jobs.push_back(j);
        }
    // ECOZ2_VQ_GPUS workers, each scoring a contiguous share of every point's sequences (independent: the scores are
    // the single worker's bit for bit)
    int max_S = 1;
    for (const auto& mv : by_M) max_S = std::max(max_S, (int)mv.second.size());
    const int workers = std::min(env_workers(), max_S), ndev = device_count();
    if (!ndev) return 1;
    if (run_workers(workers, [&](int w) -> int {
            std::vector<ScoreJob> mine;
            for (const ScoreJob& j : jobs) {
                i64 a, b;
                split_range(j.S(), workers, w, &a, &b);
                if (a >= b) continue;
                ScoreJob q = j;
                q.s_lo = j.s_lo + (int)a;
                q.s_hi = j.s_lo + (int)b;
                q.log_prob = j.log_prob + a;
                mine.push_back(q);
            }
            if (mine.empty()) return 0;
            if (require_device(worker_device(env_device(), w, ndev))) return 1;
            return score_grid_batch(mine.data(), (int)mine.size(), store);
        }))
        return 1;
    std::string summary = "N,M,models,sequences,accuracy,avg_accuracy\n";
    std::vector<std::string> lines;
    for (const auto& pv : by_point) {
        const int N = pv.first.first, M = pv.first.second;
        const std::vector<int>& seq_ids = by_M[M];
        const size_t K = pv.second.size(), S = seq_ids.size();
        std::vector<Hmm> point_models;
        std::vector<std::string> files, classes;
        std::vector<double> point_lp(S * K);
        for (size_t k = 0; k < K; ++k) {
            point_models.push_back(models[(size_t)pv.second[k]]);
            for (size_t s = 0; s < S; ++s) point_lp[s * K + k] = lp[(size_t)pv.second[k]][s];
        }
        for (int i : seq_ids) {
            files.push_back(ss.files[(size_t)i]);
            classes.push_back(ss.classes[(size_t)i]);
        }
        printf("grid point: N=%d M=%d\n", N, M);
        std::string csv;
        if (classification_dir && *classification_dir)
            csv = std::string(classification_dir) + "/N" + std::to_string(N) + "__M" + std::to_string(M) + ".csv";
        ReportFigures fig;
        if (classify_report(point_models, files, classes, point_lp, M, show_ranked != 0, csv.empty() ? nullptr : csv.c_str(), &fig)) return 1;
        char b[160];
        snprintf(b, sizeof b, "  N=%-4d M=%-5d models=%-4zu sequences=%-6zu accuracy=%.2f avg_accuracy=%.2f\n", N, M, K, fig.classified,
                 (double)fig.accuracy, (double)fig.avg_accuracy);
        lines.push_back(b);
        snprintf(b, sizeof b, "%d,%d,%zu,%zu,%.9g,%.9g\n", N, M, K, fig.classified, (double)fig.accuracy, (double)fig.avg_accuracy);
        summary += b;
    }
    printf("\ngrid summary: %zu point(s)\n", lines.size());
    for (const std::string& l : lines) printf("%s", l.c_str());
    if (summary_filename && *summary_filename) {
        if (write_file(summary_filename, std::vector<unsigned char>(summary.begin(), summary.end()))) return 1;
        printf("%s saved\n", summary_filename);
    }
    return 0;
}

// fn ecoz2_hmm_classify_predictors(model_filenames, num_models: c_uint, cb_filenames, num_codebooks: c_int,
//        prd_filenames, num_predictors: c_int, show_ranked, classification_filename)   src/ecoz2_lib/mod.rs:156-165
// Every .prd is quantised on the GPU against the codebook of each model (one codebook for all models, or one per
// class, matched by class name) and the symbol sequences are scored where they are: frames in, log-probabilities out.
extern "C" int ecoz2_hmm_classify_predictors(const char* const* model_filenames, unsigned num_models,
                                             const char* const* cb_filenames, int num_codebooks,
                                             const char* const* prd_filenames, int num_predictors, int show_ranked,
                                             const char* classification_filename)
{
    FlushStdout flush_on_return;
    if (!model_filenames || num_models < 1 || !cb_filenames || num_codebooks < 1 || !prd_filenames || num_predictors < 0)
        return e2vq_set_error("ecoz2_hmm_classify_predictors: bad arguments");
    const int device = env_device();
    if (require_device(device)) return 1;
    std::vector<Hmm> models;
    if (load_models(model_filenames, num_models, models)) return 1;
    // codebooks
    struct Cb {
        std::string cls;
        int P = 0, M = 0;
        std::vector<double> refl;
    };
    std::vector<Cb> cbs((size_t)num_codebooks);
    for (int i = 0; i < num_codebooks; ++i) {
        char cls[96];
        if (e2vq_cbook_info(cb_filenames[i], cls, &cbs[i].P, &cbs[i].M)) return 1;
        cbs[i].cls = cls;
        cbs[i].refl.resize((size_t)cbs[i].M * (cbs[i].P + 1));
        if (e2vq_cbook_read(cb_filenames[i], cbs[i].refl.data(), cbs[i].M)) return 1;
        if (cbs[i].P != cbs[0].P) return e2vq_set_error("%s: prediction order differs from the first codebook", cb_filenames[i]);
    }
    const int P = cbs[0].P;
    // which codebook feeds which model
    std::vector<int> cb_of((size_t)num_models, 0);
    for (unsigned k = 0; k < num_models; ++k) {
        int found = num_codebooks == 1 ? 0 : -1;
        for (int i = 0; i < num_codebooks && found < 0; ++i)
            if (cbs[i].cls == models[k].class_name) found = i;
        if (found < 0) return e2vq_set_error("no codebook of class '%s' for model %s", models[k].class_name.c_str(), model_filenames[k]);
        if (cbs[found].M != models[k].M)
            return e2vq_set_error("%s: model has M=%d but codebook %s has M=%d", model_filenames[k], models[k].M, cb_filenames[found], cbs[found].M);
        cb_of[k] = found;
    }
    // predictors: headers only here (file order = case order); the frames are streamed below
    std::vector<std::string> files, classes;
    std::vector<i64> offs(1, 0);
    i64 max_T = 0;
    for (int f = 0; f < num_predictors; ++f) {
        char cls[96];
        int p;
        int64_t T;
        if (e2vq_prd_info(prd_filenames[f], cls, &p, &T)) return 1;
        if (p != P) return e2vq_set_error("%s: prediction order %d differs from the codebooks' %d", prd_filenames[f], p, P);
        files.push_back(prd_filenames[f]);
        classes.push_back(cls);
        offs.push_back(offs.back() + T);
        max_T = std::max<i64>(max_T, T);
    }
    const i64 total = offs.back();
    const int S = (int)files.size();
    printf("number of HMM models: %u  number of codebooks: %d  number of predictor files: %d (%lld vectors)\n", num_models,
           num_codebooks, S, (long long)total);
    // Bounded memory (round 4): the corpus is cut into UNITS of whole files holding at most CHUNK frames together
    // (ECOZ2_VQ_CLASSIFY_CHUNK, default 2^18 = 78 MB at P = 36; at most 65 536 files), which the ECOZ2_VQ_GPUS workers pull
    // from a shared counter.  A unit's frames go through one of the worker's two pinned slots to the device, are quantised
    // against each codebook in turn and scored at once under that codebook's models: only the unit's symbols are ever
    // resident besides its frames.  Reading unit u + 1 from the files overlaps the device's work on unit u.  A file longer
    // than a chunk is a unit of its own: its frames stream through the slot piece by piece into the symbol buffer (once per
    // codebook), then its one sequence is scored.  Files are independent: the same scores for any chunk size and any
    // number of workers.
    const char* chv = getenv("ECOZ2_VQ_CLASSIFY_CHUNK");
    const i64 CHUNK = std::max<i64>(64, chv && *chv ? atoll(chv) : (1 << 18));
    constexpr int MAX_UNIT_FILES = 65536;
    struct Unit {
        int f0, f1;
    };
    std::vector<Unit> units;
    for (int f = 0; f < S;) {
        int g = f;
        i64 n = 0;
        while (g < S && g - f < MAX_UNIT_FILES && (g == f || n + (offs[(size_t)g + 1] - offs[(size_t)g]) <= CHUNK)) {
            n += offs[(size_t)g + 1] - offs[(size_t)g];
            ++g;
            if (n > CHUNK) break;  // (a single file longer than a chunk)
        }
        units.push_back(Unit{f, g});
        f = g;
    }
    int max_files = 1;
    for (const Unit& u : units) max_files = std::max(max_files, u.f1 - u.f0);
    // which models each codebook feeds
    struct Group {
        int cb;
        std::vector<const Hmm*> ms;
        std::vector<unsigned> idx;
    };
    std::vector<Group> groups;
    for (int c = 0; c < num_codebooks; ++c) {
        Group gr;
        gr.cb = c;
        for (unsigned k = 0; k < num_models; ++k)
            if (cb_of[k] == c) {
                gr.ms.push_back(&models[k]);
                gr.idx.push_back(k);
            }
        if (!gr.ms.empty()) groups.push_back(std::move(gr));
    }
    std::vector<double> lp((size_t)S * num_models, -INFINITY);
    std::atomic<int> next_unit{0};
    std::atomic<bool> failed{false};
    const int workers = std::min(env_workers(), std::max(1, (int)units.size())), ndev = device_count();
    if (!ndev) return 1;
    const int NC = P + 1;
    if (run_workers(workers, [&](int w) -> int {
            // (any way out of this worker but the last line stops the others at their next unit)
            struct FailGuard {
                std::atomic<bool>& f;
                bool ok = false;
                ~FailGuard()
                {
                    if (!ok) f.store(true);
                }
            } fail_guard{failed};
            const int dev = workers == 1 ? device : worker_device(device, w, ndev);
            if (require_device(dev)) return 1;
            struct Slot {
                PinnedBuffer<double> h_frames, h_mant;
                PinnedBuffer<i64> h_offs, h_exp;
                PinnedBuffer<int> h_st;
                DeviceBuffer<double> d_frames, d_mant;
                DeviceBuffer<unsigned short> d_sym;
                DeviceBuffer<i64> d_offs, d_exp;
                DeviceBuffer<int> d_st;
                Event done;
                int unit = -1;
            } slots[2];
            std::vector<DevModels> dms(groups.size());
            Stream st;
            if (st.create()) return 1;
            // one quantize session per codebook (its codeword images are built once), all on the worker's stream
            struct Sessions {
                std::vector<e2vq_session*> v;
                ~Sessions()
                {
                    for (e2vq_session* s : v)
                        if (s) e2vq_session_destroy(s);
                }
            } sessions;
            for (size_t g = 0; g < groups.size(); ++g) {
                e2vq_session* vq = nullptr;
                if (e2vq_session_create(dev, P, &vq)) return 1;
                sessions.v.push_back(vq);
                if (e2vq_set_stream(vq, (void*)st.s)) return 1;  // quantize and scoring are ordered on one stream
                if (e2vq_set_codebook(vq, cbs[(size_t)groups[g].cb].refl.data(), cbs[(size_t)groups[g].cb].M)) return 1;
                if (dms[g].upload(groups[g].ms, st.s)) return 1;
            }
            const size_t res_cap = (size_t)max_files * num_models;
            const size_t sym_cap = (size_t)std::max<i64>(CHUNK, max_T) + 64;
            // (the staging slots hold a unit's frames: never more than the whole corpus has)
            const i64 STAGE = std::max<i64>(64, std::min<i64>(CHUNK, offs[(size_t)S]));
            for (Slot& q : slots)
                if (q.h_frames.reserve((size_t)STAGE * NC) || q.h_offs.reserve((size_t)max_files + 1) || q.h_mant.reserve(res_cap) ||
                    q.h_exp.reserve(res_cap) || q.h_st.reserve(res_cap) || q.d_frames.reserve((size_t)STAGE * NC) ||
                    q.d_sym.reserve(sym_cap) || q.d_offs.reserve((size_t)max_files + 1) || q.d_mant.reserve(res_cap) ||
                    q.d_exp.reserve(res_cap) || q.d_st.reserve(res_cap) || q.done.create(hipEventDisableTiming))
                    return 1;
            // results of the unit in flight in a slot -> lp (layout on the device: group after group, [sequence][model of the group])
            auto harvest = [&](Slot& q) -> int {
                if (q.unit < 0) return 0;
                HIPCHK(hipEventSynchronize(q.done.e));
                const Unit& u = units[(size_t)q.unit];
                const int Su = u.f1 - u.f0;
                size_t base = 0;
                for (const Group& gr : groups) {
                    const size_t K = gr.idx.size();
                    for (int sq = 0; sq < Su; ++sq)
                        for (size_t j = 0; j < K; ++j) {
                            const size_t o = base + (size_t)sq * K + j;
                            lp[(size_t)(u.f0 + sq) * num_models + gr.idx[j]] =
                                q.h_st.get()[o] == 0 ? log_prob(q.h_mant.get()[o], q.h_exp.get()[o]) : -INFINITY;
                        }
                    base += (size_t)Su * K;
                }
                q.unit = -1;
                return 0;
            };
            auto score_groups = [&](Slot& q, int Su, size_t g0, size_t g1, size_t base) -> int {  // groups [g0, g1) on q.d_sym
                for (size_t g = g0; g < g1; ++g) {
                    const int K = (int)groups[g].idx.size();
                    e2hmm::launch_score(dms[g].table.get(), K, dms[g].maxN, q.d_sym.get(), q.d_offs.get(), Su, q.d_mant.get() + base,
                                        q.d_exp.get() + base, q.d_st.get() + base, st.s);
                    HIPCHK(hipGetLastError());
                    base += (size_t)Su * K;
                }
                return 0;
            };
            int turn = 0;
            while (!failed.load()) {
                const int ui = next_unit.fetch_add(1);
                if (ui >= (int)units.size()) break;
                Slot& q = slots[turn & 1];
                ++turn;
                if (harvest(q)) return 1;
                const Unit& u = units[(size_t)ui];
                const int Su = u.f1 - u.f0;
                const i64 n_fr = offs[(size_t)u.f1] - offs[(size_t)u.f0];
                for (int f = u.f0; f <= u.f1; ++f) q.h_offs.get()[f - u.f0] = offs[(size_t)f] - offs[(size_t)u.f0];
                HIPCHK(hipMemcpyAsync(q.d_offs.get(), q.h_offs.get(), (size_t)(Su + 1) * 8, hipMemcpyHostToDevice, st.s));
                size_t n_res = 0;
                for (const Group& gr : groups) n_res += (size_t)Su * gr.idx.size();
                if (n_fr <= CHUNK) {
                    for (int f = u.f0; f < u.f1; ++f) {
                        const i64 T = offs[(size_t)f + 1] - offs[(size_t)f];
                        bool fin = true;
                        if (T > 0 && e2vq_io::prd_read_range_mt(files[(size_t)f].c_str(), P, 0, T,
                                                                q.h_frames.get() + (size_t)(offs[(size_t)f] - offs[(size_t)u.f0]) * NC,
                                                                e2vq_io::io_threads(), &fin))
                            return 1;
                        if (!fin) return e2vq_set_error("%s: contains NaN or infinite values", files[(size_t)f].c_str());
                    }
                    if (n_fr > 0) HIPCHK(hipMemcpyAsync(q.d_frames.get(), q.h_frames.get(), (size_t)n_fr * NC * 8, hipMemcpyHostToDevice, st.s));
                    size_t base = 0;
                    for (size_t g = 0; g < groups.size(); ++g) {
                        if (n_fr > 0 && e2vq_quantize_device(sessions.v[g], q.d_frames.get(), n_fr, q.d_sym.get(), nullptr)) return 1;
                        if (score_groups(q, Su, g, g + 1, base)) return 1;
                        base += (size_t)Su * groups[g].idx.size();
                    }
                } else {
                    // one file longer than a chunk: piece by piece into the symbol buffer, once per codebook (synchronous:
                    // the one staging buffer is refilled for every piece)
                    size_t base = 0;
                    for (size_t g = 0; g < groups.size(); ++g) {
                        for (i64 t0 = 0; t0 < n_fr; t0 += CHUNK) {
                            const i64 n = std::min(CHUNK, n_fr - t0);
                            bool fin = true;
                            HIPCHK(hipStreamSynchronize(st.s));  // (the previous piece has left the staging buffer)
                            if (e2vq_io::prd_read_range_mt(files[(size_t)u.f0].c_str(), P, t0, n, q.h_frames.get(), e2vq_io::io_threads(), &fin))
                                return 1;
                            if (!fin) return e2vq_set_error("%s: contains NaN or infinite values", files[(size_t)u.f0].c_str());
                            HIPCHK(hipMemcpyAsync(q.d_frames.get(), q.h_frames.get(), (size_t)n * NC * 8, hipMemcpyHostToDevice, st.s));
                            if (e2vq_quantize_device(sessions.v[g], q.d_frames.get(), n, q.d_sym.get() + t0, nullptr)) return 1;
                        }
                        if (score_groups(q, Su, g, g + 1, base)) return 1;
                        base += (size_t)Su * groups[g].idx.size();
                    }
                }
                if (n_res) {
                    HIPCHK(hipMemcpyAsync(q.h_mant.get(), q.d_mant.get(), n_res * 8, hipMemcpyDeviceToHost, st.s));
                    HIPCHK(hipMemcpyAsync(q.h_exp.get(), q.d_exp.get(), n_res * 8, hipMemcpyDeviceToHost, st.s));
                    HIPCHK(hipMemcpyAsync(q.h_st.get(), q.d_st.get(), n_res * 4, hipMemcpyDeviceToHost, st.s));
                }
                HIPCHK(hipEventRecord(q.done.e, st.s));
                q.unit = ui;
            }
            for (int k = 0; k < 2; ++k)
                if (harvest(slots[(turn + k) & 1])) return 1;
            HIPCHK(hipStreamSynchronize(st.s));
            fail_guard.ok = !failed.load();
            return 0;
        }))
        return 1;
    return classify_report(models, files, classes, lp, models[0].M, show_ranked != 0, classification_filename);
}

// fn ecoz2_hmm_show(hmm_filename, format)        src/ecoz2_lib/mod.rs:167; default format "%Lg " (src/hmm/mod.rs:153-154)
extern "C" int ecoz2_hmm_show(const char* hmm_filename, const char* format)
{
    FlushStdout flush_on_return;
    Hmm h;
    if (hmm_load(hmm_filename, h)) return 1;
    const std::string fmt = format && *format ? format : "%Lg ";
    // the format is applied to a long double when it asks for one ("%Lg": prob_t was long double originally,
    // notes.md:17-21), to a double otherwise; exactly one conversion is accepted
    size_t pct = 0, convs = 0;
    for (size_t i = 0; i + 1 < fmt.size(); ++i)
        if (fmt[i] == '%') {
            if (fmt[i + 1] == '%') { ++i; continue; }
            ++convs;
            pct = i;
        }
    if (convs != 1) return e2vq_set_error("format '%s' must hold exactly one floating-point conversion", fmt.c_str());
    size_t e = pct + 1;
    while (e < fmt.size() && strchr("-+ #0123456789.", fmt[e])) ++e;
    const bool is_long = e < fmt.size() && fmt[e] == 'L';
    if (is_long) ++e;
    if (e >= fmt.size() || !strchr("eEfFgGaA", fmt[e])) return e2vq_set_error("format '%s' is not a floating-point format", fmt.c_str());
    auto put = [&](double v) {
        if (is_long) printf(fmt.c_str(), (long double)v);
        else printf(fmt.c_str(), v);
    };
    printf("# %s:\n# className='%s', N=%d, M=%d\n", hmm_filename, h.class_name.c_str(), h.N, h.M);
    printf("pi = ");
    for (int i = 0; i < h.N; ++i) put(h.pi[(size_t)i]);
    printf("\nA =\n");
    for (int i = 0; i < h.N; ++i) {
        printf(" [%d]: ", i);
        for (int j = 0; j < h.N; ++j) put(h.A[(size_t)i * h.N + j]);
        printf("\n");
    }
    printf("B =\n");
    for (int j = 0; j < h.N; ++j) {
        printf(" [%d]: ", j);
        for (int k = 0; k < h.M; ++k) put(h.B[(size_t)j * h.M + k]);
        printf("\n");
    }
    return 0;
}

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
    std::vector<double> lp, vlp((size_t)S);
    std::vector<int> vst((size_t)S);
    std::vector<uint16_t> path(sym.size());
    if (model && S > 0) {
        DeviceBuffer<unsigned short> d_sym;
        DeviceBuffer<i64> d_offs;
        Stream st;
        if (st.create()) return 1;
        if (d_sym.upload(sym.data(), sym.size(), st.s) || d_offs.upload(offs.data(), offs.size(), st.s)) return 1;
        if (with_prob && score_device({&h}, d_sym.get(), d_offs.get(), S, st.s, lp)) return 1;
        if (gen_q_opt && viterbi_device(h.N, h.M, lflat, d_sym.get(), d_offs.get(), offs.data(), S, st.s, path.data(), vlp.data(), vst.data()))
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
        if (with_prob) printf("  log_prob = %.17g\n", lp[b]);
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

// ==========================================================================================
// array-level entry points (tests, bench, Python mirror): same kernels, no files
// ==========================================================================================
extern "C" int e2vq_hmm_init(int N, int M, int model_type, double* pi, double* A, double* B)
{
    if (N < 1 || N > e2hmm::MAX_N || M < 1 || M > 65536) return e2vq_set_error("e2vq_hmm_init: N=%d M=%d out of range", N, M);
    Hmm h;
    h.resize(N, M);
    if (hmm_init(h, model_type)) return 1;
    memcpy(pi, h.pi.data(), h.pi.size() * 8);
    memcpy(A, h.A.data(), h.A.size() * 8);
    memcpy(B, h.B.data(), h.B.size() * 8);
    return 0;
}

static int model_from_arrays(int N, int M, const double* pi, const double* A, const double* B, Hmm& h)
{
    if (N < 1 || N > e2hmm::MAX_N || M < 1 || M > 65536) return e2vq_set_error("HMM with N=%d M=%d out of range", N, M);
    h.resize(N, M);
    memcpy(h.pi.data(), pi, h.pi.size() * 8);
    memcpy(h.A.data(), A, h.A.size() * 8);
    memcpy(h.B.data(), B, h.B.size() * 8);
    return 0;
}

extern "C" int e2vq_hmm_save(const char* path, const char* class_name, int N, int M, const double* pi, const double* A,
                             const double* B)
{
    Hmm h;
    if (model_from_arrays(N, M, pi, A, B, h)) return 1;
    h.class_name = class_name ? class_name : "";
    return hmm_save(path, h);
}

extern "C" int e2vq_hmm_info(const char* path, char class_name[96], int* N, int* M)
{
    Hmm h;
    if (hmm_load(path, h)) return 1;
    memset(class_name, 0, 96);
    memcpy(class_name, h.class_name.data(), std::min<size_t>(h.class_name.size(), 95));
    *N = h.N;
    *M = h.M;
    return 0;
}

extern "C" int e2vq_hmm_load(const char* path, double* pi, double* A, double* B)
{
    Hmm h;
    if (hmm_load(path, h)) return 1;
    memcpy(pi, h.pi.data(), h.pi.size() * 8);
    memcpy(A, h.A.data(), h.A.size() * 8);
    memcpy(B, h.B.data(), h.B.size() * 8);
    return 0;
}

// scaled forward scores of S host sequences (concatenated symbols + S+1 offsets) under K models given as arrays:
// Ns[k], shared M, pis[k] / As[k] / Bs[k].  Outputs [s * K + k]: P(O) = mant * 2^exp2, status, natural-log probability.
extern "C" int e2vq_hmm_score(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                              const double* const* Bs, const uint16_t* sym, const int64_t* offs, int S, double* mant,
                              int64_t* exp2, int* status, double* log_probs)
{
    if (K < 1 || S < 0) return e2vq_set_error("e2vq_hmm_score: bad arguments");
    std::vector<Hmm> models((size_t)K);
    std::vector<const Hmm*> ms;
    for (int k = 0; k < K; ++k) {
        if (model_from_arrays(Ns[k], M, pis[k], As[k], Bs[k], models[(size_t)k])) return 1;
        ms.push_back(&models[(size_t)k]);
    }
    if (check_offsets(offs, S) || require_device(device)) return 1;
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<i64> d_offs;
    Stream st;
    if (st.create()) return 1;
    if (d_sym.upload(sym, (size_t)offs[S], st.s) || d_offs.upload((const i64*)offs, (size_t)S + 1, st.s)) return 1;
    std::vector<double> lp, mt;
    std::vector<i64> ex;
    std::vector<int> stt;
    if (score_device(ms, d_sym.get(), d_offs.get(), S, st.s, lp, &mt, &ex, &stt)) return 1;
    const size_t n = (size_t)S * K;
    for (size_t i = 0; i < n; ++i) {
        if (mant) mant[i] = mt[i];
        if (exp2) exp2[i] = ex[i];
        if (status) status[i] = stt[i];
        if (log_probs) log_probs[i] = lp[i];
    }
    return 0;
}

// scaled forward scores of K models of any (N, M) in one batch: model k has Ns[k] states and Ms[k]
// symbols, its pi | A | B at params + param_offs[k], and scores the sequences [seq_lo[k], seq_hi[k]) (ranges may overlap;
// the symbols go to the device once); the result of sequence s at out_offs[k] + (s - seq_lo[k]) of mant / exp2 / status /
// log_probs (output ranges may not overlap).  Each result is e2vq_hmm_score's for that pair, bit for bit.  A symbol >= M_k
// is not refused: it scores status 2.
extern "C" int e2vq_hmm_score_grid(int device, int K, const int* Ns, const int* Ms, const double* params, const int64_t* param_offs,
                                   const uint16_t* sym, const int64_t* offs, int S, const int64_t* seq_lo, const int64_t* seq_hi,
                                   const int64_t* out_offs, double* mant, int64_t* exp2, int* status, double* log_probs)
{
    if (K < 1 || !Ns || !Ms || !params || !param_offs || !seq_lo || !seq_hi || !out_offs)
        return e2vq_set_error("e2vq_hmm_score_grid: bad arguments (K = %d)", K);
    if (!log_probs) return e2vq_set_error("e2vq_hmm_score_grid: log_probs is required");
    if (check_offsets(offs, S)) return 1;
    std::vector<std::pair<i64, i64>> outs;  // (offset, end) of each model's results
    for (int k = 0; k < K; ++k) {
        const int N = Ns[k], M = Ms[k];
        if (N < 1 || N > e2hmm::MAX_N || M < 1 || M > 65536) return e2vq_set_error("model %d: HMM with N=%d M=%d out of range", k, N, M);
        if (seq_lo[k] < 0 || seq_lo[k] >= seq_hi[k] || seq_hi[k] > S)
            return e2vq_set_error("model %d: sequence range [%lld, %lld) not a non-empty part of [0, %d)", k, (long long)seq_lo[k],
                                  (long long)seq_hi[k], S);
        if (param_offs[k] < 0) return e2vq_set_error("model %d: parameter offset %lld < 0", k, (long long)param_offs[k]);
        if (out_offs[k] < 0) return e2vq_set_error("model %d: output offset %lld < 0", k, (long long)out_offs[k]);
        outs.emplace_back(out_offs[k], out_offs[k] + (seq_hi[k] - seq_lo[k]));
    }
    std::sort(outs.begin(), outs.end());
    for (size_t i = 1; i < outs.size(); ++i)
        if (outs[i].first < outs[i - 1].second)
            return e2vq_set_error("output ranges overlap: [%lld, %lld) and [%lld, %lld)", (long long)outs[i - 1].first,
                                  (long long)outs[i - 1].second, (long long)outs[i].first, (long long)outs[i].second);
    std::vector<Hmm> models((size_t)K);
    std::vector<ScoreJob> jobs((size_t)K);
    for (int k = 0; k < K; ++k) {
        const int N = Ns[k];
        const double* q = params + param_offs[k];
        if (model_from_arrays(N, Ms[k], q, q + N, q + N + (size_t)N * N, models[(size_t)k])) return 1;
        ScoreJob& j = jobs[(size_t)k];
        j.h = &models[(size_t)k];
        j.s_lo = (int)seq_lo[k];
        j.s_hi = (int)seq_hi[k];
        j.log_prob = log_probs + out_offs[k];
        j.mant = mant ? mant + out_offs[k] : nullptr;
        j.exp2 = exp2 ? exp2 + out_offs[k] : nullptr;
        j.status = status ? status + out_offs[k] : nullptr;
    }
    if (require_device(device)) return 1;
    SeqStore store;
    store.sym = sym;
    store.offs = (const i64*)offs;
    return score_grid_batch(jobs.data(), K, store);
}

extern "C" int64_t e2vq_hmm_acc_words(int N, int M) { return e2hmm::acc_words(N, M); }

// one Baum-Welch E-step on the GPU: the exact expected-count accumulators (e2vq_hmm_acc_words int64 words) and the
// per-sequence P(O) / status
extern "C" int e2vq_hmm_estep(int device, int N, int M, const double* pi, const double* A, const double* B,
                              const uint16_t* sym, const int64_t* offs, int S, int64_t* acc, double* mant, int64_t* exp2,
                              int* status)
{
    Hmm h;
    if (model_from_arrays(N, M, pi, A, B, h) || check_offsets(offs, S) || require_device(device)) return 1;
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<i64> d_offs;
    Trainer tr;
    Stream st;
    if (st.create()) return 1;
    if (d_sym.upload(sym, (size_t)offs[S], st.s) || d_offs.upload((const i64*)offs, (size_t)S + 1, st.s)) return 1;
    if (tr.setup(h, S, offs[S], st.s)) return 1;
    double L;
    if (tr.estep(d_sym.get(), d_offs.get(), &L, nullptr, nullptr)) return 1;
    HIPCHK(hipMemcpy(acc, tr.d_acc.get(), (size_t)tr.W * 8, hipMemcpyDeviceToHost));
    for (int s = 0; s < S; ++s) {
        if (mant) mant[s] = tr.mant[(size_t)s];
        if (exp2) exp2[s] = tr.ex[(size_t)s];
        if (status) status[s] = tr.stat[(size_t)s];
    }
    return 0;
}

// whole training on arrays (in place): the loop of ecoz2_hmm_learn without files
extern "C" int e2vq_hmm_train(int device, int N, int M, double* pi, double* A, double* B, const uint16_t* sym,
                              const int64_t* offs, int S, double epsilon, double val_auto, int max_iterations,
                              double* sum_log_prob, int cap, int* num_esteps)
{
    Hmm h;
    if (model_from_arrays(N, M, pi, A, B, h) || check_offsets(offs, S) || require_device(device)) return 1;
    SeqSet ss;
    ss.M = M;
    ss.sym.assign(sym, sym + offs[S]);
    ss.offs.assign((const i64*)offs, (const i64*)offs + S + 1);
    ss.files.assign((size_t)S, "");
    ss.classes.assign((size_t)S, "");
    std::vector<double> hist;
    if (train(h, ss, epsilon, val_auto, max_iterations, nullptr, hist, false)) return 1;
    memcpy(pi, h.pi.data(), h.pi.size() * 8);
    memcpy(A, h.A.data(), h.A.size() * 8);
    memcpy(B, h.B.data(), h.B.size() * 8);
    for (size_t i = 0; i < hist.size() && (int)i < cap; ++i) sum_log_prob[i] = hist[i];
    if (num_esteps) *num_esteps = (int)hist.size();
    return 0;
}

// whole training of K classes on arrays, in place: class k = sequences [class_offs[k], class_offs[k + 1]),
// model k at pi + k N, A + k N^2, B + k N M; its measure at sum_log_prob + k cap, its E-step count at num_esteps[k].
// Class k's result is e2vq_hmm_train's on its slice, bit for bit.  It is e2vq_hmm_train_grid's batch with one (N, M) for
// every model and ranges that do not overlap.
extern "C" int e2vq_hmm_train_classes(int device, int N, int M, int K, double* pi, double* A, double* B, const uint16_t* sym,
                                      const int64_t* offs, int S, const int64_t* class_offs, double epsilon, double val_auto,
                                      int max_iterations, double* sum_log_prob, int cap, int* num_esteps)
{
    if (K < 1 || !pi || !A || !B || !class_offs || cap < 0 || (cap > 0 && !sum_log_prob))
        return e2vq_set_error("e2vq_hmm_train_classes: bad arguments (K = %d)", K);
    if (N < 1 || N > e2hmm::MAX_N || M < 1 || M > 65536) return e2vq_set_error("HMM with N=%d M=%d out of range", N, M);
    if (check_offsets(offs, S)) return 1;
    if (class_offs[0] != 0 || class_offs[K] != S)
        return e2vq_set_error("class_offs must run from 0 to S = %d (got %lld .. %lld)", S, (long long)class_offs[0], (long long)class_offs[K]);
    for (int k = 0; k < K; ++k)
        if (class_offs[k + 1] <= class_offs[k])
            return e2vq_set_error("class_offs not strictly increasing at class %d (%lld, %lld)", k, (long long)class_offs[k],
                                  (long long)class_offs[k + 1]);
    const size_t NN = (size_t)N * N, NM = (size_t)N * M;
    std::vector<GridJob> jobs((size_t)K);
    for (int k = 0; k < K; ++k) {
        GridJob& c = jobs[(size_t)k];
        if (model_from_arrays(N, M, pi + (size_t)k * N, A + (size_t)k * NN, B + (size_t)k * NM, c.h)) return 1;
        c.s_lo = (int)class_offs[k];
        c.s_hi = (int)class_offs[k + 1];
    }
    if (require_device(device)) return 1;
    SeqStore store;
    store.sym = sym;
    store.offs = (const i64*)offs;
    if (train_grid(jobs, store, epsilon, val_auto, max_iterations, 1, device)) return 1;
    for (int k = 0; k < K; ++k) {
        const GridJob& c = jobs[(size_t)k];
        memcpy(pi + (size_t)k * N, c.h.pi.data(), c.h.pi.size() * 8);
        memcpy(A + (size_t)k * NN, c.h.A.data(), c.h.A.size() * 8);
        memcpy(B + (size_t)k * NM, c.h.B.data(), c.h.B.size() * 8);
        for (size_t i = 0; i < c.hist.size() && (int)i < cap; ++i) sum_log_prob[(size_t)k * cap + i] = c.hist[i];
        if (num_esteps) num_esteps[k] = (int)c.hist.size();
    }
    return 0;
}

// whole training of K models of any (N, M) on arrays, in place: model k has Ns[k] states and Ms[k]
// symbols, trains on the sequences [seq_lo[k], seq_hi[k]) (ranges may overlap), its pi | A | B at params + param_offs[k]
// (blocks may not overlap); its measure at sum_log_prob + k cap, its E-step count at num_esteps[k].  Model k's result is
// e2vq_hmm_train's on its slice, bit for bit.
extern "C" int e2vq_hmm_train_grid(int device, int K, const int* Ns, const int* Ms, double* params, const int64_t* param_offs,
                                   const uint16_t* sym, const int64_t* offs, int S, const int64_t* seq_lo, const int64_t* seq_hi,
                                   double epsilon, double val_auto, int max_iterations, double* sum_log_prob, int cap,
                                   int* num_esteps)
{
    if (K < 1 || !Ns || !Ms || !params || !param_offs || !seq_lo || !seq_hi || cap < 0 || (cap > 0 && !sum_log_prob))
        return e2vq_set_error("e2vq_hmm_train_grid: bad arguments (K = %d)", K);
    if (check_offsets(offs, S)) return 1;
    std::vector<std::pair<i64, i64>> blocks;  // (offset, end) of each model's parameters
    for (int k = 0; k < K; ++k) {
        const int N = Ns[k], M = Ms[k];
        if (N < 1 || N > e2hmm::MAX_N || M < 1 || M > 65536) return e2vq_set_error("model %d: HMM with N=%d M=%d out of range", k, N, M);
        if (seq_lo[k] < 0 || seq_lo[k] >= seq_hi[k] || seq_hi[k] > S)
            return e2vq_set_error("model %d: sequence range [%lld, %lld) not a non-empty part of [0, %d)", k, (long long)seq_lo[k],
                                  (long long)seq_hi[k], S);
        if (param_offs[k] < 0) return e2vq_set_error("model %d: parameter offset %lld < 0", k, (long long)param_offs[k]);
        blocks.emplace_back(param_offs[k], param_offs[k] + (i64)N + (i64)N * N + (i64)N * M);
        for (i64 t = offs[seq_lo[k]]; t < offs[seq_hi[k]]; ++t)
            if ((int)sym[t] >= M) return e2vq_set_error("model %d: symbol %u outside the codebook size %d", k, sym[t], M);
    }
    std::sort(blocks.begin(), blocks.end());
    for (size_t i = 1; i < blocks.size(); ++i)
        if (blocks[i].first < blocks[i - 1].second)
            return e2vq_set_error("parameter blocks overlap: [%lld, %lld) and [%lld, %lld)", (long long)blocks[i - 1].first,
                                  (long long)blocks[i - 1].second, (long long)blocks[i].first, (long long)blocks[i].second);
    std::vector<GridJob> jobs((size_t)K);
    for (int k = 0; k < K; ++k) {
        GridJob& j = jobs[(size_t)k];
        const int N = Ns[k];
        const double* q = params + param_offs[k];
        if (model_from_arrays(N, Ms[k], q, q + N, q + N + (size_t)N * N, j.h)) return 1;
        j.s_lo = (int)seq_lo[k];
        j.s_hi = (int)seq_hi[k];
    }
    if (require_device(device)) return 1;
    SeqStore store;
    store.sym = sym;
    store.offs = (const i64*)offs;
    if (train_grid(jobs, store, epsilon, val_auto, max_iterations, 1, device)) return 1;
    for (int k = 0; k < K; ++k) {
        const GridJob& j = jobs[(size_t)k];
        j.h.pack(params + param_offs[k]);
        for (size_t i = 0; i < j.hist.size() && (int)i < cap; ++i) sum_log_prob[(size_t)k * cap + i] = j.hist[i];
        if (num_esteps) num_esteps[k] = (int)j.hist.size();
    }
    return 0;
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
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<i64> d_offs;
    Stream st;
    if (st.create()) return 1;
    if (d_sym.upload(sym, (size_t)offs[S], st.s) || d_offs.upload((const i64*)offs, (size_t)S + 1, st.s)) return 1;
    return viterbi_device(N, M, lflat, d_sym.get(), d_offs.get(), (const i64*)offs, S, st.s, path, log_prob, status);
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
    std::vector<Hmm> models((size_t)K);
    std::vector<const Hmm*> ms;
    for (int k = 0; k < K; ++k) {
        if (model_from_arrays(Ns[k], M, pis[k], As[k], Bs[k], models[(size_t)k])) return 1;
        ms.push_back(&models[(size_t)k]);
    }
    if (check_offsets(offs, S)) return 1;
    std::vector<i64> wo((size_t)S + 1);
    scan_window_offsets((const i64*)offs, S, window_frames, hop_frames, wo.data());
    if (win_offs) memcpy(win_offs, wo.data(), wo.size() * 8);
    if (require_device(device)) return 1;
    DeviceBuffer<unsigned short> d_sym;
    Stream st;
    if (st.create()) return 1;
    if (!sym_on_device && d_sym.upload((const unsigned short*)sym, (size_t)offs[S], st.s)) return 1;
    ScanOut out;
    out.mant = mant, out.exp2 = exp2, out.status = status, out.log_probs = log_probs;
    out.best = best, out.best_log_prob = best_log_prob, out.second = second, out.second_log_prob = second_log_prob;
    return scan_device(ms, sym_on_device ? (const unsigned short*)sym : d_sym.get(), (const i64*)offs, S, window_frames, hop_frames,
                       st.s, out);
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

// ---- input -> device symbols: the stage `hmm scan` and `hmm segment` share ----------------------------------------------------
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
struct SymStage {  // device buffers the inputs of one call reuse; symbols of the current input in d_sym
    DeviceBuffer<double> d_frames;
    DeviceBuffer<int32_t> d_status;
    DeviceBuffer<unsigned short> d_sym;
};
struct VqSessionHolder {
    e2vq_session* s = nullptr;
    ~VqSessionHolder()
    {
        if (s) e2vq_session_destroy(s);
    }
};

// the checks of the inputs against the models' M and the codebook, and the codebook itself: host only, no file written
static int sym_inputs_check(const char* who, int M, const char* cb_filename, const char* const* input_filenames, int num_inputs,
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
static int sym_input_to_device(const SymInput& in, const SymInputs& si, SymStage& stg, e2vq_session* vq, int device, int P, int W_ms,
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
    std::vector<Hmm> models;
    if (load_models(model_filenames, num_models, models)) return 1;
    const int M = models[0].M;
    std::vector<const Hmm*> ms;
    std::vector<const char*> names;
    for (unsigned k = 0; k < num_models; ++k) {
        if (models[k].M != M)
            return e2vq_set_error("%s: model has M=%d but %s has M=%d", model_filenames[k], models[k].M, model_filenames[0], M);
        ms.push_back(&models[k]);
        names.push_back(models[k].class_name.c_str());
    }
    SymInputs si;
    if (sym_inputs_check("e2vq_hmm_scan_files", M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms,
                         csv_dir_or_file, si))
        return 1;
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
        const i64 offs[2] = {0, T};
        i64 wo[2];
        scan_window_offsets(offs, 1, window_frames, hop_frames, wo);
        const size_t W = (size_t)wo[1];
        std::vector<int> best(W), second(W);
        std::vector<double> lp1(W), lp2(W);
        ScanOut out;
        out.best = best.data(), out.best_log_prob = lp1.data(), out.second = second.data(), out.second_log_prob = lp2.data();
        if (scan_device(ms, stg.d_sym.get(), offs, 1, window_frames, hop_frames, st.s, out)) return 1;
        HIPCHK(hipStreamSynchronize(st.s));  // (the host buffers of this input are locals)
        if (e2vq_hmm_scan_report(in.path.c_str(), T, (int)num_models, names.data(), (int64_t)W, window_frames, hop_frames, W_ms, O_ms,
                                 best.data(), lp1.data(), second.data(), lp2.data(), min_margin, in.csv.empty() ? nullptr : in.csv.c_str()))
            return 1;
    }
    return 0;
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
    std::vector<Hmm> models((size_t)K);
    std::vector<const Hmm*> ms;
    std::vector<std::vector<double>> lflats((size_t)K);
    for (int k = 0; k < K; ++k) {
        if (model_from_arrays(Ns[k], M, pis[k], As[k], Bs[k], models[(size_t)k]) || log_model(models[(size_t)k], lflats[(size_t)k])) return 1;
        ms.push_back(&models[(size_t)k]);
    }
    if (check_offsets(offs, S)) return 1;
    if (require_device(device)) return 1;
    DeviceBuffer<unsigned short> d_sym;
    Stream st;
    if (st.create()) return 1;
    if (!sym_on_device && d_sym.upload((const unsigned short*)sym, (size_t)offs[S], st.s)) return 1;
    SegOut out;
    out.cls = cls, out.state = state, out.entered = entered, out.gbest = gbest, out.log_prob = log_prob, out.status = status;
    return segment_device(ms, lflats, sym_on_device ? (const unsigned short*)sym : d_sym.get(), (const i64*)offs, S, ln_switch, st.s, out);
}

// CSV and stdout block of one segmented input from the per-frame outputs (host only)
extern "C" int e2vq_hmm_segment_report(const char* name, int64_t T, int K, const char* const* class_names, int W_ms, int O_ms,
                                       const uint16_t* cls, const uint8_t* entered, const double* gbest, double log_prob,
                                       double ln_switch, const char* csv_filename)
{
    FlushStdout flush_on_return;
    if (!name || K < 1 || !class_names || T < 0 || (T > 0 && (!cls || !entered || !gbest)))
        return e2vq_set_error("e2vq_hmm_segment_report: bad arguments");
    if (T > 0 && !entered[0]) return e2vq_set_error("e2vq_hmm_segment_report: frame 0 does not start a segment");
    for (int64_t t = 0; t < T; ++t)
        if (cls[t] >= K) return e2vq_set_error("e2vq_hmm_segment_report: frame %lld names a model outside [0, %d)", (long long)t, K);
    struct Seg {
        int64_t b, e;
        double lp;
    };
    std::vector<Seg> segs;
    for (int64_t b = 0; b < T;) {
        int64_t e = b + 1;
        while (e < T && !entered[e]) ++e;
        // (gbest[e] of an entered frame e is the path's own cumulative score at e - 1)
        const double hi = e == T ? log_prob : gbest[e], lo = b == 0 ? 0.0 : gbest[b] + ln_switch;
        segs.push_back(Seg{b, e, hi - lo});
        b = e;
    }
    auto begin_s = [&](int64_t b) { return (double)(b * O_ms) / 1000.0; };
    // (the end of the analysis window of the segment's last frame)
    auto end_s = [&](int64_t e) { return (double)((e - 1) * O_ms + W_ms) / 1000.0; };
    if (csv_filename && *csv_filename) {
        std::string doc = "segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame\n";
        for (size_t i = 0; i < segs.size(); ++i) {
            const Seg& g = segs[i];
            doc += std::to_string(i) + "," + std::to_string(g.b) + "," + std::to_string(g.e) + "," + fmt_17g(begin_s(g.b)) + "," +
                   fmt_17g(end_s(g.e)) + "," + class_names[cls[g.b]] + "," + fmt_17g(g.lp) + "," + fmt_17g(g.lp / (double)(g.e - g.b)) + "\n";
        }
        if (write_file(csv_filename, std::vector<unsigned char>(doc.begin(), doc.end()))) return 1;
    }
    printf("%s: T=%lld  segments=%zu  (switch penalty %g)\n", name, (long long)T, segs.size(), ln_switch);
    std::vector<int64_t> frames((size_t)K, 0);
    for (int64_t t = 0; t < T; ++t) ++frames[cls[t]];
    for (int k = 0; k < K; ++k) printf("  '%s': %lld\n", class_names[k], (long long)frames[(size_t)k]);
    printf("  segments:\n");
    for (const Seg& g : segs) printf("    %.3f - %.3f %s\n", begin_s(g.b), end_s(g.e), class_names[cls[g.b]]);
    if (csv_filename && *csv_filename) printf("  %s saved\n", csv_filename);
    return 0;
}

// `hmm segment`: every input (.wav: lpc -> quantize -> segment; .prd: quantize -> segment; .seq: segment) under the models
extern "C" int e2vq_hmm_segment_files(const char* const* model_filenames, unsigned num_models, const char* cb_filename,
                                      const char* const* input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                                      const char* csv_dir_or_file)
{
    FlushStdout flush_on_return;
    if (!model_filenames || num_models < 1) return e2vq_set_error("e2vq_hmm_segment_files: no models");
    if (!input_filenames || num_inputs < 1) return e2vq_set_error("e2vq_hmm_segment_files: no inputs");
    if (segment_check_switch("e2vq_hmm_segment_files", ln_switch)) return 1;
    if (W_ms < 1 || O_ms < 1) return e2vq_set_error("e2vq_hmm_segment_files: window %d ms / offset %d ms", W_ms, O_ms);
    std::vector<Hmm> models;
    if (load_models(model_filenames, num_models, models)) return 1;
    const int M = models[0].M;
    std::vector<const Hmm*> ms;
    std::vector<const char*> names;
    std::vector<int> Ns;
    for (unsigned k = 0; k < num_models; ++k) {
        if (models[k].M != M)
            return e2vq_set_error("%s: model has M=%d but %s has M=%d", model_filenames[k], models[k].M, model_filenames[0], M);
        ms.push_back(&models[k]);
        names.push_back(models[k].class_name.c_str());
        Ns.push_back(models[k].N);
    }
    if (segment_check_shape("e2vq_hmm_segment_files", (int)num_models, Ns.data())) return 1;
    std::vector<std::vector<double>> lflats((size_t)num_models);
    for (unsigned k = 0; k < num_models; ++k)
        if (log_model(models[k], lflats[k])) return e2vq_set_error("%s: %s", model_filenames[k], std::string(e2vq_last_error()).c_str());
    SymInputs si;
    if (sym_inputs_check("e2vq_hmm_segment_files", M, cb_filename, input_filenames, num_inputs, P, W_ms, O_ms, csv_dir_or_file, si))
        return 1;
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
        const i64 offs[2] = {0, T};
        const size_t n = (size_t)std::max<int64_t>(T, 1);
        std::vector<uint16_t> cls(n);
        std::vector<uint8_t> entered(n);
        std::vector<double> gbest(n);
        double lp = 0.0;
        int status = 0;
        SegOut out;
        out.cls = cls.data(), out.entered = entered.data(), out.gbest = gbest.data(), out.log_prob = &lp, out.status = &status;
        if (segment_device(ms, lflats, stg.d_sym.get(), offs, 1, ln_switch, st.s, out)) return 1;
        if (status == 2) return e2vq_set_error("%s: a symbol outside the models' alphabet of %d", in.path.c_str(), M);
        if (e2vq_hmm_segment_report(in.path.c_str(), T, (int)num_models, names.data(), W_ms, O_ms, cls.data(), entered.data(), gbest.data(),
                                    lp, ln_switch, in.csv.empty() ? nullptr : in.csv.c_str()))
            return 1;
    }
    return 0;
}
