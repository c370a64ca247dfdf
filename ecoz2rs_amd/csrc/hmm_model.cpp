// hmm_model.cpp -- HMM models and symbol sequences on the host: the generator (ecoz2_set_random_seed), the initial
// models, the .hmm format, models to and from caller arrays, .seq sets, and the sequence plumbing of the batches;
// ecoz2_hmm_show (the reference's src/ecoz2_lib/mod.rs:75,167) and the array-level e2vq_hmm_init / _save / _info / _load.
#include "hmm_host.h"

#include <time.h>

namespace e2hmm_host {

// ---- generator: ecoz2_set_random_seed (oracle: e2h_set_random_seed / splitmix64) ---------------------------
uint64_t g_rng = 0x9E3779B97F4A7C15ull;

static uint64_t rng_next()
{
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- model: initial models, the .hmm format, logarithms, caller arrays -----------------------------------------
// uniform draws in (0, 1] divided by their sequential sum
static void random_row(double* row, int n)
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
    if (!shape_ok((int)n, (int)m)) return e2vq_set_error("%s: implausible N=%u M=%u", path, n, m);
    const size_t need = 120 + ((size_t)n + (size_t)n * n + (size_t)n * m) * 8;
    if (raw.size() != need) return e2vq_set_error("%s: %zu bytes, expected %zu for N=%u M=%u", path, raw.size(), need, n, m);
    h.resize((int)n, (int)m);
    const unsigned char* p = raw.data() + 120;
    memcpy(h.pi.data(), p, h.pi.size() * 8);
    memcpy(h.A.data(), p + h.pi.size() * 8, h.A.size() * 8);
    memcpy(h.B.data(), p + (h.pi.size() + h.A.size()) * 8, h.B.size() * 8);
    return 0;
}

// (for the Viterbi decoders) lpi | lA | lB: the C library's log of every parameter, log 0 = -inf.  A negative, NaN or infinite parameter is refused
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

int load_models(const char* const* files, unsigned n, std::vector<Hmm>& models)
{
    models.resize(n);
    for (unsigned i = 0; i < n; ++i)
        if (hmm_load(files[i], models[i])) return 1;
    return 0;
}

int model_from_arrays(int N, int M, const double* pi, const double* A, const double* B, Hmm& h)
{
    if (!shape_ok(N, M)) return e2vq_set_error("HMM with N=%d M=%d out of range", N, M);
    h.resize(N, M);
    memcpy(h.pi.data(), pi, h.pi.size() * 8);
    memcpy(h.A.data(), A, h.A.size() * 8);
    memcpy(h.B.data(), B, h.B.size() * 8);
    return 0;
}

void model_to_arrays(const Hmm& h, double* pi, double* A, double* B)
{
    memcpy(pi, h.pi.data(), h.pi.size() * 8);
    memcpy(A, h.A.data(), h.A.size() * 8);
    memcpy(B, h.B.data(), h.B.size() * 8);
}

int models_from_arrays(int K, const int* Ns, int M, const double* const* pis, const double* const* As, const double* const* Bs,
                       std::vector<Hmm>& models, std::vector<const Hmm*>& ms)
{
    models.resize((size_t)K);
    for (int k = 0; k < K; ++k) {
        if (model_from_arrays(Ns[k], M, pis[k], As[k], Bs[k], models[(size_t)k])) return 1;
        ms.push_back(&models[(size_t)k]);
    }
    return 0;
}

// ---- sequences ---------------------------------------------------------------------------------------------------
int load_sequences(const char* const* files, unsigned n, SeqSet& ss, bool mixed_M)
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

int check_offsets(const int64_t* offs, int S)
{
    if (S < 0 || !offs) return e2vq_set_error("bad sequence count %d or offsets", S);
    if (offs[0] != 0) return e2vq_set_error("offs[0] = %lld, expected 0", (long long)offs[0]);
    for (int s = 0; s < S; ++s)
        if (offs[s + 1] < offs[s]) return e2vq_set_error("offs[%d] = %lld < offs[%d] = %lld", s + 1, (long long)offs[s + 1], s, (long long)offs[s]);
    return 0;
}

// ---- batches of many models: their sequences and the argument checks of the grid entry points ------------------
BatchSeqs::BatchSeqs(std::vector<std::pair<int, int>> ranges, const SeqStore& ss) : offs(1, 0)
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

int BatchSeqs::local(int s) const
{
    const auto it = std::upper_bound(merged.begin(), merged.end(), std::make_pair(s, INT32_MAX));
    const size_t q = (size_t)(it - merged.begin()) - 1;
    return run_at[q] + (s - merged[q].first);
}

// A run goes up in pieces of 128 KB: the store is pageable caller memory, and a copy of
// megabytes from it makes the runtime pin the pages first, at a cost that varies from call to call; pieces of this
// size go through the runtime's staging buffer instead (docs/HISTORY.md, "one batched HMM trainer")
int BatchSeqs::upload_symbols(const SeqStore& ss, unsigned short* d_sym, hipStream_t st) const
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

int grid_model_check(int k, int N, int M, i64 seq_lo, i64 seq_hi, int S, i64 param_off)
{
    if (!shape_ok(N, M)) return e2vq_set_error("model %d: HMM with N=%d M=%d out of range", k, N, M);
    if (seq_lo < 0 || seq_lo >= seq_hi || seq_hi > S)
        return e2vq_set_error("model %d: sequence range [%lld, %lld) not a non-empty part of [0, %d)", k, seq_lo, seq_hi, S);
    if (param_off < 0) return e2vq_set_error("model %d: parameter offset %lld < 0", k, param_off);
    return 0;
}

int check_disjoint(std::vector<std::pair<i64, i64>> r, const char* what)
{
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i].first < r[i - 1].second)
            return e2vq_set_error("%s overlap: [%lld, %lld) and [%lld, %lld)", what, r[i - 1].first, r[i - 1].second, r[i].first, r[i].second);
    return 0;
}

}  // namespace e2hmm_host
using namespace e2hmm_host;

// fn ecoz2_set_random_seed(seed: c_long) -> c_ulong    src/ecoz2_lib/mod.rs:75; negative = time based (src/hmm/mod.rs:73-76)
extern "C" unsigned long ecoz2_set_random_seed(long seed)
{
    const uint64_t s = seed < 0 ? (uint64_t)time(nullptr) : (uint64_t)seed;
    g_rng = s;
    return (unsigned long)s;
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

extern "C" int e2vq_hmm_init(int N, int M, int model_type, double* pi, double* A, double* B)
{
    if (!shape_ok(N, M)) return e2vq_set_error("e2vq_hmm_init: N=%d M=%d out of range", N, M);
    Hmm h;
    h.resize(N, M);
    if (hmm_init(h, model_type)) return 1;
    model_to_arrays(h, pi, A, B);
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
    model_to_arrays(h, pi, A, B);
    return 0;
}
