// hmm_transitions.cpp -- the matrix of class-to-class prices of `hmm segment --class-transitions` on the
// host: its file format (read, write, the names that may head a column) and its estimator from labelled successions
// (`hmm transitions`, e2vq_hmm_class_transitions).  No device code is reached from here.
#include "hmm_host.h"

namespace e2hmm_host {

// ---- the transitions file: "class,<name_1>,...,<name_K>", then one line "<from>,v_1,...,v_K" per class ------------------
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

namespace {

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
}  // namespace e2hmm_host
using namespace e2hmm_host;

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
    if (files_given(who, model_filenames, num_models, input_filenames && num_inputs >= 1)) return 1;
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
