// hmm_classify.cpp -- scaled forward scoring on the GPU and the classification reports: ecoz2_hmm_classify and
// ecoz2_hmm_classify_predictors (the reference's src/ecoz2_lib/mod.rs:147-165), hmm classify --grid, and the array-level
// e2vq_hmm_score / _score_grid, over the kernels of hmm_device.hip.
#include "hmm_host.h"

#include <atomic>

namespace e2hmm_host {

int DevModels::upload(const std::vector<const Hmm*>& ms, hipStream_t st)
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
        host.push_back(ms[k]->dev(params.get() + at[k]));
        maxN = std::max(maxN, ms[k]->N);
    }
    if (table.upload(host.data(), host.size(), st)) return 1;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int score_device(const std::vector<const Hmm*>& ms, const unsigned short* d_sym, const i64* d_offs, int S, hipStream_t st, Scores& sc)
{
    const int K = (int)ms.size();
    DevModels dm;
    if (dm.upload(ms, st) || sc.reserve((size_t)S * K)) return 1;
    e2hmm::launch_score(dm.table.get(), K, dm.maxN, d_sym, d_offs, S, sc.d_mant.get(), sc.d_exp.get(), sc.d_status.get(), st);
    HIPCHK(hipGetLastError());
    if (sc.download((size_t)S * K, st)) return 1;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

namespace {

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
    DeviceBuffer<double> d_params;
    DeviceBuffer<i64> d_offs;
    DeviceBuffer<int> d_blocks;
    Scores sc;
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<e2hmm::ScoreModelDev> d_table;
    DeviceBuffer<e2hmm::ScorePackDev> d_packs;
    DeviceBuffer<ModelDev> d_big;
    Stream st;  // (after the buffers: see Stream)
    if (st.create()) return 1;
    if (d_sym.reserve((size_t)offs.back()) || d_params.upload(flat.data(), flat.size(), st.s) || d_offs.upload(offs.data(), offs.size(), st.s) ||
        sc.reserve((size_t)n_res) || d_blocks.upload(blocks.data(), blocks.size(), st.s) || d_packs.upload(packs.data(), packs.size(), st.s))
        return 1;
    if (seqs.upload_symbols(ss, d_sym.get(), st.s)) return 1;
    std::vector<ModelDev> big_table;
    for (int k = 0; k < K; ++k) {
        table[(size_t)k] = e2hmm::ScoreModelDev{jobs[k].h->dev(d_params.get() + param_at[(size_t)k]), res_at[(size_t)k]};
        big_table.push_back(table[(size_t)k].md);
    }
    if (d_table.upload(table.data(), table.size(), st.s)) return 1;
    if (!bigs.empty() && d_big.upload(big_table.data(), big_table.size(), st.s)) return 1;
    int at = 0;  // one launch per N: each sized by its own LDS (N^2 G doubles a workgroup)
    for (const auto& kv : blocks_by_N) {
        const int nb = (int)(kv.second.size() / 2);
        e2hmm::launch_score_grid(d_table.get(), d_packs.get(), kv.first, width_of_N[kv.first], d_blocks.get() + 2 * at, nb, d_sym.get(),
                                 d_offs.get(), sc.d_mant.get(), sc.d_exp.get(), sc.d_status.get(), st.s);
        HIPCHK(hipGetLastError());
        at += nb;
    }
    for (const Big& g : bigs) {
        e2hmm::launch_score(d_big.get() + g.k0, g.count, jobs[g.k0].h->N, d_sym.get(), d_offs.get() + g.s_lo, g.S, sc.d_mant.get() + g.base,
                            sc.d_exp.get() + g.base, sc.d_status.get() + g.base, st.s);
        HIPCHK(hipGetLastError());
    }
    if (sc.download((size_t)n_res, st.s)) return 1;
    HIPCHK(hipStreamSynchronize(st.s));  // (the one synchronisation)
    for (int k = 0; k < K; ++k) {
        const ScoreJob& j = jobs[k];
        for (int q = 0; q < j.S(); ++q) {
            const size_t r = (size_t)(res_at[(size_t)k] + q * res_stride[(size_t)k]);
            sc.get(r, j.mant ? j.mant + q : nullptr, j.exp2 ? j.exp2 + q : nullptr, j.status ? j.status + q : nullptr, j.log_prob + q);
        }
    }
    return 0;
}

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

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
            Scores sc;
            DevSeqs seqs;  // (after the buffers: see DevSeqs)
            if (seqs.upload_slice(ss, s0, s1) || score_device(ms, seqs.sym, seqs.d_offs.get(), (int)(s1 - s0), seqs.st.s, sc)) return 1;
            for (size_t i = 0; i < (size_t)(s1 - s0) * K; ++i) lp[(size_t)s0 * K + i] = sc.log_prob(i);
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
    const SeqStore store{sym.data(), offs.data()};
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
                PinnedBuffer<double> h_frames;
                PinnedBuffer<i64> h_offs;
                DeviceBuffer<double> d_frames;
                DeviceBuffer<unsigned short> d_sym;
                DeviceBuffer<i64> d_offs;
                ScoresT<PinnedBuffer> sc;  // (pinned: the copy back is asynchronous, harvested a unit later)
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
                if (q.h_frames.reserve((size_t)STAGE * NC) || q.h_offs.reserve((size_t)max_files + 1) || q.d_frames.reserve((size_t)STAGE * NC) ||
                    q.d_sym.reserve(sym_cap) || q.d_offs.reserve((size_t)max_files + 1) || q.sc.reserve(res_cap) || q.sc.reserve_host(res_cap) ||
                    q.done.create(hipEventDisableTiming))
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
                        for (size_t j = 0; j < K; ++j) lp[(size_t)(u.f0 + sq) * num_models + gr.idx[j]] = q.sc.log_prob(base + (size_t)sq * K + j);
                    base += (size_t)Su * K;
                }
                q.unit = -1;
                return 0;
            };
            auto score_groups = [&](Slot& q, int Su, size_t g0, size_t g1, size_t base) -> int {  // groups [g0, g1) on q.d_sym
                for (size_t g = g0; g < g1; ++g) {
                    const int K = (int)groups[g].idx.size();
                    e2hmm::launch_score(dms[g].table.get(), K, dms[g].maxN, q.d_sym.get(), q.d_offs.get(), Su, q.sc.d_mant.get() + base,
                                        q.sc.d_exp.get() + base, q.sc.d_status.get() + base, st.s);
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
                if (q.sc.download(n_res, st.s)) return 1;
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

// scaled forward scores of S host sequences (concatenated symbols + S+1 offsets) under K models given as arrays:
// Ns[k], shared M, pis[k] / As[k] / Bs[k].  Outputs [s * K + k]: P(O) = mant * 2^exp2, status, natural-log probability.
extern "C" int e2vq_hmm_score(int device, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                              const double* const* Bs, const uint16_t* sym, const int64_t* offs, int S, double* mant,
                              int64_t* exp2, int* status, double* log_probs)
{
    if (K < 1 || S < 0) return e2vq_set_error("e2vq_hmm_score: bad arguments");
    std::vector<Hmm> models;
    std::vector<const Hmm*> ms;
    if (models_from_arrays(K, Ns, M, pis, As, Bs, models, ms) || check_offsets(offs, S) || require_device(device)) return 1;
    Scores sc;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    if (seqs.upload(sym, (const i64*)offs, S) || score_device(ms, seqs.sym, seqs.d_offs.get(), S, seqs.st.s, sc)) return 1;
    for (size_t i = 0; i < (size_t)S * K; ++i)
        sc.get(i, mant ? mant + i : nullptr, exp2 ? exp2 + i : nullptr, status ? status + i : nullptr, log_probs ? log_probs + i : nullptr);
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
        if (grid_model_check(k, Ns[k], Ms[k], seq_lo[k], seq_hi[k], S, param_offs[k])) return 1;
        if (out_offs[k] < 0) return e2vq_set_error("model %d: output offset %lld < 0", k, (long long)out_offs[k]);
        outs.emplace_back(out_offs[k], out_offs[k] + (seq_hi[k] - seq_lo[k]));
    }
    if (check_disjoint(outs, "output ranges")) return 1;
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
    return score_grid_batch(jobs.data(), K, SeqStore{sym, (const i64*)offs});
}
