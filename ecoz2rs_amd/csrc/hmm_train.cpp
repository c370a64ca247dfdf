// hmm_train.cpp -- Baum-Welch on the GPU: the single-model trainer (ecoz2_hmm_learn, the reference's
// src/ecoz2_lib/mod.rs:134-145, and e2vq_hmm_estep / _train) and the batched one over many models of any (N, M)
// (hmm learn --all-classes / --grid; e2vq_hmm_train_classes / _train_grid), over the kernels of hmm_device.hip.
#include "hmm_host.h"

namespace e2hmm_host {
namespace {

// ---- Baum-Welch driver over device-resident sequences -----------------------------------------------------------
struct Trainer {
    int N, M, S;
    i64 total;
    hipStream_t st;
    DeviceBuffer<double> d_params, d_alpha, d_c;
    DeviceBuffer<i64> d_acc, d_scratch;
    Scores sc;  // P(O) of each sequence
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
        md = h.dev(d_params.get());
        if (d_alpha.reserve((size_t)total * N) || d_c.reserve((size_t)total) || d_acc.reserve((size_t)W) || sc.reserve((size_t)S)) return 1;
        if (e2hmm::fb_scratch_words(N) > 0 && d_scratch.reserve((size_t)e2hmm::fb_scratch_words(N))) return 1;
        return 0;
    }
    // E-step: expected counts of this trainer's sequences into d_acc, P(O) of each into sc.
    // acc_out (optional): the count words copied to the host (several workers: summed there and handed back)
    int estep_counts(const unsigned short* d_sym, const i64* d_offs, std::vector<i64>* acc_out = nullptr)
    {
        HIPCHK(hipMemsetAsync(d_acc.get(), 0, (size_t)W * 8, st));
        e2hmm::launch_fb(md, d_sym, d_offs, S, d_alpha.get(), d_c.get(), d_acc.get(), sc.d_mant.get(), sc.d_exp.get(), sc.d_status.get(), st,
                         d_scratch.get());
        HIPCHK(hipGetLastError());
        if (sc.download((size_t)S, st)) return 1;
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

typedef void (*hmm_learn_callback_t)(char* variable, double value);
constexpr int MAX_ESTEPS = 1000;  // safety cap, same in the oracle (val_auto <= 0 with no iteration limit would never stop)

// the report line of one E-step of hmm learn
void print_iteration(int it, double L, i64 skipped)
{
    printf("  it=%d  sum log(P) = %.10g%s\n", it, L,
           skipped ? (" (" + std::to_string(skipped) + " sequence(s) the model cannot emit were skipped)").c_str() : "");
}

// the training loop of oracle/hmm_oracle.h (e2h_learn), the sequences dealt to ECOZ2_VQ_GPUS workers (SURVEY 8e:
// independent sequences).  One worker trains on the caller's thread, device and nothing else: counts and parameters
// never leave the device between the E- and the M-step.  Several: worker w on device (ECOZ2_VQ_DEVICE + w) % device
// count; the expected counts are exact int64 limb sums, so their sum over the workers -- taken on the host:
// acc_words(N, M) words, 50 KB at N = 6, M = 1024 -- is the count of a single worker bit for bit.  Every worker then runs
// the M-step on the summed counts: identical parameters everywhere, no broadcast.  L is summed on the host over all
// sequences in sequence order.
int train(Hmm& h, const SeqSet& ss, double epsilon, double val_auto, int max_iterations, hmm_learn_callback_t callback,
          std::vector<double>& hist, bool verbose)
{
    struct Worker {
        int device = 0;  // (several workers)
        Trainer tr;
        std::vector<i64> acc;
        DevSeqs seqs;  // (after the buffers: see DevSeqs)
    };
    const int workers = std::min(env_workers(), std::max(1, ss.S()));
    const bool several = workers > 1;
    const int ndev = several ? device_count() : 1;
    if (!ndev) return 1;
    std::vector<Worker> ws((size_t)workers);
    // fn(worker) on every worker's thread and device
    auto each = [&](auto fn) {
        return run_workers(workers, [&](int w) -> int {
            if (several) HIPCHK(hipSetDevice(ws[(size_t)w].device));
            return fn(ws[(size_t)w]);
        });
    };
    if (run_workers(workers, [&](int w) -> int {
            Worker& k = ws[(size_t)w];
            i64 s0, s1;
            split_range(ss.S(), workers, w, &s0, &s1);
            if (several) {
                k.device = worker_device(env_device(), w, ndev);
                if (require_device(k.device)) return 1;
            }
            if (k.seqs.upload_slice(ss, s0, s1)) return 1;
            // (redundant with setup's wait below; kept so that the sharded path's HIP calls stay what they were)
            if (several) HIPCHK(hipStreamSynchronize(k.seqs.st.s));
            return k.tr.setup(h, (int)(s1 - s0), ss.offs[(size_t)s1] - ss.offs[(size_t)s0], k.seqs.st.s);
        }))
        return 1;
    static char var[] = "sum_log_prob";
    int it = 0;
    double Lprev = 0.0;
    hist.clear();
    std::vector<i64> total;
    for (;;) {
        if ((max_iterations >= 0 && it >= max_iterations) || it >= MAX_ESTEPS) break;
        if (each([&](Worker& k) { return k.tr.estep_counts(k.seqs.sym, k.seqs.d_offs.get(), several ? &k.acc : nullptr); })) return 1;
        total.assign(ws[0].acc.size(), 0);
        double L = 0.0;
        i64 skipped = 0;
        for (const Worker& k : ws) {
            for (size_t i = 0; i < total.size(); ++i) total[i] = (i64)((unsigned long long)total[i] + (unsigned long long)k.acc[i]);
            for (size_t q = 0; q < (size_t)k.tr.S; ++q) {
                if (k.tr.sc.ok(q))
                    L = L + k.tr.sc.log_prob(q);
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
        if (each([&](Worker& k) -> int {
                if (several && k.tr.acc_upload(total)) return 1;
                if (k.tr.mstep(epsilon)) return 1;
                if (several) HIPCHK(hipStreamSynchronize(k.tr.st));
                return 0;
            }))
            return 1;
        Lprev = L;
        ++it;
    }
    if (several) HIPCHK(hipSetDevice(ws[0].device));
    return ws[0].tr.download(h);
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
i64 learn_batch_bytes() { return env_bytes("ECOZ2_HMM_LEARN_BATCH_BYTES", (i64)4 << 30); }

// ---- many models at once: a grid of (N, M) points, or every class of one (N, M) ------------------
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
    DeviceBuffer<double> d_params, d_alpha, d_c;
    DeviceBuffer<i64> d_acc, d_offs, d_scratch;
    DeviceBuffer<int> d_blocks, d_active;
    Scores sc;  // P(O) of every model's sequences, model k's from res_at
    DeviceBuffer<unsigned short> d_sym;
    DeviceBuffer<e2hmm::GridModelDev> d_models;
    Stream st;  // (after the buffers: see Stream)
    if (st.create()) return 1;
    if (d_sym.reserve((size_t)offs.back()) || d_params.upload(flat.data(), flat.size(), st.s) ||
        d_offs.upload(offs.data(), offs.size(), st.s) || d_alpha.reserve((size_t)n_alpha) || d_c.reserve((size_t)n_c) ||
        d_acc.reserve((size_t)n_acc) || sc.reserve((size_t)n_res) || d_blocks.reserve((size_t)max_blocks * 3) ||
        d_active.reserve((size_t)K))
        return 1;
    if (big_N && d_scratch.reserve((size_t)e2hmm::fb_scratch_words(big_N))) return 1;
    if (seqs.upload_symbols(ss, d_sym.get(), st.s)) return 1;
    for (int k = 0; k < K; ++k) g[(size_t)k].md = jobs[k]->h.dev(d_params.get() + g[(size_t)k].param_at);
    if (d_models.upload(g.data(), g.size(), st.s)) return 1;
    HIPCHK(hipStreamSynchronize(st.s));  // (`flat`, `offs`, `g` are locals; the copies are done)
    std::vector<int> blocks, estep_list, mstep_list;
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
                                      d_c.get(), d_acc.get(), sc.d_mant.get(), sc.d_exp.get(), sc.d_status.get(), st.s);
                HIPCHK(hipGetLastError());
                at += nb;
            }
        }
        for (int k : estep_list) {
            const e2hmm::GridModelDev& m = g[(size_t)k];
            if (m.md.N <= e2hmm::WAVE_N) continue;
            const i64 o = offs[(size_t)m.s_lo];
            e2hmm::launch_fb(m.md, d_sym.get(), d_offs.get() + m.s_lo, jobs[k]->S(), d_alpha.get() + (m.alpha_at - o * m.md.N),
                             d_c.get() + (m.c_at - o), d_acc.get() + m.acc_at, sc.d_mant.get() + m.res_at, sc.d_exp.get() + m.res_at,
                             sc.d_status.get() + m.res_at, st.s, d_scratch.get());
            HIPCHK(hipGetLastError());
        }
        if (sc.download((size_t)n_res, st.s)) return 1;
        HIPCHK(hipStreamSynchronize(st.s));
        mstep_list.clear();
        i64 max_P = 0;
        int max_N = 0;
        for (int k : estep_list) {
            const e2hmm::GridModelDev& m = g[(size_t)k];
            double L = 0.0;
            i64 skipped = 0;
            for (i64 r = m.res_at; r < m.res_at + jobs[k]->S(); ++r) {
                if (sc.ok((size_t)r))
                    L = L + sc.log_prob((size_t)r);
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
    const SeqStore store{sym.data(), offs.data()};
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

}  // namespace
}  // namespace e2hmm_host
using namespace e2hmm_host;

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

extern "C" int64_t e2vq_hmm_acc_words(int N, int M) { return e2hmm::acc_words(N, M); }

// one Baum-Welch E-step on the GPU: the exact expected-count accumulators (e2vq_hmm_acc_words int64 words) and the
// per-sequence P(O) / status
extern "C" int e2vq_hmm_estep(int device, int N, int M, const double* pi, const double* A, const double* B,
                              const uint16_t* sym, const int64_t* offs, int S, int64_t* acc, double* mant, int64_t* exp2,
                              int* status)
{
    Hmm h;
    if (model_from_arrays(N, M, pi, A, B, h) || check_offsets(offs, S) || require_device(device)) return 1;
    Trainer tr;
    DevSeqs seqs;  // (after the buffers: see DevSeqs)
    if (seqs.upload(sym, (const i64*)offs, S) || tr.setup(h, S, offs[S], seqs.st.s)) return 1;
    if (tr.estep_counts(seqs.sym, seqs.d_offs.get())) return 1;
    HIPCHK(hipMemcpy(acc, tr.d_acc.get(), (size_t)tr.W * 8, hipMemcpyDeviceToHost));
    for (int s = 0; s < S; ++s) tr.sc.get((size_t)s, mant ? mant + s : nullptr, exp2 ? exp2 + s : nullptr, status ? status + s : nullptr, nullptr);
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
    model_to_arrays(h, pi, A, B);
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
    if (!shape_ok(N, M)) return e2vq_set_error("HMM with N=%d M=%d out of range", N, M);
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
    const SeqStore store{sym, (const i64*)offs};
    if (train_grid(jobs, store, epsilon, val_auto, max_iterations, 1, device)) return 1;
    for (int k = 0; k < K; ++k) {
        const GridJob& c = jobs[(size_t)k];
        model_to_arrays(c.h, pi + (size_t)k * N, A + (size_t)k * NN, B + (size_t)k * NM);
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
        if (grid_model_check(k, N, M, seq_lo[k], seq_hi[k], S, param_offs[k])) return 1;
        blocks.emplace_back(param_offs[k], param_offs[k] + (i64)N + (i64)N * N + (i64)N * M);
        for (i64 t = offs[seq_lo[k]]; t < offs[seq_hi[k]]; ++t)
            if ((int)sym[t] >= M) return e2vq_set_error("model %d: symbol %u outside the codebook size %d", k, sym[t], M);
    }
    if (check_disjoint(blocks, "parameter blocks")) return 1;
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
    const SeqStore store{sym, (const i64*)offs};
    if (train_grid(jobs, store, epsilon, val_auto, max_iterations, 1, device)) return 1;
    for (int k = 0; k < K; ++k) {
        const GridJob& j = jobs[(size_t)k];
        j.h.pack(params + param_offs[k]);
        for (size_t i = 0; i < j.hist.size() && (int)i < cap; ++i) sum_log_prob[(size_t)k * cap + i] = j.hist[i];
        if (num_esteps) num_esteps[k] = (int)j.hist.size();
    }
    return 0;
}
