// vq_classes.cpp -- one codebook per class in one batched training: e2vq_vq_learn_classes (the classes of
// a list of .prd files) and e2vq_vq_train_classes (arrays).  Each class gets, bit for bit, what a session ladder of its frames
// alone gives: the batched pass runs the plain FP64 sweep and the per-cell tail kernels of the single path over every class
// still active at this level, and the host keeps per class what e2vq_learn keeps per session.
#include "host_util.h"
#include "vq_session.h"

#include <map>

using namespace e2hip;

namespace {

// one pass of a level as e2vq_learn prints it
struct PassLine {
    double avg, DDprv, DD, ratio;
    i64 empty;
};

struct VqClassJob {
    std::string name;
    const double* frames = nullptr;  // T x NC, row-major (host)
    i64 T = 0;
    bool want_level_codebooks = false;             // files: every level's codebook is written
    std::vector<e2vq_level_stats> levels;           // out
    std::vector<std::vector<PassLine>> passes;      // out: per level
    std::vector<std::vector<double>> level_refl;    // out (want_level_codebooks): per level, M x NC
    std::vector<double> refl;                       // out: the last codebook
    int M = 0;                                      // out: its size
};

i64 env_i64(const char* name, i64 dflt)
{
    const char* v = getenv(name);
    return v && *v ? atoll(v) : dflt;
}

// ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES: a class with more frames trains through the single-class session path (its
// prefiltered sweeps), measured in DESIGN.md 4.9.1
i64 solo_frames() { return std::max<i64>(env_i64("ECOZ2_VQ_LEARN_CLASSES_SOLO_FRAMES", (i64)1 << 19), 0); }

// ECOZ2_VQ_LEARN_BATCH_BYTES: the device memory budget of one batch (default 4 GiB)
i64 batch_budget() { return std::max<i64>(env_i64("ECOZ2_VQ_LEARN_BATCH_BYTES", (i64)4 << 30), 1); }

// the codebook size the ladder ends at: the first power of two >= max_M (1 when max_M <= 1)
int final_M(int max_M)
{
    int M = 1;
    while (M < max_M) M *= 2;
    return M;
}

// device bytes of a class in a batch: its blocked frames, rows, the codebook arrays and their images
i64 class_batch_bytes(int NC, int Mcap, i64 T)
{
    const i64 frames = (T + 63) / 64 * 64 * NC;
    const i64 rows = (i64)Mcap * e2vq::row_stride(NC);
    const i64 cb = (i64)Mcap * (3 * NC + e2vq::cb_pad(NC) + 1) + e2vq::cbm_doubles(NC, Mcap);
    return (frames + rows + cb + 2 * NC + 16) * 8;
}

// e2vq_learn's level loop on a session of the class's frames alone (orders without an MFMA sweep; classes above the solo
// threshold): the same calls, recording what e2vq_learn prints and writes
int train_solo(int device, int P, double eps, int max_M, VqClassJob& job)
{
    e2vq_session* s = nullptr;
    if (e2vq_session_create(device, P, &s)) return 1;
    struct Closer {
        e2vq_session* s;
        ~Closer() { e2vq_session_destroy(s); }
    } close{s};
    if (e2vq_set_frames_host(s, job.frames, job.T) || e2vq_prepare(s) || e2vq_init_codebook(s)) return 1;
    while (s->M < max_M) {
        if (e2vq_grow(s)) return 1;
        e2vq_level_stats ls{};
        std::vector<PassLine> lines;
        int pass = 0;
        for (;; ++pass) {
            if (e2vq_pass(s, nullptr, nullptr)) return 1;
            if (e2vq_pass_stats_impl(s, &ls, /*wait_failed=*/true)) return 1;
            const double DD = ls.DD, ratio = (s->DDprv - DD) / DD;
            lines.push_back(PassLine{ls.avg_distortion, s->DDprv, DD, ratio, ls.empty_cells});
            const bool converged = (pass > 0 && !(ratio >= eps)) || pass + 1 >= E2VQ_MAX_PASSES;
            s->DDprv = DD;
            if (converged) break;
            if (e2vq_update(s)) return 1;
        }
        ls.passes = pass + 1;
        job.levels.push_back(ls);
        job.passes.push_back(std::move(lines));
        if (job.want_level_codebooks) {
            std::vector<double> r((size_t)s->M * s->NC);
            if (e2vq_get_codebook(s, r.data(), nullptr)) return 1;
            job.level_refl.push_back(std::move(r));
        }
    }
    job.M = s->M;
    job.refl.resize((size_t)s->M * s->NC);
    return e2vq_get_codebook(s, job.refl.data(), nullptr);
}

// K classes (P <= 80) trained together on the current device.  Per pass: one launch of each kernel over the classes still
// active at this level -- zero rows, the batched sweep, statistics, centroids into the shadow codebooks, the level records --,
// one copy of those records back and one synchronisation; then the classes that go on commit their update (one codebook
// launch).  When every class has ended the level, the whole batch grows: M is the same for every class of a batch.
int train_batch(VqClassJob* const* jobs, int K, int P, double eps, int max_M)
{
    const int NC = P + 1, RS = e2vq::row_stride(NC), NPAD = e2vq::cb_pad(NC);
    const int Mcap = final_M(max_M);
    const long refl_stride = (long)Mcap * NC, cbq_stride = (long)Mcap * NPAD, cbm_stride = e2vq::cbm_doubles(NC, Mcap);
    const long rows_stride = (long)Mcap * RS, S_stride = (long)Mcap * NC, within_stride = Mcap, stats_words = 2 * NC + 3;
    std::vector<i64> bo(1, 0);  // first block of each class in the concatenated image
    i64 maxT = 0;
    for (int k = 0; k < K; ++k) {
        bo.push_back(bo.back() + (jobs[k]->T + 63) / 64);
        maxT = std::max(maxT, jobs[k]->T);
    }
    const i64 total_blocks = bo.back();
    DeviceBuffer<double> d_tmp, d_blk, d_refl, d_refl2, d_cbq, d_cbm, d_S, d_within;
    DeviceBuffer<i64> d_stats, d_rows, d_lstats, d_rec;
    DeviceBuffer<u64> d_maxabs, d_l1max;
    DeviceBuffer<int> d_flags, d_act;
    DeviceBuffer<DevScalars> d_sc;
    DeviceBuffer<e2vq::PassClassEntry> d_table;
    PinnedBuffer<i64> h_rec;
    PinnedBuffer<int> h_act;
    PinnedBuffer<e2vq::PassClassEntry> h_table;
    Stream st;  // (after the buffers: see Stream)
    if (st.create()) return 1;
    const int max_entries = (int)(total_blocks / 8 + K + 1);
    if (d_tmp.reserve((size_t)maxT * NC) || d_blk.reserve((size_t)total_blocks * 64 * NC) || d_refl.reserve((size_t)K * refl_stride) ||
        d_refl2.reserve((size_t)K * refl_stride) || d_cbq.reserve((size_t)K * cbq_stride) || d_cbm.reserve((size_t)K * cbm_stride) ||
        d_S.reserve((size_t)K * S_stride) || d_within.reserve((size_t)K * within_stride) || d_stats.reserve((size_t)K * stats_words) ||
        d_rows.reserve((size_t)K * rows_stride) || d_lstats.reserve((size_t)K * 8) || d_rec.reserve((size_t)K * 8) ||
        d_maxabs.reserve((size_t)K) || d_l1max.reserve((size_t)K) || d_flags.reserve((size_t)K * 2) || d_act.reserve((size_t)K) ||
        d_sc.reserve((size_t)K) || d_table.reserve((size_t)max_entries) || h_rec.reserve((size_t)K * 8) || h_act.reserve((size_t)K) ||
        h_table.reserve((size_t)max_entries))
        return 1;
    HIPCHK(hipMemsetAsync(d_maxabs.get(), 0, (size_t)K * 8, st.s));
    HIPCHK(hipMemsetAsync(d_flags.get(), 0, (size_t)K * 2 * sizeof(int), st.s));
    HIPCHK(hipMemsetAsync(d_stats.get(), 0, (size_t)K * stats_words * 8, st.s));
    HIPCHK(hipMemsetAsync(d_lstats.get(), 0, (size_t)K * 8 * 8, st.s));
    HIPCHK(hipMemsetAsync(d_l1max.get(), 0, (size_t)K * 8, st.s));
    // the prologue of every class: e2vq_set_frames_device + e2vq_prepare + e2vq_init_codebook's kernels on its own frames
    for (int k = 0; k < K; ++k) {
        const VqClassJob& c = *jobs[k];
        double* blk = d_blk.get() + bo[(size_t)k] * 64 * NC;
        i64* stats = d_stats.get() + (size_t)k * stats_words;
        HIPCHK(hipMemcpyAsync(d_tmp.get(), c.frames, (size_t)c.T * NC * 8, hipMemcpyHostToDevice, st.s));
        e2vq::launch_blockify(d_tmp.get(), c.T, NC, 64, blk, (long)(bo[(size_t)k + 1] - bo[(size_t)k]), d_maxabs.get() + k,
                              d_flags.get() + 2 * k, st.s);
        e2vq::launch_finish_scalars(d_maxabs.get() + k, d_sc.get() + k, st.s);
        e2vq::launch_global_sums(blk, (long)(bo[(size_t)k + 1] - bo[(size_t)k]), NC, 64, d_sc.get() + k, stats, st.s);
        HIPCHK(hipMemcpyAsync(stats + 2 * NC + 2, &c.T, 8, hipMemcpyHostToDevice, st.s));
        e2vq::launch_finish_q(stats, NC, d_sc.get() + k, st.s);
        e2vq::launch_init_codebook(stats, NC, d_sc.get() + k, d_refl.get() + (size_t)k * refl_stride, d_flags.get() + 2 * k + 1, st.s);
        HIPCHK(hipGetLastError());
    }
    std::vector<int> flags((size_t)K * 2);
    std::vector<DevScalars> sc((size_t)K);
    HIPCHK(hipMemcpyAsync(flags.data(), d_flags.get(), flags.size() * sizeof(int), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(sc.data(), d_sc.get(), sc.size() * sizeof(DevScalars), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    for (int k = 0; k < K; ++k) {
        const char* nm = jobs[k]->name.c_str();
        if (flags[(size_t)2 * k]) return e2vq_set_error("class '%s': training set contains NaN or infinite values", nm);
        if (!(sc[(size_t)k].maxabs > 0.0)) return e2vq_set_error("class '%s': training set is all zeros", nm);
        if (flags[(size_t)2 * k + 1] != 0)
            return e2vq_set_error("class '%s': Levinson recursion failed on the global centroid (status %d)", nm, flags[(size_t)2 * k + 1]);
    }
    int M = 1;
    // act: the classes of the next launches, in class order (h_act is rewritten only after a synchronisation)
    int nact = K;
    auto upload_act = [&]() -> int {
        HIPCHK(hipMemcpyAsync(d_act.get(), h_act.get(), (size_t)nact * sizeof(int), hipMemcpyHostToDevice, st.s));
        return 0;
    };
    for (int k = 0; k < K; ++k) h_act.get()[k] = k;
    if (upload_act()) return 1;
    e2vq::launch_codebook_prepare_classes(d_refl.get(), refl_stride, M, NC, d_cbq.get(), cbq_stride, d_l1max.get(), d_cbm.get(), cbm_stride,
                                          nullptr, d_act.get(), nact, st.s);
    HIPCHK(hipGetLastError());
    std::vector<double> DDprv((size_t)K, DBL_MAX / 1e5);
    std::vector<int> pass((size_t)K), next;
    std::vector<std::vector<PassLine>> lines((size_t)K);
    const int mode_cap = 256;  // workgroups of the single-set launch (grid_for(nblocks, 8, 256)): the batch aims at the same
    while (M < max_M) {
        e2vq::launch_grow_classes(d_refl.get(), M, NC, d_refl2.get(), refl_stride, K, st.s);
        std::swap(d_refl, d_refl2);
        M *= 2;
        nact = K;
        for (int k = 0; k < K; ++k) {
            h_act.get()[k] = k;
            pass[(size_t)k] = 0;
            lines[(size_t)k].clear();
        }
        if (upload_act()) return 1;
        e2vq::launch_codebook_prepare_classes(d_refl.get(), refl_stride, M, NC, d_cbq.get(), cbq_stride, d_l1max.get(), d_cbm.get(),
                                              cbm_stride, nullptr, d_act.get(), nact, st.s);
        for (;;) {
            // the block table: runs of whole blocks of one class, `per` blocks each (a multiple of the 8 waves)
            i64 blocks = 0;
            for (int i = 0; i < nact; ++i) blocks += bo[(size_t)h_act.get()[i] + 1] - bo[(size_t)h_act.get()[i]];
            const i64 per = std::max<i64>(8, (blocks + mode_cap - 1) / mode_cap + 7) / 8 * 8;
            int ne = 0;
            for (int i = 0; i < nact; ++i) {
                const int k = h_act.get()[i];
                for (i64 b = bo[(size_t)k]; b < bo[(size_t)k + 1]; b += per)
                    h_table.get()[ne++] = e2vq::PassClassEntry{(long)b, (long)(jobs[k]->T - (b - bo[(size_t)k]) * 64),
                                                              (int)std::min<i64>(per, bo[(size_t)k + 1] - b), k};
            }
            HIPCHK(hipMemcpyAsync(d_table.get(), h_table.get(), (size_t)ne * sizeof(e2vq::PassClassEntry), hipMemcpyHostToDevice, st.s));
            e2vq::launch_zero_rows_classes(d_rows.get(), rows_stride, M, NC, d_act.get(), nact, st.s);
            if (e2vq::launch_pass_classes(NC, d_blk.get(), d_table.get(), ne, d_cbm.get(), cbm_stride, M, d_sc.get(), d_l1max.get(),
                                          d_rows.get(), rows_stride, st.s))
                return e2vq_set_error("no batched sweep for prediction order %d", P);
            e2vq::launch_rows_stats_classes(d_rows.get(), rows_stride, M, NC, d_sc.get(), d_S.get(), S_stride, d_within.get(),
                                            within_stride, d_lstats.get(), d_act.get(), nact, st.s);
            e2vq::launch_centroids_classes(d_rows.get(), rows_stride, d_S.get(), S_stride, M, NC, d_refl.get(), d_refl2.get(), refl_stride,
                                           d_lstats.get(), d_act.get(), nact, st.s);
            e2vq::launch_level_record_classes(d_lstats.get(), d_l1max.get(), d_within.get(), within_stride, M, d_rec.get(), d_act.get(),
                                              nact, st.s);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_rec.get(), d_rec.get(), (size_t)nact * e2vq::LEVEL_RECORD_WORDS * 8, hipMemcpyDeviceToHost, st.s));
            HIPCHK(hipStreamSynchronize(st.s));
            // e2vq_pass_stats_impl's arithmetic on each class's record, then e2vq_learn's rule
            next.clear();
            for (int i = 0; i < nact; ++i) {
                const int k = h_act.get()[i];
                const i64* r = h_rec.get() + (size_t)i * e2vq::LEVEL_RECORD_WORDS;
                double l1max, w;
                memcpy(&l1max, &r[7], 8);
                memcpy(&w, &r[6], 8);
                const int Ed = e2vq::dist_exponent(sc[(size_t)k].maxabs, l1max);
                const double DD = e2vq::unfix(r[0], r[1], 30 - Ed);
                const double SS = e2vq::unfix(r[2], r[3], 30 - 2 * Ed);
                const double T = (double)jobs[k]->T;
                const double avg = DD / T;
                const double q = SS / T;
                const double p = avg * avg;
                double v = q - p;
                if (!(v > 0.0)) v = 0.0;
                const double ratio = (DDprv[(size_t)k] - DD) / DD;
                lines[(size_t)k].push_back(PassLine{avg, DDprv[(size_t)k], DD, ratio, r[4]});
                const int ps = pass[(size_t)k];
                const bool converged = (ps > 0 && !(ratio >= eps)) || ps + 1 >= E2VQ_MAX_PASSES;
                DDprv[(size_t)k] = DD;
                if (converged) {
                    e2vq_level_stats ls{};
                    ls.M = M;
                    ls.passes = ps + 1;
                    ls.DD = DD;
                    ls.avg_distortion = avg;
                    ls.sigma = sqrt(v);
                    ls.inertia = sc[(size_t)k].Q - w;
                    ls.empty_cells = r[4];
                    ls.failed_cells = r[5];
                    jobs[k]->levels.push_back(ls);
                    jobs[k]->passes.push_back(std::move(lines[(size_t)k]));
                    lines[(size_t)k].clear();
                } else {
                    pass[(size_t)k] = ps + 1;
                    next.push_back(k);
                }
            }
            if (next.empty()) break;
            nact = (int)next.size();
            std::copy(next.begin(), next.end(), h_act.get());
            if (upload_act()) return 1;
            // the classes that go on keep their update: the shadow codebook becomes the current one, with its images
            e2vq::launch_codebook_prepare_classes(d_refl2.get(), refl_stride, M, NC, d_cbq.get(), cbq_stride, d_l1max.get(), d_cbm.get(),
                                                  cbm_stride, d_refl.get(), d_act.get(), nact, st.s);
            HIPCHK(hipGetLastError());
        }
        bool want = false;
        for (int k = 0; k < K; ++k) want = want || jobs[k]->want_level_codebooks;
        if (want) {
            std::vector<double> all((size_t)K * refl_stride);
            HIPCHK(hipMemcpyAsync(all.data(), d_refl.get(), all.size() * 8, hipMemcpyDeviceToHost, st.s));
            HIPCHK(hipStreamSynchronize(st.s));
            for (int k = 0; k < K; ++k)
                if (jobs[k]->want_level_codebooks)
                    jobs[k]->level_refl.emplace_back(all.begin() + (size_t)k * refl_stride, all.begin() + (size_t)k * refl_stride + (size_t)M * NC);
        }
    }
    std::vector<double> all((size_t)K * refl_stride);
    HIPCHK(hipMemcpyAsync(all.data(), d_refl.get(), all.size() * 8, hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    for (int k = 0; k < K; ++k) {
        jobs[k]->M = M;
        jobs[k]->refl.assign(all.begin() + (size_t)k * refl_stride, all.begin() + (size_t)k * refl_stride + (size_t)M * NC);
    }
    return 0;
}

// every job: dealt to `workers` workers in contiguous class ranges balanced by frame count, worker w on device
// (dev0 + w) % device count.  Each worker trains its solo classes (orders without an MFMA sweep, classes above the solo
// threshold) one by one through the session path, and packs the others greedily, in class order, into batches of at most
// batch_budget() bytes (a larger class alone).  Classes are independent: neither the dealing nor the packing nor the route
// changes a bit of any result.
int train_classes(std::vector<VqClassJob>& jobs, int P, double eps, int max_M, int workers, int dev0)
{
    const int K = (int)jobs.size();
    workers = std::max(1, std::min(workers, K));
    const int ndev = device_count();
    if (!ndev) return 1;
    const int NC = P + 1, Mcap = final_M(max_M);
    const bool batched_order = e2vq::uses_mfma(NC);
    const i64 solo = solo_frames(), budget = batch_budget();
    std::vector<i64> prefix(1, 0);
    for (const VqClassJob& c : jobs) prefix.push_back(prefix.back() + c.T);
    std::vector<int> bound((size_t)workers + 1, K);
    bound[0] = 0;
    for (int w = 1; w < workers; ++w) {
        int c = bound[(size_t)w - 1];
        while (c < K && prefix[(size_t)c] * workers < prefix[(size_t)K] * w) ++c;
        bound[(size_t)w] = c;
    }
    return run_workers(workers, [&](int w) -> int {
        const int lo = bound[(size_t)w], hi = bound[(size_t)w + 1];
        if (lo >= hi) return 0;
        const int dev = worker_device(dev0, w, ndev);
        if (require_device(dev)) return 1;
        std::vector<VqClassJob*> batch;
        i64 bytes = 0;
        auto flush = [&]() -> int {
            if (batch.empty()) return 0;
            const int rc = train_batch(batch.data(), (int)batch.size(), P, eps, max_M);
            batch.clear();
            bytes = 0;
            return rc;
        };
        for (int c = lo; c < hi; ++c) {
            VqClassJob& j = jobs[(size_t)c];
            if (!batched_order || j.T > solo) {
                if (train_solo(dev, P, eps, max_M, j)) return 1;
                continue;
            }
            const i64 b = class_batch_bytes(NC, Mcap, j.T);
            if (!batch.empty() && bytes + b > budget && flush()) return 1;
            batch.push_back(&j);
            bytes += b;
        }
        return flush();
    });
}

// the checks every entry point makes before the device: the total frame count within the per-set bound of the kernels
int check_total(i64 T)
{
    if (T > (i64)INT32_MAX - 64) return e2vq_set_error("%lld frames exceed the limit of 2^31 - 65", (long long)T);
    return 0;
}

int check_order(int P)
{
    if (P < 1 || P > E2VQ_MAX_P - 1) return e2vq_set_error("prediction order %d out of range", P);
    return 0;
}

}  // namespace

// `vq learn --all-classes`: one codebook per class name of the .prd headers, classes in byte order of
// their names, each class's files in list order.  Per class the files, the stdout block and the callbacks are those of
// ecoz2_vq_learn on the class's files alone; they are written and printed class by class once every class has trained.
// All the checks run before any HIP call.
extern "C" int e2vq_vq_learn_classes(int P, double eps, const char* const* prd_files, int n, void* target,
                                     ecoz2_vq_learn_callback_t cb)
{
    e2host::FlushStdout flush_on_return;
    if (!prd_files || n < 1) return e2vq_set_error("e2vq_vq_learn_classes: no predictor files");
    if (check_order(P)) return 1;
    std::map<std::string, std::vector<int>> by_class;  // (std::string's order is the bytes', as strcmp's)
    std::vector<i64> Tf((size_t)n);
    i64 total = 0;
    for (int i = 0; i < n; ++i) {
        char cls[96];
        int p;
        int64_t t;
        if (e2vq_prd_info(prd_files[i], cls, &p, &t)) return 1;
        if (p != P) return e2vq_set_error("%s: prediction order %d, expected %d", prd_files[i], p, P);
        by_class[cls].push_back(i);
        Tf[(size_t)i] = t;
        total += t;
    }
    std::vector<VqClassJob> jobs;
    for (const auto& kv : by_class) {
        VqClassJob c;
        c.name = kv.first;
        for (int i : kv.second) c.T += Tf[(size_t)i];
        if (c.T < 1) return e2vq_set_error("class '%s' has no training vectors", c.name.c_str());
        c.want_level_codebooks = true;
        jobs.push_back(std::move(c));
    }
    if (check_total(total)) return 1;
    const int NC = P + 1;
    std::vector<std::vector<double>> frames(jobs.size());
    size_t ci = 0;
    for (const auto& kv : by_class) {
        std::vector<double>& f = frames[ci];
        f.resize((size_t)jobs[ci].T * NC);
        i64 at = 0;
        for (int i : kv.second) {
            if (Tf[(size_t)i] > 0 &&
                e2vq_io::prd_read_range_mt(prd_files[i], P, 0, Tf[(size_t)i], f.data() + (size_t)at * NC, e2vq_io::io_threads()))
                return 1;
            at += Tf[(size_t)i];
        }
        jobs[ci].frames = f.data();
        ++ci;
    }
    const int max_M = e2vq_env_int("ECOZ2_VQ_MAX_CODEBOOK_SIZE", 2048);
    if (train_classes(jobs, P, eps, max_M, env_workers(), env_device())) return 1;
    // ecoz2_vq_learn's output, class by class (learn_common's header, then e2vq_learn's report, levels and callbacks)
    const bool verbose = getenv("ECOZ2_VQ_QUIET") == nullptr;
    const char* out_root = e2vq_env_str("ECOZ2_VQ_OUT_ROOT", ".");
    char path[4096];
    for (const VqClassJob& c : jobs) {
        const char* name = c.name.c_str();
        printf("Codebook generation:\n\n%lld training vectors (ε=%g)\n", (long long)c.T, eps);
        snprintf(path, sizeof path, "%s/data/codebooks/%s/eps_%g.rpt", out_root, name, eps);
        FILE* rpt = nullptr;
        if (e2vq_io::mkdirs_for(path) == 0) rpt = fopen(path, "w");
        struct FileCloser {
            FILE*& f;
            ~FileCloser() { if (f) fclose(f); }
        } rpt_guard{rpt};
        if (rpt)
            fprintf(rpt, "# %lld training vectors, P=%d, eps=%g\n# M passes DD avg_distortion sigma inertia empty_cells\n",
                    (long long)c.T, P, eps);
        if (verbose) printf("Report: %s\n", path);
        for (size_t l = 0; l < c.levels.size(); ++l) {
            const e2vq_level_stats& ls = c.levels[l];
            snprintf(path, sizeof path, "%s/data/codebooks/%s/eps_%g_M_%04d.cbook", out_root, name, eps, ls.M);
            if (verbose) printf("%s\n", path);
            if (verbose)
                for (size_t q = 0; q < c.passes[l].size(); ++q) {
                    const PassLine& pl = c.passes[l][q];
                    printf("(%d)\tDP=%g\tDDprv=%g\tDD=%g\t%g\n", (int)q, pl.avg, pl.DDprv, pl.DD, pl.ratio);
                    if (pl.empty > 0)
                        printf("WARN: review_cells: %lld empty cell(s) for codebook size %d)\n", (long long)pl.empty, ls.M);
                }
            if (e2vq_cbook_write(path, name, P, ls.M, c.level_refl[l].data())) return 1;
            if (rpt)
                fprintf(rpt, "%d %d %.17g %.17g %.17g %.17g %lld\n", ls.M, ls.passes, ls.DD, ls.avg_distortion, ls.sigma, ls.inertia,
                        (long long)ls.empty_cells);
            if (cb) cb(target, ls.M, ls.avg_distortion, ls.sigma, ls.inertia);
        }
    }
    return 0;
}

// whole ladders of K classes on arrays: class k = frames [class_offs[k], class_offs[k + 1]) of the T x (P + 1)
// row-major `frames`; its last codebook at codebooks + k max_M (P + 1), its level records at levels + k max_levels, their
// number at num_levels[k].  Class k's results are, bit for bit, those of a session ladder of its frames alone.
extern "C" int e2vq_vq_train_classes(int device, int P, int K, const double* frames, const int64_t* class_offs, double eps, int max_M,
                                     double* codebooks, e2vq_level_stats* levels, int max_levels, int* num_levels)
{
    if (K < 1 || !frames || !class_offs || !codebooks || max_levels < 0 || (max_levels > 0 && !levels))
        return e2vq_set_error("e2vq_vq_train_classes: bad arguments (K = %d)", K);
    if (check_order(P)) return 1;
    if (max_M < 1 || max_M > 65536 || (max_M & (max_M - 1)) != 0)
        return e2vq_set_error("max_M = %d: expected a power of two in [1, 65536]", max_M);
    if (class_offs[0] != 0) return e2vq_set_error("class_offs must start at 0 (got %lld)", (long long)class_offs[0]);
    for (int k = 0; k < K; ++k)
        if (class_offs[k + 1] <= class_offs[k])
            return e2vq_set_error("class_offs not strictly increasing at class %d (%lld, %lld)", k, (long long)class_offs[k],
                                  (long long)class_offs[k + 1]);
    if (check_total(class_offs[K])) return 1;
    const int NC = P + 1;
    std::vector<VqClassJob> jobs((size_t)K);
    for (int k = 0; k < K; ++k) {
        jobs[(size_t)k].name = "class " + std::to_string(k);
        jobs[(size_t)k].frames = frames + (size_t)class_offs[k] * NC;
        jobs[(size_t)k].T = class_offs[k + 1] - class_offs[k];
    }
    if (require_device(device)) return 1;
    if (train_classes(jobs, P, eps, max_M, 1, device)) return 1;
    for (int k = 0; k < K; ++k) {
        const VqClassJob& c = jobs[(size_t)k];
        memcpy(codebooks + (size_t)k * max_M * NC, c.refl.data(), c.refl.size() * 8);
        for (size_t l = 0; l < c.levels.size() && (int)l < max_levels; ++l) levels[(size_t)k * max_levels + l] = c.levels[l];
        if (num_levels) num_levels[k] = (int)c.levels.size();
    }
    return 0;
}
