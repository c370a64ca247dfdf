// hmm_transcript.cpp -- what the commands that take a transcript share (`hmm align`, `hmm learn --embedded`, `hmm align
// --posteriors`; hmm_host.h): the checks of an array-level entry point, the transcripts of the label files, align_plan, the plan
// of the embedded forward-backward pass on the host and on the device, its parameter block, and the reports' common parts.
#include "hmm_host.h"

namespace e2hmm_host {
static constexpr int ALIGN_MAX_L = 65535;
static int embed_a_ld(int N) { return N | 1; }  // (odd: see hmm_embed.hip)

bool unit_is_initial(int l, const uint8_t* opt) { return l == 0 || (l == 1 && opt && opt[0]); }
bool unit_is_final(int l, int L, const uint8_t* opt) { return l == L - 1 || (l == L - 2 && opt && opt[L - 1]); }

int align_plan(const char* who, int K, const int* Ns, const i64* offs, int S, const int32_t* units, const i64* unit_offs,
               const uint8_t* optional, double ln_switch, AlignPlan& ap, bool embedded, bool own_looped_lds)
{
    if (segment_check_switch(who, ln_switch)) return 1;
    if (std::isinf(ln_switch)) return e2vq_set_error("%s: ln_switch = %g: a finite price (every unit has to be entered)", who, ln_switch);
    if (unit_offs[0] != 0) return e2vq_set_error("%s: unit_offs[0] = %lld, not 0", who, (long long)unit_offs[0]);
    bool force_looped = false;
    if (!embedded && loop_body_looped("ECOZ2_HMM_ALIGN_BODY", 0, &force_looped)) return 1;  // (the E-step's body: estep_plan)
    const i64 budget = env_bytes("ECOZ2_HMM_ALIGN_TABLE_BYTES", (i64)4 << 30);
    ap.cls = pack_slots(std::vector<int>(Ns, Ns + K));
    const SegPacking& cls = ap.cls;
    std::vector<bool> looped((size_t)S);
    std::vector<i64> bytes((size_t)S);
    ap.streams.resize((size_t)S);
    for (int s = 0; s < S; ++s) {
        const i64 u0 = unit_offs[s], L64 = unit_offs[s + 1] - u0;
        if (L64 < 0) return e2vq_set_error("%s: unit_offs decrease at stream %d", who, s);
        if (L64 < 1) return e2vq_set_error("%s: stream %d has an empty transcript", who, s);
        if (L64 > ALIGN_MAX_L) return e2vq_set_error("%s: stream %d has %lld units (at most %d)", who, s, (long long)L64, ALIGN_MAX_L);
        const int L = (int)L64;
        const int32_t* u = units + u0;
        const uint8_t* opt = optional ? optional + u0 : nullptr;
        std::vector<int> uN((size_t)L);
        i64 sumN = 0;
        bool mandatory = false;
        for (int l = 0; l < L; ++l) {
            if (u[l] < 0 || u[l] >= K) return e2vq_set_error("%s: stream %d, unit %d names the class %d outside [0, %d)", who, s, l, u[l], K);
            if (opt && opt[l] && l > 0 && opt[l - 1])
                return e2vq_set_error("%s: stream %d, units %d and %d are both optional (a path may pass over one unit only)", who, s, l - 1, l);
            mandatory = mandatory || !(opt && opt[l]);
            uN[(size_t)l] = Ns[u[l]];
            sumN += Ns[u[l]];
        }
        if (!mandatory) return e2vq_set_error("%s: stream %d: every unit of the transcript is optional", who, s);
        if (!e2hmm::align_fits_lds(L, (int)sumN, false))
            return e2vq_set_error("%s: stream %d: %d units of sum N = %lld states do not fit in LDS (%zu of %zu bytes)", who, s, L,
                                  (long long)sumN, e2hmm::align_lds_bytes(L, (int)sumN, 0, false, false), e2hmm::SEG_LDS_BYTES);
        const SegPacking pk = pack_slots(uN);
        looped[(size_t)s] = force_looped || pk.slots > e2hmm::SEG_MAX_WAVES;
        if (looped[(size_t)s] && !own_looped_lds && !e2hmm::align_fits_lds(L, pk.sumN, true))
            return e2vq_set_error("%s: stream %d: %d units of sum N = %d states in %d wave-slots do not fit in LDS (%zu of %zu bytes)", who,
                                  s, L, pk.sumN, pk.slots, e2hmm::align_lds_bytes(L, pk.sumN, 0, true, false), e2hmm::SEG_LDS_BYTES);
        const i64 T = offs[s + 1] - offs[s];
        bytes[(size_t)s] = T * ((i64)pk.sumN + L);
        if (bytes[(size_t)s] > budget && embedded)  // (no back-pointers there: the bound alone is `hmm align`'s)
            return e2vq_set_error("%s: stream %d: %lld frames x (%d states + %d units) = %lld exceed ECOZ2_HMM_ALIGN_TABLE_BYTES=%lld, the "
                                  "bound on a stream that `hmm align` sets and that holds here too",
                                  who, s, (long long)T, pk.sumN, L, (long long)bytes[(size_t)s], (long long)budget);
        if (bytes[(size_t)s] > budget)
            return e2vq_set_error("%s: stream %d: the back-pointers of %lld frames x (%d states + %d units) take %lld bytes: more than "
                                  "ECOZ2_HMM_ALIGN_TABLE_BYTES=%lld",
                                  who, s, (long long)T, pk.sumN, L, (long long)bytes[(size_t)s], (long long)budget);
        e2hmm::AlignStreamDev& sd = ap.streams[(size_t)s];
        sd.lane_at = (i64)ap.lanes.size();
        sd.tab_at = 0;
        sd.unit_at = u0;
        sd.comp_at = (i64)ap.comp_unit.size();
        sd.slots = pk.slots, sd.L = L, sd.sumN = pk.sumN, sd.pad = 0;
        for (const e2hmm::SegLaneDev& sl : pk.lanes) {
            e2hmm::AlignLaneDev al{-1, 0, 0, sl.seg, 0, 0, 0, 0};
            if (sl.cls >= 0) {
                const int l = sl.cls, k = u[l];
                const int flags = (unit_is_initial(l, opt) ? e2hmm::ALIGN_INIT : 0) | (l >= 1 ? e2hmm::ALIGN_PRED : 0) |
                                  (l >= 2 && opt && opt[l - 1] ? e2hmm::ALIGN_SKIP : 0) | (unit_is_final(l, L, opt) ? e2hmm::ALIGN_FINAL : 0);
                al = e2hmm::AlignLaneDev{l, sl.j, sl.N, sl.seg, sl.comp, cls.comp0[(size_t)k] + sl.j, cls.a_at[(size_t)k], flags};
            }
            ap.lanes.push_back(al);
        }
        ap.slot_info.insert(ap.slot_info.end(), pk.slot_info.begin(), pk.slot_info.end());
        ap.unit_comp0.insert(ap.unit_comp0.end(), pk.comp0.begin(), pk.comp0.end());
        ap.comp_unit.insert(ap.comp_unit.end(), pk.comp_cls.begin(), pk.comp_cls.end());
    }
    // the launches: consecutive streams of one body whose tables stay within the budget and whose largest L and sum N fit LDS
    // (the E-step cuts its own)
    for (int s0 = 0; s0 < S && !embedded;) {
        AlignPlan::Launch g{s0, s0, 0, 0, 0, looped[(size_t)s0], 0};
        int slots = 0;
        while (g.s1 < S) {
            const e2hmm::AlignStreamDev& sd = ap.streams[(size_t)g.s1];
            const int mL = std::max(g.max_L, sd.L), mN = std::max(g.max_sumN, sd.sumN);
            if (g.s1 > s0 && (looped[(size_t)g.s1] != g.looped || g.bytes + bytes[(size_t)g.s1] > budget || !e2hmm::align_fits_lds(mL, mN, g.looped)))
                break;
            ap.streams[(size_t)g.s1].tab_at = g.bytes;
            g.bytes += bytes[(size_t)g.s1];
            g.max_L = mL, g.max_sumN = mN;
            slots = std::max(slots, sd.slots);
            ++g.s1;
        }
        g.waves = body_waves(g.looped, slots);
        ap.max_bytes = std::max(ap.max_bytes, g.bytes);
        ap.launches.push_back(g);
        s0 = g.s1;
    }
    return 0;
}

int transcript_check_args(const char* who, int K, const int* Ns, int M, const double* const* pis, const double* const* As,
                          const double* const* Bs, const void* sym, const int64_t* offs, int S, const int32_t* units,
                          const int64_t* unit_offs, LoopModels& lm)
{
    return loop_check_args(who, K, Ns, pis, As, Bs, offs && unit_offs && (S <= 0 || units) && syms_given(sym, offs, S)) ||
           segment_check_shape(who, K, Ns) || lm.from_arrays(K, Ns, M, pis, As, Bs) || lm.logs() || check_offsets(offs, S);
}

// ---- the transcripts of the label files ---------------------------------------------------------------------------------------------
static int class_of(const LoopModels& fm, const std::string& name)
{
    int k = 0;
    while (k < fm.K() && name != fm.names[(size_t)k]) ++k;
    return k < fm.K() ? k : -1;
}

int Transcripts::set_filler(const char* who, const LoopModels& fm, const char* filler_class)
{
    if (filler_class && *filler_class && (filler = class_of(fm, filler_class)) < 0)
        return e2vq_set_error("%s: the filler '%s' is no model's class", who, filler_class);
    return 0;
}

int Transcripts::add_labels(const char* who, const LoopModels& fm, const char* path)
{
    if (!path) return e2vq_set_error("%s: NULL file name", who);
    std::vector<LabelRow> rows;
    if (read_label_file(path, rows)) return 1;
    if (rows.empty()) return e2vq_set_error("%s: no labelled units", path);
    auto fill = [&] {
        if (filler >= 0) units.push_back(filler), optional.push_back(1);
    };
    fill();
    for (const LabelRow& r : rows) {
        const int k = class_of(fm, r.label);
        if (k < 0) return e2vq_set_error("%s:%zu: '%s' is no model's class", path, r.line, r.label.c_str());
        units.push_back(k), optional.push_back(0);
        fill();
    }
    unit_offs.push_back((i64)units.size());
    return 0;
}

// ---- the embedded forward-backward pass: its plan, its parameter block, the plan on the device -------------------------------------
int embed_route(const char* name, bool* forced, bool* lds)
{
    const char* v = getenv(name);
    *forced = v && *v;
    if (!*forced) return 0;
    if (strcmp(v, "lds") != 0 && strcmp(v, "global") != 0) return e2vq_set_error("%s=%s: lds or global", name, v);
    *lds = strcmp(v, "lds") == 0;
    return 0;
}

int embed_body(LoopBody* body) { return opt_in_body("ECOZ2_HMM_EMBED_BODY", body); }
int align_post_body(LoopBody* body) { return opt_in_body("ECOZ2_HMM_ALIGN_POSTERIOR_BODY", body); }

int estep_plan(const char* who, int K, const int* Ns, int M, const i64* offs, int S, const int32_t* units, const i64* unit_offs,
               const uint8_t* optional, double ln_switch, const char* what, bool first_flags, LoopBody body, EStepPlan& p,
               size_t looped_unit_bytes)
{
    // the mandatory LDS of the looped body: the E-step's partial sums, V / R and per-state arrays, and what the caller's pass
    // keeps per unit on top of them
    auto looped_lds = [&](int L, int slots, int sumN) {
        return e2hmm::embed_looped_lds_bytes(L, slots, sumN, 0, false, false) + looped_unit_bytes * (size_t)L;
    };
    if (align_plan(who, K, Ns, offs, S, units, unit_offs, optional, ln_switch, p.ap, /*embedded=*/true,
                   /*own_looped_lds=*/body != LoopBody::Resident))
        return 1;
    int max_sumN = 0;
    p.looped.assign((size_t)S, 0);
    for (int s = 0; s < S; ++s) {
        const e2hmm::AlignStreamDev& sd = p.ap.streams[(size_t)s];
        const bool looped = runs_looped(body, sd.slots);
        p.looped[(size_t)s] = looped ? 1 : 0;
        if (!looped && sd.slots > e2hmm::SEG_MAX_WAVES)
            return e2vq_set_error("%s: stream %d: the units take %d wave-slots of 64 lanes (at most %d: %s)", who, s, sd.slots,
                                  e2hmm::SEG_MAX_WAVES, what);
        // (the looped body's partial sums, V / R and per-state arrays are mandatory; A and the AN table go in when they fit)
        if (looped && looped_lds(sd.L, sd.slots, sd.sumN) > e2hmm::SEG_LDS_BYTES)
            return e2vq_set_error("%s: stream %d: %d units of sum N = %d states in %d wave-slots do not fit in LDS (%zu of %zu bytes)", who,
                                  s, sd.L, sd.sumN, sd.slots, looped_lds(sd.L, sd.slots, sd.sumN), e2hmm::SEG_LDS_BYTES);
        if (!looped) {
            p.max_L = std::max(p.max_L, sd.L);
            p.max_slots = std::max(p.max_slots, sd.slots);
        }
        max_sumN = std::max(max_sumN, sd.sumN);
        const int32_t* u = units + unit_offs[s];
        const uint8_t* opt = optional ? optional + unit_offs[s] : nullptr;
        std::vector<int> first((size_t)K, -1);
        for (int l = sd.L - 1; l >= 0 && first_flags; --l) first[(size_t)u[l]] = l;
        for (int x = 0; x < sd.slots * 64; ++x) {
            e2hmm::AlignLaneDev& al = p.ap.lanes[(size_t)sd.lane_at + (size_t)x];
            if (al.unit < 0) continue;
            const int l = al.unit;
            al.flags |= (first[(size_t)u[l]] == l ? e2hmm::EMBED_FIRST : 0) | (l + 1 < sd.L ? e2hmm::EMBED_SUCC : 0) |
                        (l + 2 < sd.L && opt && opt[l + 1] ? e2hmm::EMBED_SUCC2 : 0);
        }
    }
    p.M = M;
    p.cls = pack_slots(std::vector<int>(Ns, Ns + K), embed_a_ld);
    p.row_cls = p.cls.comp_cls;
    for (int k = 0; k < K; ++k) p.classes.push_back(e2hmm::EmbedClassDev{Ns[k], p.cls.a_at[(size_t)k], 0, 0});
    if (embed_route("ECOZ2_HMM_EMBED_A", &p.a_forced, &p.a_lds)) return 1;
    // launches of whole streams whose scratch (ah and m: 8 sumN bytes a frame each, c: 8 bytes a frame and wave) stays within
    // the budget; every stream's rows are counted at the widest stream's width
    p.row_words = 2 * (i64)max_sumN + e2hmm::SEG_MAX_WAVES;
    const auto whole = plan_chunks("ECOZ2_HMM_EMBED_CHUNK_BYTES", 8 * p.row_words, offs, S, &p.max_frames);
    // a launch has one body, and the largest shapes of a looped launch fit LDS together (the bodies agree on every bit:
    // where the cuts fall is a matter of cost only)
    for (const auto& c : whole) {
        for (int s0 = c.first; s0 < c.second;) {
            EStepPlan::Shape g;
            g.looped = p.looped[(size_t)s0] != 0;
            int s1 = s0;
            while (s1 < c.second) {
                const e2hmm::AlignStreamDev& sd = p.ap.streams[(size_t)s1];
                const int mL = std::max(g.max_L, sd.L), mS = std::max(g.max_slots, sd.slots), mN = std::max(g.max_sumN, sd.sumN);
                if (s1 > s0 && ((p.looped[(size_t)s1] != 0) != g.looped ||
                                (g.looped && looped_lds(mL, mS, mN) > e2hmm::SEG_LDS_BYTES)))
                    break;
                g.max_L = mL, g.max_slots = mS, g.max_sumN = mN;
                ++s1;
            }
            p.chunks.emplace_back(s0, s1);
            p.shapes.push_back(g);
            s0 = s1;
        }
    }
    return 0;
}

std::vector<double> embed_params(const LoopModels& lm, const SegPacking& pk, double sw)
{
    const int sumN = pk.sumN, M = lm.M;
    std::vector<double> params((size_t)2 * sumN + (size_t)pk.a_words + (size_t)sumN * M, 0.0);
    for (int k = 0; k < lm.K(); ++k) {
        const Hmm& h = *lm.ms[(size_t)k];
        const int N = h.N, ld = embed_a_ld(N), c0 = pk.comp0[(size_t)k];
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

int EStepDev::upload(const EStepPlan& p, const i64* h_offs, int S, hipStream_t st)
{
    const AlignPlan& ap = p.ap;
    return lanes.upload(ap.lanes.data(), ap.lanes.size(), st) || streams.upload(ap.streams.data(), ap.streams.size(), st) ||
           slot_info.upload(ap.slot_info.data(), ap.slot_info.size(), st) || classes.upload(p.classes.data(), p.classes.size(), st) ||
           row_cls.upload(p.row_cls.data(), p.row_cls.size(), st) || offs.upload(h_offs, (size_t)S + 1, st);
}

int EStepDev::scratch(const char* who, const EStepPlan& p)
{
    if (!scr.reserve((size_t)(p.max_frames * p.row_words))) return 0;
    const std::string why = e2vq_last_error();
    return e2vq_set_error("%s: no room for the forward tables of %lld frames x %lld doubles (ECOZ2_HMM_EMBED_CHUNK_BYTES bounds "
                          "them by whole streams): %s", who, (long long)p.max_frames, (long long)p.row_words, why.c_str());
}

e2hmm::EmbedPlanDev EStepDev::plan(const EStepPlan& p, int s0, const double* d_params) const
{
    return e2hmm::EmbedPlanDev{(int)p.classes.size(), p.M, p.cls.sumN, p.cls.a_words, p.max_L, streams.get() + s0, lanes.get(),
                               slot_info.get(), d_params, classes.get(), row_cls.get()};
}

// ---- the reports --------------------------------------------------------------------------------------------------------------------
int align_report_check(const char* who, const char* name, int64_t T, int K, const char* const* class_names, int L, const int32_t* units,
                       const uint8_t* optional, const int64_t* begin, const int64_t* end, const double* score, bool rest)
{
    if (!name || K < 1 || !class_names || T < 0 || L < 1 || !units || !begin || !end || (T > 0 && !score) || !rest)
        return e2vq_set_error("%s: bad arguments", who), -1;
    int skipped = 0;
    for (int l = 0; l < L; ++l) {
        if (units[l] < 0 || units[l] >= K) return e2vq_set_error("%s: unit %d names a model outside [0, %d)", who, l, K), -1;
        if (begin[l] < 0) {
            skipped += optional && optional[l] ? 1 : 0;
            continue;
        }
        if (begin[l] >= end[l] || end[l] > T)
            return e2vq_set_error("%s: unit %d spans [%lld, %lld) of %lld frames", who, l, (long long)begin[l], (long long)end[l], (long long)T), -1;
    }
    return skipped;
}

void align_report_head(const char* name, int64_t T, int K, const char* const* class_names, int L, const int32_t* units,
                       const int64_t* begin, const int64_t* end, int skipped, double log_prob, double ln_switch)
{
    printf("%s: T=%lld  units=%d  optional units passed over=%d  log_prob=%g  (switch penalty %g)\n", name, (long long)T, L, skipped, log_prob,
           ln_switch);
    std::vector<int64_t> count((size_t)K, 0);
    for (int l = 0; l < L; ++l)
        if (begin[l] >= 0) count[(size_t)units[l]] += end[l] - begin[l];
    for (int k = 0; k < K; ++k) printf("  '%s': %lld\n", class_names[k], (long long)count[(size_t)k]);
    printf("  units:\n");
}

}  // namespace e2hmm_host
