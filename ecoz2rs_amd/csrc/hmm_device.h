// hmm_device.h -- device-side interface of the HMM kernels (internal; the C-ABI is include/ecoz2_classify.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace e2hmm {

constexpr int WAVE_N = 64;     // up to here one wavefront per sequence, one lane per state (k_hmm_score, k_hmm_fb)
constexpr int MAX_N = 512;     // beyond: one workgroup per sequence, one thread per state (k_hmm_score_wg, k_hmm_fb_wg)
constexpr int ACC_SHIFT = 29;  // expected counts are < 2: x ~= (hi*2^31 + lo) * 2^-(29+31)  (oracle: E2H_ACC_SHIFT)

struct ModelDev {
    int N, M;
    const double* pi;  // [N]
    const double* A;   // [N][N], row = from-state
    const double* B;   // [N][M], row = state
};

// int64 words of the E-step accumulators: [hi, lo] pairs  PI[N] | AN[N][N] | AD[N] | BN[N][M] | BD[N] | used, skipped
long long acc_words(int N, int M);

// scaled forward pass of every (sequence, model) pair; results at [s * K + k]: P(O) = mant * 2^exp2, status 0 ok,
// 1 the model cannot emit the sequence, 2 symbol outside the model's alphabet.  offs: S+1 symbol offsets.
void launch_score(const ModelDev* models, int K, int maxN, const unsigned short* sym, const long long* offs, int S,
                  double* mant, long long* exp2, int* status, hipStream_t st);
// Grid scoring.  One model of the batch: the result of sequence s of its pack goes to
// res_at + (s - the pack's s_lo).  One pack: the models [k0, k0 + count) of the table, which share N, M and the
// sequences [s_lo, s_hi) of the batch's offs; count <= G of its launch.
struct ScoreModelDev {
    ModelDev md;
    long long res_at;
};
struct ScorePackDev {
    int k0, count, s_lo, s_hi;
};
// models of N <= WAVE_N states one wave scores together: floor(64 / N) where that is at least 3 (N <= SCORE_PACK_MAX_N),
// else 1 -- two models to a wave (22 <= N <= 32) measured 1 to 4 % slower than one
constexpr int SCORE_PACK_MAX_N = 21;
inline int score_pack_width(int N) { return N <= SCORE_PACK_MAX_N ? WAVE_N / N : 1; }
// workgroups a pack of S sequences takes in launch_score_grid (4 waves, a sequence each)
int score_grid_workgroups(int S);
// Scores the packs of ONE N <= WAVE_N (LDS is sized by it), G models to a wave (1 <= G <= floor(64 / N)): nblocks
// workgroups, blocks[2 b], blocks[2 b + 1] = (pack, index of the workgroup within the pack).
void launch_score_grid(const ScoreModelDev* models, const ScorePackDev* packs, int N, int G, const int* blocks, int nblocks,
                       const unsigned short* sym, const long long* offs, double* mant, long long* exp2, int* status,
                       hipStream_t st);
// Window scan (hmm_scan.hip).  One window: `len` symbols of stream `stream` from its frame `first` on.
// One run: the windows [w0, w0 + count) of the table -- of one stream, starting in non-decreasing order, the last one
// ending last -- which one workgroup scores from one staged copy of the symbols they cover.
struct ScanWin {
    int stream, len;
    long long first;
};
struct ScanRun {
    int w0, count;
};
constexpr int SCAN_SPAN_CAP = 8192;  // symbols of a run staged in LDS (16 KB next to at most 32 KB of A)
int scan_waves();                    // waves of a k_hmm_scan workgroup: each takes G windows of the run at a time
// Scores every window of the runs under the nk models models[ks[0 .. nk)] of ONE N <= WAVE_N, G windows to a wave
// (1 <= G <= floor(64 / N)); results at [w * K + k] as launch_score's.  span_lds <= SCAN_SPAN_CAP: the longest span among the
// runs, all of which are staged; 0: none is (the symbols are read from global memory).  offs: the streams' S + 1 symbol offsets.
// Returns 1, having launched nothing, when the arguments are outside these bounds.
int launch_scan(const ModelDev* models, const int* ks, int nk, int K, int N, int G, const ScanWin* wins, const ScanRun* runs,
                int nruns, int span_lds, const unsigned short* sym, const long long* offs, double* mant, long long* exp2,
                int* status, hipStream_t st);
// the same for models of more than WAVE_N states (maxN: the largest among them): a workgroup per (window, model)
int launch_scan_wg(const ModelDev* models, const int* ks, int nk, int K, int maxN, const ScanWin* wins, long long W,
                   const unsigned short* sym, const long long* offs, double* mant, long long* exp2, int* status, hipStream_t st);
// best and second-best model of each of the W windows from the W x K results: top[2 w], top[2 w + 1] (second -1 when K = 1),
// their P at tmant / texp[2 w], [2 w + 1] (0, 0 where the status is not 0); ties as `hmm classify` ranks them
void launch_scan_top2(const double* mant, const long long* exp2, const int* status, long long W, int K, int* top, double* tmant,
                      long long* texp, hipStream_t st);
// Baum-Welch E-step of one model over S sequences (expected counts added to acc; per-sequence P(O) and status out).
// alpha_buf: total_symbols x N doubles, c_buf: total_symbols doubles (scratch).
// scratch (N > WAVE_N only; may be null otherwise): fb_scratch_words(N) int64 words, contents irrelevant
void launch_fb(const ModelDev& md, const unsigned short* sym, const long long* offs, int S, double* alpha_buf,
               double* c_buf, long long* acc, double* mant, long long* exp2, int* status, hipStream_t st,
               long long* scratch = nullptr);
long long fb_scratch_words(int N);
// M-step (+ epsilon restriction on B when epsilon > 0), in place
void launch_reestimate(int N, int M, const long long* acc, double epsilon, double* pi, double* A, double* B,
                       hipStream_t st);
// workgroups of a model with S sequences in launch_fb_grid: ceil(S / 4 waves), at least 1, at most 2048 (as launch_fb's grid)
int fb_class_workgroups(int S);

// One model of a training batch (the classes of `hmm learn --all-classes`, 4.8.2, are the batch of one
// (N, M) with disjoint sequences): its own (N, M) in md, the sequences [s_lo, s_hi) of the batch's offs (other models may
// train on the same ones), and where its own slices of the batch's buffers start.
struct GridModelDev {
    ModelDev md;
    int s_lo, s_hi;
    long long alpha_at;  // alpha^ of sequence s_lo's first symbol at alpha_buf + alpha_at (T_k N_k words in all)
    long long c_at;      // c at c_buf + c_at (T_k words)
    long long res_at;    // mant / exp2 / status of sequence s_lo at index res_at (S_k slots)
    long long acc_at;    // acc_words(N, M) count words at acc + acc_at
    long long param_at;  // pi | A | B at params + param_at (md's pointers, writable)
};
// Grid-batched E-step of the models of ONE N <= WAVE_N (LDS is sized by it): nblocks workgroups, blocks[3 g .. 3 g + 2] =
// (model, workgroup index within the model, workgroup count of the model; fb_class_workgroups(S_k) of them)
void launch_fb_grid(const GridModelDev* models, int N, const int* blocks, int nblocks, const unsigned short* sym,
                    const long long* offs, double* alpha_buf, double* c_buf, long long* acc, double* mant, long long* exp2,
                    int* status, hipStream_t st);
// Grid-batched M-step of the n_active models listed in `active`; max_P / max_N: the largest N + N^2 + N M and N among them
void launch_reestimate_grid(const GridModelDev* models, const int* active, int n_active, long long max_P, int max_N,
                            const long long* acc, double epsilon, double* params, hipStream_t st);

// Viterbi decoding (hmm_viterbi.hip) of S sequences under one model given as logarithms (lm.pi / lm.A / lm.B hold
// lpi, lA, lB; -inf where the probability is 0).  Out at [s]: logp = ln P*, status (0 ok, 1 logp = -inf, 2 symbol >= M),
// and with psi: qlast[s] = q_{T-1} and psi_t[j] (u16) at psi[(offs[s] - psi0 + t) * N + j], t >= 1.  psi null: neither
// (the kernels without the path).  offs: S+1 symbol offsets.
void launch_viterbi(const ModelDev& lm, const unsigned short* sym, const long long* offs, int S, long long psi0,
                    unsigned short* psi, double* logp, int* qlast, int* status, hipStream_t st);
// the path of each of the S sequences from psi / qlast / status of launch_viterbi (a launch of its own, on the same
// stream): path[offs[s] + t] = q_t, every entry 0xFFFF when status is 2
void launch_backtrack(int N, const long long* offs, int S, long long psi0, const unsigned short* psi, const int* qlast,
                      const int* status, unsigned short* path, hipStream_t st);

// Joint Viterbi over all class models (hmm_segment.hip).  The classes are packed in class order into
// wave-slots of 64 lanes, class k on N_k consecutive lanes of one slot; the composite index of (k, j) is sum_{k' < k} N_k' + j.
constexpr int SEG_MAX_N = 64;               // states of one class: a class never straddles a wave
constexpr int SEG_MAX_SUM_N = 4096;         // states of all classes
constexpr int SEG_MAX_WAVES = 16;           // waves of a workgroup: up to here a wave per slot (the resident body)
constexpr size_t SEG_LDS_BYTES = 160 * 1024;  // lA of all classes lives in LDS when it fits next to the rest
struct SegLaneDev {  // one lane of one slot; a lane without a state: cls = -1, j = N = a_at = 0, seg = its own lane
    int cls, j, N;
    int seg;   // the lane of state 0 of the class
    int comp;  // composite index
    int a_at;  // lA of the class at this many doubles into the lA area
};
struct SegPlanDev {
    int K, M, sumN, slots;
    int a_words;                      // sum_k N_k^2
    const SegLaneDev* lanes;          // [slots][64]
    const int* slot_info;             // [slots][2]: the largest N of the slot, 1 when the slot holds one class
    const double* params;             // lpi of every class (sumN) | lA of every class (a_words) | lB (sumN rows of M)
    const unsigned short* comp_cls;   // [sumN]: composite index -> class
    const int* cls_comp0;             // [K]: class -> composite index of its state 0
};
// S streams (a workgroup each) from offs[0] on; psi ((frames of the launch) x sumN u16) and gsel (frames of the launch) are
// indexed relative to psi0 = the first stream's offset, gbest by the absolute frame; logp / qlast (composite index of
// q_{T-1}) / status at [s].  looped: the body that takes any number of slots.  Returns 1 when the shape cannot be launched.
int launch_segment(const SegPlanDev& pl, bool looped, const unsigned short* sym, const long long* offs, int S, long long psi0,
                   double ln_switch, unsigned short* psi, int* gsel, double* gbest, double* logp, int* qlast, int* status,
                   hipStream_t st);
// cls / state / entered of each of the S streams (absolute frames) from what launch_segment left; a stream of status 2
// gets 0xFFFF, 0xFFFF, 0 and gbest = -inf from its frame 1 on
void launch_segment_backtrack(const SegPlanDev& pl, const long long* offs, int S, long long psi0, const unsigned short* psi,
                              const int* gsel, const int* qlast, const int* status, unsigned short* cls, unsigned short* state,
                              unsigned char* entered, double* gbest, hipStream_t st);

// The same joint Viterbi under a K x K matrix of class-to-class prices (hmm_segment_trans.hip), on the
// packing above with at most SEG_MAX_WAVES slots; pl.params as launch_segment takes them.  ltT: the K x K prices
// transposed, ltT[k * K + f] = lt[f][k].  The tables psi (sumN u16 a frame), src and xs (K u16 a frame) and Es (K doubles a
// frame) are indexed relative to psi0 = the first stream's offset; logp / qlast / status at [s].  Returns 1 when the
// shape cannot be launched.  segment_trans_layout: whether lA, and then ltT, live in LDS (the instantiation).
void segment_trans_layout(const SegPlanDev& pl, bool* a_lds, bool* lt_lds);
int launch_segment_trans(const SegPlanDev& pl, const unsigned short* sym, const long long* offs, int S, long long psi0,
                         const double* ltT, unsigned short* psi, unsigned short* src, unsigned short* xs, double* Es, double* logp,
                         int* qlast, int* status, hipStream_t st);
// cls / state / entered / exit_score of each of the S streams (absolute frames) from what launch_segment_trans left; a
// stream of status 2 gets 0xFFFF, 0xFFFF, 0 and exit_score = -inf from its frame 1 on
void launch_segment_trans_backtrack(const SegPlanDev& pl, const long long* offs, int S, long long psi0, const unsigned short* psi,
                                    const unsigned short* src, const unsigned short* xs, const double* Es, const int* qlast,
                                    const int* status, unsigned short* cls, unsigned short* state, unsigned char* entered,
                                    double* exit_score, hipStream_t st);
// The looped body of the same decode (hmm_segment_trans_looped.hip): min(slots, SEG_MAX_WAVES) waves, a wave
// serves the slots w, w + waves, .. in turn; any number of slots.  Arguments, tables and results are launch_segment_trans's,
// bit for bit, and launch_segment_trans_backtrack reads them.  Dynamic LDS: 16 SEG_MAX_WAVES + 16 K + 20 sumN bytes are
// mandatory (the pairs, E of two frames, d / best / arg per state); lA, and then ltT, go behind them while the sum stays
// within SEG_LDS_BYTES (segment_trans_looped_layout: the instantiation).  Returns 1 when the shape cannot be launched.
size_t segment_trans_looped_lds_bytes(const SegPlanDev& pl, bool a_lds, bool lt_lds);
void segment_trans_looped_layout(const SegPlanDev& pl, bool* a_lds, bool* lt_lds);
int launch_segment_trans_looped(const SegPlanDev& pl, const unsigned short* sym, const long long* offs, int S, long long psi0,
                                const double* ltT, unsigned short* psi, unsigned short* src, unsigned short* xs, double* Es,
                                double* logp, int* qlast, int* status, hipStream_t st);

// Forced alignment to a known order of units (hmm_align.hip).  The units of one stream's transcript are
// packed in unit order into wave-slots as the classes are above (unit l on N_{c_l} consecutive lanes of one slot; composite
// index = the states of the units before it + j); the parameters stay per class: pl.params holds lpi (sumN of the classes) |
// lA of every class (a_words) | lB (a row of M per class state), as launch_segment takes them.
constexpr unsigned char ALIGN_ENTER_1 = 0xFE;  // psi: entered from the unit before
constexpr unsigned char ALIGN_ENTER_2 = 0xFF;  // psi: entered from two units before, over an optional one
constexpr int ALIGN_INIT = 1;   // lane flags: the unit may hold frame 0
constexpr int ALIGN_PRED = 2;   //             the unit has a predecessor (l >= 1)
constexpr int ALIGN_SKIP = 4;   //             the unit may be entered from l - 2 (l >= 2 and unit l - 1 is optional)
constexpr int ALIGN_FINAL = 8;  //             the unit may hold the last frame
struct AlignLaneDev {  // one lane of one slot; a lane without a state: unit = -1, j = N = row = a_at = flags = 0, seg = its own lane
    int unit, j, N;
    int seg;    // the lane of state 0 of the unit
    int comp;   // composite index within the stream
    int row;    // the state's row in the classes' lpi and lB
    int a_at;   // lA of the unit's class at this many doubles into the lA area
    int flags;
};
struct AlignStreamDev {  // one stream of a launch
    long long lane_at;  // its lanes at lanes + lane_at ([slots][64]), its slot_info at slot_info + lane_at / 32
    long long tab_at;   // its tables at tab + tab_at: psi (T x sumN bytes), then xs (T x L bytes)
    long long unit_at;  // its units at [unit_at, unit_at + L) of begin / end / unit_comp0
    long long comp_at;  // its states at [comp_at, comp_at + sumN) of comp_unit
    int slots, L, sumN, pad;
};
struct AlignPlanDev {
    int M, sumN_cls, a_words, max_L, max_sumN;  // max_*: the largest among the launch's streams (they size the LDS)
    const AlignStreamDev* streams;       // [S] of the launch
    const AlignLaneDev* lanes;
    const int* slot_info;                // per slot: the largest N of the slot, 1 when the slot holds one unit
    const double* params;
    const unsigned short* comp_unit;     // composite index -> unit
    const int* unit_comp0;               // unit -> composite index of its state 0
};
// dynamic LDS of k_hmm_align for such a launch
size_t align_lds_bytes(int max_L, int max_sumN, int a_words, bool looped, bool a_lds);
// whether a stream of L units and sumN states can be launched at all (lA left in global memory)
inline bool align_fits_lds(int L, int sumN, bool looped) { return align_lds_bytes(L, sumN, 0, looped, false) <= SEG_LDS_BYTES; }
// S streams (a workgroup of `waves` waves each) from offs[0] on; logp / qlast (composite index of q_{T-1}) / status at [s].
// looped: the body that takes any number of slots; else waves >= the most slots of a stream.  Returns 1 when the shape cannot
// be launched.
int launch_align(const AlignPlanDev& pl, bool looped, int waves, const unsigned short* sym, const long long* offs, int S,
                 double ln_switch, unsigned char* tab, double* logp, int* qlast, int* status, hipStream_t st);
// unit / state / entered of each of the S streams (absolute frames) and begin / end of its units from what launch_align
// left; a stream of status 2 gets 0xFFFF, 0xFFFF, 0, and -1 / -1 for every unit
void launch_align_backtrack(const AlignPlanDev& pl, const long long* offs, int S, const unsigned char* tab, const int* qlast,
                            const int* status, unsigned short* unit, unsigned short* state, unsigned char* entered,
                            long long* begin, long long* end, hipStream_t st);

// Embedded Baum-Welch over the same chain of units (hmm_embed.hip), on k_hmm_align's packing of every
// stream with at most SEG_MAX_WAVES slots.  The lanes carry three more flags; the parameters and the accumulators are per class.
constexpr int EMBED_FIRST = 16;  // lane flags: the unit is the first of its class in the stream
constexpr int EMBED_SUCC = 32;   //             the unit has a successor (l + 1 < L)
constexpr int EMBED_SUCC2 = 64;  //             the unit may be left for l + 2 (l + 2 < L and unit l + 1 is optional)
struct EmbedClassDev {
    int N;
    int a_at;            // A of the class at this many doubles into the A area (leading dimension N | 1)
    long long acc_at;    // its acc_words(N, M) count words at acc + acc_at
    long long param_at;  // its dense pi | A | B at this many doubles into the M-step's parameter block
};
struct EmbedPlanDev {
    int K, M, sumN_cls, a_words, max_L;  // a_words: sum_k N_k (N_k | 1); max_L: the most units of a stream of the call
    const AlignStreamDev* streams;       // [S] of the launch (tab_at unused)
    const AlignLaneDev* lanes;
    const int* slot_info;
    const double* params;                // pi (sumN_cls) | e = sw pi (sumN_cls) | A (a_words) | B (sumN_cls rows of M)
    const EmbedClassDev* classes;        // [K]
    const unsigned short* row_cls;       // [sumN_cls]: a class state's row -> its class
};
// dynamic LDS of k_hmm_embed_fb: the partial sums, V / R, A (a_lds) and the AN limb table (an_lds)
size_t embed_lds_bytes(int max_L, int a_words, bool a_lds, bool an_lds);
// S streams (a workgroup of `waves` waves each, at least the most slots of a stream) from offs[0] on.  The scratch of a stream
// starts at scr + (its offset - a0) * row_words and takes T (2 sumN + slots) doubles; the counts are added to acc (zeroed by the
// caller), P(O, transcript) = mant 2^exp2 and status at [s].  Returns 1 when the shape cannot be launched.
int launch_embed_fb(const EmbedPlanDev& pl, bool a_lds, bool an_lds, int waves, const unsigned short* sym, const long long* offs, int S,
                    long long a0, long long row_words, double* scr, long long* acc, double* mant, long long* exp2, int* status,
                    hipStream_t st);
// The looped body of the same pass (hmm_embed_looped.hip): streams of any number of slots, a workgroup of min(max_slots, 16)
// waves each; the same counts, P and status bit for bit.  pl.max_L, max_slots and max_sumN are the largest of the launch's
// streams.  Dynamic LDS: 2 x max_slots partial sums, V / R, two per-state arrays of max_sumN doubles, A (a_lds) and the AN
// limb table (an_lds); the first three are mandatory.
size_t embed_looped_lds_bytes(int max_L, int max_slots, int max_sumN, int a_words, bool a_lds, bool an_lds);
// as launch_embed_fb; the scratch of a stream takes T (2 sumN + 1) doubles of its T row_words.  Returns 1 when the shape
// cannot be launched.
int launch_embed_fb_looped(const EmbedPlanDev& pl, bool a_lds, bool an_lds, int max_slots, int max_sumN, const unsigned short* sym,
                           const long long* offs, int S, long long a0, long long row_words, double* scr, long long* acc, double* mant,
                           long long* exp2, int* status, hipStream_t st);
// AD of every class from its AN, once every stream's counts are in
void launch_embed_rowsum(const EmbedClassDev* classes, int K, int max_N, long long* acc, hipStream_t st);
// M-step of all K classes on their dense blocks (+ the floor at epsilon of B when epsilon > 0), in place; max_P / max_N: the
// largest N + N^2 + N M and N among them
void launch_reestimate_embedded(const EmbedClassDev* classes, int K, int M, long long max_P, int max_N, const long long* acc,
                                double epsilon, double* params, hipStream_t st);

// How sure the alignment is (hmm_align_posterior.hip): the E-step's forward-backward over the same plan
// (of pl.classes only a_at is read), with the occupancy and the entry mass kept per unit and per frame.  Every output is
// zeroed by the caller: a stream of status != 0 writes none.
struct AlignPostDev {
    const unsigned short* path_unit;  // per frame (absolute), the decoded path's unit; may be null
    const long long* ref;             // per unit (absolute), the reference frame of the moments; may be null = 0
    const long long* occ_at;          // [S] of the launch: where the stream's T x L occupancies begin in occ
    double* occ;                      // may be null
    double* post_path;                // per frame (absolute)
    double* w;                        // w0 | w1 | w2, `units` doubles each, per unit (absolute)
    long long units;
};
// dynamic LDS of k_hmm_align_posteriors: the partial sums, V / R and A (a_lds)
size_t align_post_lds_bytes(int max_L, int a_words, bool a_lds);
// S streams from offs[0] on, as launch_embed_fb takes them (the scratch too).  Returns 1 when the shape cannot be launched.
int launch_align_posteriors(const EmbedPlanDev& pl, bool a_lds, int waves, const unsigned short* sym, const long long* offs, int S,
                            long long a0, long long row_words, double* scr, const AlignPostDev& out, double* mant, long long* exp2,
                            int* status, hipStream_t st);
// The looped body of the same pass (hmm_align_posterior_looped.hip): streams of any number of slots, a workgroup of
// min(max_slots, 16) waves each; the same outputs, P and status bit for bit.  pl.max_L, max_slots and max_sumN are the largest
// of the launch's streams.  Dynamic LDS: embed_looped_lds_bytes' mandatory part (the partial sums, V / R, two per-state arrays
// of max_sumN doubles), the three per-unit sums (3 x max_L doubles, mandatory too) and A (a_lds).
size_t align_post_looped_lds_bytes(int max_L, int max_slots, int max_sumN, int a_words, bool a_lds);
// as launch_embed_fb_looped takes them (the scratch too).  Returns 1 when the shape cannot be launched.
int launch_align_posteriors_looped(const EmbedPlanDev& pl, bool a_lds, int max_slots, int max_sumN, const unsigned short* sym,
                                   const long long* offs, int S, long long a0, long long row_words, double* scr,
                                   const AlignPostDev& out, double* mant, long long* exp2, int* status, hipStream_t st);

// Smoothed class posteriors under the same class loop (hmm_posterior.hip), on the packing above with at
// most SEG_MAX_WAVES slots.  pl.params here: pi (sumN) | e = sw pi (sumN) | A of every class with the leading dimension
// N_k | 1 (lanes[].a_at and a_words count these padded words) | B (sumN rows of M).  S streams (a workgroup each) from
// offs[0] on; the scratch tables ahs ((frames of the launch) x sumN doubles) and cs ((frames of the launch) x slots) are
// indexed relative to a0 = the first stream's offset, post (K doubles a frame) by the absolute frame; P(O | loop) =
// mant 2^exp2 and status at [s].  Returns 1 when the shape cannot be launched.
bool posteriors_a_in_lds(const SegPlanDev& pl);
int launch_loop_posteriors(const SegPlanDev& pl, const unsigned short* sym, const long long* offs, int S, long long a0, double sw,
                           double* ahs, double* cs, double* post, double* mant, long long* exp2, int* status, hipStream_t st);
// The looped body of the same pass (hmm_posterior_looped.hip): any number of slots, a workgroup of min(slots, 16) waves per
// stream; the same post, P and status bit for bit.  The same plan, parameter block and tables, except that cs takes
// (frames of the launch) x min(slots, 16) doubles: a copy of c_t per wave.  Dynamic LDS: 8 (2 slots + sumN) bytes are mandatory
// (the partial sums of GS in both parities, and one double per composite state); A, 8 a_words bytes, goes behind them when
// the sum stays within SEG_LDS_BYTES (a_lds).  Returns 1 when the shape cannot be launched.
size_t posteriors_looped_lds_bytes(const SegPlanDev& pl, bool a_lds);
int launch_loop_posteriors_looped(const SegPlanDev& pl, const unsigned short* sym, const long long* offs, int S, long long a0, double sw,
                                  double* ahs, double* cs, double* post, double* mant, long long* exp2, int* status, hipStream_t st);

// The same posteriors under a K x K matrix of class-to-class prices (hmm_posterior_trans.hip), on the
// packing above with at most SEG_MAX_WAVES slots.  pl.params here: pi (sumN) | A with the leading dimension N_k | 1 | B.
// w: 2 K^2 doubles, w[f * K + k] = exp(lt[f][k]) followed by its transpose.  The tables and outputs are
// launch_loop_posteriors'.  Dynamic LDS: 8 (32 + 2 K + sumN) bytes are mandatory (the partial sums, the class masses of two
// steps, pi); A, and then both matrices, go behind them while the sum stays within SEG_LDS_BYTES (posteriors_trans_layout:
// the instantiation).  Returns 1 when the shape cannot be launched.
void posteriors_trans_layout(const SegPlanDev& pl, bool* a_lds, bool* w_lds);
int launch_loop_posteriors_trans(const SegPlanDev& pl, const unsigned short* sym, const long long* offs, int S, long long a0,
                                 const double* w, double* ahs, double* cs, double* post, double* mant, long long* exp2, int* status,
                                 hipStream_t st);
// The looped body of the same pass (hmm_posterior_trans_looped.hip, the frames in hmm_trans_fb_looped_step.h): any number of
// slots, a workgroup of min(slots, SEG_MAX_WAVES) waves per stream in which a wave serves the slots w, w + waves, .. in turn;
// the same post, P and status bit for bit.  The same plan, parameter block, w and tables, except that cs takes (frames of the
// launch) x min(slots, 16) doubles: a copy of c_t per wave.  Dynamic LDS: 8 (2 slots + 2 K + sumN) bytes are mandatory (the
// partial sums in both parities, the class masses of two steps, one double per composite state; pi is read in place); A, and
// then both matrices, go behind them while the sum stays within SEG_LDS_BYTES (posteriors_trans_looped_layout: the
// instantiation).  Returns 1 when the shape cannot be launched.
size_t posteriors_trans_looped_lds_bytes(const SegPlanDev& pl, bool a_lds, bool w_lds);
void posteriors_trans_looped_layout(const SegPlanDev& pl, bool* a_lds, bool* w_lds);
int launch_loop_posteriors_trans_looped(const SegPlanDev& pl, const unsigned short* sym, const long long* offs, int S, long long a0,
                                        const double* w, double* ahs, double* cs, double* post, double* mant, long long* exp2,
                                        int* status, hipStream_t st);

// The expected class-to-class counts under the same loop and prices (hmm_trans_estep.hip): the E-step of
// `hmm transitions --em`.  pl, w, the scratch tables and mant / exp2 / status are launch_loop_posteriors_trans'.  acc:
// 2 K^2 + 2 int64, added to: the limb pair of C[f][k] at 2 (f K + k), then the status-0 streams and the others.  Dynamic LDS:
// the mandatory terms of 4.8.13; behind them the C table (16 K^2 bytes) when it fits -- or as c_forced says: *c_lds is then
// the caller's -- then A, then both matrices, while the sum stays within SEG_LDS_BYTES (trans_estep_layout).  Returns 1 when
// the shape cannot be launched.
size_t trans_estep_lds_bytes(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds);
void trans_estep_layout(const SegPlanDev& pl, bool c_forced, bool* c_lds, bool* a_lds, bool* w_lds);
int launch_trans_estep(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds, const unsigned short* sym, const long long* offs,
                       int S, long long a0, const double* w, double* ahs, double* cs, long long* acc, double* mant, long long* exp2,
                       int* status, hipStream_t st);
// The looped body of the same E-step (hmm_trans_estep_looped.hip): any number of slots, the workgroup and the cs table of
// launch_loop_posteriors_trans_looped; the same acc (every limb and both counters), P and status bit for bit.  Dynamic LDS:
// 8 (2 slots + 2 K + 2 sumN) bytes are mandatory (the looped posteriors' terms and S_t per composite state); behind them, in
// trans_estep_layout's order and with its c_forced, the C table, A, then both matrices (trans_estep_looped_layout).  Returns 1
// when the shape cannot be launched.
size_t trans_estep_looped_lds_bytes(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds);
void trans_estep_looped_layout(const SegPlanDev& pl, bool c_forced, bool* c_lds, bool* a_lds, bool* w_lds);
int launch_trans_estep_looped(const SegPlanDev& pl, bool c_lds, bool a_lds, bool w_lds, const unsigned short* sym,
                              const long long* offs, int S, long long a0, const double* w, double* ahs, double* cs, long long* acc,
                              double* mant, long long* exp2, int* status, hipStream_t st);

// The expected state-level counts of every class under the same loop and prices (hmm_loop_estep.hip): the
// E-step of `hmm learn --loop`.  pl, w, ahs / cs and mant / exp2 / status are launch_loop_posteriors_trans'; ms: K doubles a
// frame more, the mass that entered each class (indexed as ahs).  classes: N, a_at (leading dimension N | 1) and acc_at of every
// class; acc: their acc_words(N, M) blocks, added to (AD is launch_embed_rowsum's).  acc_trans: null, or launch_trans_estep's
// 2 K^2 + 2 words, added to.  Dynamic LDS: the mandatory terms of 4.8.13; behind them, in this order and while the sum stays
// within SEG_LDS_BYTES, the AN table of all classes (16 a_words bytes), the C table (16 K^2 bytes; with acc_trans only), A, then
// both matrices (loop_estep_layout; an_forced / c_forced: *an_lds / *c_lds are the caller's).  Returns 1 when the shape cannot
// be launched.
size_t loop_estep_lds_bytes(const SegPlanDev& pl, bool an_lds, bool c_lds, bool a_lds, bool w_lds);
void loop_estep_layout(const SegPlanDev& pl, bool gram, bool an_forced, bool c_forced, bool* an_lds, bool* c_lds, bool* a_lds,
                       bool* w_lds);
int launch_loop_estep(const SegPlanDev& pl, const EmbedClassDev* classes, bool an_lds, bool c_lds, bool a_lds, bool w_lds,
                      const unsigned short* sym, const long long* offs, int S, long long a0, const double* w, double* ahs, double* cs,
                      double* ms, long long* acc, long long* acc_trans, double* mant, long long* exp2, int* status, hipStream_t st);

}  // namespace e2hmm
