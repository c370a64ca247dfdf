/*
 * ecoz2_classify.h -- C-ABI of the consumers of the VQ path's output in libecoz2vq.so:
 * the symbol-sequence classifiers that read the `.seq` files `ecoz2 vq quantize` writes, and the HMM path that
 * quantises `.prd` files on the fly (`hmm classify --predictors --codebooks`).
 *
 * Part A (nb / mm / c12n) restates host code that IS present in the reference as Rust; each entry point cites the
 * function it mirrors.  These are host-side (CPU) in the reference and stay host-side here: they are O(symbols) table
 * look-ups over the GPU path's output, with the reference's exact arithmetic (f64 for nb, f32 for mm, libm log10).
 * Part B (hmm) replaces the reference's FFI symbols for the HMM commands (src/ecoz2_lib/mod.rs:134-167); the arithmetic
 * behind them lives in the absent C submodule, so its definitions are this repo's; scoring and training
 * run in HIP kernels, with no CPU fallback.
 *
 * Plain pointers and sizes only.  Every function returns 0 on success; on failure a message is on stderr and in
 * e2vq_last_error().
 */
#ifndef ECOZ2_CLASSIFY_H
#define ECOZ2_CLASSIFY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- .seq reader: sequence::load, src/sequence/mod.rs:49-75 ------------------------------------------------- */
int e2vq_seq_info(const char *path, char class_name[96], int *M, int64_t *T);
int e2vq_seq_read(const char *path, uint16_t *sym, int64_t capacity);

/* =========================================================================================
 * Part A -- nb / mm / c12n (pure Rust in the reference)
 * ======================================================================================= */

/* nbayes::learn (src/nb/nbayes.rs:63-114) + main_nbayes_learn (src/nb/mod.rs:99-128): symbol frequencies of the
 * given sequences -> CBOR model `<out_root>/data/nbs/M<M>/<class>.nb` (utl::save_ser, src/utl/mod.rs:263-268).
 * out_path (optional, may be NULL) receives the file name written. */
int ecoz2_nb_learn(int codebook_size, const char *const *seq_filenames, int num_sequences, char *out_path,
                   int out_path_cap);
/* nbayes::classify (src/nb/nbayes.rs:116-153): log10-probability of every sequence under every model (m-estimate,
 * f64, summed in symbol order), c12n report on stdout, `nb_<M>_classification.json` / `nb_<M>_y_true_pred.json`. */
int ecoz2_nb_classify(const char *const *nb_filenames, int num_models, const char *const *seq_filenames,
                      int num_sequences, int show_ranked, int codebook_size);
/* NBayes::show (src/nb/nbayes.rs:21-35) */
int ecoz2_nb_show(const char *nb_filename);
/* NBayes::log_prob_sequence (src/nb/nbayes.rs:50-54) of one sequence file under one model file */
int e2vq_nb_log_prob(const char *nb_filename, const char *seq_filename, double *log_prob);

/* markov::learn (src/mm/markov.rs:59-126) + main_mm_learn (src/mm/mod.rs:99-128): first-order Markov model of the
 * symbol sequences (f32 counters with add-one smoothing) -> CBOR `<out_root>/data/mms/M<M>/<class>.mm`.
 * The row-stochastic asserts of markov.rs:117,122 are checked (failure = error). */
int ecoz2_mm_learn(int codebook_size, const char *const *seq_filenames, int num_sequences, char *out_path,
                   int out_path_cap);
/* markov::classify (src/mm/markov.rs:128-167) */
int ecoz2_mm_classify(const char *const *mm_filenames, int num_models, const char *const *seq_filenames,
                      int num_sequences, int show_ranked, int codebook_size);
/* MM::show (src/mm/markov.rs:27-40), asserts included */
int ecoz2_mm_show(const char *mm_filename);
/* MM::log_prob_sequence (src/mm/markov.rs:43-49): f32 */
int e2vq_mm_log_prob(const char *mm_filename, const char *seq_filename, float *log_prob);

/* C12nResults (src/c12n/mod.rs:8-223) driven directly: `probs` is num_cases x num_models (row-major), `class_ids`
 * the true model index of every case.  Prints exactly what add_case / report_results print and writes the two JSON
 * files `<out_base_name>_classification.json`, `<out_base_name>_y_true_pred.json`.  result / confusion (optional)
 * receive the (num_models+1)^2 tables. */
int e2vq_c12n_run(const char *const *model_class_names, int num_models, const int *class_ids,
                  const char *const *case_class_names, const char *const *case_titles, const double *probs,
                  int num_cases, int show_ranked, const char *out_base_name, int *result, int *confusion);

/* =========================================================================================
 * Part B -- hmm (the reference's FFI symbols; bodies in the absent C submodule -> definitions in DESIGN.md /
 *           oracle/hmm_oracle.h; parity unpinned)
 * ======================================================================================= */

/* replaces `fn ecoz2_set_random_seed(seed: c_long) -> c_ulong`          src/ecoz2_lib/mod.rs:75
 * seed < 0: time based (src/hmm/mod.rs:73-76).  Returns the seed in use.  Feeds the random model types of hmm learn. */
unsigned long ecoz2_set_random_seed(long seed);

/* `callback: extern "C" fn(*mut c_char, c_double)`                       src/ecoz2_lib/mod.rs:144
 * called once per E-step with ("sum_log_prob", sum over the training sequences of ln P(O | model)) */
typedef void (*ecoz2_hmm_learn_callback_t)(char *variable, double value);

/* replaces `fn ecoz2_hmm_learn(N, model_type, sequence_filenames, num_sequences: c_uint, hmm_epsilon, val_auto,
 *           max_iterations, use_par, callback)`                          src/ecoz2_lib/mod.rs:134-145
 * Baum-Welch over all the given `.seq` files of ONE class (class name and M from the first sequence): E-step on the
 * GPU (one wavefront per sequence, exact fixed-point expected counts), M-step on the GPU, until the increase of
 * sum ln P drops to val_auto or max_iterations (>= 0) E+M steps ran.  hmm_epsilon > 0 floors B and renormalises.
 * Writes data/hmms/N<N>__M<M>_t<type>__a<val_auto>[_I<max>]/<class>.hmm (+ .csv with the measure per iteration).
 * use_par is accepted and ignored.
 * Limits: 1 <= N <= 512 (up to 64 states one lane of a wavefront per state, beyond a workgroup per sequence with a thread
 * per state -- same arithmetic, slower; the reference's -N is free: larger N fail with a message).
 * An empty sequence is skipped by the training (no counts, not in the pi denominator) and scores P = 1 in classify.
 * ECOZ2_VQ_GPUS = W: the sequences are dealt to W workers (devices ECOZ2_VQ_DEVICE + w modulo the device count); the
 * exact int64 expected counts are summed over the workers each E-step, so the model is the single worker's bit for
 * bit; ecoz2_hmm_classify / ecoz2_hmm_classify_predictors deal the sequences / predictor files the same way. */
int ecoz2_hmm_learn(int N, int model_type, const char *const *sequence_filenames, unsigned num_sequences,
                    double hmm_epsilon, double val_auto, int max_iterations, int use_par,
                    ecoz2_hmm_learn_callback_t callback);

/* replaces `fn ecoz2_hmm_classify(model_filenames, num_models: c_uint, sequence_filenames, num_sequences: c_uint,
 *           show_ranked, classification_filename)`                       src/ecoz2_lib/mod.rs:147-154
 * ln P(O | model) of every sequence under every model (GPU, one wavefront per pair); report in the layout of
 * src/c12n/mod.rs; classification_filename (may be NULL): the CSV of CHANGELOG.md:273-284. */
int ecoz2_hmm_classify(const char *const *model_filenames, unsigned num_models,
                       const char *const *sequence_filenames, unsigned num_sequences, int show_ranked,
                       const char *classification_filename);

/* replaces `fn ecoz2_hmm_classify_predictors(model_filenames, num_models: c_uint, cb_filenames, num_codebooks: c_int,
 *           prd_filenames, num_predictors: c_int, show_ranked, classification_filename)`   src/ecoz2_lib/mod.rs:156-165
 * The on-the-fly consumer of the nearest-codeword kernel: every `.prd` is uploaded once, quantised on the GPU against
 * the codebook of each model (a single codebook serves all models; several are matched to the models by class name)
 * and scored where the symbols are. */
int ecoz2_hmm_classify_predictors(const char *const *model_filenames, unsigned num_models,
                                  const char *const *cb_filenames, int num_codebooks,
                                  const char *const *prd_filenames, int num_predictors, int show_ranked,
                                  const char *classification_filename);

/* replaces `fn ecoz2_hmm_show(hmm_filename, format)`                      src/ecoz2_lib/mod.rs:167
 * format: one printf floating-point conversion per value, default "%Lg " (src/hmm/mod.rs:153-154) */
int ecoz2_hmm_show(const char *hmm_filename, const char *format);

/* replaces the reference's commented-out `fn ecoz2_seq_show_files(with_prob, gen_q_opt, show_sequence, hmm_filename,
 *           sequence_filenames, num_sequences)`                         src/ecoz2_lib/mod.rs:169-177
 * `seq show -P / -Q --hmm`.  The third argument follows the reference's only caller (src/ecoz2_lib/mod.rs:518-523),
 * which passes `no_sequence` there: nonzero leaves out the symbol line of each file.  Per file, in argument order:
 * what `seq show` prints for it (unless no_sequence); with_prob: "  log_prob = %.17g", the forward ln P(O | model);
 * gen_q_opt: "  q_opt = <states>" (abbreviated as the symbol line) and "  q_opt_log_prob = %.17g", ln P* of the
 * Viterbi path.  A symbol >= M prints -inf, no q_opt line and a note naming the symbol; a file
 * whose M is not the model's gets one line saying so instead.  All files are loaded first, then decoded (and scored)
 * in one batched call each. */
int ecoz2_seq_show_files(int with_prob, int gen_q_opt, int no_sequence, const char *hmm_filename,
                         const char *const *sequence_filenames, int num_sequences);
/* the same with the `seq show` flags the reference's signature lacks: full (every symbol and state, `--full`) and
 * only_length (the length instead of the symbol line, `-L`); ecoz2_seq_show_files is this with both 0 */
int e2vq_seq_show_files(int with_prob, int gen_q_opt, int no_sequence, const char *hmm_filename,
                        const char *const *sequence_filenames, int num_sequences, int full, int only_length);

/* ---- array-level entry points over the same kernels (tests, Python mirror) ---------------------------------- */
/* initial model of `hmm learn -t`: 0 random, 1 uniform, 2 cascade-2, 3 cascade-3 (random B); uses the generator
 * seeded by ecoz2_set_random_seed.  pi[N], A[N*N], B[N*M]; N <= 512. */
int e2vq_hmm_init(int N, int M, int model_type, double *pi, double *A, double *B);
int e2vq_hmm_save(const char *path, const char *class_name, int N, int M, const double *pi, const double *A,
                  const double *B);
int e2vq_hmm_info(const char *path, char class_name[96], int *N, int *M);
int e2vq_hmm_load(const char *path, double *pi, double *A, double *B);
/* scaled forward pass of S sequences (concatenated u16 symbols + S+1 offsets) under K models sharing M; outputs at
 * [s*K + k]: P(O) = mant * 2^exp2 (mant in [0.5,1)), status (0 ok, 1 cannot emit, 2 symbol >= M), ln P */
int e2vq_hmm_score(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                   const double *const *Bs, const uint16_t *sym, const int64_t *offs, int S, double *mant,
                   int64_t *exp2, int *status, double *log_probs);
/* int64 words of the E-step accumulators: [hi, lo] limb pairs  PI[N] | AN[N][N] | AD[N] | BN[N][M] | BD[N] | used, skipped */
int64_t e2vq_hmm_acc_words(int N, int M);
int e2vq_hmm_estep(int device, int N, int M, const double *pi, const double *A, const double *B, const uint16_t *sym,
                   const int64_t *offs, int S, int64_t *acc, double *mant, int64_t *exp2, int *status);
/* the loop of ecoz2_hmm_learn on arrays, in place; sum_log_prob[0..*num_esteps) = the measure per E-step */
int e2vq_hmm_train(int device, int N, int M, double *pi, double *A, double *B, const uint16_t *sym,
                   const int64_t *offs, int S, double epsilon, double val_auto, int max_iterations,
                   double *sum_log_prob, int cap, int *num_esteps);

/* ---- every class's HMM in one batched training -------------------------------------------------
 * `hmm learn --all-classes`: one model per class name of the sequences' headers, classes in byte order of their names
 * (strcmp), each class's sequences in list order.  For every class c, ecoz2_set_random_seed(s) followed by this call
 * writes and prints byte for byte what ecoz2_set_random_seed(s); ecoz2_hmm_learn(N, model_type, <c's files in list
 * order>, ...) would: every class starts from the generator state of entry, and the generator is left where that single
 * call leaves it.  (With a seed < 0 all classes therefore share one time-based draw.)  A class stops as the single loop
 * does; the classes train together -- one E-step launch and one M-step launch per iteration over the classes still
 * going.  Stdout: the single call's block per class, in class order, after all training; the callback gets the classes'
 * ("sum_log_prob", L) class after class.  An empty list, N outside [1, 512], a model type outside 0..3, differing M or a
 * symbol >= M return 1 before any HIP call; no file is written unless every class trained.
 * The classes are the grid batch below with one (N, M): ECOZ2_HMM_LEARN_BATCH_BYTES (default 4 GiB) is the device bytes
 * one batch of classes may take for alpha^, c and the accumulators ((T_k (N + 1) + e2vq_hmm_acc_words(N, M)) * 8 per class)
 * and its symbols (2 T_k); classes are packed in order, greedily, a larger class alone.  ECOZ2_VQ_GPUS = W: whole classes
 * dealt to W workers in contiguous ranges balanced by those bytes.  Neither changes a byte of the output. */
int e2vq_hmm_learn_classes(int N, int model_type, const char *const *sequence_filenames, unsigned num_sequences,
                           double hmm_epsilon, double val_auto, int max_iterations,
                           void (*callback)(char *variable, double value));
/* the same training on arrays, in place: K classes, class k = sequences [class_offs[k], class_offs[k + 1]) (class_offs:
 * K + 1 entries, strictly increasing from 0 to S), model k at pi + k N, A + k N^2, B + k N M; its measure per E-step at
 * sum_log_prob[k cap ..], its E-step count at num_esteps[k].  Class k's result equals e2vq_hmm_train on its slice, bit
 * for bit.  One device; ECOZ2_HMM_LEARN_BATCH_BYTES applies. */
int e2vq_hmm_train_classes(int device, int N, int M, int K, double *pi, double *A, double *B, const uint16_t *sym,
                           const int64_t *offs, int S, const int64_t *class_offs, double epsilon, double val_auto,
                           int max_iterations, double *sum_log_prob, int cap, int *num_esteps);

/* ---- a grid of (N, M) points in one batched training -------------------------------------------
 * `hmm learn --grid`: one model per grid point (n, m, c) of Ns x {the M values of the sequences' headers} x {the classes
 * present at that M}; N ascending, M ascending, classes in strcmp order; model (n, m, c) trains on the files of class c
 * and codebook size m in list order.  For every grid point, ecoz2_set_random_seed(s) followed by this call writes and
 * prints byte for byte what ecoz2_set_random_seed(s); e2vq_hmm_learn_classes(n, model_type, <the files of M = m>, ...)
 * writes and prints for class c (.hmm, .csv, stdout block, callback values): every model starts from the generator state
 * of entry, and the generator is left where a seeded single call for the last model leaves it.  Stdout: the blocks in
 * grid order, after all training.  An empty list, an empty or duplicated N, N outside [1, 512], a model type outside 0..3
 * or a symbol >= its file's M return 1 before any HIP call, and no file is written unless every model trained.
 * ECOZ2_HMM_LEARN_BATCH_BYTES packs models greedily in grid order, a model counting (T_k (N_k + 1) + W_k) * 8 bytes
 * (W_k = e2vq_hmm_acc_words(N_k, M_k)) and the symbols of a (class, M) counted once per batch; ECOZ2_VQ_GPUS deals whole
 * models to devices.  Neither changes a byte of the output. */
int e2vq_hmm_learn_grid(const int *Ns, int num_N, int model_type, const char *const *sequence_filenames,
                        unsigned num_sequences, double hmm_epsilon, double val_auto, int max_iterations,
                        void (*callback)(char *variable, double value));
/* the same training on arrays, in place: K models, model k with Ns[k] states and Ms[k] symbols, trained on the sequences
 * [seq_lo[k], seq_hi[k]) of offs (non-empty; ranges of different models may overlap, the symbols go to the device once),
 * its pi | A | B (Ns[k] + Ns[k]^2 + Ns[k] Ms[k] doubles) at params + param_offs[k] (blocks may not overlap); its measure
 * per E-step at sum_log_prob[k cap ..], its E-step count at num_esteps[k].  Model k's result equals e2vq_hmm_train on its
 * slice, bit for bit.  Bad ranges, overlapping parameter blocks and symbols >= M_k are refused before the device.  One
 * device; ECOZ2_HMM_LEARN_BATCH_BYTES applies. */
int e2vq_hmm_train_grid(int device, int K, const int *Ns, const int *Ms, double *params, const int64_t *param_offs,
                        const uint16_t *sym, const int64_t *offs, int S, const int64_t *seq_lo, const int64_t *seq_hi,
                        double epsilon, double val_auto, int max_iterations, double *sum_log_prob, int cap,
                        int *num_esteps);

/* ---- classification at every (N, M) point of a sweep in one batched scoring -----------------------
 * `hmm classify --grid`: a grid point is an (N, M) for which at least one model is given; points in order of N, then M.
 * A point's models are the given .hmm files with that header, in list order; its sequences the given .seq files with
 * header M, in list order.  Every sequence is scored under every model of every point in one batch (k_hmm_score_grid:
 * floor(64 / N) models of a point to a wave for N <= 21); each score is ecoz2_hmm_classify's bit for bit.  Stdout:
 * per point the line "grid point: N=<n> M=<m>" followed byte for byte by what ecoz2_hmm_classify(<the point's models>,
 * <the point's sequences>, show_ranked, <dir>/N<n>__M<m>.csv) prints, then a block "grid summary: <points> point(s)"
 * with one line per point: N, M, models, sequences classified, accuracy and avg_accuracy (%.2f).  classification_dir
 * (may be NULL): each point's CSV as <dir>/N<n>__M<m>.csv, the bytes ecoz2_hmm_classify writes.  summary_filename (may
 * be NULL): a CSV "N,M,models,sequences,accuracy,avg_accuracy" with one row per point (%.9g for the two floats).
 * An empty model or sequence list, a class name that occurs twice among a point's models, a point with no sequence of its
 * M and a sequence whose M no model has return 1 before any HIP call, and no file is written.  ECOZ2_VQ_GPUS = W deals
 * each point's sequences to W workers in contiguous shares; it changes no byte. */
int e2vq_hmm_classify_grid(const char *const *model_filenames, unsigned num_models,
                           const char *const *sequence_filenames, unsigned num_sequences, int show_ranked,
                           const char *classification_dir, const char *summary_filename);
/* the same scoring on arrays: K models, model k with Ns[k] states and Ms[k] symbols, its pi | A | B at
 * params + param_offs[k], scored on the sequences [seq_lo[k], seq_hi[k]) of offs (non-empty; ranges may overlap, the
 * symbols go to the device once).  The result of sequence s under model k is at index out_offs[k] + (s - seq_lo[k]) of
 * mant / exp2 / status (each may be NULL) and log_probs; the output ranges may not overlap.  Consecutive models of equal
 * (N, M, range) are scored together.  Each result equals e2vq_hmm_score's for that pair, bit for bit.  K < 1, an N or M
 * out of range, a bad sequence range and overlapping output ranges are refused before the device; a symbol >= M_k is
 * not: it scores status 2. */
int e2vq_hmm_score_grid(int device, int K, const int *Ns, const int *Ms, const double *params, const int64_t *param_offs,
                        const uint16_t *sym, const int64_t *offs, int S, const int64_t *seq_lo, const int64_t *seq_hi,
                        const int64_t *out_offs, double *mant, int64_t *exp2, int *status, double *log_probs);

/* ---- the trained models over whole recordings -------------------------------------------------------
 * `hmm scan`: windows of window_frames symbols every hop_frames symbols over each of S streams (concatenated u16 symbols +
 * S+1 offsets).  Stream s of T_s symbols has W_s = (T_s - L) / H + 1 windows when T_s >= L, else none: a trailing incomplete
 * window is dropped; window i starts at frame i H.  win_offs (S+1 entries, may be NULL): the windows of stream s are
 * [win_offs[s], win_offs[s+1]).  Outputs, each may be NULL: the matrix at [w*K + k] in the layout of e2vq_hmm_score (mant,
 * exp2, status, ln P) -- every value bit for bit what e2vq_hmm_score returns for that window's symbols passed as a sequence
 * of its own, a symbol >= M scoring status 2 in exactly the windows that contain it -- and per window the best and the
 * second-best model with their ln P, ranked as `hmm classify` ranks (by P = mant 2^exp2; among equal scores the model given
 * later first; second = -1 and -inf when K = 1).  Without the matrix outputs only the two results per window leave the
 * device.  The symbols are staged once per run of overlapping windows (k_hmm_scan), never materialised per window.
 * sym_on_device: `sym` is a device pointer on `device` (offs stays a host pointer).
 * L < 1, H < 1, K < 1 and an N outside [1, 512] are refused before any HIP call.
 * By default floor(64 / N) windows share a wave for N <= 21.  ECOZ2_HMM_SCAN_PACK = 0 / 1: one window per wave / floor(64 / N) windows per wave (N <= 32) whatever N; the bits are the
 * same.  e2vq_hmm_scan_windows: the window arithmetic alone (host only). */
int e2vq_hmm_scan_windows(const int64_t *offs, int S, int64_t window_frames, int64_t hop_frames, int64_t *win_offs);
int e2vq_hmm_scan(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                  const double *const *Bs, const void *sym, const int64_t *offs, int S, int64_t window_frames,
                  int64_t hop_frames, int64_t *win_offs, double *mant, int64_t *exp2, int *status, double *log_probs,
                  int *best, double *best_log_prob, int *second, double *second_log_prob, int sym_on_device);
/* HIP-event time of the kernels (scan + top-2) of this thread's last scan (-1: none yet) */
int e2vq_hmm_scan_last_kernel_ms(float *ms);
/* The file form.  Each input is a .wav (lpc with P, W_ms, O_ms -> quantize with the codebook -> scan), a .prd (quantize ->
 * scan) or a .seq (scan; no codebook needed); each is read and uploaded once, and frames and symbols stay on the device
 * between the stages (DESIGN.md 4.8.5 names the one exception).  Per input a block on stdout (name, T, windows; windows won
 * per class; the maximal runs of consecutive windows won by one class with margin ln P1 - ln P2 >= min_margin as
 * "begin_s - end_s class") and, with csv_dir_or_file, a CSV -- <dir>/<input's base name>.csv, or the named file when there
 * is one input and the name ends in .csv -- with the header
 *   window,begin_frame,end_frame,begin_s,end_s,class,log_prob,second_class,second_log_prob
 * end_frame is exclusive; begin_s = begin_frame O_ms / 1000; end_s = ((end_frame - 1) O_ms + W_ms) / 1000, the end of the
 * last frame's analysis window (.prd and .seq inputs: the W_ms / O_ms given); floats as %.17g; a class is empty where no
 * model can emit the window.  No models, no inputs, L < 1, H < 1, models of differing M, a codebook whose M differs from
 * the models' or whose P differs from a .prd's or from P (signals), a .seq of another M, signals or predictors without a
 * codebook and two inputs of one CSV name return 1 before any HIP call, and no file is written. */
int e2vq_hmm_scan_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                        const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms, int64_t window_frames,
                        int64_t hop_frames, double min_margin, const char *csv_dir_or_file);
/* CSV and stdout block of one scanned input from its two results per window (host only; what e2vq_hmm_scan_files calls) */
int e2vq_hmm_scan_report(const char *name, int64_t T, int K, const char *const *class_names, int64_t W, int64_t window_frames,
                         int64_t hop_frames, int W_ms, int O_ms, const int *best, const double *best_log_prob, const int *second,
                         const double *second_log_prob, double min_margin, const char *csv_filename);

/* Viterbi decoding of S sequences under one model: logarithms of the parameters taken on the host
 * (log 0 = -inf; a negative, NaN or infinite parameter is refused), maximisation on the GPU.  log_prob[s] = ln P*,
 * status[s]: 0 ok, 1 ln P* = -inf (the model cannot emit the sequence; the path is still written), 2 a symbol >= M
 * (ln P* = -inf, every path entry 0xFFFF).  path (may be NULL): offs[S] entries, q_t of sequence s at offs[s] + t.
 * ECOZ2_HMM_VITERBI_CHUNK_BYTES bounds the per-launch back-pointer table (default 256 MiB, whole sequences). */
int e2vq_hmm_viterbi(int device, int N, int M, const double *pi, const double *A, const double *B, const uint16_t *sym,
                     const int64_t *offs, int S, uint16_t *path, double *log_prob, int *status);

/* ---- segmentation by joint Viterbi over all class models -----------------------------------------------
 * `hmm segment`: each of S streams (concatenated u16 symbols + S+1 offsets, the layout of e2vq_hmm_scan) is decoded once
 * under the class loop of K models sharing M: the models side by side; a path may leave the class it is in at any frame and
 * enter any class -- the same one included -- through that class's pi, at the price ln_switch <= 0 (the logarithm of the
 * price of starting a segment; -inf forbids it).  Logarithms of the parameters are taken on the host exactly as
 * e2vq_hmm_viterbi takes them; the device adds and compares.  With d_0[k][j] = lpi_k[j] + lB_k[j][o_0], and for t >= 1
 * G_t = max d_{t-1} reached first by g_t in (class, state) order: per state the in-class maximum of e2vq_hmm_viterbi (ties
 * to the lowest state), then x = (G_t + ln_switch) + lpi_k[j] replaces it when strictly greater (ENTER; a tie stays in the
 * class), then + lB_k[j][o_t].  ln P* = max d_{T-1}, q_{T-1} the lowest (class, state) reaching it; backwards an ENTER at
 * t+1 gives q_t = g_{t+1} and marks frame t+1 as the start of a segment; frame 0 always starts one.
 * Outputs, each may be NULL: per frame (offs[S] entries) cls, state, entered (1: the frame starts a segment) and gbest
 * (G_t; 0.0 at frame 0 of a stream); per stream log_prob = ln P* and status: 0 ok; 1 ln P* = -inf (the path is still written
 * by the same rules); 2 a symbol >= M (ln P* = -inf, cls and state 0xFFFF, entered 0, gbest -inf except entry 0).  An empty
 * stream: status 0, ln P* = 0.0.  The segment [b, e) between two entered frames has class cls[b] and the score
 * (e == T ? ln P* : gbest[e]) - (b == 0 ? 0.0 : gbest[b] + ln_switch).
 * K < 1, an N_k outside [1, 64], more than 4096 states in all, a negative, NaN or infinite parameter and an ln_switch that
 * is NaN or > 0 are refused before any HIP call.  One device: the streams are not dealt over several GPUs.
 * sym_on_device: `sym` is a device pointer on `device` (offs stays a host pointer).
 * ECOZ2_HMM_SEGMENT_CHUNK_BYTES bounds the per-launch back-pointer table (default 256 MiB, whole streams; a table that
 * cannot be allocated is an error).  ECOZ2_HMM_SEGMENT_BODY = resident | looped forces a kernel body where it is possible
 * (resident needs a packing of at most 16 waves); the bits are the same. */
int e2vq_hmm_segment(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                     const double *const *Bs, const void *sym, const int64_t *offs, int S, double ln_switch, uint16_t *cls,
                     uint16_t *state, uint8_t *entered, double *gbest, double *log_prob, int *status, int sym_on_device);
/* HIP-event time of the kernels (forward + backtrack) of this thread's last segmentation (-1: none yet) */
int e2vq_hmm_segment_last_kernel_ms(float *ms);
/* CSV and stdout block of one segmented stream from its per-frame outputs (host only; what e2vq_hmm_segment_files calls).
 * stdout: name, T, the number of segments; frames per class; one line "begin_s - end_s class" per segment.  CSV header:
 *   segment,begin_frame,end_frame,begin_s,end_s,class,log_prob,log_prob_per_frame
 * end_frame is exclusive; begin_s = begin_frame O_ms / 1000, end_s = ((end_frame - 1) O_ms + W_ms) / 1000; floats as %.17g. */
int e2vq_hmm_segment_report(const char *name, int64_t T, int K, const char *const *class_names, int W_ms, int O_ms,
                            const uint16_t *cls, const uint8_t *entered, const double *gbest, double log_prob, double ln_switch,
                            const char *csv_filename);
/* The file form: inputs, stages and up-front refusals of e2vq_hmm_scan_files without window and hop, plus the limits on
 * N_k and on the number of states above; per input the block and CSV of e2vq_hmm_segment_report. */
int e2vq_hmm_segment_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                           const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                           const char *csv_dir_or_file);

/* ---- smoothed class posteriors under the same class loop -----------------------------------------------
 * `hmm segment --posteriors`: post[t][k] = P(class k at frame t | the whole stream) under the class loop e2vq_hmm_segment
 * decodes -- the forward-backward companion of its joint Viterbi: at every frame the whole mass may leave its class and
 * enter any class through that class's pi at the price sw = exp(ln_switch) (the C library's exp on the host; -inf gives 0).
 * Inputs and refusals are e2vq_hmm_segment's; in addition a packing of more than 16 wave-slots is refused (classes are
 * packed in class order into slots of 64 lanes, a class that does not fit the open slot opens the next) unless
 * ECOZ2_HMM_POSTERIOR_BODY chooses the looped body (the last paragraph).  The arithmetic is
 * scaled and linear, every operation one IEEE double operation in a fixed order, no fma (DESIGN.md 4.8.7 states it;
 * tests/hmm_posterior_restatement.py restates it; the GPU matches it bit for bit):
 *   x_0[k][j] = pi_k[j] B_k[j][o_0];  x_t[k][j] = (sum_i ah_{t-1}[k][i] A_k[i][j] + sw pi_k[j]) B_k[j][o_t];
 *   c_t = sum over all states of x_t;  ah_t = x_t / c_t;  P(O | loop) = prod c_t;
 *   bh_{T-1} = 1;  u = B_k[j][o_{t+1}] bh_{t+1}[k][j] / c_{t+1};  bh_t[k][i] = sum_j A_k[i][j] u[k][j] + sw sum_all pi u;
 *   post[t][k] = sum_j ah_t[k][j] bh_t[k][j].
 * Outputs, each may be NULL: post (offs[S] rows of K doubles, row offs[s] + t); per stream log_prob = ln P(O | loop) and
 * status: 0 ok; 1 the loop cannot emit the stream (the first c_t that is not > 0); 2 a symbol >= M; the first event in frame
 * order decides.  Status != 0: every post entry of the stream is 0.0 and log_prob is -inf.  An empty stream: status 0,
 * log_prob 0.0, no rows.  One device.  sym_on_device as in e2vq_hmm_segment.
 * ECOZ2_HMM_POSTERIOR_CHUNK_BYTES bounds the per-launch forward table (default 256 MiB, whole streams; a table that cannot
 * be allocated is an error).
 * The body.  ECOZ2_HMM_POSTERIOR_BODY chooses the kernel body in e2vq_hmm_segment_posteriors and
 * e2vq_hmm_segment_files_posteriors (no other entry point reads it).  Unset, empty or "resident": as above, more than 16
 * wave-slots are refused with "the classes take %d wave-slots of 64 lanes (at most 16: the posteriors have no looped body)".
 * "looped": the looped body for every packing, in which a wave serves several slots in turn.  "auto": resident up to 16
 * slots, looped above.  Any other value is refused before any HIP call: "ECOZ2_HMM_POSTERIOR_BODY=<v>: auto, resident or looped".
 * The contract above never depended on the body -- the global sum is defined for any number of slots: a butterfly per slot,
 * then the slot results added in slot order from slot 0 -- so post, log_prob and status are the same bits under either body.
 * The looped body keeps 8 (2 slots + sum N) bytes in LDS (its partial sums and one double per state); a packing whose bytes
 * exceeded the 160 KB would be refused before any HIP call ("%d wave-slots and %d states take %zu bytes of LDS in the looped
 * body of the posteriors"), which the limits on N_k and on the number of states (at most 34 832 bytes) keep out of reach. */
int e2vq_hmm_segment_posteriors(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                                const double *const *Bs, const void *sym, const int64_t *offs, int S, double ln_switch,
                                double *post, double *log_prob, int *status, int sym_on_device);
/* HIP-event time of the kernels of this thread's last posteriors call (-1: none yet) */
int e2vq_hmm_segment_posteriors_last_kernel_ms(float *ms);
/* e2vq_hmm_segment_report with the posteriors of the stream (host only; post: T rows of K).  The CSV gains two trailing
 * columns, posterior,min_posterior: the mean of post[t][class of the segment] over the segment's frames (a serial sum in
 * frame order, then one division) and its minimum; each stdout segment line gains " p=%.3f" (the mean).  With
 * frames_csv_filename (may be NULL) the per-frame table is written: header frame,begin_s,class,<class names...>, one row a
 * frame with the decoded class and the K posteriors.  Floats as %.17g. */
int e2vq_hmm_segment_report_posteriors(const char *name, int64_t T, int K, const char *const *class_names, int W_ms, int O_ms,
                                       const uint16_t *cls, const uint8_t *entered, const double *gbest, double log_prob,
                                       double ln_switch, const double *post, const char *csv_filename,
                                       const char *frames_csv_filename);
/* e2vq_hmm_segment_files with the posteriors: the symbols of an input are staged once, the segmentation and the posteriors
 * run on the same device buffer, and the report is e2vq_hmm_segment_report_posteriors'.  frames_dir (may be NULL): the
 * per-frame table of every input goes to <frames_dir>/<input's base name>.csv. */
int e2vq_hmm_segment_files_posteriors(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                      const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                      double ln_switch, const char *csv_dir_or_file, const char *frames_dir);

/* ---- the class loop under class-to-class prices ---------------------------------------------------------
 * `hmm segment --class-transitions`: e2vq_hmm_segment with the one price ln_switch replaced by lt, a row-major K x K
 * array: lt[f * K + k] is the logarithm of the price of leaving class f and entering class k through pi_k (f = k: a
 * boundary between two segments of one class).  Every entry is <= 0 or -inf.  Refused before any HIP call: what
 * e2vq_hmm_segment refuses, an entry that is NaN or > 0, and a packing of more than 16 wave-slots (classes are packed in
 * class order into slots of 64 lanes, N_k consecutive lanes each, never across a slot) unless
 * ECOZ2_HMM_SEGMENT_TRANS_BODY chooses the looped body (the last paragraph).
 * Per step: E_t[f] = max_i d_{t-1}[f][i] with x_t[f] the lowest state reaching it; base_t[k] = max_f (E_t[f] + lt[f][k])
 * with src_t[k] the lowest class reaching it; a state (k, j) is entered when base_t[k] + lpi_k[j] is strictly greater
 * than the best in-class predecessor.  Backwards an ENTER at frame t + 1 in class k gives q_t = (src_{t+1}[k], x_{t+1}[.]).
 * Outputs as e2vq_hmm_segment's with exit_score in the place of gbest: exit_score[t] = E_t[cls[t-1]] (0.0 at frame 0);
 * on an entered frame it is the path's own cumulative score at t - 1.  The segment [b, e) scores
 *   (e == T ? ln P* : exit_score[e]) - (b == 0 ? 0.0 : exit_score[b] + lt[cls[b-1]][cls[b]]).
 * With every entry equal to ln_switch, d, ln P* and exit_score on entered frames are e2vq_hmm_segment's bit for bit.
 * The body.  ECOZ2_HMM_SEGMENT_TRANS_BODY chooses the kernel body in e2vq_hmm_segment_trans, e2vq_hmm_segment_trans_files,
 * e2vq_hmm_segment_trans_stream_open (a session fixes its body at open) and e2vq_hmm_segment_trans_continuous_files; no other
 * entry point reads it -- e2vq_hmm_segment_trans_posteriors, e2vq_hmm_segment_trans_files_posteriors (whose decode follows
 * their own variable) and e2vq_hmm_transitions_estep read ECOZ2_HMM_TRANS_FB_BODY instead (4.8.13 below), and
 * e2vq_hmm_loop_estep keeps its refusal of more than 16 wave-slots.  Unset, empty
 * or "resident": as above, more than 16 wave-slots are refused with "the classes take %d wave-slots of 64 lanes (at most 16:
 * the class-transition decoder has no looped body)".  "looped": the looped body for every packing, in which a wave serves
 * several slots in turn.  "auto": resident up to 16 slots, looped above.  Any other value is refused before any HIP call:
 * "ECOZ2_HMM_SEGMENT_TRANS_BODY=<v>: auto, resident or looped".  The decode is a max-sum whose contract never depended on the
 * body: cls, state, entered, exit_score, log_prob and status are the same bits under either.  The looped body keeps
 * 256 + 16 K + 20 sum N bytes in LDS (E of two frames; d, the in-class maximum and its state per state); a packing whose bytes
 * exceeded the 160 KB would be refused before any HIP call ("%d wave-slots, %d states and %d classes take %zu bytes of LDS in
 * the looped body of the class-transition decoder"), which the limits on the number of states (at most 147 712 bytes, at
 * K = sum N = 4096) keep out of reach. */
int e2vq_hmm_segment_trans(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                           const double *const *Bs, const void *sym, const int64_t *offs, int S, const double *lt,
                           uint16_t *cls, uint16_t *state, uint8_t *entered, double *exit_score, double *log_prob, int *status,
                           int sym_on_device);
/* HIP-event time of the kernels (forward + backtrack) of this thread's last such segmentation (-1: none yet) */
int e2vq_hmm_segment_trans_last_kernel_ms(float *ms);
/* e2vq_hmm_segment_report with the segment score above (host only): lt is the K x K matrix of effective prices;
 * ln_switch is printed in the block's first line.  Columns and formats are e2vq_hmm_segment_report's. */
int e2vq_hmm_segment_trans_report(const char *name, int64_t T, int K, const char *const *class_names, int W_ms, int O_ms,
                                  const uint16_t *cls, const uint8_t *entered, const double *exit_score, double log_prob,
                                  double ln_switch, const double *lt, const char *csv_filename);
/* The transitions file (host only): a header "class,<name_1>,...,<name_K>", then one line "<from>,v_1,...,v_K" per class;
 * values are %lg or -inf.  The names must be exactly class_names, in any order; _read permutes the matrix to the order
 * of class_names (lt: K x K).  A missing, extra or repeated name, a wrong field count, or a value that is > 0 or NaN is
 * refused with the file and line.  _write writes lt in the order of class_names with %.17g. */
int e2vq_hmm_transitions_read(const char *filename, int K, const char *const *class_names, double *lt);
int e2vq_hmm_transitions_write(const char *filename, int K, const char *const *class_names, const double *lt);
/* e2vq_hmm_segment_files under the transitions file: inputs, stages and refusals are e2vq_hmm_segment_files's; the
 * effective price is lt[f][k] = file[f][k] + ln_switch (one host addition; 0 means "the file alone"). */
int e2vq_hmm_segment_trans_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                 const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                                 const char *transitions_csv, const char *csv_dir_or_file);
/* The matrix from labelled successions (host only): class bigrams are counted within each of the S label sequences
 * (labels in [0, K), offs: S + 1 offsets), and lt[f][k] = ln((c[f][k] + alpha) / (sum_k' c[f][k'] + alpha K)) with the C
 * library's log; alpha = 0 gives -inf for unseen pairs, and a row without any count is then refused. */
int e2vq_hmm_class_transitions(const int32_t *labels, const int64_t *offs, int S, int K, double alpha, double *lt);
/* `hmm transitions`: the same from files, written as a transitions file for the models' classes.  An input is one of this
 * project's segment CSVs (column `class`; consecutive rows are one succession) or a tab-separated selection table with the
 * columns `Begin Time (s)` and `Type` and `#` comment lines (rows ordered by begin time); the kind is detected by the
 * header.  A label that is no model's class is skipped and counted on stdout. */
int e2vq_hmm_transitions_files(const char *const *model_filenames, unsigned num_models, const char *const *input_filenames,
                               int num_inputs, double alpha, const char *out_csv);

/* ---- smoothed class posteriors under class-to-class prices ---------------------------------------------
 * `hmm segment --class-transitions <file> --grammar-posteriors`: e2vq_hmm_segment_posteriors with the one price replaced by
 * the matrix lt of e2vq_hmm_segment_trans -- post[t][k] = P(class k at frame t | the whole stream) under the loop that
 * e2vq_hmm_segment_trans decodes.  One step from state (f, i) to state (k, j) weighs [f = k] A_f[i][j] + w[f][k] pi_k[j]
 * with w[f][k] = exp(lt[f][k]) (the C library's exp on the host; -inf gives 0).  Refused before any HIP call: what
 * e2vq_hmm_segment_posteriors refuses for the models (a negative, NaN or infinite parameter included), what
 * e2vq_hmm_segment_trans refuses for lt (NaN or > 0), and a packing of more than 16 wave-slots ("the classes take %d
 * wave-slots of 64 lanes (at most 16: the posteriors under class-to-class prices have no looped body)") unless
 * ECOZ2_HMM_TRANS_FB_BODY chooses the looped body (the last paragraph; ECOZ2_HMM_POSTERIOR_BODY and
 * ECOZ2_HMM_SEGMENT_TRANS_BODY are not read).  The arithmetic is scaled and linear, every operation one IEEE
 * double operation in a fixed order, no fma (DESIGN.md 4.8.13 states it; tests/hmm_trans_posterior_restatement.py restates
 * it; the GPU matches it bit for bit).  With CS_k the sum over the states of class k in state order:
 *   x_0[k][j] = pi_k[j] B_k[j][o_0];  S[f] = CS_f(ah_{t-1});  m[k] = sum_f S[f] w[f][k] (f in class order);
 *   x_t[k][j] = (sum_i ah_{t-1}[k][i] A_k[i][j] + m[k] pi_k[j]) B_k[j][o_t];  c_t, ah_t and P(O | loop) as in 4.8.7;
 *   bh_{T-1} = 1;  u = B_k[j][o_{t+1}] bh_{t+1}[k][j] / c_{t+1};  R[k] = sum_j pi_k[j] u[k][j];
 *   r[f] = sum_k w[f][k] R[k] (k in class order);  bh_t[f][i] = sum_j A_f[i][j] u[f][j] + r[f];
 *   post[t][k] = sum_j ah_t[k][j] bh_t[k][j].
 * Outputs, status and the empty stream are e2vq_hmm_segment_posteriors'.  With every price -inf the figures are those of
 * e2vq_hmm_segment_posteriors at ln_switch = -inf bit for bit; with every price one finite value they agree within rounding
 * (4.8.7 replaces the sum of S by 1).  ECOZ2_HMM_POSTERIOR_CHUNK_BYTES bounds the per-launch forward table as in 4.8.7.
 * One device.  sym_on_device as in e2vq_hmm_segment.
 * The body.  ECOZ2_HMM_TRANS_FB_BODY chooses the kernel body of the two forward-backward passes under the prices, these
 * posteriors and the E-step of 4.8.14, in e2vq_hmm_segment_trans_posteriors, e2vq_hmm_segment_trans_files_posteriors,
 * e2vq_hmm_transitions_estep, e2vq_hmm_train_transitions and e2vq_hmm_learn_transitions_files (a training reads it once,
 * before its first E-step); no other entry point reads it.  Unset, empty or "resident": as above, more than 16 wave-slots are
 * refused with the words above (4.8.14: "... the E-step of the class transitions has no looped body").  "looped": the looped
 * body for every packing, min(slots, 16) waves of which each serves several slots in turn.  "auto": resident up to 16 slots,
 * looped above.  Any other value is refused before any HIP call: "ECOZ2_HMM_TRANS_FB_BODY=<v>: auto, resident or looped".  The
 * looped body is the same operations in the same order: post, acc, log_prob and status are the same bits under either.  It keeps
 * 8 (2 slots + 2 K + sum N) bytes in LDS for the posteriors and 8 (2 slots + 2 K + 2 sum N) for the E-step; a packing whose bytes
 * exceeded the 160 KB would be refused before any HIP call ("%d wave-slots, %d states and %d classes take %zu bytes of LDS in
 * the looped body of the posteriors under class-to-class prices" / "... of the E-step of the class transitions"), which the
 * limits on the number of states (at most 99 328 and 132 096 bytes, at K = sum N = 4096) keep out of reach.  The forward table's
 * c_t takes one double per frame and wave, not per slot, under the looped body. */
int e2vq_hmm_segment_trans_posteriors(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                                      const double *const *Bs, const void *sym, const int64_t *offs, int S, const double *lt,
                                      double *post, double *log_prob, int *status, int sym_on_device);
/* HIP-event time of the kernels of this thread's last such call (-1: none yet) */
int e2vq_hmm_segment_trans_posteriors_last_kernel_ms(float *ms);
/* e2vq_hmm_segment_trans_files with these posteriors: the symbols of an input are staged once, the segmentation and the
 * posteriors run on the same device buffer under the same effective prices, and the report gains what
 * e2vq_hmm_segment_report_posteriors adds (the CSV columns posterior,min_posterior, " p=%.3f", and with frames_dir -- may be
 * NULL -- the per-frame table <frames_dir>/<input's base name>.csv); the first eight CSV columns are
 * e2vq_hmm_segment_trans_files' byte for byte.  ECOZ2_HMM_TRANS_FB_BODY is the one choice of body here: where it picks the
 * looped posteriors the decode runs its looped body too (ECOZ2_HMM_SEGMENT_TRANS_BODY is not read). */
int e2vq_hmm_segment_trans_files_posteriors(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                            const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                            double ln_switch, const char *transitions_csv, const char *csv_dir_or_file,
                                            const char *frames_dir);

/* ---- Baum-Welch for the class-to-class prices ----------------------------------------------------------
 * `hmm transitions --em`: the matrix of e2vq_hmm_segment_trans re-estimated from whole unlabelled streams.  The model, the
 * inputs and the refusals are e2vq_hmm_segment_trans_posteriors': K models sharing M, N_k <= 64, S streams in sym / offs, lt
 * (row-major K x K, each entry <= 0 or -inf) with w[f][k] = exp(lt[f][k]) taken by the C library on the host.  A packing
 * of more than 16 wave-slots is refused before any HIP call ("the classes take %d
 * wave-slots of 64 lanes (at most 16: the E-step of the class transitions has no looped body)") unless ECOZ2_HMM_TRANS_FB_BODY
 * chooses the looped body (4.8.13 above: "The body").  Nothing transcendental runs
 * on the device; every operation is one IEEE double operation in a fixed order, no fma (DESIGN.md 4.8.14 states it;
 * tests/hmm_transitions_em_restatement.py restates it; the GPU matches it bit for bit).
 * E-step.  Forward, scaling, status, log_prob and backward are 4.8.13's word for word (S, m, x, c_t, ah, u, R, r, bh, the same
 * CS and GS): for a given input log_prob and status are the bits of e2vq_hmm_segment_trans_posteriors.  New are the counts.
 * For every stream of status 0, every t = 1 .. T - 1 and every pair (f, k):
 *   xi_t[f][k] = S_t[f] * (w[f][k] * R_t[k])
 * with S_t[f] = CS_f(ah_{t-1}) in the bits the forward pass used, R_t[k] the backward entry sum formed from
 * u = (B[.][o_t] * bh_t) / c_t, and w[f][k] * R_t[k] the very term the backward walk adds into r[f].  Each xi goes through
 * fix2(., 29) into the int64 limb pair of cell C[f][k]: acc[2 (f K + k)] and acc[2 (f K + k) + 1]; a zero limb adds nothing.
 * A stream of status != 0 adds nothing to C.  acc[2 K^2] counts the status-0 streams of the call, acc[2 K^2 + 1] the others.
 * acc (e2vq_hmm_transitions_acc_words(K) = 2 K^2 + 2 words) is added to and never cleared.  All sums are integers: the split
 * over workgroups, the order of the streams and the route of an atomic (the workgroup's LDS table, used when its 16 K^2
 * bytes fit next to the mandatory LDS terms, or global memory; ECOZ2_HMM_TRANS_EM_C=lds|global forces either, and a forced
 * table that does not fit is refused) change no bit.  ECOZ2_HMM_POSTERIOR_CHUNK_BYTES bounds the per-launch forward table as
 * in 4.8.13.  One device.  sym_on_device as in e2vq_hmm_segment. */
int64_t e2vq_hmm_transitions_acc_words(int K);
int e2vq_hmm_transitions_estep(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                               const double *const *Bs, const void *sym, const int64_t *offs, int S, const double *lt, int64_t *acc,
                               double *log_prob, int *status, int sym_on_device);
/* HIP-event time of the kernels of this thread's last E-step (-1: none yet) */
int e2vq_hmm_transitions_estep_last_kernel_ms(float *ms);
/* The training.  ln_p (K x K, in and out) is the matrix as the transitions file holds it; the effective price of an E-step is
 * ln_p[f][k] + ln_switch (one host addition, exactly how e2vq_hmm_segment_trans_files forms it; ln_switch <= 0 is not
 * trained).  Per iteration one E-step over all streams (acc from zero), then L = the sum of log_prob over the status-0
 * streams in stream order (reported through callback("sum_log_prob", L) and sum_log_prob[it] while it < cap).  The loop
 * stops at max_iterations (< 0: none), at 1000 E-steps, or when it > 0 and L - Lprev <= val_auto; a stopping iteration gets no
 * M-step.  If no stream has status 0 after the first E-step the call returns 1 and ln_p is as it came.
 * M-step (host, K^2 values; unfix as everywhere): D[f] = the integer sum of row f of C, both limbs, unfixed once; n_f = the
 * finite entries of the current row f; a finite entry becomes log((unfix(C[f][k]) + alpha) / (D[f] + alpha n_f)) with the C
 * library's log; a -inf entry stays -inf whatever alpha (a forbidden succession is the user's statement: smoothing does not
 * revive it); a row with D[f] + alpha n_f not > 0 keeps every byte.  alpha: finite, >= 0.  *num_esteps: the E-steps run. */
int e2vq_hmm_train_transitions(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                               const double *const *Bs, const void *sym, const int64_t *offs, int S, double *ln_p, double ln_switch,
                               double alpha, double val_auto, int max_iterations, double *sum_log_prob, int cap, int *num_esteps,
                               void (*callback)(char *variable, double value), int sym_on_device);
/* `hmm transitions --em`: the same from files.  Models, codebook and inputs (.wav / .prd / .seq) are
 * e2vq_hmm_segment_trans_files'; all streams are gathered in one device buffer, so an E-step is one call.  The start is
 * init_csv (a transitions file) or, when NULL or empty, every entry log(1.0 / K).  The result is written with
 * e2vq_hmm_transitions_write to out_csv; next to it <out_csv>.em.csv holds iteration,sum_log_prob,streams_used,streams_skipped
 * (%.17g).  A stream whose status changes is named on stderr with the iteration. */
int e2vq_hmm_learn_transitions_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                     const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                     double ln_switch, const char *init_csv, double alpha, double val_auto, int max_iterations,
                                     const char *out_csv);

/* ---- Baum-Welch for the class models under the class loop ----------------------------------------------
 * `hmm learn --loop`: pi, A and B of every class re-estimated from whole unlabelled streams under the very loop that
 * e2vq_hmm_segment_trans decodes, and on request the matrix with them, from one forward-backward pass.  The model, the inputs
 * and the refusals are e2vq_hmm_transitions_estep's: K models sharing M, N_k <= 64 (mixed N), S streams in sym / offs, lt
 * (row-major K x K, each entry <= 0 or -inf) with w[f][k] = exp(lt[f][k]) taken by the C library on the host.  Only the
 * resident layout exists: a packing of more than 16 wave-slots is refused before any HIP call ("the classes take %d
 * wave-slots of 64 lanes (at most 16: the E-step of the class models under the loop has no looped body)").  Nothing
 * transcendental runs on the device; every operation is one IEEE double operation in a fixed order, no fma (DESIGN.md 4.8.16
 * states it; tests/hmm_loop_em_restatement.py restates it; the GPU matches it bit for bit).
 * E-step.  Forward, scaling, status, log_prob and backward are 4.8.13's word for word (S, m, x, c_t, ah, u, R, r, bh with
 * bh_{T-1} = 1, the same CS and GS): for a given input log_prob and status are the bits of e2vq_hmm_segment_trans_posteriors.
 * An empty stream has status 0, log_prob 0.0 and adds nothing but its mark.  New are the state counts, for every stream of
 * status 0, each through fix2(., 29) into class k's block acc[k] of e2vq_hmm_acc_words(N_k, M) words (PI | AN | AD | BN | BD |
 * used, skipped; a zero limb adds nothing):
 *   every t:        g = ah_t[k][j] * bh_t[k][j]                      to BN[j][o_t] and BD[j]; at t = 0 also to PI[j]
 *   t < T - 1:      (ah_t[k][i] * A_k[i][j]) * u_{t+1}[k][j]         to AN[i][j]    (u_{t+1} = (B_k[j][o_{t+1}] * bh_{t+1}[k][j]) / c_{t+1})
 *   t < T - 1:      (m_{t+1}[k] * pi_k[j]) * u_{t+1}[k][j]           to PI[j]       (the entry through pi; the inner product has the
 *                                                                                    bits the forward step added to the chain)
 * AD[i] is the integer sum of row i of AN, both limbs.  used counts the status-0 streams of the call and skipped the others,
 * once a stream, in every class's block (every class is in the loop); a stream of status != 0 adds nothing else.  acc[k] is
 * overwritten, as e2vq_hmm_embedded_estep does.  acc_trans (may be NULL; e2vq_hmm_transitions_acc_words(K) words, added to):
 * 4.8.14's xi_t[f][k] = S_t[f] * (w[f][k] * R_t[k]), limb for limb the result of e2vq_hmm_transitions_estep on the same input;
 * without it the grammar products are not formed.  All sums are integers: the split over workgroups, the order of the streams
 * and the route of an atomic change no bit.  Routes: BD and PI are summed per lane and flushed once a stream, BN goes by
 * global atomics; the AN table of all classes (16 sum_k N_k (N_k | 1) bytes) and the C table (16 K^2 bytes) live in the
 * workgroup's LDS when they fit, in this order, behind the mandatory terms and ahead of A and the two price matrices;
 * ECOZ2_HMM_LOOP_EM_AN=lds|global and ECOZ2_HMM_LOOP_EM_C=lds|global force either, and a forced table that does not fit is
 * refused.  ECOZ2_HMM_POSTERIOR_CHUNK_BYTES bounds the per-launch forward table, 8 (sum N + slots + K) bytes a frame (4.8.13's
 * row and m_t of every class), by whole streams.  One device.  sym_on_device as in e2vq_hmm_segment. */
int e2vq_hmm_loop_estep(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                        const double *const *Bs, const void *sym, const int64_t *offs, int S, const double *lt, int64_t *const *acc,
                        int64_t *acc_trans, double *log_prob, int *status, int sym_on_device);
/* HIP-event time of the kernels of this thread's last E-step (-1: none yet) */
int e2vq_hmm_loop_estep_last_kernel_ms(float *ms);
/* The training.  pis / As / Bs are re-estimated in place; ln_p (K x K, in and, with train_transitions, out) is the matrix as
 * the transitions file holds it; the effective price of an E-step is ln_p[f][k] + ln_switch (one host addition; ln_switch <= 0
 * is not trained).  Per iteration one E-step over all streams, then L = the sum of log_prob over the status-0 streams in
 * stream order (callback("sum_log_prob", L); sum_log_prob[it] while it < cap).  The loop stops at max_iterations (< 0: none),
 * at 1000 E-steps, or when it > 0 and L - Lprev <= val_auto; a stopping iteration gets no M-step.  If no stream has status 0
 * after the first E-step the call returns 1 and models and matrix are as they came.
 * M-step.  e2vq_hmm_train_embedded's, all K classes in one launch: pi by the sum of its own counts, A by AD, B by BD, each
 * quotient only where its denominator is > 0 (zeros in pi and A stay zeros), then the floor of B at epsilon (> 0) for the
 * classes whose used > 0.  frozen (may be NULL): K flags; the block of a class whose flag is not 0 is zeroed before the
 * M-step, so the class keeps every byte of its model.  With train_transitions (not 0) e2vq_hmm_train_transitions' M-step is
 * applied to ln_p from the counts of the same E-step (alpha: finite, >= 0; -inf stays -inf); without it ln_p is not written. */
int e2vq_hmm_train_loop(int device, int K, const int *Ns, int M, double *const *pis, double *const *As, double *const *Bs,
                        const void *sym, const int64_t *offs, int S, double *ln_p, double ln_switch, int train_transitions,
                        const uint8_t *frozen, double alpha, double epsilon, double val_auto, int max_iterations,
                        double *sum_log_prob, int cap, int *num_esteps, void (*callback)(char *variable, double value),
                        int sym_on_device);
/* `hmm learn --loop`: the same from files.  Models, codebook and inputs (.wav / .prd / .seq) are
 * e2vq_hmm_learn_transitions_files'; all streams are gathered in one device buffer.  The start of the matrix is
 * transitions_csv or, when NULL or empty, a matrix of zeros (the effective prices are then the one ln_switch, as
 * e2vq_hmm_segment_trans_files treats a file of zeros).  frozen_classes: num_frozen class names, each some model's class.
 * Written: <out_dir>/<class>.hmm for every class, <out_dir>/loop.csv with iteration,sum_log_prob,streams_used,streams_skipped
 * (%.17g) and, with train_transitions, <out_dir>/transitions.csv through e2vq_hmm_transitions_write.  Refused: an out_dir
 * that would overwrite an input model, two models of one class, a frozen name that is no model's class.  A stream whose
 * status changes is named on stderr with the iteration. */
int e2vq_hmm_learn_loop_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                              const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms, double ln_switch,
                              const char *transitions_csv, int train_transitions, const char *const *frozen_classes, int num_frozen,
                              double alpha, double epsilon, double val_auto, int max_iterations, const char *out_dir,
                              void (*callback)(char *variable, double value));

/* ---- the same decode on a stream that arrives piece by piece -------------------------------------------
 * `hmm segment --continuous`: a session decodes ONE symbol stream of unknown length under the contract of e2vq_hmm_segment
 * (K models sharing M, one ln_switch; same recursion, ties, G_t, g_t, psi and ENTER) and gives the bits of e2vq_hmm_segment
 * on the concatenation of everything fed, whatever the feeds' lengths.  Symbols are processed in blocks of exactly B frames
 * (ECOZ2_HMM_SEGMENT_STREAM_BLOCK, read at open, default 4096; below 1 is refused); fewer than B stay buffered until the
 * next feed, a flush or close.  A block starts from the d the previous one left; the frame-0 rule holds at the absolute
 * frame 0 only.
 * Finality: after the last block of a feed, the paths of all states with d > -inf are followed back in lockstep; up to the
 * latest frame at which they are all in one state, the frames are final, and they are that path's.  (The state this reaches
 * just before the first new frame must be where the previous commit ended; otherwise an internal error is returned.)  With
 * no such state nothing becomes final.  The number of final frames after p processed frames depends on the first p symbols
 * alone.  close decides the rest from the lowest state reaching max d, as e2vq_hmm_segment does, and yields ln P* and the
 * status.  Final frames wait in host memory (13 bytes a frame) until e2vq_hmm_segment_stream_take hands them out, in order;
 * each of its outputs may be NULL.
 * Status.  The equality with e2vq_hmm_segment is claimed for a stream whose status there is 0.  2, a symbol >= M: the feed
 * or flush that meets it fails with a message naming the absolute frame, and the session takes no more symbols; close then
 * reports status 2 and ln P* = -inf, frames already final stay, and every other frame fed is delivered as cls = state =
 * 0xFFFF, entered 0, gbest -inf.  1, every state dead: nothing more becomes final before close, which backtracks by the
 * usual rules and reports status 1, ln P* = -inf; the frames of such a stream need not be e2vq_hmm_segment's, because a
 * path that died later may have left a committed prefix.  Nothing fed: status 0, ln P* = 0.0, no frames.
 * Memory.  psi and g of the frames that are not final stay on the device in a ring of 2 sum N + 4 bytes a frame, bounded by
 * ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES (default 256 MiB; a budget below two blocks is refused at open).  A feed or flush
 * whose next block does not fit fails with a message naming the variable and the number of pending frames (with ln_switch =
 * -inf paths of different classes never meet); the blocks before it stay processed, the rest of that feed is dropped, and
 * the session can still be closed (B - 1 rows beyond the budget are kept for the remainder at close).  Besides the ring a
 * session holds the parameters, O(B) staging and 5 bytes a pending frame for the results of a commit: nothing grows with
 * the stream.  ECOZ2_HMM_SEGMENT_BODY is honoured as by e2vq_hmm_segment.
 * Refused before any HIP call: what e2vq_hmm_segment refuses, a bad block length, a budget below two blocks.  A NULL
 * session, and a feed or flush after close or after status 2, are refused.  One thread at a time uses a session. */
typedef struct e2vq_segment_stream e2vq_segment_stream;
int e2vq_hmm_segment_stream_open(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                                 const double *const *Bs, double ln_switch, e2vq_segment_stream **out);
/* n >= 0 symbols (u16; sym_on_device: a device pointer on the session's device); *final_frames: all frames final so far */
int e2vq_hmm_segment_stream_feed(e2vq_segment_stream *s, const void *sym, int64_t n, int sym_on_device, int64_t *final_frames);
/* processes the buffered remainder as a short block */
int e2vq_hmm_segment_stream_flush(e2vq_segment_stream *s, int64_t *final_frames);
int e2vq_hmm_segment_stream_close(e2vq_segment_stream *s, double *log_prob, int *status, int64_t *final_frames);
int e2vq_hmm_segment_stream_take(e2vq_segment_stream *s, int64_t max_frames, uint16_t *cls, uint16_t *state, uint8_t *entered,
                                 double *gbest, int64_t *first_frame, int64_t *count);
/* HIP-event time of all kernels of the session so far (per feed: first launch to last, the copies between them included) */
int e2vq_hmm_segment_stream_kernel_ms(e2vq_segment_stream *s, float *ms);
/* the most frames that were pending at once; the device bytes of the session; the part of kernel_ms spent in coalescence
 * and backtrack.  Each may be NULL. */
int e2vq_hmm_segment_stream_stats(e2vq_segment_stream *s, int64_t *peak_pending, int64_t *device_bytes, float *commit_ms);
void e2vq_hmm_segment_stream_free(e2vq_segment_stream *s);
/* The file form: the inputs, in the order given, are consecutive pieces of ONE recording called `name`.  Models, inputs and
 * up-front refusals as e2vq_hmm_segment_files.  Each piece becomes symbols on its own -- a .wav is analysed by itself, so no
 * LPC window straddles two files -- and is fed to one session; at the end e2vq_hmm_segment_report(name, ...) writes the
 * block and the CSV (csv_dir_or_file: <dir>/<name>.csv, or the .csv file itself).  Times are frame arithmetic over the
 * whole run, as if it were one .seq. */
int e2vq_hmm_segment_continuous_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                      const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                      double ln_switch, const char *name, const char *csv_dir_or_file);

/* ---- the streaming decode under class-to-class prices ----------------------------------------------------
 * `hmm segment --class-transitions --grammar-continuous`: a session of the kind above under the contract of
 * e2vq_hmm_segment_trans (K models sharing M, the K x K prices lt; same recursion, ties, E_t, x_t, base_t, src_t, psi, ENTER
 * and exit_score), which gives the bits of e2vq_hmm_segment_trans on the concatenation of everything fed, whatever the
 * feeds' lengths and the block length.  e2vq_hmm_segment_trans_stream_open returns the session type above; feed, flush,
 * close, take, kernel_ms, stats and free serve it unchanged, and take's gbest array receives exit_score (exit_score[t] =
 * E_t of the class of frame t - 1; 0.0 at the absolute frame 0).  Blocks, carry, buffering, flush and close are those of the
 * one-price session.
 * Finality: the same rule with the matrix's back step -- state (k, j) at frame t goes to (k, psi), or on ENTER to
 * (src_t[k], x_t[src_t[k]]).  The join with the previous commit is checked as above.  close takes the lowest composite index
 * reaching max d.
 * Status.  As above, with exit_score in the place of gbest: after a symbol >= M every frame that was not final is delivered
 * as cls = state = 0xFFFF, entered 0, exit_score -inf (0.0 at the absolute frame 0, as e2vq_hmm_segment_trans fills it).
 * The equality is claimed for a stream whose status there is 0; for a stream that died (status 1) it is not, for the reason
 * given above.
 * Memory.  A pending frame keeps psi (2 sum N bytes), src and x (2 K each) and E (8 K): 2 sum N + 12 K bytes, bounded by
 * ECOZ2_HMM_SEGMENT_STREAM_PENDING_BYTES as above (a budget below two blocks is refused at open, with the row size in the
 * message; B - 1 rows more are kept for the remainder at close).  Where every price is -inf, or the finite ones do not
 * connect the classes, nothing becomes final before close, and the ring-full message says so.  The results of a commit take
 * 13 bytes a pending frame.  Nothing grows with the stream.
 * Refused before any HIP call: what e2vq_hmm_segment_trans refuses (a NaN or positive price; a packing of more than 16
 * wave-slots, the message names their number: the layout is resident only), a bad block length, a budget below two blocks. */
int e2vq_hmm_segment_trans_stream_open(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                                       const double *const *Bs, const double *lt, e2vq_segment_stream **out);
/* The file form of e2vq_hmm_segment_continuous_files under a transitions file: inputs and stages as there; the file is read
 * and permuted as e2vq_hmm_segment_trans_files reads it, the effective price is the file's plus ln_switch, and the report
 * goes through e2vq_hmm_segment_trans_report under `name`. */
int e2vq_hmm_segment_trans_continuous_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                            const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                            double ln_switch, const char *transitions_csv, const char *name,
                                            const char *csv_dir_or_file);

/* ---- the class posteriors on a stream that arrives piece by piece -------------------------------------
 * `hmm segment --continuous-posteriors`: a session over ONE symbol stream of unknown length under the contract of
 * e2vq_hmm_segment_posteriors (K models sharing M, one ln_switch; the same sw, e, forward pass, GS, scaling, backward pass,
 * posterior and scale_step, each one IEEE double operation in that order).  Two integers are fixed at open: a block length
 * B >= 1 and a look-ahead L >= 0, in frames.  Block b is the absolute frames [b B, (b + 1) B); its window end is
 * w_b = (b + 1) B + L while the stream is open, and T, the number of symbols fed, at close.
 * The result.  The K posteriors delivered for frame t of block b are, bit for bit, row t of e2vq_hmm_segment_posteriors run
 * on the prefix o[0 : w_b) of everything fed: P(class at t | the first w_b symbols).  Hence every block with
 * (b + 1) B + L >= T gets the closed pass's bits on the whole stream, and a session with L >= T is
 * e2vq_hmm_segment_posteriors bit for bit; log_prob at close is the closed pass's bit for bit (the (mantissa, exponent) pair
 * is carried in the session).  The rows, and the number of rows ready after p symbols -- the blocks with (b + 1) B + L <= p --
 * depend on (B, L) and the first p symbols alone, however they were fed; close delivers the rest.  Nothing fed: status 0,
 * log_prob 0.0, no rows.  Delivered rows wait in host memory (8 K bytes a frame) until e2vq_hmm_posterior_stream_take hands
 * them out, in order.
 * Status.  The first event in frame order decides, as there: a symbol >= M gives 2, !(c_t > 0) gives 1, and the symbol check
 * of a frame comes before its arithmetic.  The launch whose forward pass meets the event delivers no rows; rows delivered
 * earlier stay; every other row of everything fed is delivered as +0.0, by close.  2: the feed (or close) that meets it
 * fails with a message naming the absolute frame, and further feeds are refused.  1: further feeds are accepted, are counted
 * and do nothing.  In both cases close reports the status and log_prob = -inf (a close that itself meets status 2 fails
 * with the message after it has set its outputs and closed the session).  The equality with the closed pass is not claimed
 * for such a stream: the closed pass zeroes every row.
 * Memory.  ah_t, c_t and the symbol of the last B + L frames stay on the device in a ring of exactly B + L rows (frame t in
 * row t mod (B + L)), next to the parameters and the rows of one launch: nothing on the device grows with a feed or with
 * the stream.  The forward pass runs over every frame once; the backward pass of window b walks from w_b - 1 down to b B.
 * Refused before any HIP call: what e2vq_hmm_segment_posteriors refuses (more than 16 wave-slots word for word, unless
 * ECOZ2_HMM_POSTERIOR_BODY, read at open, is auto or looped), B < 1, L < 0.  A ring that cannot be allocated fails with a
 * message that gives its bytes.  A NULL session, a feed after close or after status 2, and a second close are refused.
 * One thread at a time uses a session. */
typedef struct e2vq_posterior_stream e2vq_posterior_stream;
int e2vq_hmm_posterior_stream_open(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                                   const double *const *Bs, double ln_switch, int64_t block, int64_t lookahead,
                                   e2vq_posterior_stream **out);
/* n >= 0 symbols (u16; sym_on_device: a device pointer on the session's device); *ready_frames: all frames delivered so far.
 * The launches of a feed are queued on the session's stream with one synchronisation at the end. */
int e2vq_hmm_posterior_stream_feed(e2vq_posterior_stream *s, const void *sym, int64_t n, int sym_on_device, int64_t *ready_frames);
int e2vq_hmm_posterior_stream_close(e2vq_posterior_stream *s, double *log_prob, int *status, int64_t *ready_frames);
/* up to max_frames delivered rows (K doubles each; post may be NULL) from the absolute frame *first_frame on */
int e2vq_hmm_posterior_stream_take(e2vq_posterior_stream *s, int64_t max_frames, double *post, int64_t *first_frame, int64_t *count);
/* HIP-event time of all launches of the session so far (per feed: first launch to last, the copies between them included) */
int e2vq_hmm_posterior_stream_kernel_ms(e2vq_posterior_stream *s, float *ms);
/* the device bytes of the session; the rows of its ring; the launches so far; the frames their backward passes walked.
 * Each may be NULL. */
int e2vq_hmm_posterior_stream_stats(e2vq_posterior_stream *s, int64_t *device_bytes, int64_t *ring_rows, int64_t *launches,
                                    int64_t *backward_frames);
void e2vq_hmm_posterior_stream_free(e2vq_posterior_stream *s);
/* The file form: the inputs, in the order given, are consecutive pieces of ONE recording called `name`, as
 * e2vq_hmm_segment_continuous_files takes them.  Each piece is staged once and fed, on the device, to a session of
 * e2vq_hmm_segment_stream_open and to a posterior session (block, lookahead); e2vq_hmm_segment_report_posteriors(name, ...)
 * then writes the block, the CSV with posterior,min_posterior and, with frames_dir (may be NULL), <frames_dir>/<name>.csv.
 * The host keeps the T K doubles of the posteriors for that report. */
int e2vq_hmm_segment_continuous_files_posteriors(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                                 const char *const *input_filenames, int num_inputs, int P, int W_ms, int O_ms,
                                                 double ln_switch, const char *name, const char *csv_dir_or_file,
                                                 const char *frames_dir, int64_t block, int64_t lookahead);

/* ---- forced alignment to a known order of units ----------------------------------------------------------
 * `hmm align`: where are the boundaries of units whose classes and order are known?  K models sharing M (the checks of
 * e2vq_hmm_segment), S symbol streams (sym, offs), and for stream s a transcript of L_s >= 1 units: units[unit_offs[s] ..
 * unit_offs[s + 1]) are class indices in [0, K), repeats allowed, the same class twice in a row included; optional (u8 a
 * unit, may be NULL = none) marks units a path may pass over; ln_switch <= 0, finite, is the price of every unit boundary.
 * The composite states of a stream are (l, j), l < L, j < N_{c_l}, in unit order.  All arithmetic is in the log domain on
 * the logarithms e2vq_hmm_viterbi takes; every step is additions and comparisons only, values are finite or -inf, so no
 * NaN can arise.
 *   Frame 0.  d_0(l, j) = lpi_{c_l}[j] + lB_{c_l}[j][o_0] for l = 0, and also for l = 1 when unit 0 is optional; else -inf.
 *   Step t > 0, in-class part: e2vq_hmm_segment's chain, best = max_i d_{t-1}(l, i) + lA[i][j], the lowest i wins ties.
 *   Exit of a unit: E_t[l] = max_i d_{t-1}(l, i), x_t[l] the lowest state reaching it.
 *   Entry into unit l >= 1: e = E_t[l-1], src = l - 1; when unit l - 1 is optional and l >= 2, src = l - 2 and e = E_t[l-2]
 *   if that is strictly greater.  base = e + ln_switch; the state is entered when base + lpi[j] is strictly greater than
 *   the in-class best (the addition order of e2vq_hmm_segment).  d_t = best + lB.
 *   End: the maximum of d_{T-1} over the states of unit L - 1, and of unit L - 2 as well when unit L - 1 is optional; the
 *   lowest composite index wins.
 * Status 0; 1 with ln P* = -inf when that maximum is -inf (T smaller than the number of mandatory units is the plain
 * case): the path is still what the back-pointers give by the same rules, and need then not start in an initial unit; 2 for
 * a symbol >= M: ln P* = -inf, unit = state = 0xFFFF, entered = 0, score = 0.0 at frame 0 and -inf after it, every unit
 * -1 / -1.  An empty stream: status 0, ln P* = 0.0, every unit -1 / -1.
 * Outputs.  Per frame: unit (index into the stream's transcript), state, entered (1 at frame 0 and where the path enters a
 * unit), score = the path's own cumulative score at that frame.  Per unit (at unit_offs): begin, end, the frame range
 * [begin, end) relative to the stream's first frame, -1 / -1 for a unit the path does not visit.  Per stream: log_prob,
 * status.  Any output may be NULL.
 * score is no device table: once the path is known the host replays it, one addition per term in the device's order -- an
 * entry is ((score[t-1] + ln_switch) + lpi) + lB, an in-class step (score[t-1] + lA) + lB, frame 0 lpi + lB (-inf where
 * the unit of frame 0 may not hold it) -- and score[T-1] must equal the device's ln P* on the bits, else an internal error
 * is returned.  The unit [b, e) scores score[e-1] - (b == 0 ? 0 : score[b-1] + ln_switch).
 * With L = 1 every output is e2vq_hmm_viterbi's of that model, bit for bit.
 * Layout: a workgroup per stream; the units are packed in unit order into wave-slots of 64 lanes (N consecutive lanes a
 * unit, never across a slot).  Up to 16 slots each wave keeps its d in a register; beyond (or with
 * ECOZ2_HMM_ALIGN_BODY=looped; =resident asks for the first) the waves loop over the slots with d in LDS.  Back-pointers
 * take sum N + L bytes a frame; ECOZ2_HMM_ALIGN_TABLE_BYTES (default 4 GiB) bounds a launch, streams are launched in
 * groups that fit.
 * Refused before any HIP call: what e2vq_hmm_segment refuses; an empty transcript; a unit outside [0, K); two adjacent
 * optional units; a transcript whose units are all optional; L > 65535; ln_switch > 0, NaN or -inf; a stream whose tables
 * exceed the budget (the message names the variable and the bytes); a packing that does not fit in LDS (the message names
 * sum N). */
int e2vq_hmm_align(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                   const double *const *Bs, const void *sym, const int64_t *offs, int S, const int32_t *units,
                   const int64_t *unit_offs, const uint8_t *optional, double ln_switch, uint16_t *unit, uint16_t *state,
                   uint8_t *entered, double *score, int64_t *begin, int64_t *end, double *log_prob, int *status,
                   int sym_on_device);
/* HIP-event time of the kernels (forward + backtrack) of this thread's last alignment (-1: none yet) */
int e2vq_hmm_align_last_kernel_ms(float *ms);
/* Report of one aligned stream (host only): a block on stdout and, with csv_filename, a CSV with one row per visited unit:
 * unit,class,begin_frame,end_frame,begin_s,end_s,score -- the time arithmetic and number formats of
 * e2vq_hmm_segment_report, score as defined above.  units / optional / begin / end: the stream's L entries; score: its T.
 * A unit the path passed over is left out of the CSV and counted in the block. */
int e2vq_hmm_align_report(const char *name, int64_t T, int K, const char *const *class_names, int W_ms, int O_ms, int L,
                          const int32_t *units, const uint8_t *optional, const int64_t *begin, const int64_t *end,
                          const double *score, double log_prob, double ln_switch, const char *csv_filename);
/* `hmm align`: input i (.wav, .prd or .seq, staged as e2vq_hmm_segment_files stages them) aligned to the transcript in
 * label file i -- a segment CSV (column `class`) or a tab-separated selection table (`Type`, ordered by `Begin Time (s)`),
 * as `hmm transitions` reads them; a label that is no model's class is refused with file and line.  filler_class (may be
 * NULL) names a model that is inserted as an optional unit before the first unit, between every two, and after the last.
 * csv_dir_or_file as e2vq_hmm_segment_files takes it.  Everything is checked before any HIP call. */
int e2vq_hmm_align_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                         const char *const *input_filenames, const char *const *label_filenames, int num_inputs, int P, int W_ms,
                         int O_ms, double ln_switch, const char *filler_class, const char *csv_dir_or_file);

/* ---- embedded Baum-Welch: the class models trained on transcribed streams ----------------------------------
 * `hmm learn --embedded`: re-estimate the class models from whole streams and, per stream, the order of its units -- no
 * boundaries.  Inputs are e2vq_hmm_align's: K models sharing M, N_k <= 64, mixed N allowed; S streams (sym, offs); per stream a
 * transcript c_0 .. c_{L-1} of class indices (units, unit_offs), repeats and immediate repeats allowed; a flag per unit,
 * optional (may be NULL = none); one finite ln_switch <= 0.  Everything e2vq_hmm_align refuses before a HIP call is refused
 * here too, and one thing more: a stream whose units pack into more than 16 wave-slots (the message names the slot count) --
 * unless ECOZ2_HMM_EMBED_BODY chooses the looped body (the last paragraph).
 * The arithmetic is linear and scaled; nothing transcendental runs on the device.  sw = exp(ln_switch) is the C library's exp
 * on the host; e[l][j] = sw * pi_{c_l}[j] is one host multiplication; every operation below is one IEEE double operation in
 * the stated order, no fma.  GS is the global sum of 4.8.7 over the stream's packing: a butterfly over the 64 lanes of each
 * slot (idle lanes 0.0), then the slots in slot order.
 * Sets.  Start S0 = {0} + {1 if optional[0]}.  Final F = {L-1} + {L-2 if optional[L-1]}.  pred(l) = {l-1} + {l-2 if l >= 2 and
 * optional[l-1]}; succ(l) is the mirror image: {l+1 if l+1 < L} + {l+2 if l+2 < L and optional[l+1]}.
 * Forward.  x_0[l][j] = pi[j] * B[j][o_0] for l in S0, else 0.0.  c_t = GS(x_t); !(c_t > 0) gives status 1.  ah_t = x_t / c_t.
 * For t >= 1 the in-class chain is 4.8.7's: acc = ah_{t-1}[l][0] * A[0][j], then acc = acc + ah_{t-1}[l][i] * A[i][j], i ascending;
 * the unit mass is summed on the way: V_{t-1}[l] = ah_{t-1}[l][0] + ah_{t-1}[l][1] + .. in state order (normalised).  The entering
 * mass: in = V_{t-1}[l-1], and in = in + V_{t-1}[l-2] when l-2 is in pred(l); m_t[l][j] = in * e[l][j]; x_t[l][j] = (acc +
 * m_t[l][j]) * B[j][o_t].  Unit 0 has no m (m_t[0][j] = 0.0).  The state-0 lane of a unit posts V before a barrier of the step's
 * own, the second next to the one of GS: no extra serial sum and no extra division.  (The other form -- the unnormalised mass
 * posted with the slot's partial sum, in = V / c_{t-1}, one barrier a frame -- was built and measured 8 to 14 % slower.)
 * Status.  A symbol >= M gives status 2; the symbol check of a frame comes before its arithmetic; the first event in frame
 * order decides.  A stream without frames has status 1.
 * End.  Z = GS(l in F ? ah_{T-1}[l][j] : 0.0); !(Z > 0) gives status 1 (T below the number of mandatory units is the plain
 * case).  log_prob = ln((prod_t c_t) Z), accumulated as (mantissa, exponent) with scale_step in frame order, Z last; the
 * logarithm is taken on the host as 4.8 does; -inf where the status is not 0.  This is ln P(O, transcript | models) under the
 * weighted chain.
 * Backward.  bh_{T-1}[l][j] = 1.0 / Z for l in F, else 0.0.  For t = T-2 .. 0: u[l][j] = (B[j][o_{t+1}] * bh_{t+1}[l][j]) /
 * c_{t+1}; R[l] = e[l][0] * u[l][0] + e[l][1] * u[l][1] + .. in state order; acc = A[i][0] * u[l][0] + A[i][1] * u[l][1] + ..
 * in state order; r = R[l+1], and r = r + R[l+2] when l+2 is in succ(l); bh_t[l][i] = acc + r, and acc alone for l = L-1.
 * Counts.  Each value goes through fix2(., ACC_SHIFT) into the int64 limb pairs of class c_l's block; the block's layout is
 * e2vq_hmm_acc_words(N, M)'s: PI[N] | AN[N][N] | AD[N] | BN[N][M] | BD[N] | used, skipped.  Every frame: g = ah_t[l][j] *
 * bh_t[l][j] goes to BN[j][o_t] and BD[j]; at t = 0 also to PI[j].  For t < T-1: (ah_t[l][i] * A[i][j]) * u[l][j] goes to
 * AN[i][j]; for l >= 1, m_{t+1}[l][j] * u[l][j] goes to PI[j] -- the expected number of entries through pi -- with the very bits
 * of m the forward pass used (it is stored).  AD[i] is the integer sum of row i of AN, both limbs.  The two trailing words
 * count the status-0 and the skipped streams whose transcript names the class, once a stream.  A stream of status != 0 adds
 * nothing else.  All sums are integers: the split over workgroups, the order of streams and the route of an atomic change no
 * bit.
 * M-step (k_hmm_reestimate_embedded, one thread a parameter, all K classes in a launch).  pi[j] = unfix(PI[j]) / unfix(the
 * integer sums of the hi and of the lo limbs of PI over j); A[i][j] = unfix(AN[i][j]) / unfix(AD[i]); B[j][k] = unfix(BN[j][k]) /
 * unfix(BD[j]); each only where its denominator is > 0.  Then, for epsilon > 0 and a class whose `used` word is > 0, hmm_adjustb's
 * floor of B at epsilon.  Zeros in pi and A stay zeros, so the model type survives; a class that no transcript names keeps
 * every byte.
 * Loop.  Per iteration one E-step over all streams, then L = the sum of log_prob over the status-0 streams in stream order, on
 * the host.  It stops as the other trainers do: max_iterations (< 0: none), 1000 E-steps, or it > 0 and L - Lprev <= val_auto;
 * a stopping iteration gets no M-step.  If no stream has status 0 after the first E-step the call returns 1 with a message and
 * leaves the models as they came.
 * Where the counts live while a stream runs: BD and PI in registers (a lane is one composite state for the whole stream), BN by
 * global atomics, AN in an LDS table over all K classes of the call (ds_add_u64, flushed once a stream) when it fits the 160 KB
 * next to A, else by global atomics; ECOZ2_HMM_EMBED_A / ECOZ2_HMM_EMBED_AN = lds | global force either choice (a forced layout
 * that does not fit is refused).  Scratch: ah_t and m_t per composite state, c_t per wave; whole streams per launch under
 * ECOZ2_HMM_EMBED_CHUNK_BYTES (default 256 MiB), a larger stream alone.
 * The body.  ECOZ2_HMM_EMBED_BODY chooses the kernel body of the E-step in e2vq_hmm_embedded_estep, e2vq_hmm_train_embedded and
 * e2vq_hmm_learn_embedded_files (no other entry point reads it).  Unset, empty or "resident": as above, more than 16 wave-slots
 * are refused.  "looped": every stream runs the looped body (hmm_embed_looped.hip), which takes any number of slots: a wave
 * serves several slots in turn and the per-state values live in LDS.  "auto": resident up to 16 slots, looped above; a launch
 * has one body, so the launches are cut where it changes.  Any other value is refused before a HIP call:
 * "ECOZ2_HMM_EMBED_BODY=<v>: auto, resident or looped".  The contract above never depended on the body -- GS is defined for any
 * number of slots -- so both bodies give the same limbs, the same bits of log_prob and the same status.  A looped stream needs
 * 16 (slots + L + sum N) bytes of LDS; one that does not fit in 160 KB is refused before a HIP call ("stream %d: %d units of sum
 * N = %d states in %d wave-slots do not fit in LDS").  A and the AN table go to LDS when they fit next to that, and the two
 * variables above force either choice here too.  BD and PI go by global atomics per frame under the looped body. */
/* one E-step: acc[k] receives class k's e2vq_hmm_acc_words(N_k, M) words (zeroed by the call); log_prob / status per stream
 * (either may be NULL) */
int e2vq_hmm_embedded_estep(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                            const double *const *Bs, const void *sym, const int64_t *offs, int S, const int32_t *units,
                            const int64_t *unit_offs, const uint8_t *optional, double ln_switch, int64_t *const *acc,
                            double *log_prob, int *status, int sym_on_device);
/* the whole loop, the models in place; L of E-step i at sum_log_prob[i] (i < cap), the number of E-steps at *num_esteps */
int e2vq_hmm_train_embedded(int device, int K, const int *Ns, int M, double *const *pis, double *const *As, double *const *Bs,
                            const void *sym, const int64_t *offs, int S, const int32_t *units, const int64_t *unit_offs,
                            const uint8_t *optional, double ln_switch, double epsilon, double val_auto, int max_iterations,
                            double *sum_log_prob, int cap, int *num_esteps, int sym_on_device);
/* HIP-event time of the kernels of this thread's last embedded E-step (-1: none yet) */
int e2vq_hmm_embedded_last_kernel_ms(float *ms);
/* `hmm learn --embedded`: the models of the files trained on input i (.wav, .prd or .seq, staged as e2vq_hmm_align_files
 * stages them) under the transcript in label file i (as `hmm align` reads it; filler_class, may be NULL, inserted as there).
 * Writes <out_dir>/<class>.hmm for every class, unchanged classes included, and <out_dir>/embedded.csv:
 * iteration,sum_log_prob,streams_used,streams_skipped.  An out_dir that would overwrite an input model, and two models of one
 * class, are refused.  A stream of status 1 or 2 is skipped, and named on stderr
 * with the iteration whenever its status changes (in a later iteration too); if all are skipped at first, that is an error.  Stdout: a
 * block in the style of `hmm learn`, its it=... lines unless ECOZ2_VQ_QUIET is set; the callback gets ("sum_log_prob", L)
 * per E-step.  Everything but the streams' statuses is checked before any HIP call. */
int e2vq_hmm_learn_embedded_files(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                  const char *const *input_filenames, const char *const *label_filenames, int num_inputs, int P,
                                  int W_ms, int O_ms, double ln_switch, const char *filler_class, double hmm_epsilon,
                                  double val_auto, int max_iterations, const char *out_dir,
                                  void (*callback)(char *variable, double value));

/* ---- how sure the alignment is: posteriors over the chain of units -------------------------------------------
 * `hmm align --posteriors`: per unit and frame the posterior that the unit holds the frame, and per unit the probability that a
 * path visits it with the mean and the spread of the frame it is entered at.  Inputs are e2vq_hmm_embedded_estep's.  path_unit
 * (may be NULL): one uint16 per frame at the streams' absolute offsets, e2vq_hmm_align's `unit` output.  ref (may be NULL = 0):
 * one int64 per unit at unit_offs, a reference frame for the moments below, each in [0, T) (not read for a stream without
 * frames).  Any output may be NULL.
 * Sets, Forward, Status, End, Backward are 4.8.11's word for word: the same operations in the same order, with the same GS over
 * the same packing from align_plan.  ah_t, m_t, c_t, Z, bh_t, u, log_prob and status are therefore the E-step's bits; a stream
 * without frames has status 1, as there.
 * Occupancy.  g_t[l][j] = ah_t[l][j] * bh_t[l][j]; G_t[l] = g_t[l][0] + g_t[l][1] + .. in state order: P(unit l holds frame t |
 * stream, transcript).  occ receives G_t[l] at occ_base(s) + t * L_s + l, occ_base(s) = the sum of T_s' * L_s' over s' < s.
 * Entries.  For t >= 1 and l >= 1: En_t[l] = m_t[l][0] * u_t[l][0] + m_t[l][1] * u_t[l][1] + .. in state order, u_t = (B[j][o_t] *
 * bh_t[l][j]) / c_t -- the very products the E-step sends to PI, with the stored bits of m.  En_t[0] = 0.0 for t >= 1.  En_0[l] =
 * G_0[l].  Every admissible path that visits unit l enters it exactly once: the sum of En_t[l] over t is P(the path visits l).
 * Per unit.  The sums run in the order the backward pass meets the frames, t = T-1 down to 0, each term added by one
 * addition: w0[l] += En_t[l]; w1[l] += d * En_t[l]; w2[l] += (d * d) * En_t[l]; d = (double)(t - ref[l]).  d * d is exact while
 * |d| < 2^26.5 (94 906 265 frames) and one rounded product beyond.  The unit's state-0 lane holds the three sums over the whole
 * stream (the resident body in registers, the looped body in LDS words of its own) and writes them once.
 * Per frame.  post_path[t] = G_t[path_unit[t]]; 0.0 where path_unit[t] is 0xFFFF or >= L_s, or where path_unit is NULL.  The
 * lane that owns the unit writes it; path_unit is handed out 64 frames at a time, as the symbols are.
 * Status != 0.  Every occ, post_path, w0, w1 and w2 entry of the stream is 0.0; log_prob is -inf.
 * Host (e2vq_hmm_align_unit_moments, plain C++ in this order): present = w0; q = w1 / w0; begin_mean = (double)ref + q;
 * begin_sd = sqrt(max(0, w2 / w0 - q * q)); both NaN where !(w0 > 0).
 * Refused before any HIP call: everything e2vq_hmm_embedded_estep refuses; a packing of more than 16 wave-slots, by a message of
 * this function's own that names the slot count and says that only a resident body exists (unless the looped body is chosen:
 * the last paragraph); a ref outside [0, T).
 * Scratch: ah_t, m_t and c_t as in the E-step; whole streams per launch under ECOZ2_HMM_EMBED_CHUNK_BYTES, a larger stream
 * alone; ECOZ2_HMM_EMBED_A = lds | global is honoured as there.  The outputs have device mirrors for the whole call.
 * The body.  ECOZ2_HMM_ALIGN_POSTERIOR_BODY chooses the kernel body in e2vq_hmm_align_posteriors and
 * e2vq_hmm_align_files_posteriors (no other entry point reads it).  Unset, empty or "resident": as above, more than 16
 * wave-slots are refused.  "looped": every stream runs the looped body (hmm_align_posterior_looped.hip), which takes any number
 * of slots as the E-step's looped body does.  "auto": resident up to 16 slots, looped above; a launch has one body, so the
 * launches are cut where it changes.  Any other value is refused before a HIP call:
 * "ECOZ2_HMM_ALIGN_POSTERIOR_BODY=<v>: auto, resident or looped".  Nothing above depends on the body: both give the same bits
 * of every output, of log_prob and the same status.  A looped stream needs 16 (slots + sum N) + 40 L bytes of LDS; one that
 * does not fit in 160 KB is refused before a HIP call ("stream %d: %d units of sum N = %d states in %d wave-slots do not fit in
 * LDS").  A goes to LDS when it fits next to that, per launch; ECOZ2_HMM_EMBED_A forces either choice here too, and a forced
 * layout that does not fit is refused. */
int e2vq_hmm_align_posteriors(int device, int K, const int *Ns, int M, const double *const *pis, const double *const *As,
                              const double *const *Bs, const void *sym, const int64_t *offs, int S, const int32_t *units,
                              const int64_t *unit_offs, const uint8_t *optional, double ln_switch, const uint16_t *path_unit,
                              const int64_t *ref, double *occ, double *post_path, double *w0, double *w1, double *w2,
                              double *log_prob, int *status, int sym_on_device);
/* HIP-event time of the kernels of this thread's last e2vq_hmm_align_posteriors (-1: none yet) */
int e2vq_hmm_align_posteriors_last_kernel_ms(float *ms);
/* the host arithmetic above for n units (host only; ref may be NULL = 0, any output may be NULL) */
int e2vq_hmm_align_unit_moments(int64_t n, const double *w0, const double *w1, const double *w2, const int64_t *ref,
                                double *present, double *begin_mean, double *begin_sd);
/* e2vq_hmm_align_report with five trailing CSV columns: posterior,min_posterior,p_present,begin_mean_frame,begin_sd_frames --
 * posterior: the mean of post_path over the unit's [begin, end), a serial sum in frame order, then one division; min_posterior:
 * its minimum there; the other three from e2vq_hmm_align_unit_moments(w0, w1, w2, ref); floats as %.17g.  Each stdout unit line
 * gains " p=%.3f" (posterior); a unit the path passed over stays out of the CSV and gets a line with its p_present.  With
 * frames_csv_filename a per-frame table frame,begin_s,unit,class,posterior is written (path_unit is needed then). */
int e2vq_hmm_align_report_posteriors(const char *name, int64_t T, int K, const char *const *class_names, int W_ms, int O_ms,
                                     int L, const int32_t *units, const uint8_t *optional, const int64_t *begin,
                                     const int64_t *end, const double *score, double log_prob, double ln_switch,
                                     const uint16_t *path_unit, const double *post_path, const double *w0, const double *w1,
                                     const double *w2, const int64_t *ref, const char *csv_filename,
                                     const char *frames_csv_filename);
/* `hmm align --posteriors [--frame-posteriors <dir>]`: e2vq_hmm_align_files with the report above.  The symbols of an input are
 * staged once; e2vq_hmm_align and the posteriors run on the same device buffer; ref is the path's begin (0 where it is -1),
 * path_unit its unit.  frames_dir (may be NULL): <frames_dir>/<input's base name>.csv per input.  Everything e2vq_hmm_align_files
 * and e2vq_hmm_align_posteriors refuse is refused before any HIP call, under the body that ECOZ2_HMM_ALIGN_POSTERIOR_BODY chooses
 * for the posteriors: with "auto" or "looped" a transcript of more than 16 wave-slots is decoded by e2vq_hmm_align, which picks
 * its looped body by itself, and then scored; without it such a transcript is refused. */
int e2vq_hmm_align_files_posteriors(const char *const *model_filenames, unsigned num_models, const char *cb_filename,
                                    const char *const *input_filenames, const char *const *label_filenames, int num_inputs,
                                    int P, int W_ms, int O_ms, double ln_switch, const char *filler_class,
                                    const char *csv_dir_or_file, const char *frames_dir);

#ifdef __cplusplus
}
#endif
#endif
