// vq_cbset.cpp -- a resident set of codebooks and the one-pass quantize over it (include/ecoz2_vq.h, part 2; DESIGN.md
// 4.9.2).  A set keeps, per codebook, what a session builds from e2vq_set_codebook and e2vq_quantize_device -- the
// pre-doubled codewords, the MFMA tile image and, where the prefiltered sweep runs, its limb image and scales -- in one
// session per codebook, built once.  A call routes the codebooks by what it can observe (order, size, pointer alignment):
//   * narrow MFMA orders (P = 4 .. 40), 16-byte aligned frames: every codebook that e2vq_quantize_device would sweep plainly
//     goes through ONE launch of k_quantize_set (a wave stages its frames once and walks the set's device table);
//   * a codebook e2vq_quantize_device sweeps prefiltered keeps that path (2.5 x the plain sweep's rate at M = 1024);
//   * other orders and 8-byte aligned frames: e2vq_quantize_device per codebook, on the same resident frames.
// Every route computes the canonical chain and the lowest-index argmin: results do not depend on it.
#include "vq_session.h"

struct e2vq_cbset {
    int device = 0, P = 0, NC = 0, K = 0;
    std::vector<e2vq_session*> cb;  // codebook k and its images
    e2vq::QuantizeSetEntry* d_table = nullptr;  // the codebooks of k_quantize_set
    int nset = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    i64 set_launches = 0, single_launches = 0;
    // staging of e2vq_cbset_quantize_host
    double* d_qaos = nullptr;
    unsigned short* d_qsym = nullptr;
    double* d_qdmin = nullptr;
    i64 q_cap = 0;
};

static int cbset_init(e2vq_cbset* set, const int* Ms, const double* const* reflections)
{
    HIPCHK(hipStreamCreateWithFlags(&set->own_stream, hipStreamNonBlocking));
    set->stream = set->own_stream;
    std::vector<e2vq::QuantizeSetEntry> table;
    const bool narrow = e2vq::uses_mfma(set->NC) && !e2vq::mfma_is_wide(set->NC);
    for (int k = 0; k < set->K; ++k) {
        e2vq_session* s = nullptr;
        if (e2vq_session_create(set->device, set->P, &s)) return 1;
        set->cb.push_back(s);
        if (e2vq_set_stream(s, (void*)set->stream) || e2vq_set_codebook(s, reflections[k], Ms[k])) return 1;
        if (narrow && !e2vq_quantize_is_prefiltered(s)) table.push_back({s->d_cbm, (Ms[k] + 15) / 16, Ms[k], k, 0});
    }
    set->nset = (int)table.size();
    if (set->nset) {
        HIPCHK(hipMalloc(&set->d_table, table.size() * sizeof(table[0])));
        HIPCHK(hipMemcpy(set->d_table, table.data(), table.size() * sizeof(table[0]), hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" int e2vq_cbset_create(int device, int prediction_order, int K, const int* Ms, const double* const* reflections,
                                 e2vq_cbset** out)
{
    if (!out) return e2vq_set_error("e2vq_cbset_create: no place for the set");
    *out = nullptr;
    if (prediction_order < 1 || prediction_order > E2VQ_MAX_P)
        return e2vq_set_error("prediction order %d out of range [1, %d]", prediction_order, E2VQ_MAX_P);
    if (K < 1 || K > 64) return e2vq_set_error("%d codebooks in a set: 1 .. 64", K);
    if (!Ms || !reflections) return e2vq_set_error("e2vq_cbset_create: no codebooks");
    for (int k = 0; k < K; ++k) {
        if (Ms[k] < 1 || Ms[k] > 65536) return e2vq_set_error("codebook %d: size %d out of range [1, 65536]", k, Ms[k]);
        if (!reflections[k]) return e2vq_set_error("codebook %d: no reflections", k);
    }
    if (e2hip::require_device(device)) return 1;
    e2vq_cbset* set = new e2vq_cbset();
    set->device = device;
    set->P = prediction_order;
    set->NC = prediction_order + 1;
    set->K = K;
    if (cbset_init(set, Ms, reflections)) {  // message already set; release whatever was created
        e2vq_cbset_destroy(set);
        return 1;
    }
    *out = set;
    return 0;
}

extern "C" void e2vq_cbset_destroy(e2vq_cbset* set)
{
    if (!set) return;
    (void)hipSetDevice(set->device);
    if (set->stream) (void)hipStreamSynchronize(set->stream);
    for (e2vq_session* s : set->cb) e2vq_session_destroy(s);
    for (void* p : {(void*)set->d_table, (void*)set->d_qaos, (void*)set->d_qsym, (void*)set->d_qdmin})
        if (p) (void)hipFree(p);
    if (set->own_stream) (void)hipStreamDestroy(set->own_stream);
    delete set;
}

extern "C" int e2vq_cbset_set_stream(e2vq_cbset* set, void* hip_stream)
{
    HIPCHK(hipSetDevice(set->device));
    HIPCHK(hipStreamSynchronize(set->stream));
    set->stream = hip_stream ? (hipStream_t)hip_stream : set->own_stream;
    for (e2vq_session* s : set->cb)
        if (e2vq_set_stream(s, (void*)set->stream)) return 1;
    return 0;
}

extern "C" int e2vq_cbset_quantize_device(e2vq_cbset* set, const void* device_frames, int64_t T, void* device_sym,
                                          int64_t sym_stride, void* device_dmin, int64_t dmin_stride)
{
    if (T < 1) return 0;
    if (T > (int64_t)INT32_MAX - 64) return e2vq_set_error("%lld frames per quantize call exceed 2^31 - 65 (split the call)", (long long)T);
    if (!device_frames || !device_sym) return e2vq_set_error("e2vq_cbset_quantize_device: no frames or no place for the symbols");
    if (sym_stride < T || (device_dmin && dmin_stride < T))
        return e2vq_set_error("output strides (%lld, %lld) shorter than the %lld frames", (long long)sym_stride,
                              (long long)dmin_stride, (long long)T);
    HIPCHK(hipSetDevice(set->device));
    unsigned short* sym = (unsigned short*)device_sym;
    double* dmin = (double*)device_dmin;
    const bool in_set = set->nset > 0 && ((uintptr_t)device_frames & 15) == 0;
    if (in_set) {
        if (e2vq::launch_quantize_set(set->NC, (const double*)device_frames, T, (T + 63) / 64, set->d_table, set->nset, sym,
                                      sym_stride, dmin, dmin_stride, set->stream))
            return e2vq_set_error("no set sweep for prediction order %d", set->P);
        HIPCHK(hipGetLastError());
        set->set_launches++;
    }
    for (int k = 0; k < set->K; ++k) {
        e2vq_session* s = set->cb[(size_t)k];
        if (in_set && !e2vq_quantize_is_prefiltered(s)) continue;  // (swept by the set kernel)
        if (e2vq_quantize_device(s, device_frames, T, sym + k * sym_stride, dmin ? dmin + k * dmin_stride : nullptr)) return 1;
        set->single_launches++;
    }
    return 0;
}

extern "C" int e2vq_cbset_quantize_host(e2vq_cbset* set, const double* frames, int64_t T, uint16_t* sym, double* dmin)
{
    if (T < 1) return 0;
    if (!frames || !sym) return e2vq_set_error("e2vq_cbset_quantize_host: no frames or no place for the symbols");
    HIPCHK(hipSetDevice(set->device));
    const i64 CH = std::min<i64>(T, 1 << 20);  // frames per chunk (0.3 GB of predictor vectors, 10 MB of results per codebook)
    if (CH > set->q_cap) {
        for (void* p : {(void*)set->d_qaos, (void*)set->d_qsym, (void*)set->d_qdmin})
            if (p) (void)hipFree(p);
        set->d_qaos = nullptr;
        set->d_qsym = nullptr;
        set->d_qdmin = nullptr;
        set->q_cap = 0;
        HIPCHK(hipMalloc(&set->d_qaos, (size_t)CH * set->NC * 8));
        HIPCHK(hipMalloc(&set->d_qsym, (size_t)set->K * CH * 2 + 64));
        HIPCHK(hipMalloc(&set->d_qdmin, (size_t)set->K * CH * 8));
        set->q_cap = CH;
    }
    const i64 stride = set->q_cap;
    for (i64 t0 = 0; t0 < T; t0 += CH) {
        const i64 n = std::min<i64>(CH, T - t0);
        HIPCHK(hipMemcpyAsync(set->d_qaos, frames + (size_t)t0 * set->NC, (size_t)n * set->NC * 8, hipMemcpyHostToDevice, set->stream));
        if (e2vq_cbset_quantize_device(set, set->d_qaos, n, set->d_qsym, stride, dmin ? set->d_qdmin : nullptr, stride)) return 1;
        for (int k = 0; k < set->K; ++k) {
            HIPCHK(hipMemcpyAsync(sym + (size_t)k * T + t0, set->d_qsym + (size_t)k * stride, (size_t)n * 2, hipMemcpyDeviceToHost, set->stream));
            if (dmin)
                HIPCHK(hipMemcpyAsync(dmin + (size_t)k * T + t0, set->d_qdmin + (size_t)k * stride, (size_t)n * 8, hipMemcpyDeviceToHost,
                                      set->stream));
        }
        HIPCHK(hipStreamSynchronize(set->stream));
    }
    return 0;
}

extern "C" int e2vq_cbset_launch_counts(e2vq_cbset* set, int64_t* set_launches, int64_t* single_launches)
{
    if (set_launches) *set_launches = set->set_launches;
    if (single_launches) *single_launches = set->single_launches;
    return 0;
}
