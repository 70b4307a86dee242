// C ABI, activation profiles: exact integer statistics of every int8 activation that feeds another layer, plus prediction and
// confusion counts, accumulated on the GPU in the pass that classifies (bnm_infer_device_profiled; layout in
// include/bitnetmcu_hip.h).  Where the profiling variant of the generic kernel serves the model (FC, tile classes 2 and 4) the pass
// is that one kernel; otherwise it is the layer-wise tap (every ReLUNorm output of a chunk of images written to per-stream
// scratch) followed by profile_reduce_kernel (bnm_profile.hip), which adds the chunk's statistics to the caller's counters.
#include "bnm_capi_internal.hpp"

using namespace bnm_internal;

namespace {

constexpr uint64_t kProfChunk = 1ull << 20;   // images per tap + reduce step

// widths of the profiled layers in schedule order: a CNN's 4*C front-end features, then every FC layer but the classifier
std::vector<uint32_t> profile_widths(const bnm_model &m) {
    std::vector<uint32_t> w;
    if (m.kind == BNM_KIND_CNN && !m.layers.empty()) w.push_back(m.layers[0].info.out_channels * 4u);
    const std::vector<uint32_t> fc = m.fc_layers();
    for (size_t i = 0; i + 1 < fc.size(); i++) w.push_back(m.layers[fc[i]].info.n_output);
    return w;
}

uint64_t profile_words(const std::vector<uint32_t> &widths, uint32_t n_classes) {
    uint64_t words = 0;
    for (uint32_t w : widths) words += 2ull * w + 128ull;
    return words + n_classes + (uint64_t)n_classes * n_classes + 3ull;
}

constexpr uint64_t kFusedChunk = 1ull << 22;  // images per launch of the profiling kernel (its 32-bit LDS tallies)

// the profiling variant of the generic kernel serves this context: an FC model on the generic kernel's data, a tile class and row
// length it is instantiated for, weights + tallies within the LDS
bool prof_fused_ok(const bnm_ctx *c) {
    return c->model.kind == BNM_KIND_FC && c->generic_ok && c->gfrags && bnmk_fused_generic_prof_waves(c->gdesc, c->shape.dbl) > 0 &&
           c->fc.size() >= 3 && c->fc.size() <= 4;
}

// argument checks shared by the int8 and float entry points (before anything is queued)
int profile_check(const bnm_ctx *c, const void *d_images, const uint32_t *d_cls, const int32_t *d_labels, const uint64_t *d_counters) {
    if (!d_images || !d_counters) return fail(BNM_EINVAL, "null device pointer");
    if (((uintptr_t)d_counters & 7u) || ((uintptr_t)d_labels & 3u) || ((uintptr_t)d_cls & 3u))
        return fail(BNM_EINVAL, "d_counters must be 8-byte aligned, d_labels and d_cls 4-byte aligned");
    if (profile_widths(c->model).size() > BNM_PROFILE_MAX_LAYERS) return fail(BNM_EUNSUPPORTED, "more than 16 profiled layers");
    return BNM_OK;
}

// one call of n int8 images (c->mu held, the context's device current, arguments checked)
int profiled_locked(bnm_ctx *c, const int8_t *d_images, uint64_t n, uint32_t *d_cls, const int32_t *d_labels, uint64_t *d_counters,
                    hipStream_t s) {
    if (!n) return BNM_OK;
    const std::vector<uint32_t> widths = profile_widths(c->model);
    const uint32_t ncls = c->model.num_classes();
    BnmProfileDesc d;
    d.n_layers = (uint32_t)widths.size();
    d.n_classes = ncls;
    uint64_t word = 0;
    uint32_t col = 0;
    for (uint32_t l = 0; l < d.n_layers; l++) {
        d.first[l] = d.total;
        d.width[l] = widths[l];
        d.col[l] = col;      // the tap writes the layers side by side in schedule order
        d.word[l] = word;
        d.total += widths[l];
        col += widths[l];
        word += 2ull * widths[l] + 128ull;
    }
    d.first[d.n_layers] = d.total;
    d.pred = word;
    d.tail = word + ncls + (uint64_t)ncls * ncls;
    const uint32_t stride = col + ncls;      // + the classifier's ReLUNorm output, which the tap writes too (not profiled)

    if (c->profile_mode != 2 && prof_fused_ok(c)) {
        // one pass: the profiling variant of the generic kernel classifies and tallies
        BnmFusedProf pa;
        pa.ctr = (unsigned long long *)d_counters;
        pa.n_layers = d.n_layers;
        for (uint32_t l = 0; l < d.n_layers; l++) {
            pa.width[l] = d.width[l];
            pa.word[l] = (uint32_t)d.word[l];
        }
        pa.pred = (uint32_t)d.pred;
        pa.tail = (uint32_t)d.tail;
        pa.n_classes = ncls;
        const uint64_t chunk = n < kFusedChunk ? n : kFusedChunk;
        DevBuf &buf = stream_scratch(c, s).prof;
        if (!d_cls)
            if (int e = buf.ensure((size_t)chunk * 4u + 64u)) return e;
        uint32_t *block = nullptr;
        if (int e = work_block(c, s, &block)) return e;
        for (uint64_t off = 0; off < n; off += chunk) {
            const uint64_t cn = n - off < chunk ? n - off : chunk;
            pa.labels = d_labels ? d_labels + off : nullptr;
            HIP_TRY(bnmk_fused_generic_prof(c->gdesc, c->shape.dbl, c->grid_blocks, d_images + off * 256u, cn, c->gfrags,
                                            d_cls ? d_cls + off : (uint32_t *)buf.p, block, c->work_batch, pa, s));
        }
        c->last_kernel = "fused_fc_generic_prof_kernel";
        return BNM_OK;
    }

    const uint64_t chunk = n < kProfChunk ? n : kProfChunk;
    DevBuf &buf = stream_scratch(c, s).prof;
    const size_t cls_off = ((size_t)chunk * stride + 255u) & ~(size_t)255u;
    if (int e = buf.ensure(cls_off + (size_t)chunk * 4u + 64u)) return e;
    int8_t *acts = (int8_t *)buf.p;
    const int tap_path = c->all_known ? BNM_PATH_LAYERWISE_MFMA : BNM_PATH_LAYERWISE_ALU;
    std::string names;
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint64_t cn = n - off < chunk ? n - off : chunk;
        uint32_t *cls = d_cls ? d_cls + off : (uint32_t *)((char *)buf.p + cls_off);
        if (int e = infer_device_locked(c, d_images + off * 256u, cn, cls, nullptr, acts, stride, s, tap_path)) return e;
        if (off == 0) names = c->last_kernel;
        HIP_TRY(bnmk_profile_reduce(acts, stride, cn, cls, d_labels ? d_labels + off : nullptr, d_counters, d, s));
    }
    c->last_kernel = names + "+profile_reduce_kernel";
    return BNM_OK;
}

}  // namespace

extern "C" {

uint64_t bnm_model_profile_words(const bnm_model *m, uint32_t *n_layers, uint32_t *widths) {
    if (!m) return 0;
    const std::vector<uint32_t> w = profile_widths(*m);
    if (n_layers) *n_layers = (uint32_t)w.size();
    if (widths)
        for (size_t i = 0; i < w.size(); i++) widths[i] = w[i];
    return profile_words(w, m->num_classes());
}

int bnm_ctx_set_profile_mode(bnm_ctx *c, int mode) {
    if (!c || mode < 0 || mode > 2) return fail(BNM_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    if (mode == 1 && !prof_fused_ok(c))
        return fail(BNM_EUNSUPPORTED, "no fused profiling kernel serves this model (FC models whose layers are at most 128 wide, "
                                      "up to 64 classes): its profiles run the layer-wise tap + reduction");
    c->profile_mode = mode;
    return BNM_OK;
}

int bnm_infer_device_profiled(bnm_ctx *c, const int8_t *d_images, uint64_t n, uint32_t *d_cls, const int32_t *d_labels,
                              uint64_t *d_counters, void *stream) {
    if (!c) return fail(BNM_EINVAL, "null ctx");
    if (!n) return BNM_OK;
    std::lock_guard<std::mutex> g(c->mu);
    if (int e = profile_check(c, d_images, d_cls, d_labels, d_counters)) return e;
    if ((uintptr_t)d_images & 15u) return fail(BNM_EINVAL, "d_images must be 16-byte aligned");
    DeviceGuard dg(c->device);
    HIP_TRY(dg.err);
    return profiled_locked(c, d_images, n, d_cls, d_labels, d_counters, (hipStream_t)stream);
}

int bnm_infer_float_device_profiled(bnm_ctx *c, const float *d_x, uint64_t n, uint32_t *d_cls, const int32_t *d_labels,
                                    uint64_t *d_counters, void *stream) {
    if (!c) return fail(BNM_EINVAL, "null ctx");
    if (!n) return BNM_OK;
    if ((uintptr_t)d_x & 15u) return fail(BNM_EINVAL, "d_x must be 16-byte aligned");
    std::lock_guard<std::mutex> g(c->mu);
    if (int e = profile_check(c, d_x, d_cls, d_labels, d_counters)) return e;
    DeviceGuard dg(c->device);
    HIP_TRY(dg.err);
    hipStream_t s = (hipStream_t)stream;
    // quantise a chunk into per-stream scratch (non-finite images become all zeros and are counted, as bnm_infer_float_device
    // does), then profile it as int8 images
    const uint64_t chunk = n < kProfChunk ? n : kProfChunk;
    DevBuf &q8 = stream_scratch(c, s).q8;
    if (int e = q8.ensure((size_t)chunk * 256u + 64u)) return e;
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint64_t cn = n - off < chunk ? n - off : chunk;
        HIP_TRY(bnmk_quantize_input(d_x + off * 256u, cn, (int8_t *)q8.p, c->nonfinite, s));
        if (int e = profiled_locked(c, (const int8_t *)q8.p, cn, d_cls ? d_cls + off : nullptr, d_labels ? d_labels + off : nullptr,
                                    d_counters, s))
            return e;
    }
    c->last_kernel = "quantize_input_kernel+" + c->last_kernel;
    return BNM_OK;
}

}  // extern "C"
