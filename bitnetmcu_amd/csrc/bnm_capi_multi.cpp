// C ABI, several FC models over one image batch (bnm_multi_*): the planner that groups the models into LDS-sized groups, the
// launches of fused_fc_multi_kernel (bnm_fused_multi.hip) - one per group, each reading the images once - and the models that
// run through their own single-model context because their fragment image alone does not fit a group.
#include "bnm_capi_internal.hpp"

using namespace bnm_internal;

namespace {

// LDS a group's fragment images may take: 160 KiB less the tile buffers of five waves (5 x 8 KiB).  Fewer waves per CU hide too
// little of the LDS and matrix-core latency: a group of 124 KiB (four waves) ran slower than its two models' single calls
// (profiles/probes/multi_model_rate.py)
constexpr uint32_t kGroupBudget = 160u * 1024u - 5u * 8192u;
constexpr uint64_t kFloatChunk = 1ull << 22;      // images per quantisation chunk of the float path (1 GiB of int8 scratch)
constexpr uint64_t kHostChunk = 1ull << 20;       // images per staging chunk of the host-pointer path

struct MultiGroup {
    uint32_t mclass = 2;          // tile class of the launch: the largest of its models'
    uint32_t w_bytes = 0;         // the models' fragment images back to back
    void *frags = nullptr;
    std::vector<uint32_t> rows;   // the caller's model index of each member, in order
    std::vector<BnmMultiModel> md;
};

}  // namespace

struct bnm_multi {
    int device = 0;
    uint32_t k = 0;
    std::vector<bnm_ctx *> ctx;             // one per model (the source of its fragment image, and the path of a model run alone)
    std::vector<uint32_t> ncls;
    std::vector<MultiGroup> groups;
    std::vector<uint32_t> alone;            // models run through their own context
    std::map<hipStream_t, uint32_t *> work_of;     // counter block per stream (as bnm_ctx::work_of)
    std::map<hipStream_t, DevBuf> q8;               // float path: quantised images of one chunk, per stream
    std::map<hipStream_t, hipEvent_t> float_done;   // float path: the last float call on each stream
    unsigned long long *nonfinite = nullptr;        // float calls: images that held a NaN or an infinity so far
    unsigned long long *nonfinite_host = nullptr;   // page-locked landing word of bnm_multi_float_nonfinite
    hipStream_t aux = nullptr;                      // non-blocking stream of the host path and of the counter read
    DevBuf h_in, h_cls, h_logits;
    std::mutex mu;
};

namespace {

int multi_work_block(bnm_multi *mc, hipStream_t s, uint32_t **out) {
    const hipStream_t key = stream_key(s);
    auto it = mc->work_of.find(key);
    if (it != mc->work_of.end()) { *out = it->second; return BNM_OK; }
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, BNM_WORK_BLOCK_WORDS * 4));
    mc->work_of[key] = (uint32_t *)p;
    HIP_TRY(hipMemsetAsync(p, 0, BNM_WORK_BLOCK_WORDS * 4, s));
    *out = (uint32_t *)p;
    return BNM_OK;
}

// n images [n][256] on the device -> rows of d_cls with stride `stride` (row r of model r starts at d_cls + r * stride), logits of
// model r at d_logits[r] (when given); mc->mu held, the device current
int multi_run(bnm_multi *mc, const int8_t *d_images, uint64_t n, uint32_t *d_cls, uint64_t stride, int32_t *const *d_logits, hipStream_t s) {
    if (!n) return BNM_OK;
    uint32_t *block = nullptr;
    if (!mc->groups.empty())
        if (int e = multi_work_block(mc, s, &block)) return e;
    for (const MultiGroup &g : mc->groups) {
        BnmMultiArgs a{};
        a.images = d_images;
        a.n = n;
        a.frags = g.frags;
        a.w_bytes = g.w_bytes;
        a.g = (uint32_t)g.rows.size();
        a.counter = block;
        for (uint32_t i = 0; i < a.g; i++) {
            const uint32_t r = g.rows[i];
            a.model[i] = g.md[i];
            a.model[i].cls = d_cls + (uint64_t)r * stride;
            a.model[i].logits = d_logits ? d_logits[r] : nullptr;
        }
        HIP_TRY(bnmk_fused_multi(g.mclass, 0, a, s));
    }
    for (uint32_t r : mc->alone)
        if (int e = bnm_infer_device(mc->ctx[r], d_images, n, d_cls + (uint64_t)r * stride, d_logits ? d_logits[r] : nullptr, s)) return e;
    return BNM_OK;
}

// the argument checks every inference entry point makes before anything touches the device
int check_outputs(const bnm_multi *mc, const uint32_t *cls, int32_t *const *logits) {
    if (!cls) return fail(BNM_EINVAL, "null class-id pointer");
    if ((uintptr_t)cls & 3u) return fail(BNM_EINVAL, "the class-id buffer must be 4-byte aligned");
    if (logits)
        for (uint32_t r = 0; r < mc->k; r++) {
            if (!logits[r]) return fail(BNM_EINVAL, "null logits pointer (pass NULL for the whole array to skip logits)");
            if ((uintptr_t)logits[r] & 3u) return fail(BNM_EINVAL, "logits buffers must be 4-byte aligned");
        }
    return BNM_OK;
}

int multi_plan(bnm_multi *mc) {
    MultiGroup cur;
    auto close_group = [&]() -> int {
        if (cur.rows.empty()) return BNM_OK;
        if (cur.rows.size() == 1) {
            // a group of one reads the images once either way: the model's own context runs it with its best kernel (more waves
            // per CU than the multi-model kernel's tile class leaves, or the shape-specialised kernels)
            mc->alone.push_back(cur.rows[0]);
            cur = MultiGroup{};
            return BNM_OK;
        }
        HIP_TRY(hipMalloc(&cur.frags, cur.w_bytes));
        uint32_t off = 0;
        for (uint32_t r : cur.rows) {
            const bnm_ctx *c = mc->ctx[r];
            HIP_TRY(hipMemcpy((char *)cur.frags + off, c->gfrags, c->gdesc.w_bytes, hipMemcpyDeviceToDevice));
            off += c->gdesc.w_bytes;
        }
        mc->groups.push_back(cur);
        cur = MultiGroup{};
        return BNM_OK;
    };
    for (uint32_t r = 0; r < mc->k; r++) {
        const bnm_ctx *c = mc->ctx[r];
        const BnmGenericDesc &d = c->gdesc;
        if (!c->generic_ok || d.KT0 != 8u || d.w_bytes > kGroupBudget) {
            mc->alone.push_back(r);
            continue;
        }
        if (cur.w_bytes + d.w_bytes > kGroupBudget || cur.rows.size() == BNM_MULTI_MAX_MODELS)
            if (int e = close_group()) return e;
        BnmMultiModel md{};
        for (int i = 0; i < 4; i++) {
            md.M[i] = d.M[i];
            md.frag_off[i] = cur.w_bytes + d.frag_off[i];
        }
        md.sp = d.sp;
        md.dbl = c->shape.dbl ? 1u : 0u;
        md.n_classes = d.n_classes;
        const uint32_t mc_class = bnmk_multi_class(d.mmax);
        cur.mclass = mc_class > cur.mclass ? mc_class : cur.mclass;
        cur.w_bytes += d.w_bytes;
        cur.rows.push_back(r);
        cur.md.push_back(md);
    }
    return close_group();
}

}  // namespace

extern "C" {

void bnm_multi_destroy(bnm_multi *mc) {
    if (!mc) return;
    {
        DeviceGuard dg(mc->device);
        for (auto &g : mc->groups)
            if (g.frags) (void)hipFree(g.frags);      // (hipFree waits for the device: no launch of this object is left running)
        for (auto &kv : mc->work_of) (void)hipFree(kv.second);
        for (auto &kv : mc->q8) kv.second.release(true);
        for (auto &kv : mc->float_done) (void)hipEventDestroy(kv.second);
        if (mc->nonfinite) (void)hipFree(mc->nonfinite);
        if (mc->nonfinite_host) (void)hipHostFree(mc->nonfinite_host);
        for (DevBuf *b : {&mc->h_in, &mc->h_cls, &mc->h_logits}) b->release(true);
        if (mc->aux) (void)hipStreamDestroy(mc->aux);
    }
    for (bnm_ctx *c : mc->ctx) bnm_ctx_destroy(c);
    delete mc;
}

int bnm_multi_create(const bnm_model *const *models, uint32_t k, int device, bnm_multi **out) {
    if (!out) return fail(BNM_EINVAL, "null output pointer");
    *out = nullptr;
    if (!models) return fail(BNM_EINVAL, "null model array");
    if (k == 0 || k > BNM_MULTI_MAX_MODELS) return fail(BNM_EINVAL, "k must be 1 .. 16 models");
    for (uint32_t r = 0; r < k; r++) {
        if (!models[r]) return fail(BNM_EINVAL, "null model in the array");
        if (bnm_model_kind(models[r]) != BNM_KIND_FC)
            return fail(BNM_EUNSUPPORTED, "model " + std::to_string(r) + " is a CNN: multi-model calls serve FC models only");
        if (bnm_model_input_bytes(models[r]) != 256u)
            return fail(BNM_EUNSUPPORTED, "model " + std::to_string(r) + ": multi-model calls serve 256-byte inputs only");
    }
    bnm_multi *mc = new bnm_multi();
    mc->k = k;
    for (uint32_t r = 0; r < k; r++) {
        bnm_ctx *c = nullptr;
        if (int e = bnm_ctx_create(models[r], device, &c)) {
            std::string keep = g_err;
            bnm_multi_destroy(mc);
            g_err = keep;
            return e;
        }
        mc->ctx.push_back(c);
        mc->ncls.push_back(c->model.num_classes());
        if (!c->generic_ok && !c->fused_ok) {
            const std::string msg = "model " + std::to_string(r) + " has no fused MFMA path: " + c->fused_reason;
            bnm_multi_destroy(mc);
            return fail(BNM_EUNSUPPORTED, msg);
        }
    }
    mc->device = mc->ctx[0]->device;
    DeviceGuard dg(mc->device);
    int e = dg.err == hipSuccess ? BNM_OK : fail(BNM_EHIP, "hipSetDevice failed");
    if (!e) e = multi_plan(mc);
    if (!e && hipMalloc((void **)&mc->nonfinite, sizeof(unsigned long long)) != hipSuccess) e = fail(BNM_EHIP, "hipMalloc failed");
    if (!e && hipMemset(mc->nonfinite, 0, sizeof(unsigned long long)) != hipSuccess) e = fail(BNM_EHIP, "hipMemset failed");
    if (!e && hipHostMalloc((void **)&mc->nonfinite_host, sizeof(unsigned long long)) != hipSuccess) e = fail(BNM_EHIP, "hipHostMalloc failed");
    if (!e && hipStreamCreateWithFlags(&mc->aux, hipStreamNonBlocking) != hipSuccess) e = fail(BNM_EHIP, "hipStreamCreate failed");
    if (!e && hipDeviceSynchronize() != hipSuccess) e = fail(BNM_EHIP, "hipDeviceSynchronize failed");
    if (e) {
        std::string keep = g_err;
        bnm_multi_destroy(mc);
        g_err = keep;
        return e;
    }
    *out = mc;
    return BNM_OK;
}

int bnm_multi_groups(const bnm_multi *mc) {
    if (!mc) return fail(BNM_EINVAL, "null multi-model context");
    return (int)(mc->groups.size() + mc->alone.size());
}

int bnm_multi_infer_device(bnm_multi *mc, const int8_t *d_images, uint64_t n, uint32_t *d_cls, int32_t *const *d_logits, void *stream) {
    if (!mc) return fail(BNM_EINVAL, "null multi-model context");
    if (!n) return BNM_OK;
    if (!d_images) return fail(BNM_EINVAL, "null device pointer");
    if ((uintptr_t)d_images & 15u) return fail(BNM_EINVAL, "d_images must be 16-byte aligned");
    if (int e = check_outputs(mc, d_cls, d_logits)) return e;
    std::lock_guard<std::mutex> g(mc->mu);
    DeviceGuard dg(mc->device);
    HIP_TRY(dg.err);
    return multi_run(mc, d_images, n, d_cls, n, d_logits, (hipStream_t)stream);
}

int bnm_multi_infer_float_device(bnm_multi *mc, const float *d_x, uint64_t n, uint32_t *d_cls, int32_t *const *d_logits, void *stream) {
    if (!mc) return fail(BNM_EINVAL, "null multi-model context");
    if (!n) return BNM_OK;
    if (!d_x) return fail(BNM_EINVAL, "null device pointer");
    if ((uintptr_t)d_x & 15u) return fail(BNM_EINVAL, "d_x must be 16-byte aligned");
    if (int e = check_outputs(mc, d_cls, d_logits)) return e;
    std::lock_guard<std::mutex> g(mc->mu);
    DeviceGuard dg(mc->device);
    HIP_TRY(dg.err);
    hipStream_t s = (hipStream_t)stream;
    const hipStream_t key = stream_key(s);
    DevBuf &q8 = mc->q8[key];
    if (int e = q8.ensure((size_t)(n < kFloatChunk ? n : kFloatChunk) * 256 + 64)) return e;
    // quantised ONCE per chunk, every model runs on the same int8 rows
    std::vector<int32_t *> lg(mc->k, nullptr);
    for (uint64_t off = 0; off < n; off += kFloatChunk) {
        const uint64_t cn = n - off < kFloatChunk ? n - off : kFloatChunk;
        HIP_TRY(bnmk_quantize_input(d_x + off * 256, cn, (int8_t *)q8.p, mc->nonfinite, s));
        if (d_logits)
            for (uint32_t r = 0; r < mc->k; r++) lg[r] = d_logits[r] + off * mc->ncls[r];
        if (int e = multi_run(mc, (const int8_t *)q8.p, cn, d_cls + off, n, d_logits ? lg.data() : nullptr, s)) return e;
    }
    hipEvent_t &ev = mc->float_done[key];
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev, s));
    return BNM_OK;
}

int bnm_multi_infer_host(bnm_multi *mc, const int8_t *images, uint64_t n, uint32_t *cls, int32_t *const *logits) {
    if (!mc) return fail(BNM_EINVAL, "null multi-model context");
    if (!n) return BNM_OK;
    if (!images) return fail(BNM_EINVAL, "null image pointer");
    if (int e = check_outputs(mc, cls, logits)) return e;
    std::lock_guard<std::mutex> g(mc->mu);
    DeviceGuard dg(mc->device);
    HIP_TRY(dg.err);
    const uint64_t chunk = n < kHostChunk ? n : kHostChunk;
    uint64_t lg_total = 0;
    for (uint32_t r = 0; r < mc->k; r++) lg_total += mc->ncls[r];
    if (int e = mc->h_in.ensure((size_t)chunk * 256 + 64)) return e;
    if (int e = mc->h_cls.ensure((size_t)chunk * mc->k * 4)) return e;
    if (logits)
        if (int e = mc->h_logits.ensure((size_t)chunk * lg_total * 4)) return e;
    std::vector<int32_t *> d_lg(mc->k, nullptr);
    for (uint32_t r = 0, o = 0; r < mc->k; o += mc->ncls[r], r++) d_lg[r] = logits ? (int32_t *)mc->h_logits.p + (uint64_t)o * chunk : nullptr;
    hipStream_t s = mc->aux;
    for (uint64_t off = 0; off < n; off += chunk) {
        const uint64_t cn = n - off < chunk ? n - off : chunk;
        HIP_TRY(hipMemcpyAsync(mc->h_in.p, images + off * 256, cn * 256, hipMemcpyHostToDevice, s));
        if (int e = multi_run(mc, (const int8_t *)mc->h_in.p, cn, (uint32_t *)mc->h_cls.p, cn, logits ? d_lg.data() : nullptr, s)) return e;
        for (uint32_t r = 0; r < mc->k; r++) {
            HIP_TRY(hipMemcpyAsync(cls + (uint64_t)r * n + off, (uint32_t *)mc->h_cls.p + (uint64_t)r * cn, cn * 4, hipMemcpyDeviceToHost, s));
            if (logits)
                HIP_TRY(hipMemcpyAsync(logits[r] + off * mc->ncls[r], d_lg[r], cn * mc->ncls[r] * 4, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    return BNM_OK;
}

int bnm_multi_float_nonfinite(bnm_multi *mc, uint64_t *count) {
    if (!mc || !count) return fail(BNM_EINVAL, "null argument");
    std::lock_guard<std::mutex> g(mc->mu);
    DeviceGuard dg(mc->device);
    HIP_TRY(dg.err);
    // only this object's float calls feed the counter: wait for the last one on each stream, then a copy on its own stream (no
    // device-wide synchronisation - other contexts' kernels, a resident one among them, are not waited for)
    for (auto &kv : mc->float_done) HIP_TRY(hipEventSynchronize(kv.second));
    HIP_TRY(hipMemcpyAsync(mc->nonfinite_host, mc->nonfinite, sizeof(unsigned long long), hipMemcpyDeviceToHost, mc->aux));
    HIP_TRY(hipStreamSynchronize(mc->aux));
    *count = (uint64_t)*mc->nonfinite_host;
    return BNM_OK;
}

}  // extern "C"
