// Activation profiles, reduction kernel: int8 activation rows [n][stride] (what the layer-wise tap writes: every ReLUNorm output
// of an image side by side) plus class ids and optional labels -> the profile counters of bnm_infer_device_profiled
// (include/bitnetmcu_hip.h has the layout).  gfx950.
//
// A workgroup reduces kRows consecutive images.  Thread t owns the profiled columns t, t + 256, ...: it walks its column down
// the workgroup's rows with the image count and the sum in registers and tallies every non-zero value in the workgroup's LDS
// histogram of that layer (zeros need no update: hist[0] = rows - active is added once per column).  The class ids and labels go
// to LDS counters as well.  Only then does anything reach memory: one 64-bit atomic per non-zero counter per workgroup.
// The 32-bit partials cannot overflow: a workgroup sees at most kRows images, so a sum is below 127 * kRows and a histogram
// bin below kRows * the layer's width.
#include "bnm_device.hpp"
#include "bnm_kernels.h"

namespace {

constexpr uint32_t kRows = 2048;          // images per workgroup
constexpr uint32_t kLdsClasses = 256;     // pred[] in LDS up to this many classes (else straight to the counters)
constexpr uint32_t kLdsConfusion = 64;    // confusion[][] in LDS up to this many classes (16 KiB)

__global__ __launch_bounds__(256) void profile_reduce_kernel(const uint8_t *__restrict__ acts, uint32_t stride, uint64_t n,
                                                             const uint32_t *__restrict__ cls, const int32_t *__restrict__ labels,
                                                             unsigned long long *__restrict__ ctr, BnmProfileDesc d) {
    __shared__ uint32_t hist[BNM_PROFILE_MAX_LAYERS * 128];
    __shared__ uint32_t pred[kLdsClasses];
    __shared__ uint32_t conf[kLdsConfusion * kLdsConfusion];
    __shared__ uint32_t out_of_range;
    const uint32_t t = threadIdx.x, nt = blockDim.x, nc = d.n_classes;
    const bool pred_lds = nc <= kLdsClasses, conf_lds = nc <= kLdsConfusion;
    for (uint32_t i = t; i < d.n_layers * 128u; i += nt) hist[i] = 0;
    if (pred_lds)
        for (uint32_t i = t; i < nc; i += nt) pred[i] = 0;
    if (conf_lds)
        for (uint32_t i = t; i < nc * nc; i += nt) conf[i] = 0;
    if (t == 0) out_of_range = 0;
    __syncthreads();

    const uint64_t r0 = (uint64_t)blockIdx.x * kRows;
    const uint32_t rows = n - r0 < kRows ? (uint32_t)(n - r0) : kRows;
    const uint8_t *base = acts + r0 * stride;
    for (uint32_t c = t; c < d.total; c += nt) {
        uint32_t l = 0;
        while (c >= d.first[l + 1]) l++;
        const uint32_t j = c - d.first[l];
        const uint8_t *p = base + d.col[l] + j;
        uint32_t *h = hist + 128u * l;
        uint32_t act = 0, sum = 0, r = 0;
        for (; r + 4u <= rows; r += 4u) {
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = p[(uint64_t)(r + k) * stride];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                act += v[k] != 0u;
                sum += v[k];
                if (v[k]) atomicAdd(&h[v[k] & 127u], 1u);
            }
        }
        for (; r < rows; r++) {
            const uint32_t v = p[(uint64_t)r * stride];
            act += v != 0u;
            sum += v;
            if (v) atomicAdd(&h[v & 127u], 1u);
        }
        if (rows > act) atomicAdd(&h[0], rows - act);
        if (act) atomicAdd(ctr + d.word[l] + j, (unsigned long long)act);
        if (sum) atomicAdd(ctr + d.word[l] + d.width[l] + j, (unsigned long long)sum);
    }

    unsigned long long *const conf_g = ctr + d.pred + nc;
    for (uint32_t r = t; r < rows; r += nt) {
        const uint32_t k = cls[r0 + r];
        if (k < nc) {
            if (pred_lds) atomicAdd(&pred[k], 1u);
            else atomicAdd(ctr + d.pred + k, 1ull);
        }
        if (labels) {
            const int32_t lab = labels[r0 + r];
            if (lab >= 0 && (uint32_t)lab < nc) {
                if (k < nc) {
                    if (conf_lds) atomicAdd(&conf[(uint32_t)lab * nc + k], 1u);
                    else atomicAdd(conf_g + (uint64_t)lab * nc + k, 1ull);
                }
            } else {
                atomicAdd(&out_of_range, 1u);
            }
        }
    }
    __syncthreads();

    for (uint32_t i = t; i < d.n_layers * 128u; i += nt)
        if (hist[i]) atomicAdd(ctr + d.word[i >> 7] + 2u * d.width[i >> 7] + (i & 127u), (unsigned long long)hist[i]);
    if (pred_lds)
        for (uint32_t i = t; i < nc; i += nt)
            if (pred[i]) atomicAdd(ctr + d.pred + i, (unsigned long long)pred[i]);
    if (conf_lds && labels)
        for (uint32_t i = t; i < nc * nc; i += nt)
            if (conf[i]) atomicAdd(conf_g + i, (unsigned long long)conf[i]);
    if (t == 0) {
        if (labels) {
            atomicAdd(ctr + d.tail, (unsigned long long)rows);
            if (out_of_range) atomicAdd(ctr + d.tail + 1, (unsigned long long)out_of_range);
        }
        atomicAdd(ctr + d.tail + 2, (unsigned long long)rows);
    }
}

}  // namespace

hipError_t bnmk_profile_reduce(const int8_t *acts, uint32_t stride, uint64_t n, const uint32_t *cls, const int32_t *labels,
                               uint64_t *counters, const BnmProfileDesc &d, hipStream_t s) {
    if (!n) return hipSuccess;
    if (d.n_layers > BNM_PROFILE_MAX_LAYERS) return hipErrorInvalidValue;
    const uint64_t blocks = (n + kRows - 1) / kRows;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    profile_reduce_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>((const uint8_t *)acts, stride, n, cls, labels,
                                                                      (unsigned long long *)counters, d);
    return hipGetLastError();
}
