// The profiling variant of the generic fused FC kernel (fused_fc_generic_prof_kernel, bnm_fused_generic_kernel.hpp): class ids plus
// the activation-profile tallies in the same pass.  Instantiated for one tile per wave, tile classes 2 and 4, 256-byte rows (FC
// models); every other model profiles through the layer-wise tap + profile_reduce_kernel (bnm_capi_profile.cpp).
#include "bnm_fused_generic_kernel.hpp"

namespace {
constexpr uint32_t kLdsBytes = 160u * 1024u;
typedef void (*prof_fn)(const int8_t *, uint64_t, const i32x4 *, BnmGenericDesc, uint32_t *, uint32_t *, uint32_t, BnmFusedProf);
template <int MMAX>
prof_fn pick(uint32_t sp, bool dbl) {
    if (sp == 1 && dbl) return fused_fc_generic_prof_kernel<MMAX, 8, 1, true, bnmk_generic_wps(MMAX, 8, 1, 1)>;
    if (sp == 1) return fused_fc_generic_prof_kernel<MMAX, 8, 1, false, bnmk_generic_wps(MMAX, 8, 1, 1)>;
    if (sp == 2 && !dbl) return fused_fc_generic_prof_kernel<MMAX, 8, 2, false, bnmk_generic_wps(MMAX, 8, 2, 1)>;
    return nullptr;
}
prof_fn prof_of(const BnmGenericDesc &d, bool dbl) {
    if (d.KT0 != 8) return nullptr;
    return d.mmax == 2 ? pick<2>(d.sp, dbl) : d.mmax == 4 ? pick<4>(d.sp, dbl) : nullptr;
}
}  // namespace

uint32_t bnmk_fused_generic_prof_waves(const BnmGenericDesc &d, bool dbl) {
    if (!prof_of(d, dbl) || d.n_classes == 0 || d.n_classes > 64u) return 0;
    const uint32_t fixed = d.w_bytes + 4u * kProfWords(d.n_classes);
    const uint32_t per_wave = 1024u * d.KT0 + 1024u * d.mmax;      // tile buffer + transpose buffer
    if (fixed + per_wave > kLdsBytes) return 0;
    const uint32_t w = (kLdsBytes - fixed) / per_wave, cap = 4u * (uint32_t)bnmk_generic_wps((int)d.mmax, (int)d.KT0, (int)d.sp, 1);
    return w < cap ? w : cap;
}

hipError_t bnmk_fused_generic_prof(const BnmGenericDesc &d_in, bool dbl, int grid_blocks, const int8_t *images, uint64_t n, const void *frags,
                                   uint32_t *cls, uint32_t *counter, uint32_t batch, const BnmFusedProf &pa, hipStream_t s) {
    const prof_fn fn = prof_of(d_in, dbl);
    const uint32_t waves = bnmk_fused_generic_prof_waves(d_in, dbl);
    if (!fn || !waves || !counter || !pa.ctr || pa.n_layers > 4 || pa.n_classes != d_in.n_classes) return hipErrorInvalidValue;
    if (!n) return hipSuccess;
    if (n > (1ull << 22)) return hipErrorInvalidValue;
    BnmGenericDesc d = d_in;
    d.stage = 0;
    if (!batch) batch = 4u;
    if (batch > 0xFFFFu) batch = 0xFFFFu;
    const uint32_t lds = d.w_bytes + waves * (1024u * d.KT0 + 1024u * d.mmax) + 4u * kProfWords(d.n_classes);
    const uint64_t n_units = (n + 31ull) / 32ull;
    const uint64_t want = (n_units + (uint64_t)waves * batch - 1) / ((uint64_t)waves * batch);
    const uint64_t cap = grid_blocks > 0 ? (uint64_t)grid_blocks : (uint64_t)bnm_num_cus();
    const uint64_t blocks = want < cap ? want : cap;
    const uint32_t words = ((blocks * waves) & 7ull) == 0ull ? 8u : 1u;
    if (hipError_t e = bnm_generic_allow_big_lds((const void *)fn); e != hipSuccess) return e;
    fn<<<dim3((unsigned)blocks), dim3(64u * waves), lds, s>>>(images, n, (const i32x4 *)frags, d, cls, counter, batch | (words << 16), pa);
    return hipGetLastError();
}
