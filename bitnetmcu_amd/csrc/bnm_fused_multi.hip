// Several FC models over one image stream: launch planning of fused_fc_multi_kernel (bnm_fused_multi_kernel.hpp) and its
// 2-tile class instantiation (the 4-, 6- and 8-tile classes are bnm_fused_multi_m{4,6,8}.hip, compiled side by side).
#include "bnm_fused_multi_kernel.hpp"

BNM_MULTI_LAUNCHER(bnmk_multi_launch_m2, 2)
hipError_t bnmk_multi_launch_m4(unsigned blocks, unsigned threads, unsigned lds, hipStream_t s, const BnmMultiArgs &a);
hipError_t bnmk_multi_launch_m6(unsigned blocks, unsigned threads, unsigned lds, hipStream_t s, const BnmMultiArgs &a);
hipError_t bnmk_multi_launch_m8(unsigned blocks, unsigned threads, unsigned lds, hipStream_t s, const BnmMultiArgs &a);

namespace {
constexpr uint32_t kMultiLdsBytes = 160u * 1024u;
constexpr uint32_t kMultiTileBytes = 8192u;      // one 32-image tile of 256-byte rows per wave
}  // namespace

uint32_t bnmk_multi_class(uint32_t mmax) { return mmax <= 2 ? 2u : mmax <= 4 ? 4u : mmax <= 6 ? 6u : 8u; }

uint32_t bnmk_multi_waves(uint32_t w_bytes, uint32_t mclass) {
    if (w_bytes + kMultiTileBytes > kMultiLdsBytes) return 0;
    const uint32_t w = (kMultiLdsBytes - w_bytes) / kMultiTileBytes;
    const uint32_t cap = 4u * (uint32_t)bnmk_multi_wps((int)mclass);
    return w < cap ? w : cap;
}

hipError_t bnmk_fused_multi(uint32_t mclass, int grid_blocks, BnmMultiArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    if (a.n >= (1ull << 36) || !a.counter || !a.g || a.g > BNM_MULTI_MAX_MODELS || (a.w_bytes & 1023u)) return hipErrorInvalidValue;
    const uint32_t waves = bnmk_multi_waves(a.w_bytes, mclass);
    if (!waves) return hipErrorInvalidValue;
    // tiles per take and counter words as in the generic kernel's launcher (bnm_fused_generic.hip)
    const uint32_t batch = 4u;
    const uint64_t n_units = (a.n + 31ull) / 32ull;
    const uint64_t want = (n_units + (uint64_t)waves * batch - 1) / ((uint64_t)waves * batch);
    const uint64_t cap = grid_blocks > 0 ? (uint64_t)grid_blocks : (uint64_t)bnm_num_cus();
    const uint64_t blocks = want < cap ? want : cap;
    const uint32_t words = ((blocks * waves) & 7ull) == 0ull ? 8u : 1u;
    a.batch = batch | (words << 16);
    const unsigned lds = a.w_bytes + waves * kMultiTileBytes;
    switch (mclass) {
        case 2: return bnmk_multi_launch_m2((unsigned)blocks, 64u * waves, lds, s, a);
        case 4: return bnmk_multi_launch_m4((unsigned)blocks, 64u * waves, lds, s, a);
        case 6: return bnmk_multi_launch_m6((unsigned)blocks, 64u * waves, lds, s, a);
        case 8: return bnmk_multi_launch_m8((unsigned)blocks, 64u * waves, lds, s, a);
    }
    return hipErrorInvalidValue;
}
