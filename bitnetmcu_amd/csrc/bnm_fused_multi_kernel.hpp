// Several FC models over one image stream (int8 MFMA): fused_fc_multi_kernel.  gfx950 (CDNA4 / MI355X) only.
//
// The formulation of the generic fused kernel (bnm_fused_generic_kernel.hpp, whose device functions this header reuses by
// including it): weight fragments in LDS read as A operands, run-time layer widths, ReLUNorm packed straight into the next layer's
// B operand.  What is different:
//   * the workgroup stages the fragment images of ALL G models of a group into LDS once per launch, back to back; each model
//     keeps its own widths, codec (doubled hidden weights or not) and FP1.3.0 second plane;
//   * a wave's 32-image tile arrives ONCE by LDS-DMA; its layer-1 B operands are read into VGPRs and stay there while the wave
//     walks models 0 .. G-1, so the images cross HBM once per group instead of once per model.  The refill with the wave's next
//     tile is issued as soon as those operands sit in registers: it is in flight for all G models' arithmetic;
//   * per model the (plane count, doubled weights) pair selects one of three instantiations of the layer chain by a wave-uniform
//     branch; inside it everything runs as in the generic kernel's general path.
// Inputs are 256-byte rows (KT0 = 8), one tile per wave.  Model m writes its class ids to a.model[m].cls and, when that pointer
// is set, its int32 logits to a.model[m].logits.
#pragma once
#include "bnm_fused_generic_kernel.hpp"

namespace {

// one model's layer chain on a tile whose layer-1 B operands are b0: class id in cls[0] (both halves of the wave hold it)
template <int MMAX, int SP, bool DBL>
BNM_DEVICE void multi_model(const char *smem, uint32_t l16, const BnmMultiModel &md, const i32x4 (&b0)[1][8], int h, int j, int lane,
                            uint32_t (&cls)[1], uint64_t first_img, uint64_t n, uint32_t nc) {
    const uint32_t M1 = md.M[0], M2 = md.M[1], M3 = md.M[2], M4 = md.M[3];
    i32x4 act[1][MMAX];
    static_for<1, MMAX + 1>([&](auto MI) {
        constexpr int mt = decltype(MI)::value;
        if (M1 == (uint32_t)mt) {
            i32x16 acc[1][mt];
            mma_l1<mt, 8, 0, 8, SP, true, 1>(smem + (md.frag_off[0] + l16), b0, acc);
            relunorm_pack<mt, DBL, MMAX>(acc[0], act[0], h);
        }
    });
    hidden_layer<MMAX, SP, DBL, 1>(smem, l16, md.frag_off[1], M2, M1, act, h);
    uint32_t m_last = M3, k_last = M2, off_last = md.frag_off[2];
    if (M4) {
        hidden_layer<MMAX, SP, DBL, 1>(smem, l16, md.frag_off[2], M3, M2, act, h);
        m_last = M4; k_last = M3; off_last = md.frag_off[3];
    }
    final_layer<MMAX, SP, 1>(smem, l16, off_last, m_last, k_last, act, h, j, lane, cls, md.logits, nullptr, first_img, n, nc,
                             nc <= 16u);
}

}  // namespace

// WPS: waves per SIMD the register budget is compiled for (one workgroup per CU of up to 4 * WPS waves)
template <int MMAX, int WPS>
__global__ __launch_bounds__(256 * WPS) void fused_fc_multi_kernel(BnmMultiArgs a) {
    using G = RowGeom<256>;
    constexpr int KT0 = 8;
    const uint32_t batch = a.batch & 0xFFFFu;
    const uint64_t n = a.n;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nwaves = blockDim.x >> 6;

    // ---- every model's fragment image global -> LDS, once per workgroup ----------------------------------
    const i32x4 *__restrict__ frags = (const i32x4 *)a.frags;
    for (uint32_t o = threadIdx.x * 16u; o < a.w_bytes; o += blockDim.x * 16u) *(i32x4 *)(smem + o) = frags[o >> 4];
    __syncthreads();

    const uint32_t tile_off = a.w_bytes + wave * (uint32_t)G::TILE;
    const uint32_t tile_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) char *)smem + tile_off;
    const uint32_t lane16 = 16u * (uint32_t)lane;
    const uint32_t rd_off = tile_off + (uint32_t)(lane & 31) * 256u + 16u * ((uint32_t)(lane >> 5) ^ G::mask((uint32_t)(lane & 31)));
    uint32_t voff[G::NV];
    {
        const uint32_t rl0 = (16u * (uint32_t)lane) / 256u, cs0 = (uint32_t)lane & (uint32_t)(G::SLOTS - 1);
#pragma unroll
        for (int k = 0; k < G::NV; k++) voff[k] = (rl0 * 256u + 16u * (cs0 ^ G::mask(rl0))) ^ G::xmask(k);
    }

    const uint32_t n_units = (uint32_t)((n + 31ull) >> 5);       // one tile per unit; the launcher refuses n >= 2^36
    auto dma_unit = [&](uint32_t u) {
        const int8_t *base = a.images + (uint64_t)u * (uint64_t)G::TILE;
        const uint64_t first = (uint64_t)u * 32ull;
        if (first + 32ull <= n) {
            dma_group4(tile_lds, base, voff[0], voff[1], voff[2], voff[3]);
            dma_group4(tile_lds + 4096u, base + 4096, voff[0], voff[1], voff[2], voff[3]);
        } else {
            // ragged end: rows past the last image re-read it (never out of bounds)
            const uint32_t nv = (uint32_t)(n - first);
            uint32_t l = (uint32_t)lane;
            asm volatile("" : "+v"(l));
            const uint32_t rl = (16u * l) / 256u, cs = l & (uint32_t)(G::SLOTS - 1);
            static_for<0, G::PIECES>([&](auto TI) {
                constexpr int tt = decltype(TI)::value;
                const uint32_t r = (uint32_t)(tt * G::ROWS_PER_PIECE) + rl;
                const uint32_t src = r < nv ? r : nv - 1u;
                dma_group1(tile_lds + 1024u * tt, base, src * 256u + 16u * (cs ^ G::mask(r & 31u)));
            });
        }
    };

    // ---- work distribution: as in the generic kernel (static first batch, then the split device-wide counter) -----------
    const uint32_t total_waves = gridDim.x * nwaves, wave_id = blockIdx.x * nwaves + wave;
    const uint32_t words = a.batch >> 16, wshift = (uint32_t)__builtin_ctz(words | 0x100u);
    const uint32_t my_word = wave_id & (words - 1u), first_dyn = total_waves >> wshift;
    uint32_t unit = wave_id * batch, left = batch - 1u;
    uint32_t taken = 0;
    if (unit < n_units) dma_unit(unit);

    // the LAST model's class ids of a tile leave one iteration late, behind the refill (see the generic kernel: a store at the end of
    // the body would put its write acknowledgement into the loop top's vmcnt(0) wait); the other models' ids leave as they are known
    uint32_t cls_prev = 0;
    uint32_t *dst_prev = nullptr;
    bool pend = false;
    auto flush_cls = [&]() {
        if (pend) __builtin_nontemporal_store(cls_prev, dst_prev + lane);
    };
    const uint32_t g = a.g;
    while (unit < n_units) {
        if (left == 0u) work_take_issue(taken, a.counter + 16u * my_word, 1u);
        bnm_wait_vmcnt<0>();
        uint32_t next_unit = unit + 1u, next_left = left - 1u;
        uint32_t lv = (uint32_t)lane, l16 = lane16, rd = rd_off;
        asm volatile("" : "+v"(lv), "+v"(l16), "+v"(rd));
        const int j = (int)(lv & 31u), h = (int)(lv >> 5);
        const uint64_t first_img = (uint64_t)unit * 32ull;
        // layer-1 B operands of the tile: read once, held for every model
        i32x4 b0[1][KT0];
#pragma unroll
        for (int s = 0; s < KT0; s++) b0[0][s] = *(const i32x4 *)(smem + (rd ^ (32u * (uint32_t)s)));
        retire_lds_reads();
        if (left == 0u) {
            work_take_wait(taken);
            next_unit = (((first_dyn + taken) << wshift) + my_word) * batch;
            next_left = batch - 1u;
        }
        if (next_unit < n_units) dma_unit(next_unit);
        flush_cls();
        // rows of this tile that exist (the ragged last tile stores only those)
        const uint32_t valid = n - first_img >= 32ull ? 32u : (uint32_t)(n - first_img);
        for (uint32_t m = 0; m < g; m++) {
            const BnmMultiModel &md = a.model[m];
            uint32_t nc = md.n_classes;
            asm volatile("" : "+v"(nc));
            uint32_t cls[1] = {0};
            if (md.sp == 2u) multi_model<MMAX, 2, false>(smem, l16, md, b0, h, j, lane, cls, first_img, n, nc);
            else if (md.dbl) multi_model<MMAX, 1, true>(smem, l16, md, b0, h, j, lane, cls, first_img, n, nc);
            else multi_model<MMAX, 1, false>(smem, l16, md, b0, h, j, lane, cls, first_img, n, nc);
            uint32_t *dst = md.cls + first_img;
            if (m + 1u < g) {
                if ((uint32_t)lane < valid) __builtin_nontemporal_store(cls[0], dst + lane);
            } else {
                cls_prev = cls[0];
                dst_prev = dst;
                pend = (uint32_t)lane < valid;
            }
        }
        unit = next_unit;
        left = next_left;
    }
    flush_cls();
    bnm_wait_vmcnt<0>();   // no LDS-DMA may outlive the workgroup's LDS allocation
    work_block_leave_s(a.counter, total_waves);   // the last wave to leave puts the counter block back to all-zero
}

// waves per SIMD each tile class is compiled for: one fewer than the generic kernel's where the 32 layer-1 operand registers held
// across the models would otherwise spill
constexpr int bnmk_multi_wps(int mclass) { return mclass == 2 ? 4 : mclass == 4 ? 2 : 1; }

#define BNM_MULTI_LAUNCHER(NAME, MMAX)                                                                                       \
    hipError_t NAME(unsigned blocks, unsigned threads, unsigned lds, hipStream_t s, const BnmMultiArgs &a) {               \
        auto fn = fused_fc_multi_kernel<MMAX, bnmk_multi_wps(MMAX)>;                                              \
        if (!blocks) return hipSuccess;                                                                                      \
        if (hipError_t err = bnm_generic_allow_big_lds((const void *)fn); err != hipSuccess) return err;                    \
        fn<<<dim3(blocks), dim3(threads), lds, s>>>(a);                                                                      \
        return hipGetLastError();                                                                                            \
    }
