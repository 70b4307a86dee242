// Generic fused whole-model FC kernel (int8 MFMA): ANY exporter-producible layer widths up to 256 per layer, 3 or 4 FC
// layers, any class count <= 256, input rows of 64/128/256/512 bytes, every int8-representable codec plus FP1.3.0's
// +128 (second weight plane).  gfx950 (CDNA4 / MI355X) only.  Reference semantics: BitNetMCU_inference.c:23-72
// (ReLUNorm), :88-208 (processfclayer); schedule BitNetMCU_MNIST_dll.c:48-121; widths are free parameters of the
// reference's model zoo (models.py:62-84; the documented 12 KB family docs/documentation.md:169-183).
//
// Same formulation as bnm_fused_fc.hip (Y^T = W * X^T on v_mfma_i32_32x32x32_i8, ReLUNorm output packed straight into
// the next layer's B operand).  What makes it shape-free:
//   * the weight fragments live in LDS (one copy per workgroup = per CU, staged once per launch) and are read as A
//     operands with lane-linear ds_read_b128 - no weight VGPRs, so no shape can spill;
//   * the layer widths are RUN-TIME values and nothing is padded: a layer of M 32-row tiles over K K-steps executes exactly
//     M*K MFMAs and its fragment image holds exactly M*K KiB.  Per layer the kernel switches (wave-uniformly) on the tile
//     count M - inside a case every accumulator index is a compile-time constant - and walks the K-steps in source order
//     with an early exit behind each one (K-steps are compile-time positions, so the packed activations stay in registers).
//     The fragments of a layer are stored K-step major ([plane][K-step][tile]): with M fixed inside a case, every fragment
//     address is the lane's base plus an immediate offset.  Only the upper bound MMAX of tiles per layer (2 / 4 / 8) is a
//     template parameter: it sizes the register arrays;
//   * T = 1 or 2 image tiles per wave per iteration.  With T = 2 every fragment read from LDS feeds TWO MFMAs (one per
//     tile): half the LDS traffic per image - at one fragment read per MFMA the matrix cores of a CU ask the LDS for exactly
//     its peak 128 B per clock - and two independent dependency chains inside a wave;
//   * the tile buffers are refilled with the wave's next unit by LDS-DMA as soon as the layer-1 B operands sit in registers,
//     so the load is in flight for the whole of the unit's arithmetic.
// LDS image of a tile: row r (image) at r*ROW, 16-byte slot c' holds global slot c = c' ^ mask(r) with
// mask(r) = (r >> (4-p)) & (S-1) for S = ROW/16 = 2^p slots per row (p <= 4) and r & 15 for p = 5: the ds_read_b128
// lane groups (MI355X_MICROARCH.md, LDS table) then hit 16 distinct 16-byte bank groups for every supported ROW.  The
// swizzle is applied on the SOURCE address of the DMA (its LDS destination is lane-linear).
#pragma once
#include <mutex>
#include <type_traits>
#include <set>
#include <utility>
#include "bnm_fused_tile.hpp"
#include "bnm_fused_math.hpp"

// fragment reads in flight ahead of their MFMAs (a translation unit may set it before including this header)
#ifndef BNM_FRAG_DEPTH
#define BNM_FRAG_DEPTH 4
#endif

namespace {

// Diagnostic build only (build.py --diag-timing): shader-clock stamps at the phase boundaries of the uniform path, summed per wave
// and written where the caller's `logits` point (profiles/r05/r05_generic_phases.py).  Nothing of it exists in the product build.
#ifdef BNM_DIAG_TIMING
struct PhaseStamps {
    uint64_t last;
    uint32_t sum[12];
    BNM_DEVICE void start() { last = __builtin_amdgcn_s_memtime(); }
    BNM_DEVICE void tick(int k) {
        __builtin_amdgcn_sched_barrier(0);      // (a wave issues in order: the stamp is taken once everything before it has been issued)
        const uint64_t t = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        sum[k] += (uint32_t)(t - last);
        last = t;
    }
};
#define BNM_ST_PARAM , PhaseStamps &st
#define BNM_ST_ARG , st
#define BNM_TICK(k) st.tick(k)
#else
#define BNM_ST_PARAM
#define BNM_ST_ARG
#define BNM_TICK(k)
#endif

// wave-uniform values that the compiler may nevertheless have placed in VGPRs: back to SGPRs for the "s" constraints
BNM_DEVICE uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
BNM_DEVICE const int8_t *uni(const int8_t *p) {
    uint64_t v = (uint64_t)p;
    return (const int8_t *)(((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v));
}
// up to four 1 KiB LDS-DMA pieces that share one M0 setting (the instruction offset is added to both addresses)
#define BNM_DMA_GROUP(BODY, ...)                                                                  \
    asm volatile("s_mov_b32 %0, m0\n\t"                                                           \
                 "s_mov_b32 m0, %1\n\t"                                                           \
                 "s_nop 0\n\t" BODY "s_mov_b32 m0, %0"                                            \
                 : "=&s"(keep)                                                                    \
                 : "s"(lds), "s"(base), __VA_ARGS__                                               \
                 : "memory")
BNM_DEVICE void dma_group4(uint32_t lds_, const int8_t *base_, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
    uint32_t keep;
    const uint32_t lds = uni(lds_);
    const int8_t *base = uni(base_);
    BNM_DMA_GROUP("global_load_lds_dwordx4 %3, %2 nt\n\t"
                  "global_load_lds_dwordx4 %4, %2 offset:1024 nt\n\t"
                  "global_load_lds_dwordx4 %5, %2 offset:2048 nt\n\t"
                  "global_load_lds_dwordx4 %6, %2 offset:3072 nt\n\t",
                  "v"(v0), "v"(v1), "v"(v2), "v"(v3));
}
BNM_DEVICE void dma_group2(uint32_t lds_, const int8_t *base_, uint32_t v0, uint32_t v1) {
    uint32_t keep;
    const uint32_t lds = uni(lds_);
    const int8_t *base = uni(base_);
    BNM_DMA_GROUP("global_load_lds_dwordx4 %3, %2 nt\n\t"
                  "global_load_lds_dwordx4 %4, %2 offset:1024 nt\n\t",
                  "v"(v0), "v"(v1));
}
BNM_DEVICE void dma_group1(uint32_t lds_, const int8_t *base_, uint32_t v0) {
    uint32_t keep;
    const uint32_t lds = uni(lds_);
    const int8_t *base = uni(base_);
    BNM_DMA_GROUP("global_load_lds_dwordx4 %3, %2 nt\n\t", "v"(v0));
}
// before overwriting a buffer: this wave's own ds_reads of it must have returned (hipcc only waits before the USE of
// a ds_read's result); the s_nop covers a VALU-written SGPR feeding M0
BNM_DEVICE void retire_lds_reads() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 4" ::: "memory"); }
// a point no memory operation may be moved across by the compiler (no instruction is emitted): keeps a fragment read that is
// issued ahead of a branch from being sunk into the block that uses it
BNM_DEVICE void pin_memory_order() { asm volatile("" ::: "memory"); }

template <int ROW>
struct RowGeom {
    static constexpr int SLOTS = ROW / 16;
    static constexpr int P = ROW == 64 ? 2 : ROW == 128 ? 3 : ROW == 256 ? 4 : 5;
    static_assert(ROW == 64 || ROW == 128 || ROW == 256 || ROW == 512, "row bytes must be 64, 128, 256 or 512");
    static constexpr int TILE = 32 * ROW;
    static constexpr int PIECES = TILE / 1024;
    static constexpr int ROWS_PER_PIECE = 1024 / ROW;
    // distinct per-piece source offsets: xmask() below has this period
    static constexpr int NV = ROW == 64 ? 1 : ROW == 128 ? 2 : ROW == 256 ? 4 : 8;
    BNM_DEVICE static uint32_t mask(uint32_t r) { return P == 5 ? (r & 15u) : ((r >> (4 - P)) & (uint32_t)(SLOTS - 1)); }
    // what piece t XORs into the lane's piece-relative source offset (see the derivation in DESIGN.md §4.1b)
    static constexpr uint32_t xmask(int t) { return P == 5 ? ((32u * t) & 0xF0u) : ((64u * t) & (uint32_t)(ROW - 16)); }
};

// ---- MFMA streams ------------------------------------------------------------------------------------------------
// Items are (plane p, K-step s, tile m), K-step outermost inside a plane so that consecutive MFMAs go to DIFFERENT
// accumulators (no dependent-accumulator stalls); every item reads ONE fragment and issues T MFMAs (one per image tile of the
// wave).  Fragment reads are issued DEPTH items ahead of their MFMAs in source order and the order is pinned with
// sched_group_barrier - left to itself hipcc put every ds_read directly in front of its MFMA and paid the full LDS latency per
// item.  Fragment (p, s, m) of a layer with MT tiles and KTOT K-steps sits at ((p*KTOT + s)*MT + m) KiB, lane-linear.

// NS compile-time K-steps S0 .. S0+NS-1 of KTOT: layer 1 (or a chunk of its K-steps), and every layer of the uniform fast path
template <int MT, int NS, int S0, int KTOT, int SP, bool INIT, int T, int NB = NS>
BNM_DEVICE void mma_l1(const char *a, const i32x4 (&b)[T][NB], i32x16 (&acc)[T][MT]) {
    static_assert(NS <= NB, "operand array too short");
    constexpr int N = SP * NS * MT;
    constexpr int DEPTH = N < BNM_FRAG_DEPTH ? N : BNM_FRAG_DEPTH;
    auto frag = [&](auto I) -> i32x4 {
        constexpr int i = decltype(I)::value;
        constexpr int pp = i / (NS * MT), ss = (i % (NS * MT)) / MT, mm = i % MT;
        return *(const i32x4 *)(a + ((pp * KTOT + S0 + ss) * MT + mm) * 1024);
    };
    __builtin_amdgcn_sched_barrier(0);      // the stream is its own scheduling region
    i32x4 ring[DEPTH];
    static_for<0, DEPTH>([&](auto I) { ring[decltype(I)::value] = frag(I); });
    static_for<0, N>([&](auto I) {
        constexpr int i = decltype(I)::value;
        constexpr int pp = i / (NS * MT), ss = (i % (NS * MT)) / MT, mm = i % MT;
#pragma unroll
        for (int t = 0; t < T; t++) {
            const i32x16 c = (INIT && pp == 0 && ss == 0) ? zero16() : acc[t][mm];
            acc[t][mm] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ring[i % DEPTH], b[t][ss], c, 0, 0, 0);
        }
        if constexpr (i + DEPTH < N) ring[i % DEPTH] = frag(std::integral_constant<int, i + DEPTH>{});
    });
    // pin the issue order: DEPTH fragment reads, then { T MFMAs, one read } groups (0x100 = DS read, 0x008 = MFMA)
    __builtin_amdgcn_sched_group_barrier(0x100, DEPTH, 0);
    static_for<0, N>([&](auto I) {
        __builtin_amdgcn_sched_group_barrier(0x008, T, 0);
        if constexpr (decltype(I)::value + DEPTH < N) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    });
    __builtin_amdgcn_sched_barrier(0);
}

// layers 2..4, one plane: K (run-time, 1 .. MMAX) K-steps.  K-step S is a compile-time position (its B operands are the
// registers in[.][S]); behind every K-step the chain leaves when K is reached.  The ring is primed by the caller; reads run
// DEPTH items ahead across the exits (an exit drops at most DEPTH reads of fragments that exist but are not needed - or of
// whatever follows the layer's last fragment in LDS: the next layer's fragments or the tile buffers, never out of bounds).
template <int S, int MT, int T, int MMAX, int DEPTH, bool INIT>
BNM_DEVICE void hidden_steps(const char *a, uint32_t K, const i32x4 (&in)[T][MMAX], i32x16 (&acc)[T][MT], i32x4 (&ring)[DEPTH]) {
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, MT>([&](auto MI) {
        constexpr int m = decltype(MI)::value, i = S * MT + m;
#pragma unroll
        for (int t = 0; t < T; t++) {
            const i32x16 c = (INIT && S == 0) ? zero16() : acc[t][m];
            acc[t][m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ring[i % DEPTH], in[t][S], c, 0, 0, 0);
        }
        if constexpr (i + DEPTH < MMAX * MT) ring[i % DEPTH] = *(const i32x4 *)(a + (i + DEPTH) * 1024);
    });
    static_for<0, MT>([&](auto MI) {
        __builtin_amdgcn_sched_group_barrier(0x008, T, 0);
        if constexpr (S * MT + decltype(MI)::value + DEPTH < MMAX * MT) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    });
    __builtin_amdgcn_sched_barrier(0);
    pin_memory_order();
    if constexpr (S + 1 < MMAX) {
        if (K > (uint32_t)(S + 1)) hidden_steps<S + 1, MT, T, MMAX, DEPTH, INIT>(a, K, in, acc, ring);
    }
}

template <int MT, int SP, int T, int MMAX>
BNM_DEVICE void hidden_mma(const char *a, uint32_t K, const i32x4 (&in)[T][MMAX], i32x16 (&acc)[T][MT]) {
    constexpr int DEPTH = MMAX * MT < BNM_FRAG_DEPTH ? MMAX * MT : BNM_FRAG_DEPTH;
    static_for<0, SP>([&](auto PI) {
        constexpr int p = decltype(PI)::value;
        const char *ap = a;
        if constexpr (p == 1) ap = a + K * (uint32_t)(MT * 1024);      // the second plane follows the first one's K*MT fragments
        i32x4 ring[DEPTH];
        static_for<0, DEPTH>([&](auto I) { ring[decltype(I)::value] = *(const i32x4 *)(ap + decltype(I)::value * 1024); });
        hidden_steps<0, MT, T, MMAX, DEPTH, p == 0>(ap, K, in, acc, ring);
    });
}

// what a layer's activations are handed to in the plain kernels: nothing (the profiling variant tallies them)
struct NoTally {
    template <class MI, class A>
    BNM_DEVICE void operator()(MI, A &, int) const {}
};
// hidden layer: MFMAs + ReLUNorm (M tiles, K K-steps, both run-time), IN PLACE: the packed activations act[.][0..K) are the B
// operands, act[.][0..M) receive the layer's outputs once the last MFMA has been issued.  (With separate in / out arrays the
// cases' outputs met in PHI nodes whose undefined inputs hipcc filled with copies of `in`: a dozen v_mov per layer and tile.)
template <int MMAX, int SP, bool DBL, int T, class TALLY = NoTally>
BNM_DEVICE void hidden_layer(const char *smem, uint32_t lane16, uint32_t off, uint32_t M, uint32_t K, i32x4 (&act)[T][MMAX], int h,
                             TALLY &&tally = TALLY{}, int layer = 0) {
    static_for<1, MMAX + 1>([&](auto MI) {
        constexpr int mt = decltype(MI)::value;
        if (M == (uint32_t)mt) {
            i32x16 acc[T][mt];
            hidden_mma<mt, SP, T, MMAX>(smem + (off + lane16), K, act, acc);
#pragma unroll
            for (int t = 0; t < T; t++) relunorm_pack<mt, DBL, MMAX>(acc[t], act[t], h);
            tally(MI, act, layer);
        }
    });
}

// first-maximum argmax of a classifier layer's accumulators (+ logits)
template <int MT, int T>
BNM_DEVICE void classify(const i32x16 (&acc)[T][MT], int h, int j, int lane, uint32_t (&cls)[T], int32_t *logits_out, int32_t *stage,
                         uint64_t first_img, uint64_t n, uint32_t n_classes, bool few_classes) {
    // up to 16 classes sit in the first two register groups of tile 0 (rows 0..15): the common case examines 8 registers
    // instead of 16 per tile (wave-uniform branch)
    if (few_classes) {
#pragma unroll
        for (int t = 0; t < T; t++) cls[t] = argmax_rows<MT, 2>(acc[t], h);
    } else {
#pragma unroll
        for (int t = 0; t < T; t++) cls[t] = argmax_rows<MT, 0>(acc[t], h);
    }
    if (logits_out) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const uint64_t tile_first = first_img + 32ull * (uint64_t)t;
            if (tile_first >= n) continue;
            int32_t *tile_dst = logits_out + tile_first * n_classes;
            if (stage != nullptr && tile_first + 32ull <= n) {
                // a whole tile through the staging area: contiguous nontemporal 16 B/lane stores, every line written whole
                store_logits_tile<MT, 0, 0>(acc[t], stage, tile_dst, j, h, lane, n_classes);
            } else if (tile_first + (uint64_t)j < n) {
                store_logits<MT>(acc[t], tile_dst + (uint32_t)j * n_classes, h, n_classes);
            }
        }
    }
}

// classifier layer, general path: MFMAs (M tiles, K K-steps, both run-time) + classify
template <int MMAX, int SP, int T>
BNM_DEVICE void final_layer(const char *smem, uint32_t lane16, uint32_t off, uint32_t M, uint32_t K, const i32x4 (&in)[T][MMAX], int h,
                            int j, int lane, uint32_t (&cls)[T], int32_t *logits_out, int32_t *stage, uint64_t first_img, uint64_t n,
                            uint32_t n_classes, bool few_classes) {
    static_for<1, MMAX + 1>([&](auto MI) {
        constexpr int mt = decltype(MI)::value;
        if (M == (uint32_t)mt) {
            i32x16 acc[T][mt];
            hidden_mma<mt, SP, T, MMAX>(smem + (off + lane16), K, in, acc);
            classify<mt, T>(acc, h, j, lane, cls, logits_out, stage, first_img, n, n_classes, few_classes);
        }
    });
}

// ---- the uniform fast path -----------------------------------------------------------------------------------------
// When every hidden layer has the same tile count MT (the shapes the reference documents: 64-64-64, 96-96-96, 128-128-112,
// 160-160-160) and the classifier fits one tile, everything behind layer 1 is ONE straight-line piece of code per MT: K-steps
// are compile-time counts (no exits), no case boundaries between the layers (no PHI copies of the packed activations: the
// general path spends 7-26 v_mov per layer on them), and hipcc schedules across layers as in the shape-specialised kernels.
template <int MT, int MMAX, int SP, bool DBL, int T>
BNM_DEVICE void uniform_layer(const char *a, i32x4 (&act)[T][MMAX], int h BNM_ST_PARAM, int k0 = 0) {
    i32x16 acc[T][MT];
    mma_l1<MT, MT, 0, MT, SP, true, T, MMAX>(a, act, acc);
    BNM_TICK(k0);
#pragma unroll
    for (int t = 0; t < T; t++) relunorm_pack<MT, DBL, MMAX>(acc[t], act[t], h);
    BNM_TICK(k0 + 1);
}
template <int MT, int MMAX, int SP, bool DBL, int T, class TALLY = NoTally>
BNM_DEVICE void uniform_tail(const char *smem, uint32_t lane16, const BnmGenericDesc &d, i32x4 (&act)[T][MMAX], int h, int j, int lane,
                             uint32_t (&cls)[T], int32_t *logits_out, int32_t *stage, uint64_t first_img, uint64_t n, uint32_t n_classes,
                             bool few_classes BNM_ST_PARAM, TALLY &&tally = TALLY{}) {
    uniform_layer<MT, MMAX, SP, DBL, T>(smem + (d.frag_off[1] + lane16), act, h BNM_ST_ARG, 3);
    tally(std::integral_constant<int, MT>{}, act, 1);
    uint32_t off_last = d.frag_off[2];
    if (d.M[3]) {
        uniform_layer<MT, MMAX, SP, DBL, T>(smem + (d.frag_off[2] + lane16), act, h BNM_ST_ARG, 5);
        tally(std::integral_constant<int, MT>{}, act, 2);
        off_last = d.frag_off[3];
    }
    i32x16 acc[T][1];
    mma_l1<1, MT, 0, MT, SP, true, T, MMAX>(smem + (off_last + lane16), act, acc);
    BNM_TICK(7);
    classify<1, T>(acc, h, j, lane, cls, logits_out, stage, first_img, n, n_classes, few_classes);
    BNM_TICK(8);
}

}  // namespace

// ---- activation profiles (the profiling variant, PROF = true; bnm_fused_generic_prof.hip) ------------------------------------
// The statistics live in LDS behind every wave's tile buffers: per workgroup 32-bit active / sum / hist words per profiled layer
// and pred / confusion, per wave a 1 KiB-per-tile transpose buffer.  After each hidden layer's relunorm_pack the wave writes its
// packed activations (lane (j, h), byte t of K-step s = neuron 32s + 8(t >> 2) + 4h + (t & 3) of image j) to its buffer; lane k
// then walks neuron k down the tile's valid images.  Zeros need no histogram update: hist[0] += images - active.  The workgroup's
// words leave with one 64-bit atomic per non-zero word when the kernel ends; the launcher bounds a launch to 2^22 images, so no
// 32-bit word can overflow.
template <int MMAX>
struct ProfLds {
    uint32_t *act, *sum, *hist, *pred, *conf, *oor;      // workgroup words (profiled layer l: act + l * 256, hist + l * 128)
    char *tb;                                            // this wave's transpose buffer (MMAX KiB)
};
constexpr uint32_t kProfWords(uint32_t n_classes) { return 4u * (256u + 256u + 128u) + n_classes + n_classes * n_classes + 1u; }
template <int MT, int MMAX, int T>
BNM_DEVICE void prof_tally(const ProfLds<MMAX> &p, const BnmFusedProf &pa, const i32x4 (&act)[T][MMAX], uint32_t lane, uint32_t valid,
                           int layer) {
    const uint32_t W = pa.width[layer];
    char *tb = p.tb;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the wave's reads of the previous layer have returned
#pragma unroll
    for (int m = 0; m < MT; m++) *(i32x4 *)(tb + m * 1024 + lane * 16u) = act[0][m];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint32_t *ha = p.act + 256u * (uint32_t)layer, *hs = p.sum + 256u * (uint32_t)layer, *hh = p.hist + 128u * (uint32_t)layer;
    for (uint32_t k = lane; k < (uint32_t)(32 * MT) && k < W; k += 64u) {
        const uint32_t r = k & 31u;
        const uint8_t *col = (const uint8_t *)tb + (k >> 5) * 1024u + ((r >> 2) & 1u) * 512u + (((r >> 3) << 2) | (r & 3u));
        uint32_t a = 0, sm = 0;
        for (uint32_t jj = 0; jj < valid; jj++) {
            const uint32_t v = col[jj * 16u] & 127u;
            a += v != 0u;
            sm += v;
            if (v) atomicAdd(&hh[v], 1u);
        }
        if (a) atomicAdd(&ha[k], a);
        if (sm) atomicAdd(&hs[k], sm);
        if (valid > a) atomicAdd(&hh[0], valid - a);
    }
}

// WPS: waves per SIMD the register budget is compiled for (the workgroup holds up to 4*WPS waves, ONE workgroup per CU).
// The body is shared with the profiling variant below (bnm_fused_generic_body.inc; BNM_GENERIC_PROF selects the tallies).
template <int MMAX, int KT0, int SP, bool DBL, int T, int WPS>
__global__ __launch_bounds__(256 * WPS) void fused_fc_generic_kernel(const int8_t *__restrict__ images, uint64_t n,
                                                                     const i32x4 *__restrict__ frags, BnmGenericDesc d,
                                                                     uint32_t *__restrict__ cls_out,
                                                                     int32_t *__restrict__ logits_out, uint32_t *__restrict__ counter,
                                                                     uint32_t batch_arg) {
#define BNM_GENERIC_PROF 0
#include "bnm_fused_generic_body.inc"
#undef BNM_GENERIC_PROF
}
// the profiling variant (one tile per wave, no logits): the same kernel plus the tallies of ProfLds
template <int MMAX, int KT0, int SP, bool DBL, int WPS>
__global__ __launch_bounds__(256 * WPS) void fused_fc_generic_prof_kernel(const int8_t *__restrict__ images, uint64_t n,
                                                                          const i32x4 *__restrict__ frags, BnmGenericDesc d,
                                                                          uint32_t *__restrict__ cls_out, uint32_t *__restrict__ counter,
                                                                          uint32_t batch_arg, BnmFusedProf pa) {
    constexpr int T = 1;
    int32_t *logits_out = nullptr;
#define BNM_GENERIC_PROF 1
#include "bnm_fused_generic_body.inc"
#undef BNM_GENERIC_PROF
}

// ---- per-class launcher: each (tile class, tiles per wave) pair is its own translation unit (bnm_fused_generic_m{2,4,8}[_t2].hip)
// so that they compile side by side.  Instantiations per row length: doubled hidden weights; plain; plain with FP1.3.0's second
// weight plane.  T = 2 is instantiated for rows of 128 and 256 bytes (32 / 64 B-operand registers per wave).
// hipFuncSetAttribute costs about a microsecond per call: launch-bound callers pay it once per kernel and device
inline hipError_t bnm_generic_allow_big_lds(const void *fn) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({fn, dev})) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done.insert({fn, dev});
    return e;
}

#define BNM_GENERIC_PICK(MMAX, K0, T)                                                                                       \
    if (kt0 == K0) {                                                                                                        \
        if (sp == 1 && dbl) fn = fused_fc_generic_kernel<MMAX, K0, 1, true, T, bnmk_generic_wps(MMAX, K0, 1, T)>;           \
        else if (sp == 1) fn = fused_fc_generic_kernel<MMAX, K0, 1, false, T, bnmk_generic_wps(MMAX, K0, 1, T)>;            \
        else if (sp == 2 && !dbl) fn = fused_fc_generic_kernel<MMAX, K0, 2, false, T, bnmk_generic_wps(MMAX, K0, 2, T)>;    \
    }
#define BNM_GENERIC_LAUNCHER_BEGIN(NAME)                                                                                    \
    hipError_t NAME(uint32_t kt0, uint32_t sp, bool dbl, unsigned blocks, unsigned threads, unsigned lds, hipStream_t s,     \
                    const int8_t *images, uint64_t n, const void *frags, const BnmGenericDesc &d, uint32_t *cls,            \
                    int32_t *logits, uint32_t *counter, uint32_t batch) {                                                    \
        typedef void (*fn_t)(const int8_t *, uint64_t, const i32x4 *, BnmGenericDesc, uint32_t *, int32_t *, uint32_t *, uint32_t); \
        fn_t fn = nullptr;
#define BNM_GENERIC_LAUNCHER_END                                                                                             \
        if (!fn) return hipErrorInvalidValue;                                                                                \
        if (!blocks) return hipSuccess;   /* probe: is there an instantiation? */                                            \
        /* opt in to > 64 KiB of dynamic LDS: a per-device function attribute, set once per (kernel, device) */               \
        if (hipError_t err = bnm_generic_allow_big_lds((const void *)fn); err != hipSuccess) return err;                     \
        fn<<<dim3(blocks), dim3(threads), lds, s>>>(images, n, (const i32x4 *)frags, d, cls, logits, counter, batch);        \
        return hipGetLastError();                                                                                            \
    }
#define BNM_GENERIC_LAUNCHER_T1(NAME, MMAX)                                                                                  \
    BNM_GENERIC_LAUNCHER_BEGIN(NAME)                                                                                         \
    BNM_GENERIC_PICK(MMAX, 2, 1) BNM_GENERIC_PICK(MMAX, 4, 1) BNM_GENERIC_PICK(MMAX, 8, 1) BNM_GENERIC_PICK(MMAX, 16, 1)     \
    BNM_GENERIC_LAUNCHER_END
// one row length per translation unit (the 8-tile class: a single unit with all four took 6.5 minutes to compile)
#define BNM_GENERIC_LAUNCHER_T1_K(NAME, MMAX, K0)                                                                            \
    BNM_GENERIC_LAUNCHER_BEGIN(NAME)                                                                                         \
    BNM_GENERIC_PICK(MMAX, K0, 1)                                                                                            \
    BNM_GENERIC_LAUNCHER_END
#define BNM_GENERIC_LAUNCHER_T2(NAME, MMAX)                                                                                  \
    BNM_GENERIC_LAUNCHER_BEGIN(NAME)                                                                                         \
    BNM_GENERIC_PICK(MMAX, 4, 2) BNM_GENERIC_PICK(MMAX, 8, 2)                                                                \
    BNM_GENERIC_LAUNCHER_END
// (Two tiles per wave exist for the 2-tile class only.  A wave addresses at most 256 VGPRs; two tiles' accumulators of a 4-tile
// layer are 128 of them, of an 8-tile layer all 256 - what does not fit goes to AGPRs, which ReLUNorm can only read through a
// v_accvgpr_read per value, or to scratch: the 4-tile instantiation spilled 22,000 registers.)
