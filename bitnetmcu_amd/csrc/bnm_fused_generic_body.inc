// Body of fused_fc_generic_kernel and fused_fc_generic_prof_kernel (bnm_fused_generic_kernel.hpp), included inside each: the kernel
// defines BNM_GENERIC_PROF (1: the profiling tallies, with their arguments in pa) in front of it; with 0 the text is the plain kernel's.

    using G = RowGeom<32 * KT0>;
    const uint32_t batch = batch_arg & 0xFFFFu;
    constexpr int ROW = 32 * KT0;
    // layer-1 K-steps whose B operands are held in VGPRs at a time (x T tiles x 4 registers): all of a 256-byte row with one
    // tile per wave, half of it with two (the refill then starts after the first half's MFMAs)
    // (4-tile class with two tiles: two K-steps at a time - its two tiles' 128 accumulator registers leave room for no more)
    constexpr int KC = KT0 * T <= 8 ? KT0 : (MMAX >= 4 && T == 2) ? 2 : 8 / T;
    constexpr int UNIT = T * G::TILE;              // bytes of the T consecutive tiles a wave handles per iteration
    static_assert(T == 1 || T == 2, "one or two tiles per wave");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nwaves = blockDim.x >> 6;

    // ---- weights: fragment image global -> LDS, once per workgroup -------------------------------------
    for (uint32_t o = threadIdx.x * 16u; o < d.w_bytes; o += blockDim.x * 16u) *(i32x4 *)(smem + o) = frags[o >> 4];
#if BNM_GENERIC_PROF
    ProfLds<MMAX> pl{};
    {
        // behind the weights and every wave's tile buffers: the transpose buffers (MMAX KiB per wave), then the workgroup's words
        char *pbase = smem + d.w_bytes + (blockDim.x >> 6) * (uint32_t)(T * 32 * 32 * KT0);
        pl.tb = pbase + (threadIdx.x >> 6) * (uint32_t)(MMAX * 1024);
        uint32_t *w = (uint32_t *)(pbase + (blockDim.x >> 6) * (uint32_t)(MMAX * 1024));
        pl.act = w;
        pl.sum = w + 4u * 256u;
        pl.hist = w + 8u * 256u;
        pl.pred = w + 8u * 256u + 4u * 128u;
        pl.conf = pl.pred + pa.n_classes;
        pl.oor = pl.conf + pa.n_classes * pa.n_classes;
        for (uint32_t i = threadIdx.x; i < kProfWords(pa.n_classes); i += blockDim.x) w[i] = 0u;
    }
#endif
    __syncthreads();

    const uint32_t tile_off = d.w_bytes + wave * (uint32_t)UNIT;                       // this wave's T tile buffers
    const uint32_t tile_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) char *)smem + tile_off;
    // logits staging area of the wave (2 KiB behind all tile buffers) when the launcher reserved one
    int32_t *const stage = d.stage ? (int32_t *)(smem + d.w_bytes + nwaves * (uint32_t)UNIT + wave * 2048u) : nullptr;
    // Lane constants that stay in registers across the persistent loop: the lane id, the B-operand base, the fragment base and
    // the NV distinct DMA source offsets (DMA piece t, lane l: LDS byte 1024t + 16l = row t*RPP + rl, slot c'; source slot
    // c = c' ^ mask(row)).  The loop body works on opaque per-iteration copies of them: left to itself hipcc hoists dozens of
    // DERIVED operand / fragment addresses out of the loop and spills them.
    // B operand of K-step s: image j, global slot 2s+h -> LDS slot (2s+h) ^ mask(j): XOR 32*s into the byte offset rd_off
    const uint32_t lane16 = 16u * (uint32_t)lane;
    const uint32_t rd_off = tile_off + (uint32_t)(lane & 31) * (uint32_t)ROW + 16u * ((uint32_t)(lane >> 5) ^ G::mask((uint32_t)(lane & 31)));
    // rows of up to 256 bytes: the K-steps' B-operand addresses themselves stay in registers (no XOR per K-step and tile)
    // (not in the 4-tile class with two tiles: eight loop-carried registers it does not have)
    constexpr bool PRE_RD = KT0 <= 8 && !(MMAX >= 4 && T == 2);
    uint32_t rda[PRE_RD ? KT0 : 1];
    if constexpr (PRE_RD) {
#pragma unroll
        for (int s = 0; s < KT0; s++) rda[s] = rd_off ^ (32u * (uint32_t)s);
    }
    uint32_t voff[G::NV];
    {
        const uint32_t rl0 = (16u * (uint32_t)lane) / (uint32_t)ROW, cs0 = (uint32_t)lane & (uint32_t)(G::SLOTS - 1);
#pragma unroll
        for (int k = 0; k < G::NV; k++) voff[k] = (rl0 * (uint32_t)ROW + 16u * (cs0 ^ G::mask(rl0))) ^ G::xmask(k);
    }

    const uint32_t n_tiles = (uint32_t)((n + 31ull) >> 5);       // the launcher refuses n >= 2^36
    const uint32_t n_units = (n_tiles + (uint32_t)(T - 1)) / (uint32_t)T;
    auto dma_unit = [&](uint32_t u) {
        const int8_t *base = images + (uint64_t)u * (uint64_t)UNIT;
        const uint64_t first = (uint64_t)u * (uint64_t)(32 * T);
        if (first + (uint64_t)(32 * T) <= n) {
            constexpr int NP = T * G::PIECES;
            static_for<0, (NP + 3) / 4>([&](auto GI) {
                constexpr int t0 = 4 * decltype(GI)::value;
                if constexpr (NP - t0 >= 4)
                    dma_group4(tile_lds + 1024u * t0, base + 1024 * t0, voff[t0 % G::NV], voff[(t0 + 1) % G::NV], voff[(t0 + 2) % G::NV],
                               voff[(t0 + 3) % G::NV]);
                else if constexpr (NP - t0 == 2)
                    dma_group2(tile_lds + 1024u * t0, base + 1024 * t0, voff[t0 % G::NV], voff[(t0 + 1) % G::NV]);
                else
                    dma_group1(tile_lds + 1024u * t0, base + 1024 * t0, voff[t0 % G::NV]);
            });
        } else {
            // ragged end: rows past the last image re-read it (never out of bounds); a tile wholly past the end reads the last
            // image 32 times and stores nothing
            const uint32_t nv = (uint32_t)(n - first);                                 // valid rows from `first` on (1 .. 32 T - 1)
            uint32_t l = (uint32_t)lane;
            asm volatile("" : "+v"(l));
            const uint32_t rl = (16u * l) / (uint32_t)ROW, cs = l & (uint32_t)(G::SLOTS - 1);
            static_for<0, T * G::PIECES>([&](auto TI) {
                constexpr int tt = decltype(TI)::value;
                const uint32_t r = (uint32_t)(tt * G::ROWS_PER_PIECE) + rl;            // row within the unit
                const uint32_t src = r < nv ? r : nv - 1u;
                dma_group1(tile_lds + 1024u * tt, base, src * (uint32_t)ROW + 16u * (cs ^ G::mask(r & 31u)));
            });
        }
    };

    // ---- units in batches of `batch` consecutive ones: a wave's first batch is static, every later one comes from the
    // device-wide counter (work_take_*; the wave that runs out of batch asks while it still has one unit to go).
    // The counter is split into `words` words (upper half of the argument: 8 when the wave count is a multiple of 8, else 1):
    // wave w takes from word w % words, which hands out the batches g = t * words + w % words - every word is shared by waves
    // of all CUs, so the balance stays device-wide while a word sees an eighth of the takes (DESIGN.md, work distribution).
    const uint32_t total_waves = gridDim.x * nwaves, wave_id = blockIdx.x * nwaves + wave;
    const uint32_t words = batch_arg >> 16, wshift = (uint32_t)__builtin_ctz(words | 0x100u);
    const uint32_t my_word = wave_id & (words - 1u), first_dyn = total_waves >> wshift;
    uint32_t unit = wave_id * batch, left = batch - 1u;      // `left`: units of the batch after this one
    uint32_t taken = 0;
    if (unit < n_units) dma_unit(unit);

    const uint32_t M1 = d.M[0], M2 = d.M[1], M3 = d.M[2], M4 = d.M[3];
    const bool few_classes = d.n_classes <= 16u;
    // the uniform fast path (see uniform_tail): equal tile counts in all hidden layers, near the class's maximum, one classifier tile
    const bool uniform = M2 == M1 && (M4 ? (M3 == M1 && M4 == 1u) : M3 == 1u) && M1 + 1u >= (uint32_t)MMAX;
    // Class ids leave one iteration LATE, right behind the refill: the loop's top waits for vmcnt(0) (the tile), and a store
    // issued at the end of the body would make that wait sit on its write acknowledgement every iteration.  Every class word is
    // written exactly once (bnm_infer_host's latency path polls them), so the first iteration stores nothing.
    uint32_t cls_prev = 0, unit_prev = 0;
    bool pend = false;
    auto flush_cls = [&]() {
        if (!pend) return;
        // T = 2: lanes 0..31 hold tile 0's ids, lanes 32..63 tile 1's - one 256-byte store per unit; T = 1: the lower half stores
        uint32_t l = (uint32_t)lane;
        asm volatile("" : "+v"(l));
        const uint64_t img = (uint64_t)unit_prev * (uint64_t)(32 * T) + (uint64_t)(T == 2 ? l : (l & 31u));
        if (img < n && (T == 2 || l < 32u)) __builtin_nontemporal_store(cls_prev, cls_out + img);
    };
#ifdef BNM_DIAG_TIMING
    PhaseStamps st{};
    int32_t *const records = logits_out;
    logits_out = nullptr;
    uint32_t iters = 0;
    st.start();
#endif
    while (unit < n_units) {
        if (left == 0u) work_take_issue(taken, counter + 16u * my_word, 1u);
        BNM_TICK(9);                 // loop overhead behind the previous tile's last stamp
        bnm_wait_vmcnt<0>();
        BNM_TICK(0);                 // the wait for the tile
        uint32_t next_unit = unit + 1u, next_left = left - 1u;
        // per-iteration opaque copies of the three lane values the arithmetic starts from (one v_mov each): what is derived from
        // them inside the iteration cannot be hoisted out of the persistent loop
        uint32_t lv = (uint32_t)lane, rd = rd_off, l16 = lane16;
        asm volatile("" : "+v"(lv), "+v"(rd), "+v"(l16));
        const int j = (int)(lv & 31u), h = (int)(lv >> 5);
        i32x4 act[T][MMAX];       // packed layer outputs = the next layer's B operands (updated in place, layer by layer)
        const uint64_t first_img = (uint64_t)unit * (uint64_t)(32 * T);
        // per-iteration copy: keeps the (row < n_classes) predicates of every accumulator register of every case from being
        // hoisted out of the persistent loop as hundreds of live 64-bit masks
        uint32_t nc = d.n_classes;
        asm volatile("" : "+v"(nc));
        uint32_t cls[T];
#pragma unroll
        for (int t = 0; t < T; t++) cls[t] = 0;
        bool done = false;
#if BNM_GENERIC_PROF
        // the profiling variant's tally of a hidden layer
        const uint32_t valid = n - first_img < 32ull ? (uint32_t)(n - first_img) : 32u;
        auto prof_layer = [&](auto MI, i32x4 (&a)[T][MMAX], int layer) {
            prof_tally<decltype(MI)::value, MMAX, T>(pl, pa, a, lv, valid, layer);
        };
#endif
        // ---- layer 1: B operands from the tile buffers, KC K-steps at a time; the buffers are refilled with the wave's
        // next unit as soon as the last operand has been read (the load is then in flight for the rest of the iteration)
        static_for<1, MMAX + 1>([&](auto MI) {
            constexpr int mt = decltype(MI)::value;
            if (M1 == (uint32_t)mt) {
                i32x16 acc[T][mt];
                static_for<0, KT0 / KC>([&](auto CI) {
                    constexpr int ch = decltype(CI)::value;
                    i32x4 b0[T][KC];
#pragma unroll
                    for (int t = 0; t < T; t++)
#pragma unroll
                        for (int s = 0; s < KC; s++)
                            if constexpr (PRE_RD) b0[t][s] = *(const i32x4 *)(smem + (rda[ch * KC + s] + (uint32_t)(t * G::TILE)));
                            else b0[t][s] = *(const i32x4 *)(smem + ((rd + (uint32_t)(t * G::TILE)) ^ (32u * (uint32_t)(ch * KC + s))));
                    if constexpr (ch == KT0 / KC - 1) {
                        retire_lds_reads();
                        if (left == 0u) {
                            work_take_wait(taken);
                            next_unit = (((first_dyn + taken) << wshift) + my_word) * batch;
                            next_left = batch - 1u;
                        }
                        if (next_unit < n_units) dma_unit(next_unit);
                        flush_cls();
                    }
                    mma_l1<mt, KC, ch * KC, KT0, SP, ch == 0, T>(smem + (d.frag_off[0] + l16), b0, acc);
                });
                BNM_TICK(1);
#pragma unroll
                for (int t = 0; t < T; t++) relunorm_pack<mt, DBL, MMAX>(acc[t], act[t], h);
                BNM_TICK(2);
#if BNM_GENERIC_PROF
                prof_layer(MI, act, 0);
#endif
                if constexpr (mt >= MMAX - 1) {
                    if (uniform) {      // all hidden layers have mt tiles, one classifier tile: straight-line code from here on
                        uniform_tail<mt, MMAX, SP, DBL, T>(smem, l16, d, act, h, j, lane, cls, logits_out, stage, first_img, n, nc, few_classes BNM_ST_ARG
#if BNM_GENERIC_PROF
                                                           , prof_layer
#endif
                                                           );
                        done = true;
                    }
                }
            }
        });
        if (!done) {
#if BNM_GENERIC_PROF
            hidden_layer<MMAX, SP, DBL, T>(smem, l16, d.frag_off[1], M2, M1, act, h, prof_layer, 1);
#else
            hidden_layer<MMAX, SP, DBL, T>(smem, l16, d.frag_off[1], M2, M1, act, h);
#endif
            uint32_t m_last = M3, k_last = M2, off_last = d.frag_off[2];
            if (M4) {
#if BNM_GENERIC_PROF
                hidden_layer<MMAX, SP, DBL, T>(smem, l16, d.frag_off[2], M3, M2, act, h, prof_layer, 2);
#else
                hidden_layer<MMAX, SP, DBL, T>(smem, l16, d.frag_off[2], M3, M2, act, h);
#endif
                m_last = M4; k_last = M3; off_last = d.frag_off[3];
            }
            final_layer<MMAX, SP, T>(smem, l16, off_last, m_last, k_last, act, h, j, lane, cls, logits_out, stage, first_img, n, nc, few_classes);
        }
        // both halves of the wave hold every tile's result: T = 2 keeps tile 0's ids in lanes 0..31 and tile 1's in lanes 32..63
        // (one 256-byte store per unit), T = 1 stores from the lower half
        if constexpr (T == 2) cls_prev = h ? cls[1] : cls[0];   // (h: this iteration's copy)
        else cls_prev = cls[0];
#if BNM_GENERIC_PROF
        {   // T == 1: lanes 0..31 hold images 0..31 of the tile
            if (lv < valid) {
                const uint32_t k = cls[0], ncl = pa.n_classes;
                atomicAdd(&pl.pred[k], 1u);
                if (pa.labels) {
                    const int32_t lab = pa.labels[first_img + lv];
                    if (lab >= 0 && (uint32_t)lab < ncl) atomicAdd(&pl.conf[(uint32_t)lab * ncl + k], 1u);
                    else atomicAdd(pl.oor, 1u);
                }
            }
        }
#endif
        unit_prev = unit;
        pend = true;
        unit = next_unit;
        left = next_left;
#ifdef BNM_DIAG_TIMING
        iters++;
#endif
    }
#ifdef BNM_DIAG_TIMING
    if (records != nullptr && lane == 0) {
        int32_t *r = records + 16u * wave_id;
        for (int k = 0; k < 12; k++) r[k] = (int32_t)st.sum[k];
        r[12] = (int32_t)iters;
        r[13] = (int32_t)(__builtin_amdgcn_s_getreg((31 << 11) | 4));
        r[14] = (int32_t)wave;
    }
#endif
    flush_cls();
    bnm_wait_vmcnt<0>();   // no LDS-DMA may outlive the workgroup's LDS allocation
#if BNM_GENERIC_PROF
    {
        // the workgroup's words -> the counters: one 64-bit atomic per non-zero word
        __syncthreads();
        unsigned long long *ctr = pa.ctr;
        const uint32_t ncl = pa.n_classes;
        for (uint32_t l = 0; l < pa.n_layers; l++) {
            const uint32_t W = pa.width[l];
            for (uint32_t i = threadIdx.x; i < W; i += blockDim.x) {
                if (pl.act[256u * l + i]) atomicAdd(ctr + pa.word[l] + i, (unsigned long long)pl.act[256u * l + i]);
                if (pl.sum[256u * l + i]) atomicAdd(ctr + pa.word[l] + W + i, (unsigned long long)pl.sum[256u * l + i]);
            }
            for (uint32_t i = threadIdx.x; i < 128u; i += blockDim.x)
                if (pl.hist[128u * l + i]) atomicAdd(ctr + pa.word[l] + 2u * W + i, (unsigned long long)pl.hist[128u * l + i]);
        }
        for (uint32_t i = threadIdx.x; i < ncl; i += blockDim.x)
            if (pl.pred[i]) atomicAdd(ctr + pa.pred + i, (unsigned long long)pl.pred[i]);
        for (uint32_t i = threadIdx.x; i < ncl * ncl; i += blockDim.x)
            if (pl.conf[i]) atomicAdd(ctr + pa.pred + ncl + i, (unsigned long long)pl.conf[i]);
        if (threadIdx.x == 0) {
            if (*pl.oor) atomicAdd(ctr + pa.tail + 1u, (unsigned long long)*pl.oor);
            if (blockIdx.x == 0) {
                if (pa.labels) atomicAdd(ctr + pa.tail, (unsigned long long)n);
                atomicAdd(ctr + pa.tail + 2u, (unsigned long long)n);
            }
        }
    }
#endif
    work_block_leave_s(counter, total_waves);   // the last wave to leave puts the counter block back to all-zero
