// tile_bits_kernel.inc — body of the K2tb output kernels, included by storm_hip_mfma.hip once per MFMA shape
// (STORM_TI_SHAPE 16 -> tile16_bits_kernel on v_mfma_f32_16x16x128_f8f6f4, 32 -> tile32_bits_kernel on
// v_mfma_f32_32x32x64_f8f6f4 — the unscaled forms: the operand codes are reciprocal per class, ti_infl1 / ti_inflb; STORM_TI_NAME = the kernel's name). Design notes: storm_hip_mfma.hip, "K2tb".
__global__ __launch_bounds__(kTiThreads, 2) void STORM_TI_NAME(
    TileOperands ops, const MfmaItem* __restrict__ items, uint32_t n_items, OutWindow window, uint32_t split_from) {
    const OutWindow w = window.loaded();
    extern __shared__ __attribute__((aligned(1024))) uint8_t ti_lds[];

    // blocks 16 g .. 16 g + 7 are the first halves of items 8 g .. 8 g + 7, the next eight their second halves:
    // item i stays on XCD i % 8 (block b runs on XCD b % 8), which is what the launch order was made for
    const uint32_t item_idx = (blockIdx.x >> 4) * 8u + (blockIdx.x & 7u);
    const uint32_t half = (blockIdx.x >> 3) & 1u;
    if (item_idx >= n_items) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const MfmaItem it = items[item_idx];
    const uint32_t a_row0 = (uint32_t)it.I * kTile, b_row0 = (uint32_t)it.J * kTile + 128u * half;
    const uint32_t C = it.n_stages / 4u;          // chunks of 64 B
    const uint32_t kbyte0 = it.stage0 * 16u;
    const uint32_t pitch = (uint32_t)ops.pitch;
    const uint32_t col_limit = w.col_end();
    if (b_row0 >= col_limit) return;   // the whole half lies beyond the output (ragged last tile column)

    const uint8_t *a_base, *b_base;
    uint32_t a_bytes, b_bytes;
    ops.tile_rows(a_row0, (uint32_t)kTile, a_base, a_bytes);
    ops.tile_rows(b_row0, 128u, b_base, b_bytes);

    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)&ti_lds[0];
    // B pieces of this wave: pieces 2 w and 2 w + 1 of the half's 8 (16 rows x 64 B each); lanes 4 g .. 4 g + 3 hold
    // the quarters of one row, the two rows of an 8-lane group are 8 apart (conflict-free image writes, see K2b)
    const uint32_t prl = (lane >> 3) + 8u * ((lane >> 2) & 1u);
    const uint32_t b_voff = (wave * 32u + prl) * pitch + (lane & 3u) * 16u;   // piece j: + 16 j rows
    const uint32_t bits_rd = lds_base + kTiBits0 + wave * 2048u + lane * 16u;
    uint32_t img_wr[2][2];   // [piece][kk]: row pr, slot (kk * 4 + quarter) ^ (pr / 2) % 8 of a pair image
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t pr = wave * 32u + 16u * (uint32_t)j + prl;
        img_wr[j][0] = lds_base + pr * 128u + (((lane & 3u) ^ ((pr >> 1) & 7u)) * 16u);
        img_wr[j][1] = img_wr[j][0] ^ 64u;
    }
#if STORM_TI_SHAPE == 16
    // fragment (class k, block n): row n * 16 + (lane & 15), slot ((k & 1) * 4 + (lane >> 4)) ^ swizzle of pair k / 2
    const uint32_t swz = ((lane & 15u) >> 1) & 7u;
    uint32_t boff[2];
    boff[0] = lds_base + (lane & 15u) * 128u + (((lane >> 4) ^ swz) * 16u);
    boff[1] = boff[0] ^ 64u;
    // A rows of this lane: 64 w + 16 m + (lane & 15), quarter lane >> 4 of the chunk
    const uint32_t a_voff = (wave * 64u + (lane & 15u)) * pitch + (lane >> 4) * 16u;
#else
    // 32x32x64: lane l holds row l & 31 and the k-half l >> 5 of a 64-element step; a class of a chunk is two steps
    // j = 0, 1 (quarters 2 j + (l >> 5) of the chunk). Fragment (class k, step j, block n): row n * 32 + (l & 31),
    // slot ((k & 1) * 4 + 2 j + (l >> 5)) ^ (row / 2) % 8 — the same image, and conflict free for these reads too
    // (a 16-lane group holds rows {0-3, 12-15, 20-27}: their (row / 2) % 8 are all different per row parity).
    const uint32_t swz = ((lane & 31u) >> 1) & 7u;
    uint32_t boff[4];   // [(k & 1) * 2 + j]
#pragma unroll
    for (uint32_t x = 0; x < 4; ++x)
        boff[x] = lds_base + (lane & 31u) * 128u + ((((x >> 1) * 4u + (x & 1u) * 2u + (lane >> 5)) ^ swz) * 16u);
    // A operand (block m of 32 rows, step j): row 64 w + 32 m + (l & 31), quarter 2 j + (l >> 5): aw[.][m * 2 + j]
    const uint32_t a_voff = (wave * 64u + (lane & 31u)) * pitch + (lane >> 5) * 16u;
#endif

    auto issue_b = [&](uint32_t c, uint32_t slot) __attribute__((always_inline)) {
        const uint32_t koff = kbyte0 + c * 64u;
        const uint32_t bytes = c < C ? b_bytes : 0u;
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(b_base + koff), 0, bytes ? bytes - koff : 0u, 0x00020000);
        uint8_t* dst = ti_lds + kTiBits0 + slot * kTiBitsSlot + wave * 2048u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lptr_t)dst, 16, (int)b_voff, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lptr_t)(dst + 1024u), 16, (int)(b_voff + 16u * pitch), 0, 0, 0);
    };
    typedef unsigned v4u_ti __attribute__((ext_vector_type(4)));
    v4i aw[2][4];   // [chunk parity][A block]: the bits of the wave's A rows
    auto load_a = [&](uint32_t c, v4i (&dst)[4]) __attribute__((always_inline)) {
        const uint32_t koff = kbyte0 + c * 64u;
        const uint32_t bytes = c < C ? a_bytes : 0u;
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(a_base + koff), 0, bytes ? bytes - koff : 0u, 0x00020000);
#if STORM_TI_SHAPE == 16
#pragma unroll
        for (int m = 0; m < 4; ++m)
            dst[m] = (v4i)(v4u_ti)__builtin_amdgcn_raw_buffer_load_b128(r, (int)(a_voff + (uint32_t)m * 16u * pitch), 0, 0);
#else
#pragma unroll
        for (int x = 0; x < 4; ++x)   // x = m * 2 + j
            dst[x] = (v4i)(v4u_ti)__builtin_amdgcn_raw_buffer_load_b128(
                r, (int)(a_voff + (uint32_t)(x >> 1) * 32u * pitch + (uint32_t)(x & 1) * 32u), 0, 0);
#endif
    };

    const bool interior =
        item_idx < split_from && w.covers(a_row0, (uint32_t)kTile, b_row0, 128u) &&
        (w.ld & 3u) == 0 && ((uintptr_t)w.out & 15u) == 0 && ((w.j_base & 3u) == 0);
    (void)interior;
    auto run = [&](auto nlo_c, auto nhi_c) __attribute__((always_inline)) {
    // this wave multiplies the 32-row B blocks [NLO, NHI) of its half only (diagonal tiles: the blocks wholly below
    // the diagonal drop out; ragged last tile column: the blocks beyond the output). Fragment reads and everything the
    // workgroup shares stay as they are: the lgkmcnt values count them.
    constexpr int NLO = decltype(nlo_c)::value, NHI = decltype(nhi_c)::value;
#if STORM_TI_SHAPE == 16
    v4f acc[4][8];    // [A block of 16 rows][B block of 16 rows]
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 8; ++n) acc[m][n] = v4f{};
#else
    v16f acc[2][4];   // [A block of 32 rows][B block of 32 rows]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = v16f{};
#endif
    v4i ainf[4];      // [A block]: the inflated A operand of the class being multiplied
    v4i fr0 = {}, fr1 = {}, fr2 = {}, wb = {}, e = {};

#define STORM_TI_LGKM(n)                                    \
    asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0)
#define STORM_TI_VM_A()                              \
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0)
#define STORM_TI_BITS(j, SLOT) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(wb) : "v"(bits_rd), "n"((1 - (SLOT)) * kTiBitsSlot + (j) * 1024))
#if STORM_TI_SHAPE == 16
#define STORM_TI_FETCH(reg, SLOT, k, n) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(reg) : "v"(boff[(k) & 1]), "n"((SLOT) * kTiImgSlot + ((k) >> 1) * kTiImgBytes + (n) * 2048))
#else   // step n of class k: k-step j = n / 4, B block n % 4 (32 rows x 128 B = 4096 bytes apart)
#define STORM_TI_FETCH(reg, SLOT, k, n) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(reg) : "v"(boff[((k) & 1) * 2 + (n) / 4]), "n"((SLOT) * kTiImgSlot + ((k) >> 1) * kTiImgBytes + ((n) % 4) * 4096))
#endif
#define STORM_TI_WRITE(j, cls, SLOT) \
    asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(img_wr[j][(cls) & 1]), "v"(e), "n"((1 - (SLOT)) * kTiImgSlot + ((cls) >> 1) * kTiImgBytes) : "memory")
#ifdef STORM_TI_X_NOBINF   /* timing experiments (tools only, wrong results): tile kernels' loop minus one ingredient */
#define STORM_TI_BINF(j, cls) e = wb
#else
#define STORM_TI_BINF(j, cls) \
    e = v4i{ti_inflb<cls>(wb.x), ti_inflb<cls>(wb.y), ti_inflb<cls>(wb.z), ti_inflb<cls>(wb.w)}
#endif
#ifdef STORM_TI_X_NOAINF
#define STORM_TI_AINF_ONE(cls, v) (v)
#else
#define STORM_TI_AINF_ONE(cls, v) v4i{ti_infl1<cls>((v).x), ti_infl1<cls>((v).y), ti_infl1<cls>((v).z), ti_infl1<cls>((v).w)}
#endif
#define STORM_TI_AINF_ALL(cls, from_next, SLOT)                                                       \
    _Pragma("unroll") for (int m = 0; m < 4; ++m) {                                                    \
        const v4i src_ = aw[(from_next) ? 1 - (SLOT) : (SLOT)][m];                                      \
        asm volatile("" ::"v"(src_));   /* the loads stay, whatever this instantiation multiplies */     \
        ainf[m] = STORM_TI_AINF_ONE(cls, src_); \
    }
#if STORM_TI_SHAPE == 16
#define STORM_TI_MUL(k, n, frag)                                                                                  \
    /* (a fragment this wave does not multiply is still fetched — the lgkmcnt values count it — and must stay      \
       alive up to here: hipcc hands the registers of a dead asm output to the next value, and the LDS data lands    \
       on top of it later — it overwrote the inflated B piece in front of its ds_write) */                           \
    if constexpr (!((n) / 2 >= NLO && (n) / 2 < NHI)) asm volatile("" ::"v"(frag));                               \
    else                                                                                                          \
    _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                                 \
        acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(                                             \
            v8i{ainf[m].x, ainf[m].y, ainf[m].z, ainf[m].w, 0, 0, 0, 0},                                         \
            v8i{frag.x, frag.y, frag.z, frag.w, 0, 0, 0, 0}, acc[m][n], 4, 4, 0, 0, 0, 0)
#else
#define STORM_TI_MUL(k, n, frag)                                                                                  \
    if constexpr (!((n) % 4 >= NLO && (n) % 4 < NHI)) asm volatile("" ::"v"(frag));                               \
    else                                                                                                          \
    _Pragma("unroll") for (int m = 0; m < 2; ++m)                                                                 \
        acc[m][(n) % 4] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(                                        \
            v8i{ainf[m * 2 + (n) / 4].x, ainf[m * 2 + (n) / 4].y, ainf[m * 2 + (n) / 4].z, ainf[m * 2 + (n) / 4].w, 0, 0, 0, 0}, \
            v8i{frag.x, frag.y, frag.z, frag.w, 0, 0, 0, 0}, acc[m][(n) % 4], 4, 4, 0, 0, 0, 0)
#endif
    // one chunk: every wave past the images of the chunk before, the next A bits and the B pieces after next on
    // their way, the pieces of the next chunk landed (6 younger operations may fly: 4 A loads, 2 pieces)
#ifdef STORM_TI_X_NOBARRIER
#define STORM_TI_BARRIER() (void)0
#else
#define STORM_TI_BARRIER() __builtin_amdgcn_s_barrier()
#endif
#define STORM_TI_ITER(SLOT, cc)                               \
    STORM_TI_BARRIER();                                       \
    load_a((cc) + 1u, aw[1 - (SLOT)]);                        \
    issue_b((cc) + 2u, (SLOT));                               \
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);                        \
    STORM_TI_CHUNK(SLOT)

    // ---- prologue: chunk 0's images and class-0 A operand, built without overlap
    issue_b(0u, 0u);
    load_a(0u, aw[0]);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    {
        // (chunk 0 lives in bits slot 0: read it with the macro's "next chunk" form for SLOT = 1)
        STORM_TI_BITS(0, 1);
        STORM_TI_LGKM(0);
        STORM_TI_BINF(0, 0); STORM_TI_WRITE(0, 0, 1);
        STORM_TI_BINF(0, 1); STORM_TI_WRITE(0, 1, 1);
        STORM_TI_BINF(0, 2); STORM_TI_WRITE(0, 2, 1);
        STORM_TI_BINF(0, 3); STORM_TI_WRITE(0, 3, 1);
        STORM_TI_BITS(1, 1);
        STORM_TI_LGKM(0);
        STORM_TI_BINF(1, 0); STORM_TI_WRITE(1, 0, 1);
        STORM_TI_BINF(1, 1); STORM_TI_WRITE(1, 1, 1);
        STORM_TI_BINF(1, 2); STORM_TI_WRITE(1, 2, 1);
        STORM_TI_BINF(1, 3); STORM_TI_WRITE(1, 3, 1);
        STORM_TI_AINF_ALL(0, 0, 0);
        STORM_TI_LGKM(0);
    }
    issue_b(1u, 1u);   // the pieces of chunk 1 (older than everything iteration 0 issues)
    // Chunks in pairs, no exit in the middle (with one, hipcc shuffled the 128 accumulators between the two bodies
    // and spilled them). An odd count runs one chunk more: its A bits read as zero (empty descriptor), so it adds 0.
#pragma unroll 1
    for (uint32_t c = 0; c < C; c += 2u) {
        STORM_TI_ITER(0, c);
        STORM_TI_ITER(1, c + 1u);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the empty pieces and loads of the tail, too
#undef STORM_TI_ITER
#undef STORM_TI_BARRIER
#undef STORM_TI_AINF_ONE
#undef STORM_TI_MUL
#undef STORM_TI_AINF_ALL
#undef STORM_TI_BINF
#undef STORM_TI_WRITE
#undef STORM_TI_FETCH
#undef STORM_TI_BITS
#undef STORM_TI_VM_A
#undef STORM_TI_LGKM

#if STORM_TI_SHAPE == 16
    // ---- epilogue: C/D map of a 16 x 16 block: col = lane & 15, row = 4 * (lane >> 4) + reg
    const bool whole = item_idx < split_from;   // the item spans all of k: plain stores; else it adds into a cleared window
#pragma unroll
    for (int n = 2 * NLO; n < 2 * NHI; ++n) {
        const uint32_t j = b_row0 + 16u * (uint32_t)n + (lane & 15u);
        const bool j_ok = w.wants_col(j);
        const uint32_t nj = w.nj(j);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t i = a_row0 + wave * 64u + 16u * (uint32_t)m + 4u * (lane >> 4) + (uint32_t)r;
                if (j_ok && w.writes_row(i, j)) {
                    const uint32_t val = w.part_value((uint32_t)acc[m][n][r], i, nj, whole || it.stage0 == 0);
                    if (whole) *w.at(i, j) = val;
                    else atomicAdd(w.at(i, j), val);
                }
            }
    }
#else
#ifdef STORM_TI_NO_EPILOGUE   // timing experiment (tools only): the loop without its stores
    {
        float sum_ = 0.0f;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum_ += acc[m][n][r];
        if (sum_ == -1.0f) w.out[0] = 1u;
        return;
    }
#endif
    // ---- epilogue: C/D map of a 32 x 32 block: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const bool whole = item_idx < split_from;   // the item spans all of k: plain stores; else it adds into a cleared window
    if constexpr (NLO == 0 && NHI == 4) {
        if (interior) {
            // A half that lies wholly inside the output: the accumulators hold 16 rows of one column per lane, so storing
            // them directly is a 4-byte store per element in 128-byte runs. Each wave turns its 64 x 128 block through a
            // private 16 KiB of the (now idle) images, 32 rows at a time, and stores 16 bytes per lane in 512-byte runs
            // (tilebits8_kernel's epilogue: 5 % of a call there).
            __builtin_amdgcn_s_barrier();   // every wave has left the images
            uint32_t* w32 = reinterpret_cast<uint32_t*>(ti_lds + wave * 16384u);
            const uint4* r128 = reinterpret_cast<const uint4*>(ti_lds + wave * 16384u);
            const uint32_t i0 = a_row0 + wave * 64u;
            uint32_t* out_tile = w.at(i0, b_row0);
            const OutWindow::counts_ptr_t row_counts = w.counts();
            const uint64_t ld = w.ld;
            uint32_t njv[4] = {0u, 0u, 0u, 0u};
            if (row_counts) {
#pragma unroll
                for (int n = 0; n < 4; ++n) njv[n] = row_counts[b_row0 + (uint32_t)n * 32u + (lane & 31u)];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t il = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
                    const uint32_t ni = row_counts ? row_counts[i0 + (uint32_t)m * 32u + il] : 0u;
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const uint32_t cnt = (uint32_t)acc[m][n][r];
                        w32[il * 128u + (uint32_t)n * 32u + (lane & 31u)] = row_counts ? ni + njv[n] - w.and_weight * cnt : cnt;
                    }
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const uint32_t row = (uint32_t)q * 2u + (lane >> 5);
                    const uint4 v = r128[row * 32u + (lane & 31u)];
                    *reinterpret_cast<uint4*>(&out_tile[(uint64_t)((uint32_t)m * 32u + row) * ld + 4u * (lane & 31u)]) = v;
                }
            }
            return;
        }
    }
#pragma unroll
    for (int n = NLO; n < NHI; ++n) {
        const uint32_t j = b_row0 + 32u * (uint32_t)n + (lane & 31u);
        const bool j_ok = w.wants_col(j);
        const uint32_t nj = w.nj(j);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t i = a_row0 + wave * 64u + 32u * (uint32_t)m + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
                if (j_ok && w.writes_row(i, j)) {
                    const uint32_t val = w.part_value((uint32_t)acc[m][n][r], i, nj, whole || it.stage0 == 0);
                    if (whole) *w.at(i, j) = val;
                    else atomicAdd(w.at(i, j), val);
                }
            }
    }
#endif
    };   // run

    // blocks of 32 B rows this wave needs: [n_lo, n_hi) (any superset is correct: the epilogue masks)
    const uint32_t n_hi = min(4u, (col_limit - b_row0 + 31u) / 32u);
    const uint32_t below = (!w.rect() && a_row0 == (uint32_t)it.J * kTile && wave * 64u > 128u * half) ? (wave * 64u - 128u * half) / 32u : 0u;
    const uint32_t n_lo = min(below, 4u);
    using std::integral_constant;
    if (n_lo >= n_hi) run(integral_constant<int, 4>{}, integral_constant<int, 4>{});
    else if (n_lo >= 2u) run(integral_constant<int, 2>{}, integral_constant<int, 4>{});
    else if (n_hi == 1u) run(integral_constant<int, 0>{}, integral_constant<int, 1>{});
    else if (n_hi == 2u) run(integral_constant<int, 0>{}, integral_constant<int, 2>{});
    else if (n_hi == 3u) run(integral_constant<int, 0>{}, integral_constant<int, 3>{});
    else run(integral_constant<int, 0>{}, integral_constant<int, 4>{});
}
