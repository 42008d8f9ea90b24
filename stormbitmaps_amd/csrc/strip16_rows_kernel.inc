// strip16_rows_kernel: K2b with 128 A rows per wave on 128-bit k-slices (option k2_strip_rows = 128). Included once by
// storm_hip_mfma.hip; the comment block in front of the include has the dataflow and the counts per stage.
__global__ __launch_bounds__(256, 4) void strip16_rows_kernel(
    const uint8_t* __restrict__ X, uint64_t row_bytes, const StripItem* __restrict__ items,
    unsigned long long* __restrict__ slots, unsigned long long* __restrict__ out, uint32_t fold_slots, uint32_t n_rows) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds_raw[kSr16ImgBytes + kSr16BitRing * kSr16BitStage];

    constexpr uint32_t kW = kStripRowsWaves;        // waves per workgroup; wave w keeps blocks w and 7 - w of the A tile
    static_assert(kSr16PerTile == kStripRowsBlocks && kSr16ImgBytes >= kStripRowsBlocks * kSr16StageBytes, "eight resident images");
    STORM_CLOCK_BEGIN();
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const StripItem it = items[blockIdx.x];
    const uint64_t kbyte = (uint64_t)it.ks * (uint64_t)kSr16SliceBytes;
    // Pipelined stage s (B block j1 - 1 - s) lives in ring slot s % 3 of both rings: the three instances of the loop body
    // address their images and pieces with immediate offsets (as strip16_bits_kernel). The diagonal phase in front of it
    // is no stage of the rings. An item that has only its diagonal (T == 0) still issues its three pieces — of the tile's
    // own first block, a valid address — and drains them at the end.
    // Rows from n_rows on are zero (storm_hip_plan.h: kStripRowsNoTrim switches this off). A run whose top block j1 - 1 has
    // rows in only 1 or 2 of its fragments is walked from j1 - 2 down, Tl = T - 1 whole stages, and the top block is stage
    // T - 1: its image is complete when the loop ends, and those fragments alone are multiplied behind the loop — no barrier,
    // no ring upkeep. Stage s is block blk_first - s for s < s_turn and blk_rest from there on (the stale pieces too).
    const uint32_t T = it.j1 - it.j0;
    const uint32_t top_frags = strip_rows_top_trimmed(it.j0, it.j1, n_rows) ? strip_rows_real_frags(it.j1 - 1u, n_rows) : 0u;   // 0: nothing trimmed
    const uint32_t Tl = top_frags ? T - 1u : T;
    const uint32_t s_turn = top_frags ? Tl : T ? T - 1u : 0u;
    const uint32_t blk_first = T ? it.j1 - (top_frags ? 2u : 1u) : it.a_row0 / (uint32_t)kStripBRows;
    const uint32_t blk_rest = top_frags ? it.j1 - 1u : blk_first - s_turn;
    const uint32_t blk_lo = strip_rows_block(wave, 0u), blk_hi = strip_rows_block(wave, 1u);

    const uint32_t lds_base =
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)&lds_raw[0];
    // the wave's piece of a B stage: 16 rows x 16 bytes, 4 bytes per lane — row lane >> 2, dword lane & 3
    const uint32_t pr = wave * 16u + (lane >> 2);
    const uint32_t goff0 = pr * (uint32_t)row_bytes + (lane & 3u) * 4u;
    const uint32_t bits_rd = lds_base + kSr16ImgBytes + wave * 256u + lane * 4u;
    // where the four classes of that dword go in an FP4 image: row pr (64 bytes), 16-byte slot dword ^ h[(row >> 2) & 3],
    // h = {0, 2, 3, 1} = 0x78 in 2-bit fields. A store's 8-lane group covers two whole rows (128 contiguous bytes): free of
    // conflicts under any slot permutation. A fragment read (row 16 j + (lane & 15), dword lane >> 4) puts the 16 lanes of
    // every ds_read_b128 lane group ({0-3, 12-15, 20-27}, ...) on 16 different (row & 3, slot) pairs = all 64 banks.
    const uint32_t img_wr = lds_base + pr * 64u + (((lane & 3u) ^ ((0x78u >> (2u * ((pr >> 2) & 3u))) & 3u)) * 16u);

    // LDS-DMA of the wave's piece of stage s into bit slot `slot`. Stages beyond the last one re-read the
    // last block (never consumed): every iteration issues exactly one piece, so every wait is vmcnt(2).
    auto issue = [&](uint32_t s, uint32_t slot) {
        const uint32_t blk = s < s_turn ? blk_first - s : blk_rest;
        const uint8_t* base = X + (uint64_t)(blk * (uint32_t)kStripBRows) * row_bytes + kbyte;
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, -1, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rsrc, (lptr_t)(lds_raw + kSr16ImgBytes + slot * kSr16BitStage + wave * 256u), 4,
            (int)goff0, 0, 0, 0);
    };

    // A fragments: a[m] = the four classes of dword lane >> 4 of the slice of row
    //   m < 4 : a_row0 + 64 wave + 16 m + (lane & 15)               (block wave of the tile: the low half)
    //   m >= 4: a_row0 + 64 (7 - wave) + 16 (m - 4) + (lane & 15)   (block 7 - wave: the high half)
    // Element order inside the k-step: (dword, class, nibble), the image's order.
    // (loaded in front of the DMA pieces, so that the wait for them leaves the pieces in flight)
    v4i a[8];
    {
        const uint8_t* ap = X + (uint64_t)(it.a_row0 + (lane & 15u)) * row_bytes + kbyte + (lane >> 4) * 4u;
        uint32_t aw[8];
#pragma unroll
        for (int m = 0; m < 8; ++m)
            aw[m] = *reinterpret_cast<const uint32_t*>(
                ap + (uint64_t)((m < 4 ? blk_lo : blk_hi) * (uint32_t)kStripBRows + (uint32_t)(m & 3) * 16u) * row_bytes);
        issue(0u, 0u);
        issue(1u, 1u);
        issue(2u, 2u);
#pragma unroll
        for (int m = 0; m < 8; ++m) a[m] = sr16_inflate(aw[m]);
    }

    v4f acc[8][2];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = v4f{};

    // fragment j of an image: row 16 j + (lane & 15), slot (lane >> 4) ^ h[(lane & 15) >> 2]
    const uint32_t boff = lds_base + (lane & 15u) * 64u + (((lane >> 4) ^ ((0x78u >> (2u * ((lane & 15u) >> 2))) & 3u)) * 16u);

#pragma unroll
    for (int m = 0; m < 8; ++m) asm volatile("" ::"v"(a[m]));  // retire the A loads here

    // fragment j of the image at byte offset `img` (a constant)
#define STORM_FETCH16(dst, img, j)                                                        \
    asm volatile("ds_read_b128 %0, %1 offset:%2"                                          \
                 : "=&v"(dst)                                                             \
                 : "v"(boff), "n"((img) + (j) * 16 * 64))
#define STORM_FETCH16V(dst, img, j)                                                       \
    asm volatile("ds_read_b128 %0, %1 offset:%2"                                          \
                 : "=&v"(dst)                                                             \
                 : "v"(boff + (img)), "n"((j) * 16 * 64))
#define STORM_MUL1(m, j, frag)                                                            \
    acc[m][(j) & 1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(                   \
        v8i{a[m].x, a[m].y, a[m].z, a[m].w, 0, 0, 0, 0},                                  \
        v8i{frag.x, frag.y, frag.z, frag.w, 0, 0, 0, 0}, acc[m][(j) & 1], 4, 4, 0, 0, 0, 0)
#define STORM_MUL16(j, frag)                                                              \
    _Pragma("unroll") for (int m = 0; m < 8; ++m) STORM_MUL1(m, j, frag)
#define STORM_LGKM_STR(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory")
#define STORM_LGKM(n)    \
    STORM_LGKM_STR(n);   \
    __builtin_amdgcn_sched_barrier(0)
#define STORM_VM2()                                         \
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");        \
    __builtin_amdgcn_sched_barrier(0)

    uint32_t wb = 0;
    // the wave's quarter of the image of stage s, start to finish (prologue)
    auto build_image = [&](uint32_t s) {
        uint32_t slot = s % 3u;
        asm volatile("" : "+s"(slot));   // (opaque: the two addresses below are one addition each, not induction variables)
        asm volatile("ds_read_b32 %0, %1" : "=&v"(wb) : "v"(bits_rd + slot * kSr16BitStage));
        STORM_LGKM(0);
        const v4i e = sr16_inflate(wb);
        asm volatile("ds_write_b128 %0, %1" ::"v"(img_wr + slot * kSr16StageBytes), "v"(e) : "memory");
        __builtin_amdgcn_sched_barrier(0);
    };

    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // scalar loads of the item record

    v4i b0 = {}, b1 = {}, b2 = {}, b3 = {};
    uint32_t t = 0;
    // ---- the A tile's own 8 blocks, from RESIDENT images: the 8 B blocks of this phase are the tile's own 512 rows, which
    //      the four waves already hold inflated — a[m] has the bytes and the lane layout a fragment read returns (row
    //      16 j + (lane & 15), the four classes of dword lane >> 4). Every wave stores its 8 fragments at the address a
    //      fragment read uses, image blk = its block, fragment j = m & 3; one barrier publishes the tile, and behind it the
    //      phase has no DMA, no read-back, no inflation and no barrier. (A store is served in groups of 8 lanes on banks
    //      (a / 4) mod 32, a period of 128 bytes: lanes 8 g .. 8 g + 7 are rows 8 (g & 1) .. + 7 of the fragment at dword
    //      g >> 1, and rows r and r + 2 of a run of 4 share a slot, so every one of these stores is a 2-way conflict — 8
    //      LDS cycles each, 64 per wave and item, measured. The layout is the one the fragment reads need.)
    //      At block d the low half of wave w (block w, m < 4) keeps the strict upper triangle of its own 64 x 64 block at
    //      d == w and takes d > w whole; the high half (block 7 - w, m >= 4) does the same around d == 7 - w
    //      (strip_rows_role, storm_hip_plan.h): 7 whole products and 2 triangles for every wave, so the waves start at
    //      block w and finish together. Own block, A sub-block i = m & 3 against B sub-block j: only i <= j is multiplied,
    //      and the accumulator of (j, j) is masked IN PLACE (row < col of the C/D map) right behind fragment j. That is
    //      exact: acc[base + i][n] takes the fragments j = n and j = n + 2 with i <= j, so when (j, j) is masked
    //      acc[base + j][j & 1] holds nothing else — a half's own block is the first thing its accumulators see, and of
    //      that block (j, j - 2) was skipped and (j, j + 2) is still to come: acc[.][0] of i = 0 and acc[.][1] of i = 1 are
    //      masked before fragments 2 and 3 add to them, acc[i = 2][0] and acc[i = 3][1] are empty until (2, 2) and (3, 3)
    //      because (2, 0) and (3, 1) were skipped.
    //      The phase is four runs of blocks, each with ONE dataflow (a loop that branched per block made the register
    //      allocator shuffle the 64 accumulators between the paths and spill): low own | low whole | low whole + high own |
    //      both whole. A block step asks for its four fragments up front and multiplies behind counted waits (the four
    //      registers as a rotation across the steps, every wait lgkmcnt(3), measured the same: LAB_NOTES).
    if (it.diag) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            uint32_t ib = (m < 4 ? blk_lo : blk_hi) * kSr16StageBytes;
            asm volatile("" : "+s"(ib));
            asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(boff + ib), "v"(a[m]), "n"((m & 3) * 16 * 64) : "memory");
        }
        STORM_LGKM(0);
        __builtin_amdgcn_s_barrier();    // the eight images are complete
        // C/D map: col = lane & 15 (B row), row = 4 * (lane >> 4) + reg (A row): reg r survives where r < tri
#define STORM_SR16_MASK(m, n)                                                             \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) acc[m][n][r] = r < tri ? acc[m][n][r] : 0.0f;
        // fragment j of block d against the half's four A sub-blocks
#define STORM_SR16_WHOLE(base, j, frag)                                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) STORM_MUL1((base) + i, j, frag);
        // fragment j of the half's own block: sub-blocks i <= j, (j, j) masked
#define STORM_SR16_OWN01(base, j, frag)                                                   \
    _Pragma("unroll") for (int i = 0; i <= (j); ++i) STORM_MUL1((base) + i, j, frag);     \
    STORM_SR16_MASK((base) + (j), j)
#define STORM_SR16_OWN23(base, j, frag)                                                   \
    _Pragma("unroll") for (int i = 0; i <= (j); ++i) STORM_MUL1((base) + i, j, frag);     \
    STORM_SR16_MASK((base) + (j), (j) - 2)
        // (sb: the image's offset as an opaque scalar, added to the fragment address at every use — as an induction
        //  variable in a vector register it costs what the loops do not have)
#define STORM_SR16_HEAD()                                                                 \
    uint32_t sb = d * kSr16StageBytes;                                                    \
    asm volatile("" : "+s"(sb));                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    STORM_FETCH16V(b0, sb, 0);                                                            \
    STORM_FETCH16V(b1, sb, 1);                                                            \
    STORM_FETCH16V(b2, sb, 2);                                                            \
    STORM_FETCH16V(b3, sb, 3)
        // Blocks from nb on hold no row below n_rows: nothing is multiplied against them, and a half whose own block is one of
        // them multiplies nothing. The four runs keep their dataflow and are bounded by uniform conditions alone.
        const uint32_t nb = strip_rows_real_blocks(it.a_row0, n_rows);
        uint32_t d = strip_rows_diag_begin(wave);
        if (blk_lo < nb) {
        {                                // d == blk_lo: low own
            STORM_SR16_HEAD();
            const uint32_t lane_d = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const int tri = (int)(lane_d & 15u) - (int)(4u * (lane_d >> 4));
            STORM_LGKM(3); STORM_SR16_OWN01(0, 0, b0) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(2); STORM_SR16_OWN01(0, 1, b1) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(1); STORM_SR16_OWN23(0, 2, b2) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(0); STORM_SR16_OWN23(0, 3, b3) __builtin_amdgcn_sched_barrier(0);
            ++d;
        }
#pragma unroll 1
        for (; d < min(blk_hi, nb); ++d) {   // low whole
            STORM_SR16_HEAD();
            STORM_LGKM(3); STORM_SR16_WHOLE(0, 0, b0) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(2); STORM_SR16_WHOLE(0, 1, b1) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(1); STORM_SR16_WHOLE(0, 2, b2) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(0); STORM_SR16_WHOLE(0, 3, b3) __builtin_amdgcn_sched_barrier(0);
        }
        if (blk_hi < nb) {
        {                                // d == blk_hi: low whole, high own
            STORM_SR16_HEAD();
            const uint32_t lane_d = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            const int tri = (int)(lane_d & 15u) - (int)(4u * (lane_d >> 4));
            STORM_LGKM(3); STORM_SR16_WHOLE(0, 0, b0) STORM_SR16_OWN01(4, 0, b0) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(2); STORM_SR16_WHOLE(0, 1, b1) STORM_SR16_OWN01(4, 1, b1) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(1); STORM_SR16_WHOLE(0, 2, b2) STORM_SR16_OWN23(4, 2, b2) __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(0); STORM_SR16_WHOLE(0, 3, b3) STORM_SR16_OWN23(4, 3, b3) __builtin_amdgcn_sched_barrier(0);
            ++d;
        }
#pragma unroll 1
        for (; d < min(strip_rows_diag_end(wave), nb); ++d) {   // both whole
            STORM_SR16_HEAD();
            STORM_LGKM(3); STORM_MUL16(0, b0); __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(2); STORM_MUL16(1, b1); __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(1); STORM_MUL16(2, b2); __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(0); STORM_MUL16(3, b3); __builtin_amdgcn_sched_barrier(0);
        }
        }   // blk_hi < nb
        }   // blk_lo < nb
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();    // every wave has read images 0 and 1: the pipelined ring is overlaid on images 0 .. 2
#undef STORM_SR16_HEAD
#undef STORM_SR16_OWN23
#undef STORM_SR16_OWN01
#undef STORM_SR16_WHOLE
#undef STORM_SR16_MASK
    }
    // ---- later blocks, software-pipelined across stage boundaries. Iteration t, behind barrier t: LDS operations in flight
    //      on entry: fragments 0 and 1 of image t (fa, fb), nothing else. A stage is 4 fragments of 8 MFMAs (128 pipe clocks
    //      each); they are read two ahead into a rotation of three registers, which a stage rotates by one, as it does the
    //      ring slot: the body is instantiated three times, I = the slot of the image it multiplies. The piece of stage t + 2
    //      is read in front of the fragments, inflated beside fragment 1's MFMAs and written as image t + 2 — ONE store; it
    //      has retired at the last wait of the body, so the barrier behind it publishes the image. The lgkmcnt values count
    //      the operations that may stay in flight behind the one needed:
    //        in flight                 wait  then
    //        fa fb wb fc               3     fragment 0 (fa)
    //        fb wb fc fa'              2     the piece; fragment 1 (fb); the store
    //        fc fa' wr fb'             3     fragment 2 (fc)
    //        fa' wr fb' fc'            2     fragment 3 (fa'); the store has retired
    //      A fragment register is asked for again right behind the 8 MFMAs that read it as their B operand (fa above): the
    //      read is issued in order behind the last of them, which has taken its operands long before an LDS read can return
    //      — strip16_bits_kernel's convention, with 4 MFMAs in front of the reload there.
    //      Beyond the last stage the next image, the piece and the image written are stale and never consumed: the body is
    //      branch-free.
    //      Exactness: an accumulator gains at most 2 x 128 = 256 per stage and runs are capped at 4096 stages (+ 8 blocks of
    //      the diagonal phase): below 2^24.
#define STORM_SR16_BODY(I, fa, fb, fc)                                                                      \
    {                                                                                                       \
        issue(t + 4u, ((I) + 1) % 3);   /* into the slot of stage t + 1, read an iteration ago */           \
        STORM_VM2();                    /* the piece of stage t + 2 has landed */                           \
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(wb) : "v"(bits_rd), "n"((((I) + 2) % 3) * kSr16BitStage)); \
        v4i e;                                                                                              \
        STORM_FETCH16(fc, (I) * kSr16StageBytes, 2); STORM_LGKM(3); STORM_MUL16(0, fa); __builtin_amdgcn_sched_barrier(0); \
        STORM_FETCH16(fa, (I) * kSr16StageBytes, 3); STORM_LGKM(2);   /* the piece and fb have landed */    \
        e = sr16_inflate(wb); STORM_MUL16(1, fb); __builtin_amdgcn_sched_barrier(0);                        \
        asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(img_wr), "v"(e), "n"((((I) + 2) % 3) * kSr16StageBytes) : "memory"); \
        STORM_FETCH16(fb, (((I) + 1) % 3) * kSr16StageBytes, 0); STORM_LGKM(3); STORM_MUL16(2, fc); __builtin_amdgcn_sched_barrier(0); \
        STORM_FETCH16(fc, (((I) + 1) % 3) * kSr16StageBytes, 1); STORM_LGKM(2); STORM_MUL16(3, fa); __builtin_amdgcn_sched_barrier(0); \
        ++t;                                                                                                \
        if (t >= Tl) break;                                                                                 \
        __builtin_amdgcn_s_barrier();                                                                       \
    }
    if (T != 0u) {
        // Invariant at the top of iteration t, in front of its issue: the pieces of stages <= t + 3 have been
        // issued, those of stages <= t + 1 have landed and been turned into images.
        STORM_VM2();        // stage 0 (1 and 2 in flight)
        build_image(0u);
        STORM_LGKM(0);      // the piece has been read: its slot takes stage 3
        issue(3u, 0u);
        STORM_VM2();        // stage 1
        build_image(1u);
        STORM_LGKM(0);
        __builtin_amdgcn_s_barrier();
        STORM_FETCH16(b0, 0, 0);   // stage 0 sits in slot 0
        STORM_FETCH16(b1, 0, 1);
        if (Tl != 0u)
            for (;;) {
                STORM_SR16_BODY(0, b0, b1, b2)   // leaves fragments 0, 1 of the next image in b1, b2
                STORM_SR16_BODY(1, b1, b2, b0)   // ... in b2, b0
                STORM_SR16_BODY(2, b2, b0, b1)   // ... in b0, b1
            }
        STORM_LGKM(0);
        // The trimmed top block: image Tl in slot Tl % 3, published by the barrier in front of body Tl - 1 (or the prologue's);
        // body Tl - 1 of any wave still writes slot (Tl + 1) % 3 only. Its fragments 0 and 1 are in flight in the registers of
        // the exit site — b0, b1 | b1, b2 | b2, b0 — but MFMAs on three paths, or one path behind selects, made the register
        // allocator move the accumulators and spill: the two fragments are read AGAIN, at a scalar offset, into b0 and b1.
        // One dataflow, two ds_read_b128 and one LDS round trip per trimmed item; no barrier, no ring upkeep.
        if (top_frags) {
            uint32_t sb = (Tl % 3u) * kSr16StageBytes;
            asm volatile("" : "+s"(sb));
            STORM_FETCH16V(b0, sb, 0);
            STORM_FETCH16V(b1, sb, 1);
            STORM_LGKM(1); STORM_MUL16(0, b0); __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(0);
            if (top_frags == 2u) { STORM_MUL16(1, b1); __builtin_amdgcn_sched_barrier(0); }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pieces issued beyond the last stage: none may land in a successor's LDS
    asm volatile("" ::"v"(b0), "v"(b1), "v"(b2), "v"(b3), "v"(wb));   // (every asm load's output lives up to its wait)
#undef STORM_SR16_BODY
#undef STORM_VM2
#undef STORM_FETCH16V
#undef STORM_FETCH16
#undef STORM_MUL16
#undef STORM_MUL1
#undef STORM_LGKM
#undef STORM_LGKM_STR

    STORM_CLOCK_END();
    uint64_t mine = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {  // 8 entries below 2^24 each: a uint32 cannot overflow
        uint32_t part = 0;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) part += (uint32_t)acc[m][n][r];
        mine += part;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    // (lane and thread index are taken afresh, as in strip16_bits_kernel: kept alive across the stage loop they cost registers)
    const uint32_t lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t tid_e = wave * 64u + lane_e;
    if (out == nullptr) {   // the partial sums stay in the slots: a fold launch follows (fold_slots_kernel)
        if (lane_e == 0 && mine != 0)
            atomicAdd(&slots[(blockIdx.x * kW + wave) & (kSlots - 1)],
                      (unsigned long long)mine);
        return;
    }
    // ---- the fold inside the launch: strip16_bits_kernel's, word for word (sum and arrival in one fire-and-forget atomic,
    //      the workgroup dispatched last polls, writes the total and leaves the slots zeroed)
    if (lane_e == 0)
        atomicAdd(&slots[(blockIdx.x * kW + wave) & (fold_slots - 1u)],
                  (unsigned long long)mine + (1ull << 48));
    if (blockIdx.x != gridDim.x - 1u) return;
    const unsigned long long expected = (unsigned long long)gridDim.x * (unsigned long long)kW;
    unsigned long long* wsum = reinterpret_cast<unsigned long long*>(lds_raw);   // [0 .. kW) arrivals, [kW .. 2 kW) sums per wave
    unsigned long long total = 0;
    for (;;) {
        unsigned long long cnt = 0, sum = 0;
        for (uint32_t i = tid_e; i < fold_slots; i += (kW * 64u)) {
            const unsigned long long v = __hip_atomic_load(&slots[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cnt += v >> 48;
            sum += v & ((1ull << 48) - 1ull);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_down(cnt, o, 64);
            sum += __shfl_down(sum, o, 64);
        }
        __syncthreads();   // (the previous round's reads of wsum are done)
        if (lane_e == 0) {
            wsum[wave] = cnt;
            wsum[kW + wave] = sum;
        }
        __syncthreads();
        cnt = 0;
        total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kW; ++w) {
            cnt += wsum[w];
            total += wsum[kW + w];
        }
        if (cnt == expected) break;
        if (fold_slots > (kW * 64u)) __builtin_amdgcn_s_sleep(8);   // (long launches: poll gently)
    }
    for (uint32_t i = tid_e; i < fold_slots; i += (kW * 64u))
        __hip_atomic_store(&slots[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid_e == 0) out[0] = total;
}
