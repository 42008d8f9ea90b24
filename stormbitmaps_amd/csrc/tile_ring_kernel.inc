// tile_ring_kernel.inc — K2r: the materialised-output kernel of round 5 (option k2_tile_shape = 5, the default).
// Included by storm_hip_mfma.hip inside namespace storm. Prototype, ablations and the schedule experiments:
// tools/probes/tile_ring.hip, profiles/r05_b_*; design notes: DESIGN.md §4.
//
// One 256 x 256 output tile per workgroup over its k range, on v_mfma_f32_16x16x128_f8f6f4 — the shape that draws the
// least socket power per FLOP (1110 W against 1310 W for 32x32x64 at the same rate on one-hot operands,
// profiles/r05_a_clock_power.jsonl) — with BOTH operands read as fragments from FP4 images that the workgroup builds
// once in the LDS (K2b's image, swizzle and rotate-and-mask codes: every product 1.0, plain unscaled MFMAs):
//   workgroup : 8 waves, two per SIMD; wave (wa, wb) owns A rows 128 wa .. + 127 against B rows 64 wb .. + 63 = 8 x 4
//               blocks of 16 x 16 (128 accumulator registers); SIMD partners are (wa, wb) and (1 - wa, 3 - wb), which
//               on a diagonal tile hold complementary shares of the triangle.
//   stage     : one class of one 512-bit chunk = one k-step of 128 bits: images of 256 A rows + 256 B rows x 64 B =
//               32 KiB, ring of 4 (128 KiB). Stage s multiplies image s FROM REGISTERS — its fragments were read during
//               stage s - 1: fa[m] is reloaded right behind the last MFMA of row m and has a whole stage to arrive, the
//               B fragments go into the other of two register sets — and stores the wave's share of image s + 3: 4 of
//               the 32 pieces of 16 rows x 64 B (shift, mask, ds_write_b128), one piece per second row.
//   bits      : raw buffer loads straight into registers (rows beyond the matrix and chunks beyond the item's k range
//               read as zero through the descriptor's range), issued five stages ahead of their first use; two chunks
//               live in registers.
//   sync      : one s_barrier per stage. What it orders is two stages old by then (an image stored in stage s is first
//               read in stage s + 2), so no wave waits for an LDS operation at the barrier, only for the other waves.
//   lgkmcnt   : LDS operations of a wave complete in order and every stage issues the same sequence of them; the
//               waits in front of the rows are counted from that sequence (tr_waits).
//   what the LDS costs (ablations of the prototype, sustained runs, one box): every ds_write_b128 holds its SIMD for
//               ~11 clocks (8 per SIMD and stage: 9 %), every fragment read for ~2.5 (24: 6 %), the inflation's vector
//               operations 2 %, the per-stage barrier 8 %; the same loop with MFMAs only runs at 0.97 of the pipe.
// A wave multiplies only the blocks it needs: rows [0, MH) x columns [0, NH) of its 8 x 4, instantiated for MH = 4 / 8
// and NH = 1 / 4 (diagonal tiles: the blocks wholly below the diagonal drop out; ragged last row block: the blocks
// beyond the output); a wave with nothing to multiply still loads, inflates and stores its pieces.
// Items, output conventions (triangle / band / rectangle, AND / OR / XOR through row_counts, k-split items that add
// into a cleared window) are tilebits8_kernel's. Extends the reference (README.md:165-167: per-pair counts for LD);
// the loop it stands for is storm.c:1199-1238 with the leaf's result kept per pair.
constexpr int kTrThreads = 512;
constexpr uint32_t kTrRowBytes = 128u;                      // two k-steps of 64 B per image row
constexpr uint32_t kTrPairBytes = (uint32_t)kTile * kTrRowBytes;   // 32 KiB: two ring slots of one operand
constexpr uint32_t kTrOperandBytes = 2u * kTrPairBytes;    // 64 KiB: the four ring slots of one operand
constexpr uint32_t kTrLdsBytes = 2u * kTrOperandBytes;     // 128 KiB

template <int C>
__device__ __forceinline__ v4i tr_inflate(v4i w) {   // class C (bits 4 n + C) to E2M1 1.0 = bit 1 of every nibble
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    if constexpr (C == 0) return (v4i)(((v4u)w << 1u) & kSb16Mask);
    else if constexpr (C == 1) return w & (int)kSb16Mask;
    else return (v4i)(((v4u)w >> (unsigned)(C - 1)) & kSb16Mask);
}
template <int OFF>
__device__ __forceinline__ void tr_read128(v4i& dst, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(OFF));
}
template <int OFF>
__device__ __forceinline__ void tr_write128(uint32_t addr, const v4i& e) {
    asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(e), "n"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void tr_lgkm() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void tr_keep(const v4i& v) { asm volatile("" ::"v"(v)); }
// one arrival on the counter at cnt_addr + OFF: an LDS add from lane 0 alone (64 adds to one address would serialise)
template <int OFF>
__device__ __forceinline__ void tr_signal(uint32_t cnt_addr) {
    uint64_t saved;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tds_add_u32 %1, %2 offset:%3\n\ts_mov_b64 exec, %0"
                 : "=&s"(saved)
                 : "v"(cnt_addr), "v"(1u), "n"(OFF)
                 : "memory");
}
template <int OFF>
__device__ __forceinline__ void tr_cnt_read(uint32_t& dst, uint32_t cnt_addr) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=&v"(dst) : "v"(cnt_addr), "n"(OFF));
}

// The LDS operations of one stage, in issue order, for a wave that multiplies MH x NH blocks: row m issues the reload
// of fa[m], the read of fb'[m] (m < NH), with kFlags in row MH / 2 the early read of the counter the NEXT stage checks, in
// every (MH / 4)-th row the store of a piece, and behind the last row the wave's signal (an LDS add). From that
// sequence: how many operations may stay in flight when ...
template <int MH, int NH, bool kFlags>
struct tr_waits {
    static constexpr int kPer = MH / 4;                                  // rows per stored piece
    enum { RA = 0, RB = 1, ST = 2, CK = 3, SG = 4 };
    // position of operation (kind, index) in the stage's sequence, or the sequence's length for kind < 0
    static constexpr int pos(int kind, int idx) {
        int n = 0;
        for (int m = 0; m < MH; ++m) {
            if (kind == RA && idx == m) return n;
            ++n;
            if (m < NH) {
                if (kind == RB && idx == m) return n;
                ++n;
            }
            if (kFlags && m == MH / 2) {   // (in front of the row's store: the check then never waits for a store)
                if (kind == CK) return n;
                ++n;
            }
            if (m % kPer == 0) {
                if (kind == ST && idx == m / kPer) return n;
                ++n;
            }
        }
        if (kFlags) {
            if (kind == SG) return n;
            ++n;
        }
        return n;
    }
    static constexpr int kOps = pos(-1, 0);
    static constexpr int cap(int v) { return v < 15 ? v : 15; }
    // ... row m starts: fa[m] was reloaded exactly one stage of operations ago (operations issued in this stage before
    // row m = pos(RA, m))
    static constexpr int kRow = cap(kOps - 1);
    // ... row 0 starts: all of fb' must have landed; the last of them is fb'[NH - 1]
    static constexpr int kRow0 = cap(kOps - 1 - pos(RB, NH - 1)) < kRow ? cap(kOps - 1 - pos(RB, NH - 1)) : kRow;
    // ... the next stage looks at the counter read early: the operations behind it
    static constexpr int kCheck = cap(kOps - 1 - pos(CK, 0));
    // ... the stage ends in a barrier (no flags): the stores of the PREVIOUS stage must have landed (a whole stage of
    // operations is younger)
    static constexpr int kEnd = cap(kOps);
    // ... a wave running half a stage behind reaches its barrier (behind row MH / 2 - 1): the stores of the half stage at the
    // head of the interval (rows MH / 2 .. MH - 1 of the previous stage) must have landed
    static constexpr int kLateEnd = cap(kOps - 1 - pos(ST, 3) + pos(RA, MH / 2));
};

//   sync (kFlags) : instead of the barrier, one LDS counter per ring slot: a wave adds 1 behind its last LDS operation of a
//               stage (LDS operations of a wave execute in order: the add is behind its image stores and fragment reads) and,
//               at the top of stage s, wants 8 arrivals for stage s - 2 — the stage in which image s + 1 (read now) was stored
//               and image s - 1 (whose slot is stored into now) was last read. The counter is read half a stage early, so a
//               wave spins only when it is more than half a stage ahead of the slowest; waves may drift a stage apart.
template <bool kFlags>
__global__ __launch_bounds__(kTrThreads, 2) void tilering_kernel(
    TileOperands ops, const MfmaItem* __restrict__ items, OutWindow window, uint32_t split_from, uint32_t* __restrict__ parts) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[kTrLdsBytes + 64u];   // + the four arrival counters
    STORM_CLOCK_BEGIN();

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wq = wave & 3u;
    const uint32_t wa = wave < 4u ? (wq & 1u) : 1u - (wq & 1u);   // waves w and w + 4 share a SIMD
    const uint32_t wb = wave < 4u ? (wq >> 1) : 3u - (wq >> 1);
    const uint32_t item_idx = blockIdx.x;
    const MfmaItem it = items[item_idx];
    const uint32_t a_row0 = (uint32_t)it.I * kTile, b_row0 = (uint32_t)it.J * kTile;
    const uint32_t S = it.n_stages / 4u;          // chunks of 64 B (512 bits of k)
    const uint32_t kbyte0 = it.stage0 * 16u;
    const uint32_t pitch = (uint32_t)ops.pitch;

    const uint8_t *a_base, *b_base;
    uint32_t a_bytes, b_bytes;
    ops.tile_rows(a_row0, (uint32_t)kTile, a_base, a_bytes);
    ops.tile_rows(b_row0, (uint32_t)kTile, b_base, b_bytes);

    // blocks this wave multiplies: rows [0, mh) x columns [0, nh) of its 8 x 4
    const uint32_t col_limit = window.col_end();
    const uint32_t vc = col_limit > b_row0 ? min(col_limit - b_row0, (uint32_t)kTile) : 0u;
    const uint32_t va = window.n_rows > a_row0 ? min(window.n_rows - a_row0, (uint32_t)kTile) : 0u;
    const uint32_t nh = vc > 64u * wb ? min((vc - 64u * wb + 15u) / 16u, 4u) : 0u;
    uint32_t mh = va > 128u * wa ? min((va - 128u * wa + 15u) / 16u, 8u) : 0u;
    const bool diag = !window.rect() && a_row0 == b_row0;
    if (diag) {   // rows at or beyond the wave's last column meet no column behind them
        const uint32_t jmax = 64u * wb + 16u * nh;
        mh = jmax > 128u * wa ? min(mh, (jmax - 128u * wa + 15u) / 16u) : 0u;
    }

    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)&lds[0];
    // fragment (block b, ring slot S): row 16 b + (lane & 15), 16-byte slot (4 (S & 1) + (lane >> 4)) ^ swizzle of pair S >> 1
    const uint32_t fr0 = lds_base + (lane & 15u) * kTrRowBytes + (((lane >> 4) ^ (((lane & 15u) >> 1) & 7u)) * 16u);
    const uint32_t fa_addr[2] = {fr0 + wa * 8u * 2048u, (fr0 ^ 64u) + wa * 8u * 2048u};
    const uint32_t fb_addr[2] = {fr0 + kTrOperandBytes + wb * 4u * 2048u, (fr0 ^ 64u) + kTrOperandBytes + wb * 4u * 2048u};
    // the wave's pieces: rows 32 wave + 16 (p & 1) + pr of the A tile (p = 0, 1) and of the B tile (p = 2, 3); lanes 4 g ..
    // 4 g + 3 hold the four 16-byte quarters of one row, the two rows of an 8-lane group are 8 apart (conflict-free stores)
    const uint32_t pr = (lane >> 3) + 8u * ((lane >> 2) & 1u);
    const uint32_t wr0 = lds_base + (wave * 32u + pr) * kTrRowBytes + (((lane & 3u) ^ ((pr >> 1) & 7u)) * 16u);
    const uint32_t wr_addr[2][2] = {{wr0, wr0 ^ 64u}, {wr0 + kTrOperandBytes, (wr0 ^ 64u) + kTrOperandBytes}};
    const uint32_t cnt_addr = lds_base + kTrLdsBytes;   // counter of ring slot S (the stages s = S mod 4) at + 4 S
    const uint32_t voff0 = (wave * 32u + pr) * pitch + (lane & 3u) * 16u;
    const uint32_t voff1 = voff0 + 16u * pitch;

    typedef unsigned v4u_tr __attribute__((ext_vector_type(4)));
    v4i bits[2][4];   // [chunk parity][piece]
    auto load_chunk = [&](int par, uint32_t c) __attribute__((always_inline)) {
        const uint32_t koff = kbyte0 + c * 64u;
        const uint32_t ab = c < S ? a_bytes : 0u, bb = c < S ? b_bytes : 0u;
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(a_base + koff), 0, ab ? ab - koff : 0u, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(b_base + koff), 0, bb ? bb - koff : 0u, 0x00020000);
        bits[par][0] = (v4i)(v4u_tr)__builtin_amdgcn_raw_buffer_load_b128(ra, (int)voff0, 0, 0);
        bits[par][1] = (v4i)(v4u_tr)__builtin_amdgcn_raw_buffer_load_b128(ra, (int)voff1, 0, 0);
        bits[par][2] = (v4i)(v4u_tr)__builtin_amdgcn_raw_buffer_load_b128(rb, (int)voff0, 0, 0);
        bits[par][3] = (v4i)(v4u_tr)__builtin_amdgcn_raw_buffer_load_b128(rb, (int)voff1, 0, 0);
    };

    // [r5] a k-part writes its counts into its own 256 x 256 window of `parts` (plain stores; reduce_parts_kernel adds a tile's
    // windows up): see tilebits8_kernel. parts == nullptr: the parts add into the cleared output with atomics.
    uint32_t* part_tile = (item_idx >= split_from && parts) ? parts + (uint64_t)(item_idx - split_from) * (kTile * kTile) : nullptr;
    const bool full_tile = window.covers(a_row0, (uint32_t)kTile, b_row0, (uint32_t)kTile);
    const bool interior = full_tile && (part_tile ? true
                                                  : (item_idx < split_from && (window.ld & 3u) == 0 && ((uintptr_t)window.out & 15u) == 0 && (window.j_base & 3u) == 0));

    auto run = [&](auto mhc, auto nhc, auto latec) __attribute__((always_inline)) {
        constexpr int MH = decltype(mhc)::value, NH = decltype(nhc)::value;   // MH = 0: nothing to multiply
        constexpr bool kLate = decltype(latec)::value != 0;                   // waves 4 - 7: half a stage behind their SIMD partners
        constexpr int MHA = MH ? MH : 1, NHA = MH ? NH : 1;
        using W = tr_waits<MH ? MH : 4, MH ? NH : 1, kFlags>;
        v4f acc[MHA][NHA];
#pragma unroll
        for (int m = 0; m < MHA; ++m)
#pragma unroll
            for (int n = 0; n < NHA; ++n) acc[m][n] = v4f{};
        v4i fa[MHA], fb[2][NHA];

        // ---- prologue: chunks 0 and 1 in registers, images 0, 1, 2 (classes 0, 1, 2 of chunk 0) stored, the fragments of
        //      image 0 read
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // scalar loads of the item record
        if (kFlags && tid < 4u) reinterpret_cast<uint32_t*>(&lds[kTrLdsBytes])[tid] = 0u;
        load_chunk(0, 0u);
        load_chunk(1, 1u);
        tb_static_for<3>([&](auto cc) __attribute__((always_inline)) {
            constexpr int c = decltype(cc)::value;
            tb_static_for<4>([&](auto pc) __attribute__((always_inline)) {
                constexpr int p = decltype(pc)::value;
                tr_write128<(c >> 1) * kTrPairBytes + (p & 1) * 16 * kTrRowBytes>(wr_addr[p >> 1][c & 1], tr_inflate<c>(bits[0][p]));
            });
        });
        tr_lgkm<0>();
        __builtin_amdgcn_s_barrier();
        if constexpr (MH > 0) {
            tb_static_for<MH>([&](auto mc) __attribute__((always_inline)) {
                constexpr int m = decltype(mc)::value;
                tr_read128<m * 2048>(fa[m], fa_addr[0]);
            });
            tb_static_for<NH>([&](auto nc) __attribute__((always_inline)) {
                constexpr int n = decltype(nc)::value;
                tr_read128<n * 2048>(fb[0][n], fb_addr[0]);
            });
        }
        tr_lgkm<0>();
        uint32_t ck = 0u;   // the counter read early for the next stage's check
        if constexpr (kFlags) tr_signal<3 * 4>(cnt_addr);   // "stage -1": the prologue's reads of image 0 are done

        // ---- stages, eight per trip (two chunks): stage j multiplies image j (ring slot j & 3), reads image j + 1 and
        //      stores image j + 3. A trip beyond the item's last chunk multiplies images of zeros.
        const uint32_t n_trips = (S + 1u) / 2u;
        if constexpr (!kFlags) {
        // ---- barrier form, STAGGERED: SIMD partners w and w + 4 run the same program behind the same barriers, and in step they
        //      ask for the vector issue, the LDS and the matrix pipe at the same moments. Waves 4 - 7 therefore run half a stage
        //      BEHIND: between two barriers waves 0 - 3 execute stage s, waves 4 - 7 the second half of stage s - 1 and the first
        //      half of stage s (MI355X_MICROARCH.md, "Two waves per SIMD", item 9). Same instruction sequence per wave, same
        //      number of barriers; what a barrier orders is still at least half a stage old on both sides (derivation: DESIGN §4).
        auto half = [&](auto jc, auto hc, uint32_t trip) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value, h = decltype(hc)::value;
            constexpr int S1 = (j + 1) & 3;                                  // ring slot read
            constexpr int T = j + 3, S3 = T & 3, C3 = T & 3, PAR3 = (T >> 2) & 1;   // image stored: slot, class, chunk parity
            constexpr int cur = j & 1;                                       // fb set multiplied in this stage
            if constexpr (MH > 0) {
                tb_static_for<MH / 2>([&](auto mc) __attribute__((always_inline)) {
                    constexpr int m = h * (MH / 2) + decltype(mc)::value;
                    constexpr bool stores = (m % W::kPer) == 0;
                    constexpr int p = m / W::kPer;
                    tr_lgkm<(m == 0 ? W::kRow0 : W::kRow)>();
                    __builtin_amdgcn_sched_barrier(0);
                    v4i e = {};
                    if constexpr (stores) e = tr_inflate<C3>(bits[PAR3][p]);
                    tb_static_for<NH>([&](auto nc) __attribute__((always_inline)) {
                        constexpr int n = decltype(nc)::value;
                        acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                            v8i{fa[m].x, fa[m].y, fa[m].z, fa[m].w, 0, 0, 0, 0},
                            v8i{fb[cur][n].x, fb[cur][n].y, fb[cur][n].z, fb[cur][n].w, 0, 0, 0, 0}, acc[m][n], 4, 4, 0, 0, 0, 0);
                    });
                    __builtin_amdgcn_sched_barrier(0);
                    tr_read128<(S1 >> 1) * kTrPairBytes + m * 2048>(fa[m], fa_addr[S1 & 1]);
                    if constexpr (m < NH) tr_read128<(S1 >> 1) * kTrPairBytes + m * 2048>(fb[cur ^ 1][m], fb_addr[S1 & 1]);
                    if constexpr (stores)
                        tr_write128<(S3 >> 1) * kTrPairBytes + (p & 1) * 16 * kTrRowBytes>(wr_addr[p >> 1][S3 & 1], e);
                    __builtin_amdgcn_sched_barrier(0);
                });
            } else {
                tb_static_for<2>([&](auto pc) __attribute__((always_inline)) {
                    constexpr int p = 2 * h + decltype(pc)::value;
                    tr_write128<(S3 >> 1) * kTrPairBytes + (p & 1) * 16 * kTrRowBytes>(wr_addr[p >> 1][S3 & 1],
                                                                                        tr_inflate<C3>(bits[PAR3][p]));
                });
            }
            if constexpr (h == 1 && (j & 3) == 0) load_chunk(PAR3, 2u * trip + (uint32_t)(T >> 2) + 2u);   // two chunks behind the one just finished
        };
        // in front of a barrier: the stores the OTHER waves read next must have landed. Waves 0 - 3: those of the previous stage
        // (a whole stage of operations is younger); waves 4 - 7: those of the half stage at the head of this interval.
        auto sync = [&]() __attribute__((always_inline)) {
            if constexpr (MH > 0) tr_lgkm<(kLate ? W::kLateEnd : W::kEnd)>();
            else tr_lgkm<(kLate ? 2 : 4)>();
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        };
        if constexpr (kLate) {
            half(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, 0u);
            sync();
        }
        for (uint32_t trip = 0; trip < n_trips; ++trip) {
            tb_static_for<8>([&](auto jc) __attribute__((always_inline)) {
                constexpr int j = decltype(jc)::value;
                if constexpr (!kLate) {
                    half(jc, std::integral_constant<int, 0>{}, trip);
                    half(jc, std::integral_constant<int, 1>{}, trip);
                } else {   // (behind the last stage: one more first half, of an image of zeros)
                    half(jc, std::integral_constant<int, 1>{}, trip);
                    half(std::integral_constant<int, (j + 1) & 7>{}, std::integral_constant<int, 0>{}, trip);
                }
                sync();
            });
        }
        if constexpr (!kLate) __builtin_amdgcn_s_barrier();   // (waves 4 - 7 have passed one barrier more: behind their first half stage)
        } else {
        for (uint32_t trip = 0; trip < n_trips; ++trip) {
            tb_static_for<8>([&](auto jc) __attribute__((always_inline)) {
                constexpr int j = decltype(jc)::value;
                constexpr int S1 = (j + 1) & 3;                                  // ring slot read
                constexpr int T = j + 3, S3 = T & 3, C3 = T & 3, PAR3 = (T >> 2) & 1;   // image stored: slot, class, chunk parity
                constexpr int cur = j & 1;                                       // fb set multiplied in this stage
                if constexpr (kFlags) {
                    // all eight waves are through stage j - 2: its counter (slot (j + 2) & 3) shows 8 arrivals per use of the
                    // slot so far (slot 3 was also used by the prologue, "stage -1")
                    constexpr int kArrivals = j == 0 ? 0 : j < 5 ? 8 : 16;
                    const uint32_t want = 16u * trip + (uint32_t)kArrivals;
                    // (ONE asm statement, loop and all: with the spin loop as C++ control flow the 8-stage body is cut into
                    //  basic blocks and hipcc spills accumulators between the MFMAs — 592 bytes of scratch in the loop)
                    uint32_t seen;
                    asm volatile(
                        "s_waitcnt lgkmcnt(%[k])\n\t"
                        "v_readfirstlane_b32 %[seen], %[ck]\n\t"
                        "s_cmp_ge_u32 %[seen], %[want]\n\t"
                        "s_cbranch_scc1 1f\n"
                        "0:\n\t"
                        "s_sleep 1\n\t"
                        "ds_read_b32 %[ck], %[addr] offset:%[off]\n\t"
                        "s_waitcnt lgkmcnt(0)\n\t"
                        "v_readfirstlane_b32 %[seen], %[ck]\n\t"
                        "s_cmp_lt_u32 %[seen], %[want]\n\t"
                        "s_cbranch_scc1 0b\n"
                        "1:"
                        : [ck] "+v"(ck), [seen] "=&s"(seen)
                        : [want] "s"(want), [addr] "v"(cnt_addr), [k] "n"(MH > 0 ? W::kCheck : 0), [off] "n"(((j + 2) & 3) * 4)
                        : "memory", "scc");
                }
                if constexpr (MH > 0) {
                    tb_static_for<MH>([&](auto mc) __attribute__((always_inline)) {
                        constexpr int m = decltype(mc)::value;
                        constexpr bool stores = (m % W::kPer) == 0;
                        constexpr int p = m / W::kPer;
                        // (the waits define the fragments they cover: nothing that reads them may move in front)
                        if constexpr (!kFlags) {
                            // (one basic block per trip: the plain waits hold; tying the fragments to them makes hipcc pad
                            //  every row with s_nop and reshuffle the vector operations: 0.322 -> ? ms per round of tiles)
                            tr_lgkm<(m == 0 ? W::kRow0 : W::kRow)>();
                        } else if constexpr (m == 0) {
                            if constexpr (NH == 4)
                                asm volatile("s_waitcnt lgkmcnt(%5)"
                                             : "+v"(fa[0]), "+v"(fb[cur][0]), "+v"(fb[cur][1]), "+v"(fb[cur][2]), "+v"(fb[cur][3])
                                             : "n"(W::kRow0));
                            else
                                asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(fa[0]), "+v"(fb[cur][0]) : "n"(W::kRow0));
                        } else {
                            asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(fa[m]) : "n"(W::kRow));
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        v4i e = {};
                        if constexpr (stores) e = tr_inflate<C3>(bits[PAR3][p]);
                        tb_static_for<NH>([&](auto nc) __attribute__((always_inline)) {
                            constexpr int n = decltype(nc)::value;
                            acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                                v8i{fa[m].x, fa[m].y, fa[m].z, fa[m].w, 0, 0, 0, 0},
                                v8i{fb[cur][n].x, fb[cur][n].y, fb[cur][n].z, fb[cur][n].w, 0, 0, 0, 0}, acc[m][n], 4, 4, 0, 0, 0, 0);
                        });
                        __builtin_amdgcn_sched_barrier(0);
                        tr_read128<(S1 >> 1) * kTrPairBytes + m * 2048>(fa[m], fa_addr[S1 & 1]);
                        if constexpr (m < NH) tr_read128<(S1 >> 1) * kTrPairBytes + m * 2048>(fb[cur ^ 1][m], fb_addr[S1 & 1]);
                        if constexpr (kFlags && m == MH / 2) tr_cnt_read<((j + 3) & 3) * 4>(ck, cnt_addr);   // what stage j + 1 checks
                        if constexpr (stores)
                            tr_write128<(S3 >> 1) * kTrPairBytes + (p & 1) * 16 * kTrRowBytes>(wr_addr[p >> 1][S3 & 1], e);
                        __builtin_amdgcn_sched_barrier(0);
                    });
                    if constexpr (kFlags) tr_signal<(j & 3) * 4>(cnt_addr);
                    else tr_lgkm<W::kEnd>();
                } else {
                    tb_static_for<4>([&](auto pc) __attribute__((always_inline)) {
                        constexpr int p = decltype(pc)::value;
                        tr_write128<(S3 >> 1) * kTrPairBytes + (p & 1) * 16 * kTrRowBytes>(wr_addr[p >> 1][S3 & 1],
                                                                                            tr_inflate<C3>(bits[PAR3][p]));
                    });
                    if constexpr (kFlags) {
                        tr_signal<(j & 3) * 4>(cnt_addr);
                        tr_cnt_read<((j + 3) & 3) * 4>(ck, cnt_addr);   // what stage j + 1 checks (the newest operation: that check waits for lgkmcnt(0))
                    } else {
                        tr_lgkm<4>();   // the stores of the previous stage have landed
                    }
                }
                if constexpr ((j & 3) == 0) load_chunk(PAR3, 2u * trip + (uint32_t)(T >> 2) + 2u);   // two chunks behind the one just finished
                if constexpr (!kFlags) __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        STORM_CLOCK_END();
        if constexpr (MH > 0) {
            tb_static_for<MH>([&](auto mc) __attribute__((always_inline)) { tr_keep(fa[decltype(mc)::value]); });
            tb_static_for<NH>([&](auto nc) __attribute__((always_inline)) {
                tr_keep(fb[0][decltype(nc)::value]);
                tr_keep(fb[1][decltype(nc)::value]);
            });
        }
        tb_static_for<4>([&](auto pc) __attribute__((always_inline)) {
            tr_keep(bits[0][decltype(pc)::value]);
            tr_keep(bits[1][decltype(pc)::value]);
        });
        if constexpr (MH == 0) return;

        // ---- epilogue. C/D map of a 16 x 16 block: col = lane & 15, row = 4 (lane >> 4) + reg.
        // (the window's fields are read here, behind the k-loop, and once: the kernel holds 256 VGPRs, and SGPRs kept live across
        //  the loop end up in spilled lanes; read where the members use them they would be fetched again behind every branch)
        const OutWindow w = window.loaded();
        const uint32_t le = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const uint32_t i0 = a_row0 + wa * 128u, j0 = b_row0 + wb * 64u;
        if constexpr (MH == 8 && NH == 4) {
            if (interior) {   // every wave of an interior tile runs this instantiation
                // Direct stores would be one 4-byte store per element in 64-byte runs. Each wave turns 32 rows x 64 columns
                // at a time through a private 16 KiB of the (now idle) ring — row pitch 68 words: conflict-free 4-byte stores —
                // and stores 16 bytes per lane: four 256-byte runs per instruction.
                __builtin_amdgcn_s_barrier();   // every wave has left the ring
                uint32_t* w32 = reinterpret_cast<uint32_t*>(&lds[0] + wave * 16384u);
                const OutWindow::counts_ptr_t rcs = part_tile ? nullptr : w.counts();   // (a part holds raw AND counts)
                const uint64_t ldx = part_tile ? (uint64_t)kTile : w.ld;
                uint32_t* out_tile = part_tile ? &part_tile[(i0 - a_row0) * (uint32_t)kTile + (j0 - b_row0)] : w.at(i0, j0);
                uint32_t nj[4] = {0u, 0u, 0u, 0u};
                if (rcs) {
#pragma unroll
                    for (int n = 0; n < 4; ++n) nj[n] = rcs[j0 + (uint32_t)n * 16u + (le & 15u)];
                }
#pragma unroll
                for (int mp = 0; mp < 4; ++mp) {
#pragma unroll
                    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const uint32_t il = (uint32_t)mm * 16u + 4u * (le >> 4) + (uint32_t)r;
                            const uint32_t ni = rcs ? rcs[i0 + (uint32_t)mp * 32u + il] : 0u;
#pragma unroll
                            for (int n = 0; n < 4; ++n) {
                                const uint32_t c = (uint32_t)acc[2 * mp + mm][n][r];
                                w32[il * 68u + (uint32_t)n * 16u + (le & 15u)] = rcs ? ni + nj[n] - w.and_weight * c : c;
                            }
                        }
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const uint32_t row = (uint32_t)q * 4u + (le >> 4);
                        const uint4 v = *reinterpret_cast<const uint4*>(&w32[row * 68u + 4u * (le & 15u)]);
                        *reinterpret_cast<uint4*>(&out_tile[(uint64_t)((uint32_t)mp * 32u + row) * ldx + 4u * (le & 15u)]) = v;
                    }
                }
                return;
            }
        }
#pragma unroll
        for (int n = 0; n < NH; ++n) {
            const uint32_t j = j0 + (uint32_t)n * 16u + (le & 15u);
            const bool j_ok = w.wants_col(j);
            const uint32_t njv = w.nj(j);
#pragma unroll
            for (int m = 0; m < MH; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t i = i0 + (uint32_t)m * 16u + 4u * (le >> 4) + (uint32_t)r;
                    if (j_ok && w.writes_row(i, j)) {
                        const uint32_t c = (uint32_t)acc[m][n][r];
                        uint32_t* dst = w.at(i, j);
                        if (item_idx < split_from) {
                            *dst = w.value(c, i, njv);
                        } else if (part_tile) {
                            part_tile[(i - a_row0) * (uint32_t)kTile + (j - b_row0)] = c;
                        } else {
                            atomicAdd(dst, w.part_value(c, i, njv, it.stage0 == 0));
                        }
                    }
                }
        }
    };

    // (the two halves of the workgroup run the same rows of code half a stage apart: see the barrier form above)
    auto go = [&](auto latec) __attribute__((always_inline)) {
        if (mh == 0u || nh == 0u) run(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, latec);
        else if (mh > 4u) {
            if (nh > 1u) run(std::integral_constant<int, 8>{}, std::integral_constant<int, 4>{}, latec);
            else run(std::integral_constant<int, 8>{}, std::integral_constant<int, 1>{}, latec);
        } else {
            if (nh > 1u) run(std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{}, latec);
            else run(std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{}, latec);
        }
    };
    if (kFlags || wave < 4u) go(std::integral_constant<int, 0>{});
    else go(std::integral_constant<int, 1>{});
}
