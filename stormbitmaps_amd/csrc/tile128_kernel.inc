// tile128_kernel.inc — K2h: the materialised-output kernel for matrices of FEW 256 x 256 tiles (round 6).
// Included by storm_hip_mfma.hip inside namespace storm; design notes: DESIGN.md §4.
//
// The 256 x 256 kernels (tilering_kernel, tilebits8_kernel) hold one workgroup per CU, so a matrix of fewer than a few
// hundred tiles (N below ~6000 rows) left CUs idle unless every tile was cut along k into parts that cleared, and then
// atomically added into, a whole 256 x 256 window each: 52 MB of atomics at 1024 rows (the chip adds 1.3 TB/s), 64 us for
// 7 us of MFMAs. This kernel works on 128 x 128 tiles, two workgroups per CU, and where even those are too few to fill the
// chip it cuts a tile along k into a handful of parts whose sums meet INSIDE the launch:
//   workgroup : 4 waves, one 128 x 128 tile over its item's k range; wave (wa, wb) owns A rows 64 wa .. + 63 against B rows
//               64 wb .. + 63 = 2 x 2 blocks of 32 x 32 (v_mfma_scale_f32_32x32x64_f8f6f4, 64 accumulator registers).
//   stage     : one 512-bit chunk: the bits of 128 A rows + 128 B rows x 64 B = 16 KiB by LDS-DMA, 4 pieces of 16 rows per
//               wave (lanes 4 g .. 4 g + 3 fetch the four quarters of one row: whole 64-byte runs per row — loading the
//               MFMA fragment layout straight from global memory touches four cache lines per lane quad and cost the
//               vector L1 64 clocks per instruction: the first form of this kernel, 2 x off its MFMA floor), ring of 4
//               (64 KiB: two workgroups per CU), ONE barrier per chunk (32 MFMAs per wave), three chunks in flight.
//   operands  : fragments by ds_read_b128 (lane l: row l & 31, 16-byte slot 2 j + (l >> 5) of the row for k-step j; the DMA
//               stores slot s of row r at s ^ ((r / 4) % 4): conflict free), one piece (k-step) ahead; tilebits8_kernel's
//               classes — class c = bits 4 n + c of every dword already sit in nibble n as the E2M1 code 1 << c (0.5, 1, 2;
//               class 3 is the sign bit and moves down once), block scales 128 / 127 / 126 / 126 on both operands make every
//               product 1.0 — inflated for the NEXT multiply step beside the MFMAs of the current one: 5 vector operations
//               per MFMA.
//   diagonal  : on a tile that straddles the diagonal wave (1, 0) has nothing to multiply (it still moves its pieces and
//               joins the barriers) and waves (0, 0), (1, 1) skip the block below the diagonal.
//   k-parts   : an item may cover a part of the tile's k range (host: as many parts as fill the CUs' two slots, never more
//               than needed). Every part stores its accumulators AS THEY LIE (register layout: 1 KiB runs, write-through
//               sc1 stores) into its own 64 KiB window, drains them, and takes a ticket on the tile (one agent-scope atomic
//               by one lane behind the workgroup's barrier); the part whose ticket is the last invalidates its L1 (agent
//               acquire), adds the other parts' windows to its own accumulators (sc1 loads) and writes the tile. No window
//               of the output is cleared or added into; nobody waits for anybody (MI355X_MICROARCH.md, "Valid forms").
// f32 accumulation is exact while an item's k range stays below 2^24 bits (the host cuts longer rows into parts).
// Output conventions (triangle / band / rectangle, AND / OR / XOR through row_counts) are tilebits8_kernel's. Extends the
// reference (README.md:165-167: per-pair counts for LD); the loop it stands for is storm.c:1199-1238 with the leaf's
// result kept per pair.
//
// Lag form (kLag, DESIGN.md §4 "lag layout"; the window's form is OutForm::Lag): the triangle's pairs with j - i <= L =
// w.lag only, written as out[(i - i_lo) * ld + (j - i - 1)]: an n x L matrix instead of n x n. The host lists only
// the tiles that hold such a pair; a wave whose 64 x 64 block holds none takes the "nothing to multiply" dispatch, and the
// epilogue is the per-element one (a row's columns shift by one word per row: no 16-byte row runs to store).
constexpr int kThThreads = 256;
// (kThTile = 128 rows per tile side, the item record PartItem and kThNarrow: storm_hip_plan.h)
constexpr uint32_t kThSlotBytes = 2u * kThTile * 64u;   // 16 KiB: A rows 0 .. 127, then B rows 0 .. 127, 64 B of bits each
constexpr uint32_t kThRing = 4u;
constexpr uint32_t kThWindowWords = kThTile * kThTile;   // a part's window: 64 KiB of uint32

// Dosage form (kBits = 2, DESIGN.md §4 "K2h, dosage form"): a row holds VALUES 0 .. 3 in 2 bits each instead of bits, and
// the kernel writes the dot products sum_k v_i[k] v_j[k]. A nibble then holds two values, and the low two bits of a nibble
// read as E2M1 are 0, 0.5, 1.0, 1.5: linear in the value. So there are two classes per piece instead of four — class 0:
// w & 0x33333333, class 1: (w >> 2) & 0x33333333 — and block scale 128 (x 2) on both operands of both makes the operand
// the value itself; 16 multiply steps per trip instead of 32. A chunk (256 values) adds up to 9 x 256 = 2304 to an
// accumulator: the host plans the k-parts and the narrow windows by that weight (plan_tile128, chunk_weight). Every output
// form (kLag too: the lag dispatch and the per-element epilogue do not ask what a word holds), row_counts null.
template <int C>
__device__ __forceinline__ v4i th_inflate2(v4i w) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    if constexpr (C == 1) return (v4i)(((v4u)w >> 2u) & 0x33333333u);
    else return w & (int)0x33333333u;
}

template <bool kLag, int kBits = 1>
__global__ __launch_bounds__(kThThreads, 2) void tile128_kernel(
    TileOperands ops, const PartItem* __restrict__ items, OutWindow window, uint32_t* __restrict__ parts, uint32_t* __restrict__ tickets) {
    const OutWindow w = window.loaded();
    __shared__ __attribute__((aligned(1024))) uint8_t lds[kThRing * kThSlotBytes];
    __shared__ uint32_t ticket_seen;
    static_assert(kBits == 1 || kBits == 2, "bits, or 2-bit values");
    constexpr int kClasses = kBits == 1 ? 4 : 2;   // multiply steps per piece
    STORM_CLOCK_BEGIN();

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wa = wave & 1u, wb = wave >> 1;
    const PartItem it = items[blockIdx.x];
    const uint32_t a_row0 = (uint32_t)it.I * kThTile, b_row0 = (uint32_t)it.J * kThTile;
    const uint32_t nC = it.n_stages / 4u;                      // chunks of 64 B (512 bits of k)
    const uint32_t kbyte0 = it.stage0 * 16u;
    const uint32_t pitch = (uint32_t)ops.pitch;

    const uint8_t *a_base, *b_base;
    uint32_t a_bytes, b_bytes;
    ops.tile_rows(a_row0, kThTile, a_base, a_bytes);
    ops.tile_rows(b_row0, kThTile, b_base, b_bytes);

    // DMA: piece g of an operand = rows 16 g .. 16 g + 15; wave w moves pieces w and w + 4 of A and of B. Lane l: row l / 4
    // of the piece, quarter (l % 4) ^ swizzle of that row ((row / 4) % 4 = (l / 16) % 4 whatever the piece).
    const uint32_t dma_voff = (lane >> 2) * pitch + (((lane & 3u) ^ ((lane >> 4) & 3u)) * 16u);
    auto issue_chunk = [&](uint32_t c, uint32_t slot) __attribute__((always_inline)) {
        const uint32_t koff = kbyte0 + c * 64u;
        const bool live = c < nC;
        // (readfirstlane: hipcc turns the clamped difference into a VALU saturating subtract and then wraps every load
        //  in a waterfall loop over a descriptor it no longer knows to be uniform)
        const uint32_t ab = __builtin_amdgcn_readfirstlane((live && a_bytes > koff) ? a_bytes - koff : 0u);
        const uint32_t bb = __builtin_amdgcn_readfirstlane((live && b_bytes > koff) ? b_bytes - koff : 0u);
        const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a_base + koff), 0, ab, 0x00020000);
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(b_base + koff), 0, bb, 0x00020000);
        uint8_t* dst = lds + slot * kThSlotBytes + wave * 1024u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)dst, 16, (int)dma_voff, (int)(16u * wave * pitch), 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(dst + 4096u), 16, (int)dma_voff, (int)(16u * (wave + 4u) * pitch), 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lptr_t)(dst + 8192u), 16, (int)dma_voff, (int)(16u * wave * pitch), 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lptr_t)(dst + 12288u), 16, (int)dma_voff, (int)(16u * (wave + 4u) * pitch), 0, 0);
    };

    // fragment of block x (0, 1: the wave's A blocks, 2, 3: its B blocks), k-step j, ring slot s:
    //   row 32 (x & 1) + (l & 31) of the wave's 64, 16-byte slot (2 j + (l >> 5)) ^ ((row / 4) % 4)
    const uint32_t frow = lane & 31u;
    const uint32_t fq = (lane >> 5) ^ ((frow >> 2) & 3u);
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)&lds[0];
    const uint32_t fa0 = lds_base + (64u * wa + frow) * 64u + fq * 16u, fa1 = fa0 ^ 32u;
    const uint32_t fb0 = lds_base + kThTile * 64u + (64u * wb + frow) * 64u + fq * 16u, fb1 = fb0 ^ 32u;

    // block offset of the wave's B rows from its A rows: block (m, n) holds a pair i < j iff n + d >= m
    int32_t d = w.rect() ? 64 : (int32_t)((b_row0 + 64u * wb) / 32u) - (int32_t)((a_row0 + 64u * wa) / 32u);
    if constexpr (kLag)   // the block's nearest pair (i0 + 63, j0) is already beyond the lag: every part of the tile agrees
        if (b_row0 + 64u * wb > a_row0 + 64u * wa + 63u + w.lag) d = -1;

    auto run = [&](auto dc) __attribute__((always_inline)) {
        constexpr int D = decltype(dc)::value;          // 64: every block; 0: the block below the diagonal drops out; -1: nothing
        constexpr bool kWork = D >= 0;
        auto needed = [](int m, int n) constexpr { return D >= 0 && n + D >= m; };
        v16f acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = v16f{};
        v4i raw[2][4];   // [piece parity][block]: the bits of a piece's fragments
        v4i fr[2][4];    // [step parity][block]: the inflated operands of a multiply step
        // (asm reads: a C++ LDS load makes hipcc wait for EVERY LDS-DMA in flight first — vmcnt(0) behind the pieces it has
        //  just issued; the waits for the fragments are the lgkmcnt(0) in front of the step that inflates them)
        auto read_piece = [&](auto pc) __attribute__((always_inline)) {
            // piece P of a trip (chunk P / 2 of the trip = ring slot (P / 2) % 4, k-step P % 2) into raw[P % 2]
            constexpr int P = decltype(pc)::value;
            constexpr int off = ((P >> 1) & 3) * (int)kThSlotBytes;
            tb_fetch<off>(raw[P & 1][0], (P & 1) ? fa1 : fa0);
            tb_fetch<off + 2048>(raw[P & 1][1], (P & 1) ? fa1 : fa0);
            tb_fetch<off>(raw[P & 1][2], (P & 1) ? fb1 : fb0);
            tb_fetch<off + 2048>(raw[P & 1][3], (P & 1) ? fb1 : fb0);
        };

        // ---- prologue: chunks 0, 1, 2 on their way; chunk 0 landed for everybody; piece 0 read, its class 0 inflated
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // scalar loads of the item record
        issue_chunk(0u, 0u);
        issue_chunk(1u, 1u);
        issue_chunk(2u, 2u);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (kWork) {
            read_piece(std::integral_constant<int, 0>{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            tb_static_for<4>([&](auto gc) __attribute__((always_inline)) {
                constexpr int g = decltype(gc)::value;
                if constexpr (kBits == 1) fr[0][g] = tb_inflate<0>(raw[0][g]);
                else fr[0][g] = th_inflate2<0>(raw[0][g]);
            });
        }

        // ---- four chunks per trip: 8 pieces x 4 classes = 32 multiply steps of 4 MFMAs (2-bit values: x 2 classes = 16)
        const uint32_t n_trips = (nC + 3u) / 4u;
        for (uint32_t trip = 0; trip < n_trips; ++trip) {
            tb_static_for<8 * kClasses>([&](auto sc) __attribute__((always_inline)) {
                constexpr int s = decltype(sc)::value;
                constexpr int c = s % kClasses, P = s / kClasses, cur = s & 1;
                if constexpr (c == 0 && (P & 1) == 0) {
                    // top of chunk q = P / 2: the NEXT chunk has landed for everybody (this wave's share: all but its 4
                    // youngest pieces), and everybody has read the last of the chunk before — its slot takes the chunk
                    // three ahead
                    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    issue_chunk(4u * trip + (uint32_t)(P >> 1) + 3u, (uint32_t)(((P >> 1) + 3) & 3));
                }
                if constexpr (kWork) {
                    // the piece after this one: its registers held the piece before (every class inflated two steps ago)
                    if constexpr (c == 0) read_piece(std::integral_constant<int, (P + 1) & 7>{});
                    if constexpr (c == kClasses - 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the next piece's fragments
                    __builtin_amdgcn_sched_barrier(0);
                    // what the NEXT step multiplies: class c + 1 of this piece, or class 0 of the next piece
                    constexpr int cn = (c + 1) % kClasses;
                    constexpr int pn = c == kClasses - 1 ? ((P + 1) & 1) : (P & 1);
                    const int scale = kBits == 1 ? tb_scale<c>() : 128;
                    tb_static_for<4>([&](auto qc) __attribute__((always_inline)) {
                        constexpr int q = decltype(qc)::value;
                        constexpr int m = q >> 1, n = q & 1;
                        if constexpr (needed(m, n))
                            acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                                v8i{fr[cur][m].x, fr[cur][m].y, fr[cur][m].z, fr[cur][m].w, 0, 0, 0, 0},
                                v8i{fr[cur][2 + n].x, fr[cur][2 + n].y, fr[cur][2 + n].z, fr[cur][2 + n].w, 0, 0, 0, 0},
                                acc[m][n], 4, 4, 0, scale, 0, scale);
                        if constexpr (kBits == 1) fr[cur ^ 1][q] = tb_inflate<cn>(raw[pn][q]);
                        else fr[cur ^ 1][q] = th_inflate2<cn>(raw[pn][q]);
                        __builtin_amdgcn_sched_barrier(0);
                    });
                }
            });
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the empty pieces of the tail
        STORM_CLOCK_END();

        // ---- epilogue. C/D map of a 32 x 32 block: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
        uint32_t cnt[2][2][16];
        if constexpr (kWork) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) cnt[m][n][r] = (uint32_t)acc[m][n][r];
        }
        if (it.n_parts > 1u) {
            // this part's accumulators as they lie: window [part][wave][block][register quad][lane] x 16 B of 32-bit counts
            // (16 KiB per wave), or — every part of the tile below 2^16 bits of k — of 16-bit counts, two registers to a
            // dword (8 KiB per wave): the part that ends the tile reads what all the others wrote, from beyond its L2
            typedef unsigned v4u_th __attribute__((ext_vector_type(4)));
            const uint32_t my_part = (uint32_t)(it.part & (uint16_t)~kThNarrow);
            const bool narrow = (it.part & kThNarrow) != 0;
            auto window_of = [&](uint32_t p, bool valid = true) {
                return __builtin_amdgcn_make_buffer_rsrc(parts + (uint64_t)(it.win0 + p) * kThWindowWords + wave * (kThWindowWords / 4u), 0,
                                                         valid ? 16384u : 0u, 0x00020000);
            };
            if constexpr (kWork) {
                const __amdgpu_buffer_rsrc_t rw = window_of(my_part);
                // (all of a window's registers are packed BEFORE the first store: packed one quad at a time, hipcc reuses the
                //  quad's registers for the next one and the v_lshl_or_b32 right behind a buffer_store_dwordx4 with an SGPR
                //  offset overwrote the first data register of some lane quads before the store had read it — gfx950, ROCm
                //  7.2: dword 0 of every 16 bytes of four lanes in sixteen came out as the NEXT quad's. The hazard
                //  recognizer knows the case only for stores without an SGPR offset.)
                if (narrow) {
                    v4u_th pk[8];
                    tb_static_for<8>([&](auto gc) __attribute__((always_inline)) {
                        constexpr int g = decltype(gc)::value, b = g >> 1, h = g & 1;
                        if constexpr (needed(b >> 1, b & 1)) {
                            const uint32_t* c = &cnt[b >> 1][b & 1][8 * h];
                            pk[g] = v4u_th{c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16)};
                        }
                    });
                    __builtin_amdgcn_sched_barrier(0);
                    tb_static_for<8>([&](auto gc) __attribute__((always_inline)) {
                        constexpr int g = decltype(gc)::value, b = g >> 1;
                        if constexpr (needed(b >> 1, b & 1))
                            __builtin_amdgcn_raw_buffer_store_b128(pk[g], rw, (int)(lane * 16u), g * 1024, 16 /* sc1: write through */);
                    });
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    tb_static_for<16>([&](auto gc) __attribute__((always_inline)) {
                        constexpr int g = decltype(gc)::value, b = g >> 2, r4 = g & 3;
                        if constexpr (needed(b >> 1, b & 1)) {
                            const uint32_t* c = &cnt[b >> 1][b & 1][4 * r4];
                            const v4u_th v = {c[0], c[1], c[2], c[3]};
                            __builtin_amdgcn_raw_buffer_store_b128(v, rw, (int)(lane * 16u), g * 1024, 16 /* sc1: write through */);
                        }
                    });
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its stores ...
            __syncthreads();                                     // ... before the one lane takes the ticket
            if (tid == 0u)
                ticket_seen = __hip_atomic_fetch_add(&tickets[it.tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if (ticket_seen != (uint32_t)it.n_parts - 1u) return;   // another part writes the tile
            if (tid == 0u) {
                __hip_atomic_store(&tickets[it.tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __syncthreads();
            if constexpr (kWork) {
                // the other parts' windows, two in flight (a single CU pulls ~35 GB/s from beyond its L2 with one window in
                // flight per wave, ~65 with two: MI355X_MICROARCH.md, handoff-payload)
                const uint32_t others = (uint32_t)it.n_parts - 1u;
                auto other = [&](uint32_t q) { return q < my_part ? q : q + 1u; };
                // unit = 8 loads of 1 KiB per wave: a narrow window is one unit, a wide one two (register quads 0 .. 7, 8 .. 15)
                auto reduce = [&](auto narrowc) __attribute__((always_inline)) {
                    constexpr bool kNarrow = decltype(narrowc)::value != 0;
                    constexpr uint32_t kUnits = kNarrow ? 1u : 2u;
                    v4u_th w0[8], w1[8];
                    // (every fetch is issued, one beyond the last unit through an empty descriptor: with fetches under
                    //  conditions hipcc carries the buffers through copies behind vmcnt(0) and nothing overlaps)
                    auto fetch = [&](v4u_th (&w)[8], uint32_t u) __attribute__((always_inline)) {
                        const bool valid = u < others * kUnits;
                        const __amdgpu_buffer_rsrc_t rq = window_of(valid ? other(u / kUnits) : 0u, valid);
                        const int half = (int)(u % kUnits) * 8192;
                        tb_static_for<8>([&](auto gc) __attribute__((always_inline)) {
                            constexpr int g = decltype(gc)::value;
                            w[g] = __builtin_amdgcn_raw_buffer_load_b128(rq, (int)(lane * 16u), half + g * 1024, 16 /* sc1 */);
                        });
                    };
                    auto add = [&](const v4u_th (&w)[8], uint32_t u) __attribute__((always_inline)) {
                        if constexpr (kNarrow) {
                            tb_static_for<8>([&](auto gc) __attribute__((always_inline)) {
                                constexpr int g = decltype(gc)::value, b = g >> 1, h = g & 1;
                                if constexpr (needed(b >> 1, b & 1)) {
                                    uint32_t* c = &cnt[b >> 1][b & 1][8 * h];
#pragma unroll
                                    for (int k = 0; k < 4; ++k) {
                                        c[2 * k] += w[g][k] & 0xffffu;
                                        c[2 * k + 1] += w[g][k] >> 16;
                                    }
                                }
                            });
                        } else {
                            auto add_half = [&](auto hc) __attribute__((always_inline)) {
                                constexpr int H = decltype(hc)::value;
                                tb_static_for<8>([&](auto gc) __attribute__((always_inline)) {
                                    constexpr int g = 8 * H + decltype(gc)::value, b = g >> 2, r4 = g & 3;
                                    if constexpr (needed(b >> 1, b & 1)) {
                                        uint32_t* c = &cnt[b >> 1][b & 1][4 * r4];
#pragma unroll
                                        for (int k = 0; k < 4; ++k) c[k] += w[g & 7][k];
                                    }
                                });
                            };
                            if (u & 1u) add_half(std::integral_constant<int, 1>{});
                            else add_half(std::integral_constant<int, 0>{});
                        }
                    };
                    const uint32_t units = others * kUnits;
                    fetch(w0, 0u);
                    for (uint32_t u = 0; u < units; u += 2u) {
                        fetch(w1, u + 1u);
                        add(w0, u);
                        fetch(w0, u + 2u);
                        add(w1, u + 1u);
                    }
                };
                if (narrow) reduce(std::integral_constant<int, 1>{});
                else reduce(std::integral_constant<int, 0>{});
            }
        }
        __syncthreads();   // every wave has left the ring: the waves below turn their counts through it
        if constexpr (kWork) {
            const uint32_t i0 = a_row0 + 64u * wa, j0 = b_row0 + 64u * wb;
            const uint32_t col = lane & 31u;
            // a wave whose 64 x 64 lies wholly inside the output and above the diagonal: the accumulators hold 16 ROWS of one
            // column per lane, so storing them directly is one 4-byte store per element with a 64-bit address and a predicate
            // each (5 us of a 29 us item at 1024 rows). 32 rows at a time go through 8.5 KiB of the idle ring (row pitch 68
            // words: conflict-free 4-byte stores) and leave as 16 bytes per lane, four 256-byte runs per instruction.
            if constexpr (D > 0 && !kLag) {
                if (w.covers(i0, 64u, j0, 64u) && (w.ld & 3u) == 0 && ((uintptr_t)w.out & 15u) == 0 && (w.j_base & 3u) == 0) {
                    uint32_t* w32 = reinterpret_cast<uint32_t*>(lds + wave * (32u * 68u * 4u));
                    uint32_t* out_tile = w.at(i0, j0);
                    const OutWindow::counts_ptr_t row_counts = w.counts();
                    const uint64_t ld = w.ld;
                    uint32_t nj[2] = {0u, 0u};
                    if (row_counts) {
                        nj[0] = row_counts[j0 + col];
                        nj[1] = row_counts[j0 + 32u + col];
                    }
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const uint32_t il = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
                            const uint32_t ni = row_counts ? row_counts[i0 + 32u * (uint32_t)m + il] : 0u;
#pragma unroll
                            for (int n = 0; n < 2; ++n)
                                w32[il * 68u + 32u * (uint32_t)n + col] =
                                    row_counts ? ni + nj[n] - w.and_weight * cnt[m][n][r] : cnt[m][n][r];
                        }
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const uint32_t row = (uint32_t)q * 4u + (lane >> 4);
                            const uint4 v = *reinterpret_cast<const uint4*>(&w32[row * 68u + 4u * (lane & 15u)]);
                            *reinterpret_cast<uint4*>(&out_tile[(uint64_t)(32u * (uint32_t)m + row) * ld + 4u * (lane & 15u)]) = v;
                        }
                    }
                    return;
                }
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const uint32_t jj = j0 + 32u * (uint32_t)n + col;
                const bool j_ok = w.wants_col(jj);
                const uint32_t nj = w.nj(jj);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    if (!needed(m, n)) continue;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const uint32_t ii = i0 + 32u * (uint32_t)m + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
                        // (lag form: a register's 32 lanes of one half-wave are one row, 32 consecutive columns = one 128-byte run)
                        if (j_ok && w.writes_row<kLag>(ii, jj)) *w.at<kLag>(ii, jj) = w.value(cnt[m][n][r], ii, nj);
                    }
                }
            }
        }
    };

    if (d >= 1) run(std::integral_constant<int, 64>{});
    else if (d == 0) run(std::integral_constant<int, 0>{});
    else run(std::integral_constant<int, -1>{});
}
