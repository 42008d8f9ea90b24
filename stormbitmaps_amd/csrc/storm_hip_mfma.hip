// storm_hip_mfma.hip — K2: the all-pairs AND+popcount total through the gfx950 matrix cores.
//
// Why: the popcount path (K1, storm_hip.hip) is bound by VALU issue — v_bcnt_u32_b32 is a
// half-rate instruction, so a 64-bit word pair costs 2x2 + 2x4 = 12 SIMD cycles per 64 lanes
// (measured ceiling 1.24e13 word pairs/s, profiles/r01_b_*). popcount(a & b) is the dot
// product of the two bit vectors, and 0/1 are exact in FP4 (E2M1: 0b0010 = 1.0), so
// v_mfma_f32_32x32x64_f8f6f4 with FP4 operands does 32x32 row pairs x 64 bits per 32 cycles
// per SIMD: measured 6.4e13 word pairs/s peak (tools/mfma_fp4_probe), 5x the VALU ceiling.
// The f32 accumulators hold exact integers below 2^24, guaranteed by k-slicing.
//
// Pipeline per all-pairs call
//   1. expand_fp4_kernel: bit-packed rows -> nibble rows (4 bits per bit), once per call:
//      an O(N*M) pass, HBM-bound, 8-9 % of a pass at the headline shape ("keep_shadow" keeps
//      the result while the matrix is unchanged).
//   2. strip_fp4_kernel (K2s, the default): A-stationary strips, see below.
//      pairw_fp4_kernel (K2 tiles: variant 3 and every materialised-output entry point):
//      work item = (256x256 row-block tile with I <= J, k-slice).
//      512 threads = 8 waves as 2 (M) x 4 (N); each wave owns 128x64 of the tile = 4x2
//      MFMA blocks (128 accumulator registers). Per stage (128 bits of k = 64 B per row) the
//      A and B row blocks go global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds, ring of 4
//      stages, one barrier per stage), XOR-swizzled through the SOURCE address so that the
//      ds_read_b128 operand fetches are bank-conflict free; 2 k-steps x 8 MFMAs per stage.
//      Sum mode: off-diagonal tiles add every entry; diagonal tiles add (all - trace) / 2,
//      the strict upper triangle because the tile is symmetric — no global correction term,
//      so any subset of items (a multi-GPU shard) yields an exact partial. Write mode: the
//      accumulators go to the output matrix (AND / OR / XOR counts, triangle, band, rectangle).
//   3. tile items are ordered k-slice-major and dealt to the 8 XCDs in groups of 32
//      neighbouring tiles (4 x 8 row blocks), so the 32 CUs of one XCD share 12 row-block
//      slices in L2.
#include "storm_hip_internal.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <type_traits>
#include <utility>

namespace storm {

// In-kernel clock witness (tools build only — in the shipped library no stamp executes): a workgroup reads the shader
// clock counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) when it starts and when it ends and adds both
// differences to a device array that nothing else reads; sum(dt) / sum(dr) x 100 MHz is the clock the kernel's
// workgroups ran at, weighted by their lifetimes (MI355X_MICROARCH.md, "DVFS give-back" (6)). Read and cleared by
// storm_hip_probe_clock (tools/clock_power.py).
#ifdef STORM_HIP_PROBES
__device__ unsigned long long g_clock_probe[4];
#define STORM_CLOCK_BEGIN()                                  \
    const uint64_t ck_t0 = __builtin_amdgcn_s_memtime();     \
    const uint64_t ck_r0 = __builtin_amdgcn_s_memrealtime()
#define STORM_CLOCK_END()                                                                           \
    do {                                                                                            \
        if (threadIdx.x == 0) {                                                                     \
            atomicAdd(&g_clock_probe[0], (unsigned long long)(__builtin_amdgcn_s_memtime() - ck_t0)); \
            atomicAdd(&g_clock_probe[1], (unsigned long long)(__builtin_amdgcn_s_memrealtime() - ck_r0)); \
            atomicAdd(&g_clock_probe[2], 1ull);                                                     \
        }                                                                                           \
    } while (0)
#else
#define STORM_CLOCK_BEGIN() do {} while (0)
#define STORM_CLOCK_END() do {} while (0)
#endif

// The end of a synchronous call whose kernels have just been queued: hipStreamSynchronize parks the thread and is woken
// by an interrupt (5 - 8 us of a call that runs 20 - 40); a few hundred hipStreamQuery polls see the end of a short
// launch sooner. Option sync_poll_us: how long to poll before parking (0: park at once).
hipError_t wait_stream(storm_hip_ctx_t* ctx) {
    if (ctx->sync_poll_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0;; ++spin) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q != hipErrorNotReady) return q;
            if ((spin & 15u) == 15u &&
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > ctx->sync_poll_us)
                break;
        }
    }
    return hipStreamSynchronize(ctx->stream);
}

// (kTile = 256 rows per tile side, kStageBytes = 64, kGroupStages and the item record MfmaItem: storm_hip_plan.h)
constexpr int kMfmaThreads = 512;
constexpr int kTileStageBytes = kTile * kStageBytes;  // 16 KiB per operand per stage
constexpr int kRing = 4;             // LDS stages (4 x 32 KiB = 128 KiB of the CU's 160 KiB)

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

using gptr_t = const __attribute__((address_space(1))) void*;
using lptr_t = __attribute__((address_space(3))) void*;

#include "tile_window.inc"   // TileOperands, OutWindow

// 8 bits -> 8 nibbles holding `nib` (0b0010 = 1.0 in E2M1; other codes only for the power probe)
__device__ __forceinline__ uint32_t spread8_fp4(uint32_t b, uint32_t nib = 2u) {
    uint32_t x = (b | (b << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return x * nib;
}

// Which columns a shard (multi-GPU rank) expands: the ownership unit is a run of 2^unit_shift
// 32-bit half words of a row (5: four strip k-slices = one 128-byte line of the bit matrix, so that a
// shard reads whole lines; 7: one k-group = 64 words, the tile kernel's k-slice), numbered from
// h_begin. Units below modulo_units (a multiple of count) belong to shard unit % count; the units from
// there on (the strips' leftover slices, whose ITEMS are dealt to the shards) are expanded by every
// shard.
struct ExpandOwn {
    uint32_t rank, count, unit_shift, modulo_units;
};
constexpr ExpandOwn kExpandAll = {0u, 1u, 7u, 0u};

// One thread per 32-bit half word: 16 output bytes, fully coalesced on both sides.
// Rows >= n_rows_src (padding up to a multiple of 256) are written as zeros. The half words
// [h_begin, h_end) of every row are expanded (default: the whole row) and land at shadow column
// h - h_dst0, so that a k-chunk of a matrix whose full shadow would not fit gets a compact shadow of
// its own; half words beyond the end of the row read as zero (the last chunk may overhang).
// A shard walks a COMPACT index over the units it owns, so that its expansion costs 1 / count of the
// whole (round 2's first version tested ownership per element: 37 us for a 1/8 shard of the headline
// matrix where 69 / 8 were due).
__global__ __launch_bounds__(256) void expand_fp4_kernel(const uint64_t* __restrict__ X,
                                                         uint64_t stride_words,
                                                         uint64_t n_rows_src, uint64_t n_rows_dst,
                                                         uint4* __restrict__ X4, ExpandOwn own,
                                                         uint32_t nib = 2u, uint64_t out_pitch_u4 = 0,
                                                         uint64_t h_begin = 0, uint64_t h_end = 0,
                                                         uint64_t h_dst0 = 0) {
    // out_pitch_u4: row pitch of the shadow in 16-byte units (0 = dense, stride_words * 2)
    if (out_pitch_u4 == 0) out_pitch_u4 = stride_words * 2;
    const uint64_t halves_per_row = stride_words * 2;
    if (h_end == 0) h_end = halves_per_row;
    const uint32_t shift = own.unit_shift;
    const uint64_t units = (h_end - h_begin + (1ull << shift) - 1) >> shift;      // in [h_begin, h_end)
    const uint64_t modulo = own.count > 1 ? min((uint64_t)own.modulo_units, units / own.count * own.count) : 0;
    const uint64_t whole = own.count > 1 ? modulo / own.count : 0;                // units owned outright
    const uint64_t compact = (whole + (units - modulo)) << shift;                 // half words this shard expands
    // grid = (column chunks of 256 halves, rows): no division per element (a 64-bit divide per
    // 16 output bytes made the first version VALU-bound just below the HBM rate)
    for (uint64_t row = blockIdx.y; row < n_rows_dst; row += gridDim.y)
        for (uint64_t hc = (uint64_t)blockIdx.x * 256 + threadIdx.x; hc < compact;
             hc += (uint64_t)gridDim.x * 256) {
            const uint64_t uc = hc >> shift;
            const uint64_t unit = uc < whole ? uc * own.count + own.rank : modulo + (uc - whole);
            const uint64_t h = h_begin + (unit << shift) + (hc & ((1ull << shift) - 1));
            if (h >= h_end) continue;  // the last unit may be cut short
            uint32_t w = 0;
            if (row < n_rows_src && h < halves_per_row)
                w = reinterpret_cast<const uint32_t*>(X)[row * halves_per_row + h];
            uint4 o;
            o.x = spread8_fp4(w & 0xFFu, nib & 7u);
            o.y = spread8_fp4((w >> 8) & 0xFFu, nib & 7u);
            o.z = spread8_fp4((w >> 16) & 0xFFu, nib & 7u);
            o.w = spread8_fp4(w >> 24, nib & 7u);
            X4[row * out_pitch_u4 + (h - h_dst0)] = o;  // (non-temporal stores: slower)
        }
}

// Half words a shard expands in a range of `halves` (host mirror of the kernel's arithmetic: grid size).
static inline uint64_t expand_compact_halves(const ExpandOwn& own, uint64_t halves) {
    const uint64_t units = (halves + (1ull << own.unit_shift) - 1) >> own.unit_shift;
    if (own.count <= 1) return units << own.unit_shift;
    const uint64_t modulo = std::min<uint64_t>(own.modulo_units, units / own.count * own.count);
    return (modulo / own.count + (units - modulo)) << own.unit_shift;
}

// Launch geometry of expand_fp4_kernel for n_rows_dst rows of `halves` half words each.
static inline dim3 expand_grid(uint64_t n_rows_dst, uint64_t stride_words, uint64_t halves = 0) {
    if (halves == 0) halves = stride_words * 2;
    const uint64_t chunks = (halves + 255) / 256;
    const uint64_t cx = std::max<uint64_t>(1, std::min<uint64_t>(chunks, 1024));
    // ~8192 workgroups in all, each walking down the rows of its column chunk
    return dim3((uint32_t)cx, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_rows_dst, 8192 / cx)));
}

// LDS image of one operand stage: 256 rows x 64 B, the 16-byte slot s of row r stored at
// slot s ^ ((r >> 2) & 3). A wave's ds_read_b128 of 32 rows x one slot then touches all 16
// slots of the 256-byte bank row once per 16-lane group (conflict free).
__device__ __forceinline__ void stage_tile(uint8_t* lds_tile, const uint8_t* __restrict__ X4,
                                           uint64_t row_bytes, uint32_t row0, uint64_t kbyte,
                                           uint32_t wave, uint32_t lane) {
    // buffer_load ... lds: scalar descriptor of the tile's k position + 32-bit lane offsets
    // (global_load_lds with 64-bit lane addresses costs the wave far more beside MFMA bursts,
    // tools/ubench_feed). 256 rows x row pitch < 2^32 is checked on the host.
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(X4 + (uint64_t)row0 * row_bytes + kbyte), 0, -1, 0x00020000);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t n = (uint32_t)q * 8u + wave;  // wave-instruction index, 1 KiB each
        const uint32_t p = n * 64u + lane;           // 16-byte piece of the LDS image
        const uint32_t r = p >> 2;
        const uint32_t slot = (p & 3u) ^ ((r >> 2) & 3u);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)(lds_tile + n * 1024u), 16,
                                                 (int)(r * (uint32_t)row_bytes + slot * 16u), 0, 0, 0);
    }
}

// kWrite: instead of summing, store every pair count i < j of the tile to out[i * ld + j]
// (materialised XX^T upper triangle); the item then spans the whole k range.
template <uint32_t probe, bool kWrite = false>
__global__ __launch_bounds__(kMfmaThreads, 2) void pairw_fp4_kernel(
    const uint8_t* __restrict__ X4, uint64_t row_bytes, const MfmaItem* __restrict__ items,
    unsigned long long* __restrict__ slots, OutWindow window = OutWindow{}, uint32_t split_from = 0xffffffffu) {
    // kWrite: the counts go to the window (triangle, or the rectangle A x B of a shadow holding [A ; B]).
    // Items from index split_from on cover only a part of k of their tile (several per tile, to
    // fill the last round of workgroups): they ADD into the window, which zero_tiles_kernel cleared.
    __shared__ __attribute__((aligned(1024))) uint8_t lds[kRing][2][kTileStageBytes];  // [stage][A|B]

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wm = wave >> 2, wn = wave & 3u;
    const uint32_t item_idx = blockIdx.x;
    const MfmaItem it = items[item_idx];
    const uint32_t a_row0 = (uint32_t)it.I * kTile, b_row0 = (uint32_t)it.J * kTile;

    // per-lane byte offset of its 16-byte operand piece inside a 32-row block, per k-step
    const uint32_t swz = (lane >> 2) & 3u;
    const uint32_t off0 = (lane & 31u) * kStageBytes + (((0u + (lane >> 5)) ^ swz) * 16u);
    const uint32_t off1 = (lane & 31u) * kStageBytes + (((2u + (lane >> 5)) ^ swz) * 16u);

    v16f acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = v16f{};

    // Ring of kRing LDS stages with the operand fetch software-pipelined ACROSS the barrier:
    //   iteration s:  wait(stage s+1 landed) ; barrier ; issue DMA of stage s+3 ;
    //                 read frags(s, k-step 1) ; 8 MFMAs on frags(s, k-step 0)   [read last iteration]
    //                 read frags(s+1, k-step 0) ; 8 MFMAs on frags(s, k-step 1)
    // so every ds_read_b128 is issued >= 8 MFMAs (256 cycles) before its use, and the wave
    // reaches the next wait/barrier with 8 MFMAs still executing — the barrier and LDS latency
    // hide behind them instead of idling the matrix cores (the first version, with a plain
    // double buffer and reads after the barrier, ran them 51 % busy: profiles/r01_c_k2_*).
    // Ring safety: the DMA of stage s+3 overwrites the buffer of stage s-1, whose last read
    // (k-step 1) every wave completed before it arrived at this iteration's barrier. A stage is
    // first read one iteration AFTER the wait+barrier that retires it. Each wave issues 4
    // LDS-DMA instructions per stage, hence the counted vmcnt(4 x stages allowed in flight);
    // raw s_barrier, because __syncthreads() would drain vmcnt(0).
    const uint32_t S = it.n_stages;
    // `probe` (timing experiments only, results are then wrong): bit 2 = issue no LDS-DMA,
    // bit 3 = issue no MFMA
    auto issue = [&](uint32_t s) {
        if constexpr ((probe & 4u) != 0) return;
        const uint64_t kb = (uint64_t)(it.stage0 + s) * kStageBytes;
        stage_tile(lds[s % kRing][0], X4, row_bytes, a_row0, kb, wave, lane);
        stage_tile(lds[s % kRing][1], X4, row_bytes, b_row0, kb, wave, lane);
    };
    auto fetch = [&](uint32_t s, uint32_t off, v8i (&a)[4], v8i (&b)[2]) {
        const uint8_t* la = lds[s % kRing][0] + wm * (128u * kStageBytes) + off;
        const uint8_t* lb = lds[s % kRing][1] + wn * (64u * kStageBytes) + off;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const v4i t = *reinterpret_cast<const v4i*>(la + m * (32u * kStageBytes));
            a[m] = v8i{t.x, t.y, t.z, t.w, 0, 0, 0, 0};
        }
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const v4i t = *reinterpret_cast<const v4i*>(lb + n * (32u * kStageBytes));
            b[n] = v8i{t.x, t.y, t.z, t.w, 0, 0, 0, 0};
        }
    };
    auto multiply = [&](const v8i (&a)[4], const v8i (&b)[2]) {
        if constexpr ((probe & 8u) != 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) asm volatile("" ::"v"(a[m]));
#pragma unroll
            for (int n = 0; n < 2; ++n) asm volatile("" ::"v"(b[n]));
            return;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                    a[m], b[n], acc[m][n], 4 /*A: FP4*/, 4 /*B: FP4*/, 0, 0, 0, 0);
    };

    for (uint32_t s = 0; s < kRing - 1; ++s)
        if (s < S) issue(s);
    // stage 0 must have landed before its first read: stages 1 and 2 may stay in flight
    if (S >= 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (S == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    v8i a0[4], b0[2], a1[4], b1[2];
    fetch(0, off0, a0, b0);
    for (uint32_t s = 0; s < S; ++s) {
        // retire stage s+1 (stage s+2, if any, may stay in flight)
        if (s + 2 < S) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (s + kRing - 1 < S) issue(s + kRing - 1);
        fetch(s, off1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of the MFMAs (see strip kernel)
        multiply(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < S) fetch(s + 1, off0, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        multiply(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue ----
    // C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if constexpr (kWrite) {
        const OutWindow w = window.loaded();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const uint32_t j = b_row0 + wn * 64u + n * 32u + (lane & 31u);
                // union / symmetric difference: n_i + n_j - and_weight * |i & j|
                // (row_counts is indexed by shadow row)
                const bool j_ok = w.wants_col(j);
                const uint32_t nj = w.nj(j);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = a_row0 + wm * 128u + m * 32u + (r & 3) + 8 * (r >> 2) +
                                       4 * (lane >> 5);
                    if (j_ok && w.writes_row(i, j)) {
                        const uint32_t c = (uint32_t)acc[m][n][r];
                        uint32_t* dst = w.at(i, j);
                        if (item_idx < split_from) {
                            *dst = w.value(c, i, nj);
                        } else {  // partial over k: the n_i + n_j term once, mod 2^32 throughout
                            atomicAdd(dst, w.part_value(c, i, nj, it.stage0 == 0));
                        }
                    }
                }
            }
        return;
    }
    // exact integer sum of this wave's 128x64 block
    const bool diag_tile = it.I == it.J;
    uint32_t all = 0, trace = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const bool diag_block = diag_tile && (wm * 4u + m == wn * 2u + n);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t v = (uint32_t)acc[m][n][r];
                all += v;
                const uint32_t row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (diag_block && row == (lane & 31u)) trace += v;
            }
        }
    uint64_t mine = all;
    if (diag_tile) {
        // symmetric tile: strict upper triangle = (all - trace) / 2, exact on the WAVE sums only
        // after adding the mirrored block — so reduce `all` and `trace` over the workgroup first
        // (the reduction words live in the staging array: a second __shared__ object next to
        //  an LDS-DMA target makes hipcc drain vmcnt(0) before every ds_read of the main loop)
        unsigned long long* red = reinterpret_cast<unsigned long long*>(&lds[0][0][0]);
        __syncthreads();
        if (tid < 2) red[tid] = 0;
        __syncthreads();
        uint64_t wa = all, wt = trace;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            wa += __shfl_down(wa, o, 64);
            wt += __shfl_down(wt, o, 64);
        }
        if (lane == 0) {
            atomicAdd(&red[0], (unsigned long long)wa);
            atomicAdd(&red[1], (unsigned long long)wt);
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned long long upper = (red[0] - red[1]) / 2;
            if (upper) atomicAdd(&slots[blockIdx.x & (kSlots - 1)], upper);
        }
        return;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (lane == 0 && mine != 0)
        atomicAdd(&slots[(blockIdx.x * 8u + wave) & (kSlots - 1)], (unsigned long long)mine);
}

// ------------------------------------------------------------------------------------------
// K2s "strip" kernel: the off-diagonal part of the triangle, A-stationary.
//
// Ablating the tile kernel above (k2_debug probes, profiles/r01_d_*) showed that its limit is
// operand delivery, not the matrix cores (its two waves per SIMD run in lockstep behind one
// barrier, and 32 KiB of DMA + 96 KiB of ds_read per stage left the MFMA pipe 55 % busy). Only
// the grand total is wanted, so the accumulators never have to be flushed per B block — which
// allows K1's dataflow on the matrix cores:
//   work item = (A row block I of 256 rows, k-slice of 256 bits, the A tile's own 4 blocks
//               and/or a run of later 64-row B blocks).
//   A operand : this wave's 64 rows x 256 bits live in 32 VGPRs for the whole item
//               (8 fragment loads straight from global memory, once per item).
//   B operand : one stage = 64 B rows x the k-slice = 64 rows x 128 B, FULL 128-byte lines,
//               2 LDS-DMA instructions per wave (buffer_load_dwordx4 ... lds); ring of 4
//               stages (3 in flight) = 32 KiB.
//   per stage : 4 k-steps x (2 ds_read_b128 + 4 MFMA) per wave into 4 accumulator blocks that
//               are never flushed (f32 exact: <= 256 bits x 4096 stages < 2^24).
//   occupancy : 4 waves (one per SIMD, 64 A rows each), 126 VGPRs -> FOUR workgroups per CU,
//               i.e. 4 waves per SIMD from four independent barrier domains: while one wave
//               sits at its barrier or in an item's prologue, the others feed the matrix pipe.
// Per MFMA this moves half the DMA bytes of the tile kernel. Items of one k-slice are dealt to
// one XCD (longest first within the slice), whose L2 then holds that slice of all rows
// (N x 128 B = 1.3 MB at N = 10000); the shadow's row pitch is padded off powers of two, so the
// strips miss L2 for only ~2.6x the shadow's size per launch.
// ------------------------------------------------------------------------------------------
// (kStripRowBytes = 128, kStripBRows = 64, kStripWaves = 4, kStripATile = 256, kStripRingDefault = 4: storm_hip_plan.h)
constexpr int kStripStageBytes = kStripBRows * kStripRowBytes;  // 8 KiB
constexpr int kStripThreads = 64 * kStripWaves;
[[maybe_unused]] constexpr int kStripPieces = 8 / kStripWaves;            // LDS-DMA instructions per wave and stage
static_assert(kStripWaves == 4 || kStripWaves == 8, "a B stage is 8 DMA pieces");

// (the item record StripItem: storm_hip_plan.h)

// kProbe: timing probes with WRONG results: bit 0 no barriers, bit 1 no LDS-DMA, bit 2 no ds_read
// kMB: 32-row MFMA blocks of A per wave. 2 = 64 rows per wave, 256-row A tile, 4 workgroups per
// CU; 4 = 128 rows per wave, 512-row A tile, 2 workgroups per CU ("wide": every B byte that
// crosses the LDS feeds twice the MFMAs).
// kPersist: the grid is one workgroup per resident slot (CUs x workgroups per CU) and every
// workgroup pulls items until its XCD's queue — then the other XCDs' — is empty. The hardware
// dispatcher hands workgroup b to XCD b % 8 strictly in order, so with one item per workgroup
// a full XCD blocks the refill of all the others: the schedule trace (tools/strip_trace.py)
// showed ~700 of the 1024 slots occupied in steady state. Queues in memory do not block.
struct StripQueues {
    uint32_t base[8];   // first item of XCD x's list in the item table
    uint32_t count[8];  // its length
};
[[maybe_unused]] constexpr uint32_t kNoItem = 0xffffffffu;

#ifdef STORM_HIP_PROBES  // 32x32x64 strips (plain, wide, persistent) and their timing probes: tools build (make probes)
#include "../../tools/probes/strip_fp4_32.hip"
#endif  // STORM_HIP_PROBES

// ------------------------------------------------------------------------------------------
// K2s16: the same strips on v_mfma_scale_f32_16x16x128_f8f6f4.
//
// Same work items, same B stages and LDS image, same ring protocol as strip_fp4_kernel; only the
// matrix instruction differs. The chip is power-limited in this loop (tools/ubench_shape,
// profiles/r02_ubench_shape.txt): with the strip kernel's stage traffic beside the MFMAs the
// 32x32x64 form holds 2.04 GHz and the 16x16x128 form 2.21 GHz at nearly the same cycles per
// bit-MAC, 8.0 against 8.26 PFLOP/s in the bare loop (MI355X_MICROARCH.md "DVFS give-back" (7)
// reports the same for bf16).
//   wave tile : 64 A rows = 4 blocks of 16, k-slice of 256 bits = 2 k-steps of 128 bits;
//               A = 8 fragments of 4 VGPRs (as before), accumulators 4 x 4 blocks of 4 VGPRs.
//   operands  : lane l holds row l & 15 and the 16-byte quarter l >> 4 of a 64-byte k-step
//               (tools/mfma_fp4_probe checks both lane maps); C/D: col = l & 15,
//               row = 4 * (l >> 4) + reg.
//   B reads   : one ds_read_b128 per (k-step, 16-row B block) = 8 per stage, each feeding 4 MFMAs
//               (64 cycles); issued THREE steps ahead into a rotation of 4 fragment registers,
//               retired by lgkmcnt(3). The stage image's XOR swizzle (slot ^ (row / 2) % 8) is
//               conflict free for this fragment shape too: a 16-lane group of ds_read_b128 holds
//               rows {0-3, 12-15} at quarter q and rows {4-11} at quarter q + 1 (or the mirror
//               image), which lands on 16 different 16-byte bank groups.
// ------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));

template <int kStripRing>
__global__ __launch_bounds__(kStripThreads, 4) void strip16_fp4_kernel(
    const uint8_t* __restrict__ X4, uint64_t row_bytes, const StripItem* __restrict__ items,
    unsigned long long* __restrict__ slots) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds_raw[kStripRing * kStripStageBytes];
    auto lds = reinterpret_cast<uint8_t(*)[kStripStageBytes]>(lds_raw);

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wm = wave;
    const uint32_t item_idx = blockIdx.x;
    const StripItem it = items[item_idx];
    const uint64_t kbyte = (uint64_t)it.ks * kStripRowBytes;
    const uint32_t D = it.diag ? (uint32_t)(kStripATile / kStripBRows) : 0u;
    const uint32_t T = D + (it.j1 - it.j0);

    // B stage DMA: identical to strip_fp4_kernel (see there)
    const uint32_t r0 = (wave * 64u + lane) >> 3;
    const uint32_t goff0 = r0 * (uint32_t)row_bytes + (((lane & 7u) ^ ((r0 >> 1) & 7u)) * 16u);
    auto issue = [&](uint32_t t) {
        const uint32_t blk = t < D ? it.a_row0 / (uint32_t)kStripBRows + t : it.j1 - 1u - (t - D);
        const uint8_t* base = X4 + (uint64_t)(blk * (uint32_t)kStripBRows) * row_bytes + kbyte;
        uint8_t* dst = lds[t % kStripRing] + wave * 1024u;
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, -1, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)dst, 16, (int)goff0, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)(dst + 4096u), 16, (int)goff0,
                                                 (int)(32u * (uint32_t)row_bytes), 0, 0);
    };

    // A fragments: a[kk][m] = rows wm*64 + m*16 + (lane & 15), bytes kk*64 + (lane >> 4)*16 .. +16
    v4i a[2][4];
    {
        const uint8_t* ap = X4 + (uint64_t)(it.a_row0 + wm * 64u + (lane & 15u)) * row_bytes + kbyte +
                            (lane >> 4) * 16u;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                a[kk][m] = *reinterpret_cast<const v4i*>(ap + (uint64_t)m * 16u * row_bytes + kk * 64);
    }
#pragma unroll
    for (uint32_t t = 0; t < kStripRing - 1; ++t)
        if (t < T) issue(t);

    v4f acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = v4f{};

    // fragment (kk, n) of a stage: row n*16 + (lane & 15), 16-byte slot kk*4 + (lane >> 4), swizzled
    const uint32_t swz = ((lane & 15u) >> 1) & 7u;
    const uint32_t lds_base =
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)&lds[0][0];
    uint32_t boff[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
        boff[kk] = lds_base + (lane & 15u) * kStripRowBytes +
                   ((((uint32_t)kk * 4u + (lane >> 4)) ^ swz) * 16u);

#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int m = 0; m < 4; ++m) asm volatile("" ::"v"(a[kk][m]));  // retire the A loads here

    auto retire = [&](uint32_t t, uint32_t newest_issued) {
        const uint32_t younger = min(T - 1u, newest_issued) - t;
        if (younger >= 3u) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (younger == 2u) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (younger == 1u) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    static_assert(kStripRing >= 3 && kStripRing <= 5, "vmcnt cases above cover rings of 3..5");

    // step s of a stage = (k-step s >> 2, B block s & 3): 1 fragment read, 4 MFMAs
#define STORM_FETCH16(dst, stage_base, s)                                                 \
    asm volatile("ds_read_b128 %0, %1 offset:%2"                                          \
                 : "=&v"(dst)                                                             \
                 : "v"(boff[(s) >> 2] + (stage_base)), "n"(((s) & 3) * 16 * kStripRowBytes))
#define STORM_MUL16(s, frag)                                                              \
    _Pragma("unroll") for (int m = 0; m < 4; ++m)                                         \
        acc[m][(s) & 3] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(               \
            v8i{a[(s) >> 2][m].x, a[(s) >> 2][m].y, a[(s) >> 2][m].z, a[(s) >> 2][m].w, 0, 0, 0, 0}, \
            v8i{frag.x, frag.y, frag.z, frag.w, 0, 0, 0, 0}, acc[m][(s) & 3], 4, 4, 0, 0, 0, 0)
#define STORM_LGKM(n)                                       \
    asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0)

    v4i b0 = {}, b1 = {}, b2 = {}, b3 = {};
    uint32_t t = 0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // scalar loads of the item record
    // ---- the A tile's own 4 blocks: wave wm skips the blocks before its own rows, keeps the
    //      strict upper triangle of its own 64 x 64 block and takes the later blocks whole
#pragma unroll 1
    for (; t < D; ++t) {
        retire(t, t + kStripRing - 2);
        if (t + kStripRing - 1 < T) issue(t + kStripRing - 1);
        __builtin_amdgcn_sched_barrier(0);
        if (t >= wm) {
            const uint32_t sb = (t % kStripRing) * kStripStageBytes;
            STORM_FETCH16(b0, sb, 0);
            STORM_FETCH16(b1, sb, 1);
            STORM_FETCH16(b2, sb, 2);
            STORM_FETCH16(b3, sb, 3);
            STORM_LGKM(3); STORM_MUL16(0, b0); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b0, sb, 4);
            STORM_LGKM(3); STORM_MUL16(1, b1); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b1, sb, 5);
            STORM_LGKM(3); STORM_MUL16(2, b2); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b2, sb, 6);
            STORM_LGKM(3); STORM_MUL16(3, b3); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b3, sb, 7);
            STORM_LGKM(3); STORM_MUL16(4, b0); __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(2); STORM_MUL16(5, b1); __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(1); STORM_MUL16(6, b2); __builtin_amdgcn_sched_barrier(0);
            STORM_LGKM(0); STORM_MUL16(7, b3); __builtin_amdgcn_sched_barrier(0);
            if (t == wm) {
                // The accumulators hold exactly this wave's own 64 x 64 block (earlier stages were
                // skipped): clear the pairs i >= j in place. Block (m, n) covers rows m*16.. and
                // columns n*16..; C/D map: col = lane & 15, row = 4 * (lane >> 4) + reg.
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        if (m > n) acc[m][n] = v4f{};
                        if (m == n) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const uint32_t row = 4u * (lane >> 4) + (uint32_t)r;
                                acc[m][n][r] = row < (lane & 15u) ? acc[m][n][r] : 0.0f;
                            }
                        }
                    }
            }
        }
    }
    // ---- later blocks, software-pipelined three steps ahead across stage boundaries: iteration t
    //      retires stage t+1 before its own MFMAs, so its last three steps may already fetch the
    //      first three fragments of stage t+1
    if (t < T) {
        retire(t, t + kStripRing - 2);
        {
            const uint32_t sb = (t % kStripRing) * kStripStageBytes;
            STORM_FETCH16(b0, sb, 0);
            STORM_FETCH16(b1, sb, 1);
            STORM_FETCH16(b2, sb, 2);
        }
        for (; t < T; ++t) {
            if (t + 1 < T) retire(t + 1, t + kStripRing - 2);
            else __builtin_amdgcn_s_barrier();
            if (t + kStripRing - 1 < T) issue(t + kStripRing - 1);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t sb = (t % kStripRing) * kStripStageBytes;
            // (after the last stage this re-reads the same stage: never consumed; keeps the body branch-free)
            const uint32_t sn = ((t + 1 < T ? t + 1 : t) % kStripRing) * kStripStageBytes;
            STORM_FETCH16(b3, sb, 3); STORM_LGKM(3); STORM_MUL16(0, b0); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b0, sb, 4); STORM_LGKM(3); STORM_MUL16(1, b1); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b1, sb, 5); STORM_LGKM(3); STORM_MUL16(2, b2); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b2, sb, 6); STORM_LGKM(3); STORM_MUL16(3, b3); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b3, sb, 7); STORM_LGKM(3); STORM_MUL16(4, b0); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b0, sn, 0); STORM_LGKM(3); STORM_MUL16(5, b1); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b1, sn, 1); STORM_LGKM(3); STORM_MUL16(6, b2); __builtin_amdgcn_sched_barrier(0);
            STORM_FETCH16(b2, sn, 2); STORM_LGKM(3); STORM_MUL16(7, b3); __builtin_amdgcn_sched_barrier(0);
        }
        STORM_LGKM(0);
    }
#undef STORM_FETCH16
#undef STORM_MUL16
#undef STORM_LGKM
#undef STORM_LGKM_STR

    uint64_t mine = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {  // 16 x 64 entries below 2^24 each: a uint32 cannot overflow
        uint32_t part = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) part += (uint32_t)acc[m][n][r];
        mine += part;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (lane == 0 && mine != 0)
        atomicAdd(&slots[(item_idx * (uint32_t)kStripWaves + wave) & (kSlots - 1)],
                  (unsigned long long)mine);
}

// ------------------------------------------------------------------------------------------
// K2b: the 16x16x128 strips on BIT operands — no FP4 shadow, no expansion pass, one launch.
//
// strip16_fp4_kernel's stage loop is fed from an FP4 image of the B stage in the LDS; where that
// image comes from is all that changes. There the image is DMA'd from a shadow matrix that an
// HBM-bound pass (expand_fp4_kernel: 84 MB in, 335 MB out, 70 us of the headline shape's 823)
// rebuilt in front of every call. Here the workgroup builds the image itself, once per stage, from
// the bits:
//   * k-slice `ks` of an item = 256 bit-MACs per row pair, as before, but taken out of the 64-byte
//     CHUNK ks / 2 of the bit rows (512 bits) as two of its four bit CLASSES: class c = the bits
//     4n + c of every dword, which already sit in nibble n. Rotating the dword right by c - 1 and
//     masking with 0x22222222 turns class c into E2M1 code 0b0010 = 1.0 per set bit (two VALU
//     operations per dword; the rotation wraps only into bits the mask drops). ks & 1 selects the
//     classes {0, 1} or {2, 3}. A sum over k does not care in which order k is walked as long as A
//     and B agree, and both sides are built by the same function.
//   * B stage: 64 rows x 64 B of bits = 4 KiB, ONE LDS-DMA instruction per wave (the FP4 strips: two,
//     8 KiB) into a ring of kBitRing stages in which every wave only ever touches its OWN 1 KiB
//     piece (it waits for its own DMA with vmcnt; no barrier is involved). Two stages ahead of the
//     multiplication the wave reads its piece back (one ds_read_b128 per lane), inflates the two
//     classes (16 VALU operations per wave and stage, against 32 MFMAs) and writes the two k-steps of
//     its 16 rows into the FP4 image (2 x ds_write_b128, the FP4 strips' XOR swizzle: conflict free).
//   * FP4 images: ring of 3 x 8 KiB. Iteration t multiplies image t (and, in its last three steps,
//     already reads the first fragments of image t + 1) while every wave writes its quarter of
//     image t + 2 into the slot image t - 1 left. ONE barrier per stage, as before: barrier t
//     separates the reads of image t - 1 from the writes of image t + 2 and publishes image t + 1.
//     LDS operations of a wave complete in order, so the fragment-read rotation's lgkmcnt waits also
//     retire the image writes in front of them — no extra waits.
//   * A operand: the wave's 64 rows x 64 B of bits come straight from global memory (4 x 16 B per
//     lane) and are inflated once per item into the same 32 registers the FP4 strips hold.
//   * the partial sums are folded by the last workgroup to arrive (ticket behind the slots, as in
//     bitstream_kernel) when `out` is given: a pass is ONE launch.
// 40 KiB of LDS and <= 128 registers: four workgroups per CU, as the FP4 strips need
// (profiles/r02_b_panels.txt). Work items, launch order, diagonal phase and the multi-GPU
// ownership are the FP4 strips' (build_strip_items); slices 2j and 2j + 1 read the same bits and go
// to the same XCD. Reference loop being replaced: storm.c:1199-1238 with the leaf of
// storm.c:1205,1217,1227,1236.
// ------------------------------------------------------------------------------------------
constexpr int kSb16ImgRing = 3;                                   // FP4 images (8 KiB each)
constexpr int kSb16BitRing = 3;                                   // bit stages (4 KiB each; a wave touches only its own 1 KiB piece)
[[maybe_unused]] constexpr int kSb16BitStage = kStripBRows * 64;                   // 4 KiB of bits per B stage (the kernels keep one 1 KiB piece per WAVE: 4 or 8 KiB)
constexpr uint32_t kSb16ImgBytes = kSb16ImgRing * kStripStageBytes;
constexpr uint32_t kSb16Mask = 0x22222222u;

__device__ __forceinline__ v4i sb16_inflate(v4i w, uint32_t rot) {
    v4i e;
    e.x = (int)(__builtin_amdgcn_alignbit((uint32_t)w.x, (uint32_t)w.x, rot) & kSb16Mask);
    e.y = (int)(__builtin_amdgcn_alignbit((uint32_t)w.y, (uint32_t)w.y, rot) & kSb16Mask);
    e.z = (int)(__builtin_amdgcn_alignbit((uint32_t)w.z, (uint32_t)w.z, rot) & kSb16Mask);
    e.w = (int)(__builtin_amdgcn_alignbit((uint32_t)w.w, (uint32_t)w.w, rot) & kSb16Mask);
    return e;
}

#define STORM_SB16_WAVES 4
#define STORM_SB16_NAME strip16_bits_kernel
#include "strip16_bits_kernel.inc"
#undef STORM_SB16_WAVES
#undef STORM_SB16_NAME
// [r6] The same with 8 waves and 512-row A tiles: waves w and w + 4 multiply different A rows by the SAME image and share
// its construction — each holds the piece of wave w & 3 (its own LDS-DMA copy: no cross-wave wait) and writes one of the
// two k-steps. Option k2_strip_operands = 6; measured against the default in profiles/r06_c_k2b_two_a_tiles.txt.
#define STORM_SB16_WAVES 8
#define STORM_SB16_NAME strip16_bits2_kernel
#include "strip16_bits_kernel.inc"
#undef STORM_SB16_WAVES
#undef STORM_SB16_NAME

// K2b with 128 A rows per wave (strip16_rows_kernel, option k2_strip_rows = 128): the same 96 registers spent the other way
// round. strip16_bits_kernel keeps 64 A rows x 256 bit-MACs per wave (a[2][4]) and accumulates 64 x 64: a B fragment meets
// the 4 A fragments of its k-step. Here a wave keeps 128 A rows x 128 bit-MACs — 8 A fragments of ONE k-step, blocks w and
// 7 - w of a 512-row A tile — and accumulates 128 x 32 (acc[8][2]): every B fragment feeds 8 MFMAs.
//   * k-slice `ks` = the 16 bytes [16 ks, 16 ks + 16) of every row, all four bit classes of its four dwords; element order
//     inside the k-step = (dword, class, nibble) on both sides (sr16_inflate builds both).
//   * B stage = 64 rows x 16 B = 1 KiB of bits: wave w DMAs its 16 rows as 4 bytes per lane (256 B per wave and slot, ring
//     of 3, own vmcnt), reads its dword back (ds_read_b32), inflates the four classes (7 VALU) and writes ONE ds_write_b128
//     into the image: 64 rows x 64 B = 4 KiB, ring of 3.
//   * diagonal phase (items with `diag`): the 8 B blocks are the A tile's own rows, which the waves hold inflated. Every wave
//     stores its 8 A fragments as the images of its two blocks (8 ds_write_b128 at the fragment-read address), ONE barrier
//     publishes the 8 resident images, and every wave walks the blocks d = w .. 7 without a barrier, a DMA or an inflation:
//     block w's triangle, whole products up to block 7 - w, that block's triangle beside them, both halves whole behind it
//     (strip_rows_role, storm_hip_plan.h) — 7 whole products and 2 triangles = 132 MFMAs for every wave. Four fragments of
//     a block are asked for at once and multiplied behind lgkmcnt(3 .. 0). The pieces of the first three pipelined stages
//     are in flight meanwhile; one more barrier, and the pipelined ring of 3 images is overlaid on resident images 0 .. 2.
//   * zero rows past the matrix's end (argument n_rows, storm_hip_plan.h): a run's top block with rows in 1 or 2 of its 4
//     fragments is the run's last stage and multiplies those alone (8 or 16 MFMAs per wave behind the loop, where a stage
//     has 32); the diagonal phase walks only the tile's blocks that hold a row. 10000 rows: 1.08 % fewer MFMAs per launch.
//   per 64 B rows and wave   strip16_bits_kernel    strip16_rows_kernel    its diagonal phase (per block step)
//   MFMAs                     32                     32                     10 / 16 / 26 / 32
//   fragment ds_read_b128     8                      4                      4
//   image ds_write_b128       2                      1                      0 (8 per item)
//   inflation VALU            16                     7                      0
//   piece read-back           ds_read_b128           ds_read_b32            none
//   barriers                  1                      1                      0 (2 per item)
//   LDS per workgroup         36 KiB                 35 KiB: 8 images of 4 KiB (the ring of 3 overlaid) + 3 KiB of bits
// 35 KiB x 4 workgroups = 140 of a CU's 160 KiB: the registers (<= 128) already cap a CU at 4 workgroups.
// Ring protocol, barrier per stage, epilogue and fold: strip16_bits_kernel's.
constexpr uint32_t kSr16SliceBytes = 16;                          // a k-slice of a row: 128 bits
constexpr uint32_t kSr16PerTile = kStripRowsATile / kStripBRows;  // 8 own blocks
constexpr uint32_t kSr16StageBytes = kStripBRows * 64;            // an FP4 image: 64 rows x 64 B
constexpr uint32_t kSr16ImgBytes = kSr16PerTile * kSr16StageBytes;   // the diagonal phase's 8 resident images; the ring of 3 is images 0 .. 2
constexpr uint32_t kSr16BitRing = 3;
constexpr uint32_t kSr16BitStage = 4 * 256;                       // 1 KiB of bits per B stage, 256 B per wave

__device__ __forceinline__ v4i sr16_inflate(uint32_t w) {   // the four classes of one dword: class c = rotate right by c - 1
    v4i e;
    e.x = (int)(__builtin_amdgcn_alignbit(w, w, 31u) & kSb16Mask);
    e.y = (int)(w & kSb16Mask);
    e.z = (int)(__builtin_amdgcn_alignbit(w, w, 1u) & kSb16Mask);
    e.w = (int)(__builtin_amdgcn_alignbit(w, w, 2u) & kSb16Mask);
    return e;
}
#include "strip16_rows_kernel.inc"

// ------------------------------------------------------------------------------------------
// K2t16: write-mode tile kernel on v_mfma_scale_f32_16x16x128_f8f6f4 (materialised XX^T, AND /
// OR / XOR counts, triangle / band / rectangle). Same items and output conventions as
// pairw_fp4_kernel<., true>; the dataflow borrows what made the strips fast:
//   workgroup : one 256 x 256 tile, 8 waves; wave w owns A rows [32 w, 32 w + 32) against ALL 256
//               B rows: 2 x 16 accumulator blocks of 16 x 16 (128 VGPRs). Nothing of A is shared
//               between waves, so
//   A operand : goes global -> registers directly (4 x 16-byte loads per lane and stage, one stage
//               ahead into the other of two fragment sets) — plain loads cost the issuing wave next
//               to nothing beside MFMAs (profiles/r01_h_ubench_feed.txt) —
//   B operand : alone crosses the LDS: stage = 256 rows x 128 B (two k-steps, FULL 128-byte lines:
//               half the L2 requests of 64-byte pieces) = 32 KiB, 4 LDS-DMA instructions per wave and
//               stage — per MFMA the strip kernel's count, half of the 32x32 tile kernel's, and the
//               DMA issue is the expensive part of feeding the matrix pipe
//               (profiles/r02_ubench_shape.txt) — ring of 4 stages (128 KiB), the strips' image
//               (slot ^ (row / 2) % 8: conflict free for the 16-row fragment reads);
//   per stage : 32 steps of (1 ds_read_b128 three steps ahead, 2 MFMAs); the reads of a stage's last
//               three steps already fetch from the next stage; ONE barrier per 64 MFMAs per wave.
//   stagger   : waves w and w + 4 share a SIMD and run the same program behind the same barrier. The
//               LDS-DMA issue stalls its wave for 100+ cycles; waves 0-3 issue theirs at the head of
//               the stage, waves 4-7 half a stage later, so that one partner multiplies while the
//               other issues (MI355X_MICROARCH.md, "Two waves per SIMD", item 9).
// Measured at the headline shape (profiles/r02_i_matrix_tile16.txt): 1.435 ms per call against 1.52
// for pairw_fp4_kernel in the same order and pitch. Three differently built kernels (this one; the
// same with 32x32x64 MFMAs: 1.47 ms; pairw_fp4_kernel) end within 6 % of each other, reading 7 steps
// ahead instead of 3 changes nothing, and an L2 prefetch of the lines 2..12 stages ahead (one 4-byte
// load per lane and stage) made it SLOWER (1.70-2.10 ms): what the 256 x 256 tiling costs is the
// delivery of its 13.8 GB of operand pieces (8 rows x 128 B per wave-instruction) from L2 to the CUs,
// ~10 TB/s here, not latency and not the matrix pipe. A tile twice as large does not fit the
// accumulators a CU can hold next to two waves per SIMD.
// vmcnt bookkeeping: every iteration issues A(s+1) (4 loads) and then the DMA of stage s+3 (4), so
// at the top of iteration s exactly the 4 DMA instructions of stage s+2 may stay in flight behind
// A(s); everything older — A(s) and the B stages up to s+1 — has landed. The last iterations, where
// fewer operations are issued, drain with vmcnt(0).
// ------------------------------------------------------------------------------------------
[[maybe_unused]] constexpr int kT16Ring = 4;
constexpr int kT16RowBytes = 128;                       // two k-steps of 128 bits
[[maybe_unused]] constexpr int kT16StageBytes = kTile * kT16RowBytes;    // B only: 32 KiB

#ifdef STORM_HIP_PROBES  // FP4-shadow output kernel on 16x16x128 MFMAs (45 % slower than tilebits8_kernel): tools build (make probes)
#include "../../tools/probes/tile16_fp4.hip"
#endif  // STORM_HIP_PROBES

// ------------------------------------------------------------------------------------------
// K2t-bits: the materialised-output kernel on the BIT matrix itself (default, option k2_tile_shape = 1).
//
// tile16_fp4_kernel above pulls 64 KiB of FP4 operands into the CU per 256 x 256 x 256 tile step
// (13.8 GB per headline call). The operands are 4 x inflated bits, so this kernel moves the bits and
// inflates them in registers, where it costs ONE v_and_b32 per operand dword instead of the ~10-op bit
// spread of expand_fp4_kernel:
//   * a sum over k does not care in which order k is walked, as long as A and B agree. A lane
//     holds 128 consecutive bits of its row as four dwords w0..w3 (one ds_read_b128). MFMA "class" c
//     takes the operand {w0 & K_c, .., w3 & K_c} with K_c = 0x11111111 << c: bit 4 n + c of each word
//     sits in nibble n ALREADY, as E2M1 code 1 << c = 0.5, 1.0, 2.0 for c = 0, 1, 2. Bit 3 of a nibble
//     is the sign, so class 3 is shifted down once: (w >> 1) & K_2. Four MFMAs (one per class)
//     consume the 128 bits of each lane; with the two k-halves of the 32x32x64 form, 256 bits of k.
//   * both operands of class c carry the same value v_c, so a set pair contributes v_c^2; the
//     block scale of the scaled MFMA (E8M0, 2^(s - 127), applied to both operands) restores 1:
//     s = 128, 127, 126, 126. Every partial sum is a small multiple of 1/4: exact in f32.
// There is no FP4 shadow and no expansion pass for this path: the operands are the matrix rows.
// What shapes the kernel is ISSUE bandwidth, not bytes (first version, 8 waves of 64 x 128 with
// 16x16x128 MFMAs, two per SIMD: 1.36 ms, matrix pipe 57 % busy — a 16-cycle MFMA holds the SIMD's
// vector issue for 8 cycles and each v_and costs 4, MI355X_MICROARCH.md "vector-instruction ISSUE
// cost"; 1.9 inflation ops per MFMA did not fit beside it). Hence:
//   * ONE wave per SIMD with the whole register file: 4 waves, wave w owns A rows 128 (w % 2) .. + 127
//     against B rows 128 (w / 2) .. + 127 = 4 x 4 blocks of 32 x 32 (256 accumulator registers).
//     Inflation work goes with operand rows per MFMA: (4 + 4) blocks x 5 ops per 16 MFMAs of
//     32 cycles each = 2.5 ops (10 issue cycles) + the MFMA's own 8 per 32-cycle slot.
//   * stage = 512 bits of k: 256 A rows + 256 B rows x 64 B = 32 KiB by LDS-DMA (8 pieces per wave,
//     one per class phase), ring of 4; k-group = 256 bits = one ds_read_b128 per lane and block, read
//     one k-group ahead; per class phase 16 MFMAs with the next B operand and the next phase's A
//     operands inflated between them.
// LDS image: row r at 64 r, 16-byte slot s at s ^ ((r / 4) % 4) (conflict free for 16 consecutive rows).
// Rows beyond the matrix read as zero through the buffer descriptor's range (num_records = valid
// rows x pitch, rebuilt per stage with the k offset folded into the base).
// ------------------------------------------------------------------------------------------
[[maybe_unused]] constexpr int kTbThreads = 256;
constexpr int kTbRing = 4;
constexpr int kTbRowBytes = 64;                          // 512 bits of k per stage
constexpr int kTbImageBytes = kTile * kTbRowBytes;       // 16 KiB per operand
constexpr int kTbStageBytes = 2 * kTbImageBytes;         // A image, then B image

template <int C>
__device__ __forceinline__ v4i tb_inflate(v4i w) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    if constexpr (C == 3) return (v4i)(((v4u)w >> 1u) & 0x44444444u);
    else return w & (int)(0x11111111u << C);
}
template <int C>
__device__ __forceinline__ int tb_scale() {  // E8M0 block scale undoing v_c on each operand
    return C == 0 ? 128 : C == 1 ? 127 : 126;
}

// Epilogue of the bit-operand kernels for a tile that lies wholly inside the output (no diagonal,
// no edge, no k-parts, 16-byte aligned rows): the accumulators hold 16 ROWS of one column per
// lane, so storing them directly costs one 4-byte store per element, two 128-byte runs per
// wave-instruction (measured: 16 us per tile item, 5 % of the call). Here each wave turns its block
// through a private 16 KiB of the (now idle) ring, 32 rows x 128 columns at a time, and stores
// 16 bytes per lane: two 512-byte runs per instruction, a quarter of the instructions.
template <int MB>
__device__ __forceinline__ void tb_store_interior(const v16f (&acc)[MB][4], uint8_t* lds_wave,
                                                  uint32_t* __restrict__ out_tile, uint64_t ld,
                                                  uint32_t lane, const uint32_t* __restrict__ row_counts,
                                                  uint32_t i0, uint32_t j0, uint32_t and_weight) {
    uint32_t* w32 = reinterpret_cast<uint32_t*>(lds_wave);
    const uint4* r128 = reinterpret_cast<const uint4*>(lds_wave);
    uint32_t nj[4] = {0u, 0u, 0u, 0u};
    if (row_counts) {
#pragma unroll
        for (int n = 0; n < 4; ++n) nj[n] = row_counts[j0 + (uint32_t)n * 32u + (lane & 31u)];
    }
#pragma unroll
    for (int m = 0; m < MB; ++m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t il = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
            const uint32_t ni = row_counts ? row_counts[i0 + (uint32_t)m * 32u + il] : 0u;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const uint32_t c = (uint32_t)acc[m][n][r];
                w32[il * 128u + (uint32_t)n * 32u + (lane & 31u)] = row_counts ? ni + nj[n] - and_weight * c : c;
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t row = (uint32_t)q * 2u + (lane >> 5);
            const uint4 v = r128[row * 32u + (lane & 31u)];
            *reinterpret_cast<uint4*>(&out_tile[(uint64_t)((uint32_t)m * 32u + row) * ld + 4u * (lane & 31u)]) = v;
        }
    }
}


#ifdef STORM_HIP_PROBES  // bit-operand output kernel, one wave per SIMD (3 % slower than tilebits8_kernel): tools build (make probes)
#include "../../tools/probes/tilebits.hip"
#endif  // STORM_HIP_PROBES

// ------------------------------------------------------------------------------------------
// The same with TWO waves per SIMD (default, option k2_tile_shape = 2): 8 waves, wave (wa, wb) owns A rows
// 64 wa .. + 63 (2 blocks of 32) against the B blocks 64 n + 32 wb .. + 31, n = 0..3 (interleaved between
// the two B halves): 128 accumulator registers, 3.75 inflation ops per MFMA instead of 2.5, but a wave's
// DMA issue and waits overlap with its SIMD partner's MFMAs (3 % faster than one wave per SIMD).
// A wave multiplies only the blocks it needs, a contiguous range [n_lo, n_hi):
//   * columns beyond the output (the ragged last row block: 16 of 256 rows at N = 10000, 40 of the 820
//     tiles) drop out through n_hi;
//   * on a diagonal tile, blocks wholly below the diagonal drop out through n_lo = wa; the A quarters are
//     dealt so that SIMD partners hold wa and 3 - wa (5 of 8 blocks per SIMD instead of 8).
// The loop body is instantiated for 1..4 blocks (tb_static_for: indices are compile-time constants, the
// accumulators stay in registers); every instantiation issues the same DMA pieces and barriers, so the
// waves of one workgroup may run different ones. The host orders diagonal and ragged tiles last and cuts
// the tiles beyond the last full round of workgroups into k-parts of equal COST (plan_matrix_tiles).
// ------------------------------------------------------------------------------------------
template <class F, int... I>
__device__ __forceinline__ void tb_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void tb_static_for(F&& f) {
    tb_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

template <int OFF>
__device__ __forceinline__ void tb_fetch(v4i& dst, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(addr), "n"(OFF));
}

__global__ __launch_bounds__(kMfmaThreads, 2) void tilebits8_kernel(
    TileOperands ops, const MfmaItem* __restrict__ items, OutWindow window, uint32_t split_from, uint32_t* __restrict__ parts) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[kTbRing][kTbStageBytes];
    const OutWindow w = window.loaded();

    STORM_CLOCK_BEGIN();
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wb = wave >> 2;
    const uint32_t wa = wb ? 3u - (wave & 3u) : (wave & 3u);  // SIMD partners: wa and 3 - wa
    const uint32_t item_idx = blockIdx.x;
    const MfmaItem it = items[item_idx];
    const uint32_t a_row0 = (uint32_t)it.I * kTile, b_row0 = (uint32_t)it.J * kTile;
    const uint32_t S = it.n_stages / 4u;
    const uint32_t kbyte0 = it.stage0 * 16u;
    const uint32_t pitch = (uint32_t)ops.pitch;

    const uint8_t *a_base, *b_base;
    uint32_t a_bytes, b_bytes;
    ops.tile_rows(a_row0, (uint32_t)kTile, a_base, a_bytes);
    ops.tile_rows(b_row0, (uint32_t)kTile, b_base, b_bytes);

    // blocks of B this wave multiplies: [n_lo, n_hi)
    const uint32_t col_limit = w.col_end();
    const uint32_t vc = col_limit > b_row0 ? min(col_limit - b_row0, (uint32_t)kTile) : 0u;
    const uint32_t n_hi = vc > 32u * wb ? min((vc - 32u * wb + 63u) / 64u, 4u) : 0u;
    const uint32_t n_lo = (!w.rect() && a_row0 == b_row0) ? min(wa, n_hi) : 0u;
    const uint32_t nb = n_hi - n_lo;

    const uint32_t voff0 = (wave * 16u + (lane >> 2)) * pitch + (((lane & 3u) ^ ((lane >> 4) & 3u)) * 16u);
    auto issue_piece = [&](uint32_t s, uint32_t p) __attribute__((always_inline)) {
        const uint32_t koff = kbyte0 + s * kTbRowBytes;
        const bool second = p >= 2u;
        const uint32_t bytes = s < S ? (second ? b_bytes : a_bytes) : 0u;
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>((second ? b_base : a_base) + koff), 0, bytes ? bytes - koff : 0u, 0x00020000);
        uint8_t* dst = lds[s % kTbRing] + (second ? kTbImageBytes : 0) + (wave + 8u * (p & 1u)) * 1024u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lptr_t)dst, 16, (int)(voff0 + (p & 1u) * 128u * pitch), 0, 0, 0);
    };

    const uint32_t lds_base =
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)&lds[0][0];
    const uint32_t slot = (lane >> 5) ^ (((lane & 31u) >> 2) & 3u);
    const uint32_t a_frag0 = lds_base + (wa * 64u + (lane & 31u)) * kTbRowBytes + slot * 16u;
    const uint32_t a_frag1 = lds_base + (wa * 64u + (lane & 31u)) * kTbRowBytes + (slot ^ 2u) * 16u;
    const uint32_t b_delta = kTbImageBytes + (64u * n_lo + 32u * wb) * kTbRowBytes - wa * 64u * kTbRowBytes;

#pragma unroll
    for (uint32_t s = 0; s < 3; ++s)
#pragma unroll
        for (uint32_t p = 0; p < 4; ++p) issue_piece(s, p);

    // [r5] option k2_matrix_parts: an item that covers only a part of k (the cut last round; every tile of a matrix with fewer
    // tiles than CUs) writes its counts into ITS OWN 256 x 256 window of `parts` with plain stores and reduce_parts_kernel adds
    // the windows of a tile up. parts == nullptr (the default): the parts add into the cleared output with atomics. Measured
    // (profiles/r05_k_matrix_sizes.jsonl): the atomics are 10 of this kernel's 51 us at 1024 rows, not the 36 a count of
    // L2 atomic operations suggested, and the second kernel costs more than that.
    uint32_t* part_tile = (item_idx >= split_from && parts) ? parts + (uint64_t)(item_idx - split_from) * (kTile * kTile) : nullptr;
    const bool full_tile = w.covers(a_row0, (uint32_t)kTile, b_row0, (uint32_t)kTile);
    const bool interior = full_tile && (part_tile ? true : (item_idx < split_from && (w.ld & 3u) == 0 && ((uintptr_t)w.out & 15u) == 0));

    auto run = [&](auto nbc) __attribute__((always_inline)) {
        constexpr int NB = decltype(nbc)::value;
        v16f acc[2][NB];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NB; ++n) acc[m][n] = v16f{};
        v4i ba[2][2], bb[2][NB];   // [k-group parity][block]: bits of the k-group in use / of the next one
        v4i aop[2][2], bop[2];     // inflated A blocks per class-phase parity, inflated B block per block parity
        bop[1] = v4i{};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // scalar loads of the item record
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            const uint32_t b0 = a_frag0 + b_delta;
            tb_fetch<0>(ba[0][0], a_frag0);
            tb_fetch<32 * kTbRowBytes>(ba[0][1], a_frag0);
            tb_static_for<NB>([&](auto nc) __attribute__((always_inline)) {
                constexpr int n = decltype(nc)::value;
                tb_fetch<n * 64 * kTbRowBytes>(bb[0][n], b0);
            });
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            aop[0][0] = tb_inflate<0>(ba[0][0]);
            aop[0][1] = tb_inflate<0>(ba[0][1]);
            bop[0] = tb_inflate<0>(bb[0][0]);
        }
        for (uint32_t s = 0; s < S; ++s) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const uint32_t cur = (s % kTbRing) * kTbStageBytes;
            const uint32_t nxs = ((s + 1 < S ? s + 1 : s) % kTbRing) * kTbStageBytes;
            const uint32_t a1 = a_frag1 + cur, b1 = a1 + b_delta;
            const uint32_t a0n = a_frag0 + nxs, b0n = a0n + b_delta;
            const uint32_t dma_stage = s + kTbRing - 1;
            tb_static_for<8>([&](auto pc) __attribute__((always_inline)) {
                constexpr int p = decltype(pc)::value;
                constexpr int kg = p / 4, c = p % 4, cn = (c + 1) % 4;
                constexpr int src = c < 3 ? kg : 1 - kg;  // bits the next phase's operands come from
                if constexpr (p % 2 == 0) issue_piece(dma_stage, p / 2);
                const uint32_t an = kg == 0 ? a1 : a0n, bn = kg == 0 ? b1 : b0n;
                if constexpr (c == 0) {
                    tb_fetch<0>(ba[1 - kg][0], an);
                    tb_fetch<32 * kTbRowBytes>(ba[1 - kg][1], an);
                    tb_fetch<0>(bb[1 - kg][0], bn);
                    if constexpr (NB > 1) tb_fetch<64 * kTbRowBytes>(bb[1 - kg][1], bn);
                }
                if constexpr (c == 1) {
                    if constexpr (NB > 2) tb_fetch<2 * 64 * kTbRowBytes>(bb[1 - kg][2], bn);
                    if constexpr (NB > 3) tb_fetch<3 * 64 * kTbRowBytes>(bb[1 - kg][3], bn);
                }
                if constexpr (c == 3) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                tb_static_for<NB>([&](auto bc) __attribute__((always_inline)) {
                    constexpr int b = decltype(bc)::value;
                    constexpr int g = p * NB + b;  // blocks since the top of the stage: parity of the B operand
                    acc[0][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                        v8i{aop[p & 1][0].x, aop[p & 1][0].y, aop[p & 1][0].z, aop[p & 1][0].w, 0, 0, 0, 0},
                        v8i{bop[g & 1].x, bop[g & 1].y, bop[g & 1].z, bop[g & 1].w, 0, 0, 0, 0}, acc[0][b], 4, 4, 0,
                        tb_scale<c>(), 0, tb_scale<c>());
                    v4i nextb;
                    if constexpr (b + 1 < NB) nextb = tb_inflate<c>(bb[kg][b + 1]);
                    else nextb = tb_inflate<cn>(bb[src][0]);
                    acc[1][b] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                        v8i{aop[p & 1][1].x, aop[p & 1][1].y, aop[p & 1][1].z, aop[p & 1][1].w, 0, 0, 0, 0},
                        v8i{bop[g & 1].x, bop[g & 1].y, bop[g & 1].z, bop[g & 1].w, 0, 0, 0, 0}, acc[1][b], 4, 4, 0,
                        tb_scale<c>(), 0, tb_scale<c>());
                    bop[(g + 1) & 1] = nextb;
                    // the next phase's A operands: in the last two blocks (one block: both here)
                    if constexpr (NB == 1) {
                        aop[(p + 1) & 1][0] = tb_inflate<cn>(ba[src][0]);
                        aop[(p + 1) & 1][1] = tb_inflate<cn>(ba[src][1]);
                    } else if constexpr (b >= NB - 2) {
                        aop[(p + 1) & 1][b - (NB - 2)] = tb_inflate<cn>(ba[src][b - (NB - 2)]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
            });
            // the operands of the next stage's first phase are final here: keep them in their registers
            // across the back edge (hipcc otherwise re-inflates all 12 dwords at the top of every stage)
            asm volatile("" : "+v"(aop[0][0]), "+v"(aop[0][1]), "+v"(bop[0]));
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the empty pieces of the tail, too
        STORM_CLOCK_END();

        // ---- epilogue: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of a 32 x 32 block
        if constexpr (NB == 4) {
            if (interior) {  // every wave of an interior tile runs this instantiation
                __builtin_amdgcn_s_barrier();  // every wave has left the ring
                uint8_t* mine = &lds[0][0] + wave * 16384u;
                uint32_t* w32 = reinterpret_cast<uint32_t*>(mine);
                const uint4* r128 = reinterpret_cast<const uint4*>(mine);
                const uint32_t i0 = a_row0 + wa * 64u, j0 = b_row0 + 32u * wb;
                const OutWindow::counts_ptr_t rcs = part_tile ? nullptr : w.counts();   // (a part holds raw AND counts)
                const uint64_t ldx = part_tile ? (uint64_t)kTile : w.ld;
                uint32_t* out_tile = part_tile ? &part_tile[(i0 - a_row0) * (uint32_t)kTile + (j0 - b_row0)] : w.at(i0, j0);
                uint32_t nj[4] = {0u, 0u, 0u, 0u};
                if (rcs) {
#pragma unroll
                    for (int n = 0; n < 4; ++n) nj[n] = rcs[j0 + (uint32_t)n * 64u + (lane & 31u)];
                }
#pragma unroll
                for (int m = 0; m < 2; ++m) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const uint32_t il = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * (lane >> 5);
                        const uint32_t ni = rcs ? rcs[i0 + (uint32_t)m * 32u + il] : 0u;
#pragma unroll
                        for (int n = 0; n < 4; ++n) {
                            const uint32_t c = (uint32_t)acc[m][n][r];
                            w32[il * 128u + (uint32_t)n * 32u + (lane & 31u)] = rcs ? ni + nj[n] - w.and_weight * c : c;
                        }
                    }
                    // lane piece p = lane & 31: columns 4 p .. 4 p + 3 of the wave's 128 = block p / 8
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const uint32_t row = (uint32_t)q * 2u + (lane >> 5);
                        const uint32_t pc = lane & 31u;
                        const uint4 v = r128[row * 32u + pc];
                        *reinterpret_cast<uint4*>(
                            &out_tile[(uint64_t)((uint32_t)m * 32u + row) * ldx + 64u * (pc >> 3) + 4u * (pc & 7u)]) = v;
                    }
                }
                return;
            }
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const uint32_t j = b_row0 + 64u * (n_lo + (uint32_t)n) + 32u * wb + (lane & 31u);
            const bool j_ok = w.wants_col(j);
            const uint32_t nj = w.nj(j);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = a_row0 + wa * 64u + (uint32_t)m * 32u + (uint32_t)((r & 3) + 8 * (r >> 2)) +
                                       4u * (lane >> 5);
                    if (j_ok && w.writes_row(i, j)) {
                        const uint32_t c = (uint32_t)acc[m][n][r];
                        uint32_t* dst = w.at(i, j);
                        if (item_idx < split_from) {
                            *dst = w.value(c, i, nj);
                        } else if (part_tile) {
                            part_tile[(i - a_row0) * (uint32_t)kTile + (j - b_row0)] = c;
                        } else {
                            atomicAdd(dst, w.part_value(c, i, nj, it.stage0 == 0));
                        }
                    }
                }
        }
    };

    switch (nb) {
        case 4: run(std::integral_constant<int, 4>{}); break;
        case 3: run(std::integral_constant<int, 3>{}); break;
        case 2: run(std::integral_constant<int, 2>{}); break;
        case 1: run(std::integral_constant<int, 1>{}); break;
        default:  // nothing to multiply: this wave's share of the DMA and the barriers only
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            for (uint32_t s = 0; s < S; ++s) {
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                __builtin_amdgcn_s_barrier();
#pragma unroll
                for (uint32_t p = 0; p < 4; ++p) issue_piece(s + kTbRing - 1, p);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            break;
    }
}

// ------------------------------------------------------------------------------------------
// K2tb: the materialised-output kernel in K2b's form (option k2_tile_shape = 3) [r4].
//
// tilebits8_kernel inflates every operand it multiplies in registers: 3.75 vector operations per 32x32x64 MFMA,
// the matrix pipe 79 % busy at the 2.0 GHz that body holds: 0.68 of the FP4 peak. What K2b showed for the totals
// holds here: an operand that several waves multiply should be inflated ONCE, into an FP4 image in the LDS, and
// the 16x16x128 shape holds more clock.
//   workgroup : 4 waves, one 256 x 128 half of a 256 x 256 tile item over all of its k (two workgroups per
//               item, the two B halves; 80 KiB of LDS each: two workgroups per CU, from two barrier domains);
//               wave w owns A rows 64 w .. + 63 against the half's 128 B rows: 4 x 8 blocks of 16 x 16
//               (128 accumulator registers), 32 MFMAs per class of a 512-bit chunk, 128 per chunk.
//   B operand : the half's bits (128 rows x 64 B = 8 KiB per chunk) arrive by LDS-DMA, 2 pieces per wave, in a
//               2-deep ring in which a wave touches only its own pieces; one chunk ahead the wave reads its pieces
//               back, inflates them into all four classes and writes them into the images of the next chunk
//               (2 slots x 2 class pairs x 16 KiB, K2b's layout and swizzle). ONE barrier per chunk (128 MFMAs).
//   A operand : nobody shares a wave's A rows: their bits come straight from global memory (4 x 16 B per lane
//               and chunk, one chunk ahead) and are inflated in registers, the next class beside the MFMAs of
//               the current one.
//   classes   : class c = bits 4 n + c of every dword as E2M1 code 1 << c (c = 3: shifted down once), undone by
//               the block scales 128 / 127 / 126 / 126 on both operands (tilebits8_kernel's scheme): one
//               vector operation per operand dword and class instead of two. Per MFMA: 0.94 vector operations
//               (A 80 + B 40 per 128 MFMAs) against 3.75.
//   body      : generated (tools/gen_tile16_body.py -> tile16_bits_chunk.inc): 32 steps of 4 MFMAs per chunk,
//               fragments read two steps ahead into a rotation of three registers, the lgkmcnt values computed by
//               walking the wave's in-order LDS queue.
// Items, output conventions (triangle / band / rectangle, AND / OR / XOR through row_counts, k-split items that
// add into a cleared window) are tilebits8_kernel's. Extends the reference (README.md:165-167: per-pair counts
// for LD); the loop it stands for is storm.c:1199-1238 with the leaf's result kept per pair.
// ------------------------------------------------------------------------------------------
constexpr int kTiThreads = 256;
constexpr uint32_t kTiImgBytes = 128u * 128u;                 // one class pair of a 128-row half: 16 KiB
constexpr uint32_t kTiImgSlot = 2u * kTiImgBytes;             // both pairs of a chunk
constexpr uint32_t kTiBits0 = 2u * kTiImgSlot;                // the bits ring behind the images
constexpr uint32_t kTiBitsSlot = 128u * 64u;                  // 8 KiB
constexpr uint32_t kTiLdsBytes = kTiBits0 + 2u * kTiBitsSlot; // 80 KiB

#include "tile16_bits_chunk.inc"

// Class c of a dword (bits 4 n + c) as E2M1 codes with ONE set bit per nibble: bit 0 = 0.5, bit 1 = 1.0, bit 2 = 2.0.
// The A side keeps its bit where it is (one operation; class 3 moves down to 2.0): values 0.5, 1, 2, 2. The B side —
// inflated once per workgroup into the LDS image — takes the reciprocal: 2, 1, 0.5, 0.5. Every product is 1.0, so the
// multiplies need no block scales: the compiler emits the plain v_mfma_f32_*_f8f6f4 (the scaled form costs ~6 % in
// these loops: a 16-byte encoding and two more register reads, measured on K2b, LAB_NOTES.md).
template <int C>
__device__ __forceinline__ int ti_infl1(int w) {
    if constexpr (C == 3) return (int)(((uint32_t)w >> 1) & 0x44444444u);
    else return w & (int)(0x11111111u << C);
}
template <int C>
__device__ __forceinline__ int ti_inflb(int w) {
    if constexpr (C == 0) return (int)(((uint32_t)w << 2) & 0x44444444u);
    else if constexpr (C == 1) return w & 0x22222222;
    else return (int)(((uint32_t)w >> (C == 2 ? 2 : 3)) & 0x11111111u);
}

#define STORM_TI_SHAPE 16
#define STORM_TI_NAME tile16_bits_kernel
#include "tile_bits_kernel.inc"
#undef STORM_TI_SHAPE
#undef STORM_TI_NAME
#define STORM_TI_SHAPE 32
#define STORM_TI_NAME tile32_bits_kernel
#include "tile_bits_kernel.inc"
#undef STORM_TI_SHAPE
#undef STORM_TI_NAME

#include "tile_ring_kernel.inc"
#include "tile128_kernel.inc"

// ------------------------------------------------------------------------------------------
// K2sb: the strips on BIT operands (option k2_strip_operands = 1; the default stays the FP4 shadow).
//
// Same work items, ring protocol and accumulator handling as strip_fp4_kernel, but the rows travel as
// bits and are inflated to FP4 in registers (the output kernels' operand trick, tilebits_kernel above):
// no FP4 shadow (4 x the matrix), no expansion pass (8 % of a headline pass) and a quarter of the
// L2 -> LDS DMA. Measured at the headline shape, same box, interleaved (profiles/r02_p_strip_operands.txt):
// 0.857 ms per launch against 0.737 for strip16_fp4_kernel — the pass is 6 % SLOWER (0.865 against
// 0.815 ms) although it has nothing to expand: B is streamed, so every wave inflates every B operand it
// multiplies (2.5 ops per MFMA), the 64 stationary A registers leave 3 waves per SIMD instead of 4, and
// real rows (39 % of the bits set, all four classes busy) hold this body at 2.09 GHz against the FP4
// strips' 2.30 (matrix pipe 86 % busy). tools/ubench_shape had promised 8.8 PFLOP/s at 2.29 GHz while it
// fed the NIBBLE image as bits (10 % density, one class of four non-zero); with real densities it says
// 8.3 at 2.17 GHz against 8.1-8.2 for the FP4-fed stage. Kept for matrices whose FP4 shadow does not fit.
//   k-slice   : 512 bits (StripItem.ks counts 64-byte pieces of the bit rows).
//   A operand : this wave's 64 rows x 512 bits, inflated ONCE per item into all four classes:
//               2 row blocks x 2 k-groups x 4 classes x 4 VGPRs = 64 VGPRs.
//   B operand : stage = 64 rows x 64 B of bits = 4 KiB, ONE LDS-DMA piece per wave, ring of 4 (16 KiB);
//               per stage 4 ds_read_b128 (2 blocks of 32 rows x 2 k-groups), each inflated into the four
//               classes (20 ops) behind the MFMAs it feeds: 32 MFMAs of 32 cycles and 80 inflation ops per
//               stage and wave.
//   asm reads : every fetched word is kept alive up to the wait that covers it (STORM_SB_KEEP; see there).
//   exactness : an accumulator gains at most 512 per stage, runs are capped at 4096 stages: < 2^24.
// storm_hip_matrix_create keeps rows up to a multiple of 256 zero, so every row an item touches exists;
// with this option set it also pads the row pitch off multiples of 1 KiB (L2 sets).
// ------------------------------------------------------------------------------------------
constexpr int kSbRowBytes = 64;                                  // 512 bits of k
constexpr int kSbStageBytes = kStripBRows * kSbRowBytes;         // 4 KiB

#ifdef STORM_HIP_PROBES  // bit-operand strips, one item per workgroup, operands inflated in registers (superseded by K2q and K2b): tools build (make probes)
#include "../../tools/probes/stripbits.hip"
#endif  // STORM_HIP_PROBES

// ------------------------------------------------------------------------------------------
// K2q: bit-operand strips as ONE stream of stages per workgroup (option k2_strip_operands = 2; the
// default for matrices up to a few thousand rows).
//
// What the strips cost at N = 1024 ... 4096 is not their stage loop but everything around it
// (tools/strip_trace.py, profiles/r03_a_*): three launches, an expansion that writes 4 x the matrix
// only to have it read back once, a first touch of that shadow by every workgroup at the same moment
// (4.6 us at N = 1024), a diagonal phase that is not pipelined, work items of 4 ... 32 stages dealt to
// slots that all start and all finish together, and a fold. This kernel removes them:
//   * bits in, total out, ONE launch: operands inflated in registers (stripbits_kernel's stage body),
//     partial sums folded by the last workgroup to arrive (a ticket), slots and ticket left zeroed;
//   * the work is a STREAM of stages cut into equal shares on the host (build_bitstream): a workgroup
//     walks a list of segments {A tile, k-slice, the tile's own four 64-row blocks, a run of later
//     blocks} with the LDS ring running across segment boundaries; the accumulators are never flushed;
//   * every A tile meets the SAME number of later blocks: the tile pairs are dealt CYCLICALLY (tile I
//     takes the (T - 1) / 2 tiles behind it, wrapping around; popcount(a & b) is symmetric), so the
//     segments of one matrix are all the same length and shares of equal length are shares of equal
//     work;
//   * the A rows come through the ring too: a tile's own four blocks are the first four stages of
//     its segment, and wave w takes its operand (block w, rotated per segment so that the SIMDs share
//     the diagonal work) out of stage w before it multiplies it — no global loads into registers, no
//     second kind of memory traffic to count in vmcnt. A segment that continues a cut one brings the
//     four blocks in without multiplying them;
//   * no masking of the wave's own 64 x 64 block: it is multiplied whole at HALF weight (the block
//     scale of the B operand one lower) and sums to U + D / 2, where U is its strict upper triangle and
//     D the set bits of the wave's rows in this k-slice; D is counted with v_bcnt when the rows are
//     taken and subtracted at the end. Every accumulator stays a multiple of 1/2 below 2^23: exact.
// Stage, ring, swizzle and operand registers are stripbits_kernel's. Reference loop being replaced:
// storm.c:1199-1238 (blocked upper triangle), whose order of pairs the cyclic deal does not keep —
// the total does not depend on it.
// ------------------------------------------------------------------------------------------
// (the segment record BitSeg and kBsDiag: storm_hip_plan.h)
constexpr int kBsFoldSlots = 64;             // partial sums of this kernel: slots[0 .. 64)
constexpr int kBsTicket = kSlots + 6;        // arrival counter (behind the strip queue heads; zero between passes)
constexpr int kBsRing = 8;                   // LDS stages of 4 KiB; ONE barrier serves two stages (four, with a ring
                                             // of 12: faster at N = 512 only, 12.0 against 12.2 us, slower from 2048 up)

template <bool kTrace>
__global__ __launch_bounds__(kStripThreads, 3) void bitstream_kernel(
    const uint8_t* __restrict__ X, uint64_t pitch64, const BitSeg* __restrict__ segs,
    const uint32_t* __restrict__ first, const uint32_t* __restrict__ bases,
    const uint32_t* __restrict__ first_stage, unsigned long long* __restrict__ slots,
    unsigned long long* __restrict__ out, unsigned long long* __restrict__ trace) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds_raw[kBsRing * kSbStageBytes];
    auto lds = reinterpret_cast<uint8_t(*)[kSbStageBytes]>(lds_raw);

    unsigned long long t_start = 0, t_ready = 0;
    unsigned long long c_wait = 0, c_issue = 0, c_body = 0, c_mark = 0;  // shader clocks of wave 0 (trace build)
    uint32_t n_mul = 0;
    if (kTrace) t_start = __builtin_amdgcn_s_memrealtime();
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t pitch = (uint32_t)pitch64;
    const uint32_t s_begin = first[blockIdx.x], s_end = first[blockIdx.x + 1];

    // B stage = 4 LDS-DMA pieces of 16 rows x 64 B, one per wave (stripbits_kernel's image:
    // slot s of row r at s ^ ((r / 4) % 4))
    const uint32_t goff = (wave * 16u + (lane >> 2)) * pitch + (((lane & 3u) ^ ((lane >> 4) & 3u)) * 16u);
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)&lds[0][0];
    const uint32_t slot0 = (lane >> 5) ^ (((lane & 31u) >> 2) & 3u);
    const uint32_t baddr0 = lds_base + (lane & 31u) * kSbRowBytes + slot0 * 16u;
    const uint32_t baddr1 = lds_base + (lane & 31u) * kSbRowBytes + (slot0 ^ 2u) * 16u;

    v16f acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = v16f{};
    v4i a[2][4][2];  // [k-group][class][row block]: the wave's 64 A rows x 512 bits, all four classes
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int m = 0; m < 2; ++m) a[g][c][m] = v4i{};
    uint32_t dbits = 0;  // set bits of the rows this lane took as A in multiplied diagonal stages

    // ---- the stream. The DMA side reads the address of every stage's 64 rows from a table the host wrote
    // (64-byte units from X; build_bitstream): a wave alone on its SIMD issues one instruction every four cycles,
    // and the first version's address arithmetic between the barrier and the first MFMA of a stage (the cursor
    // over the segment records, a 64-bit multiply) cost a lone wave 265 of its 1760 cycles per stage
    // (tools/archive/stream_trace.py). The consume side walks the segment records (what a stage is to this wave).
    const uint32_t bs0 = first_stage[blockIdx.x];
    const uint32_t T = first_stage[blockIdx.x + 1] - bs0;
    uint32_t issued = 0;     // stages handed to the DMA so far
    uint32_t prepared = 0;   // stages whose address has been fetched
    uint32_t off_next = T ? bases[bs0] : 0u;
    uint64_t nbase = 0;      // the next piece to hand over ...
    bool nvalid = false;     // ... if there is one
    BitSeg rc = {};
    if (s_begin < s_end) rc = segs[s_begin];
    auto prep = [&]() {
        nvalid = prepared < T;
        nbase = (uint64_t)(uintptr_t)X + ((uint64_t)off_next << 6);
        ++prepared;
        off_next = bases[bs0 + min(prepared, T ? T - 1u : 0u)];
    };
    auto fire = [&]() {
        if (nvalid) {
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                reinterpret_cast<uint8_t*>((uintptr_t)nbase), 0, -1, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)(lds[issued % kBsRing] + wave * 1024u), 16,
                                                     (int)goff, 0, 0, 0);
            ++issued;
        }
    };
    prep();
#pragma unroll
    for (int k = 0; k < kBsRing - 2; ++k) {  // stages 0 .. 5: the ring's eight slots minus the pair a barrier frees
        fire();
        prep();
    }

#define STORM_BS_FETCH(dst, t, n, g) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(dst) : "v"(((g) ? baddr1 : baddr0) + ((t) % kBsRing) * kSbStageBytes), "n"((n) * 32 * kSbRowBytes))
    // one class of one B word against both A row blocks; the next operand is inflated BETWEEN the two MFMAs
    // (in the shadow of the first: the second cannot start before the first has left the pipe's front anyway)
#define STORM_BS_STEP(n, g, C, ecur, enxt, NEXT)                                                          \
    {                                                                                                     \
        acc[0][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(                                      \
            v8i{a[g][C][0].x, a[g][C][0].y, a[g][C][0].z, a[g][C][0].w, 0, 0, 0, 0},                      \
            v8i{ecur.x, ecur.y, ecur.z, ecur.w, 0, 0, 0, 0}, acc[0][n], 4, 4, 0, tb_scale<C>(), 0, sb[C]); \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        const v4i en_ = NEXT;                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        acc[1][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(                                      \
            v8i{a[g][C][1].x, a[g][C][1].y, a[g][C][1].z, a[g][C][1].w, 0, 0, 0, 0},                      \
            v8i{ecur.x, ecur.y, ecur.z, ecur.w, 0, 0, 0, 0}, acc[1][n], 4, 4, 0, tb_scale<C>(), 0, sb[C]); \
        enxt = en_;                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                \
    }
#define STORM_BS_WAIT() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0)
#define STORM_BS_KEEP() asm volatile("" ::"v"(w0), "v"(w1), "v"(e0))
    // One stage (stripbits_kernel's): on entry w0 holds the bits of (block 0, k-group 0) of stage `tc` and
    // e0 their class 0; on exit the same of stage `tn`.
#define STORM_BS_STAGE(tc, tn)                                      \
    STORM_BS_FETCH(w1, tc, 1, 0);                                   \
    __builtin_amdgcn_sched_barrier(0);                              \
    STORM_BS_STEP(0, 0, 0, e0, e0, tb_inflate<1>(w0));              \
    STORM_BS_STEP(0, 0, 1, e0, e0, tb_inflate<2>(w0));              \
    STORM_BS_STEP(0, 0, 2, e0, e0, tb_inflate<3>(w0));              \
    STORM_BS_WAIT();                                                \
    STORM_BS_STEP(0, 0, 3, e0, e0, tb_inflate<0>(w1));              \
    STORM_BS_FETCH(w0, tc, 0, 1);                                   \
    __builtin_amdgcn_sched_barrier(0);                              \
    STORM_BS_STEP(1, 0, 0, e0, e0, tb_inflate<1>(w1));              \
    STORM_BS_STEP(1, 0, 1, e0, e0, tb_inflate<2>(w1));              \
    STORM_BS_STEP(1, 0, 2, e0, e0, tb_inflate<3>(w1));              \
    STORM_BS_WAIT();                                                \
    STORM_BS_STEP(1, 0, 3, e0, e0, tb_inflate<0>(w0));              \
    STORM_BS_FETCH(w1, tc, 1, 1);                                   \
    __builtin_amdgcn_sched_barrier(0);                              \
    STORM_BS_STEP(0, 1, 0, e0, e0, tb_inflate<1>(w0));              \
    STORM_BS_STEP(0, 1, 1, e0, e0, tb_inflate<2>(w0));              \
    STORM_BS_STEP(0, 1, 2, e0, e0, tb_inflate<3>(w0));              \
    STORM_BS_WAIT();                                                \
    STORM_BS_STEP(0, 1, 3, e0, e0, tb_inflate<0>(w1));              \
    STORM_BS_FETCH(w0, tn, 0, 0);                                   \
    __builtin_amdgcn_sched_barrier(0);                              \
    STORM_BS_STEP(1, 1, 0, e0, e0, tb_inflate<1>(w1));              \
    STORM_BS_STEP(1, 1, 1, e0, e0, tb_inflate<2>(w1));              \
    STORM_BS_STEP(1, 1, 2, e0, e0, tb_inflate<3>(w1));              \
    STORM_BS_WAIT();                                                \
    STORM_BS_STEP(1, 1, 3, e0, e0, tb_inflate<0>(w0))

    v4i w0 = {}, w1 = {}, e0 = {};
    int sb[4] = {tb_scale<0>(), tb_scale<1>(), tb_scale<2>(), tb_scale<3>()};  // B-side block scales of the stage
    uint32_t ci = 0;  // stage of the consume cursor in its segment rc
    uint32_t sc = s_begin;
    uint32_t t = 0;   // stages consumed
    if (issued > 0) {
        // stage 0 has landed (the younger pieces may stay in flight: the loop's first barrier waits for more)
        if (issued >= 6u) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        STORM_BS_FETCH(w0, 0u, 0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w0)::"memory");
        __builtin_amdgcn_sched_barrier(0);
        e0 = tb_inflate<0>(w0);
    }
    if (kTrace) t_ready = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
    while (t < T) {
        // ONE barrier serves two stages (a lone wave spends ~230 clocks per barrier: arrival skew of the four
        // waves + the DMA wait). At the top of an EVEN stage t: stages up to t + 2 have landed (t and t + 1 are
        // multiplied before the next barrier, and the end of t + 1 already reads the first word of t + 2), every
        // wave is done with the stages before t, and the two pieces behind the six in flight are handed over
        // (invariant: issued == min(T, t + 6) at an even t).
        const bool has_next = t + 1u < T;
        if (kTrace) c_mark = __builtin_readcyclecounter();
        if ((t & 1u) == 0u) {
            if (issued >= t + 6u) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");   // t + 3 .. t + 5 may fly
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      // the stream's last stages
            __builtin_amdgcn_s_barrier();
            if (kTrace) {
                const unsigned long long now = __builtin_readcyclecounter();
                c_wait += now - c_mark;
                c_mark = now;
            }
            fire();
            prep();
            fire();
            prep();
        }
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t tn = has_next ? t + 1u : t;
        // what this wave does with the stage
        const uint32_t wm = (wave + (rc.flags >> 8)) & 3u;  // its A rows are block wm of the tile
        const bool own = ci == wm;
        const bool diag = (rc.flags & kBsDiag) != 0u;
        const bool mul = ci >= 4u || (diag && ci >= wm);
        if (kTrace) {
            const unsigned long long now = __builtin_readcyclecounter();
            c_issue += now - c_mark;
            c_mark = now;
        }
        if (own) {
            // the wave's A rows are this stage's rows: all four words, every class
            v4i x1, x2, x3;
            STORM_BS_FETCH(x1, t, 1, 0);
            STORM_BS_FETCH(x2, t, 0, 1);
            STORM_BS_FETCH(x3, t, 1, 1);
            // (the wait DEFINES the words it covers: hipcc moves code that only depends on an asm's outputs
            //  across basic blocks, past a bare s_waitcnt — sched_barrier pins the order inside one block only)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(x1), "+v"(x2), "+v"(x3)::"memory");
            __builtin_amdgcn_sched_barrier(0);
            a[0][0][0] = tb_inflate<0>(w0); a[0][1][0] = tb_inflate<1>(w0);
            a[0][2][0] = tb_inflate<2>(w0); a[0][3][0] = tb_inflate<3>(w0);
            a[0][0][1] = tb_inflate<0>(x1); a[0][1][1] = tb_inflate<1>(x1);
            a[0][2][1] = tb_inflate<2>(x1); a[0][3][1] = tb_inflate<3>(x1);
            a[1][0][0] = tb_inflate<0>(x2); a[1][1][0] = tb_inflate<1>(x2);
            a[1][2][0] = tb_inflate<2>(x2); a[1][3][0] = tb_inflate<3>(x2);
            a[1][0][1] = tb_inflate<0>(x3); a[1][1][1] = tb_inflate<1>(x3);
            a[1][2][1] = tb_inflate<2>(x3); a[1][3][1] = tb_inflate<3>(x3);
            if (diag) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    dbits += __builtin_popcount((uint32_t)w0[k]) + __builtin_popcount((uint32_t)x1[k]) +
                             __builtin_popcount((uint32_t)x2[k]) + __builtin_popcount((uint32_t)x3[k]);
            }
        }
        if (mul) {
            const int half = (own && ci < 4u) ? 1 : 0;  // the wave's own block: half weight
            sb[0] = tb_scale<0>() - half;
            sb[1] = tb_scale<1>() - half;
            sb[2] = tb_scale<2>() - half;
            sb[3] = tb_scale<3>() - half;
            __builtin_amdgcn_sched_barrier(0);
            STORM_BS_STAGE(t, tn);
            STORM_BS_WAIT();
            STORM_BS_KEEP();
        } else {
            // nothing to multiply: only the look-ahead word of the next stage (the first version wrote
            // `e0 = inflate(w0)` behind a bare wait shared with the other branch; hipcc hoisted it into this
            // block, in front of the wait, and the waves that skip stages multiplied stale words)
            STORM_BS_FETCH(w0, tn, 0, 0);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w0)::"memory");
            __builtin_amdgcn_sched_barrier(0);
            e0 = tb_inflate<0>(w0);
        }
        if (kTrace) {
            const unsigned long long now = __builtin_readcyclecounter();
            c_body += now - c_mark;
            c_mark = now;
            n_mul += mul ? 1u : 0u;
        }
        if (kTrace) c_issue += __builtin_readcyclecounter() - c_mark;
        ++t;
        ++ci;
        if (ci == 4u + rc.n_b) {
            ci = 0;
            ++sc;
            rc = segs[min(sc, s_end - 1u)];
        }
    }
#undef STORM_BS_STAGE
#undef STORM_BS_KEEP
#undef STORM_BS_WAIT
#undef STORM_BS_STEP
#undef STORM_BS_FETCH

    // ---- the wave's total: accumulators in halves (exact), minus the diagonal's set bits, halved
    long long mine2 = 0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        uint32_t part = 0;  // 32 values below 2^23 each
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) part += (uint32_t)(acc[m][n][r] * 2.0f);
        mine2 += part;
    }
    mine2 -= (long long)dbits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine2 += __shfl_down(mine2, o, 64);
    // the four waves through the (drained) ring, one atomic per workgroup, then the ticket
    __builtin_amdgcn_s_barrier();
    long long* wsum = reinterpret_cast<long long*>(lds_raw);
    if (lane == 0) wsum[wave] = mine2;
    __syncthreads();
    if (tid == 0) {
        const long long tot2 = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot2 != 0) atomicAdd(&slots[blockIdx.x & (kBsFoldSlots - 1)], (unsigned long long)(tot2 / 2));
        __threadfence();
        const unsigned long long arrived = atomicAdd(&slots[kBsTicket], 1ull);
        wsum[4] = (arrived == (unsigned long long)gridDim.x - 1ull) ? 1 : 0;
        if (kTrace) {
            trace[blockIdx.x * 8ull + 0] = t_start;
            trace[blockIdx.x * 8ull + 1] = __builtin_amdgcn_s_memrealtime();
            trace[blockIdx.x * 8ull + 2] = ((t_ready - t_start) & 0xffffffffull) | ((unsigned long long)t << 32);
            trace[blockIdx.x * 8ull + 3] = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11)) |
                                           ((unsigned long long)__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)) << 32);
            trace[blockIdx.x * 8ull + 4] = c_wait;
            trace[blockIdx.x * 8ull + 5] = c_issue;
            trace[blockIdx.x * 8ull + 6] = c_body;
            trace[blockIdx.x * 8ull + 7] = n_mul;
        }
    }
    __syncthreads();
    if (wsum[4] != 0 && wave == 0) {
        // last workgroup to arrive: every other one's sum is in the slots (its atomic add is ordered
        // before its ticket). Fold, hand over the total, leave slots and ticket zero for the next pass.
        __threadfence();
        unsigned long long v = __hip_atomic_exchange(&slots[lane], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) {
            out[0] = v;
            __hip_atomic_store(&slots[kBsTicket], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#ifdef STORM_HIP_PROBES  // K2w: the stage stream with a private ring per wave: tools build (make probes)
#include "../../tools/probes/bitwave.hip"
#endif  // STORM_HIP_PROBES

static void release_panel_lists(storm_hip_ctx_t* ctx) {
    for (PanelList& l : ctx->panel_lists) {
        l.list.release();
        if (l.landed) (void)hipEventDestroy(l.landed);
    }
    ctx->panel_lists.clear();
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    ctx->copy_stream = nullptr;
}

// One empty launch per translation unit at context creation: the runtime loads a TU's code object at the first launch of
// one of its kernels (a few ms for this file's), and the first storm.h call — the only one the reference's harness times,
// benchmark.cpp:605-613 — used to pay for it.
__global__ void warm_mfma_kernel() {}
void warm_mfma_code(hipStream_t stream) { hipLaunchKernelGGL(warm_mfma_kernel, dim3(1), dim3(64), 0, stream); }

void release_mfma_state(storm_hip_ctx_t* ctx) {
    release_panel_lists(ctx);
    ctx->d_x4.release();
    ctx->items.release();
    ctx->strips.release();
    ctx->d_trace.release();
    ctx->d_counts.release();
    ctx->d_band.release();
    ctx->d_dosage_rows.release();
    ctx->d_dosage_sums.release();
    ctx->d_parts.release();
    ctx->d_tickets.release();
    ctx->d_bitsegs.release();
    ctx->bitfirst.release();
}

// The list buffers start at 4096 records: the lists of small matrices never reallocate them.
constexpr size_t kItemsFloorBytes = 4096 * sizeof(MfmaItem);
constexpr size_t kStripItemsFloorBytes = 4096 * sizeof(StripItem);

// The summing tile kernel's list (plan_tile_sum, storm_hip_plan.cpp), cached by its request.
static int ensure_items(storm_hip_ctx_t* ctx, const std::vector<RowRange>& ranges,
                        uint32_t total_stages, uint32_t shard_rank, uint32_t shard_count,
                        bool diag_only) {
    const TileSumRequest rq = {ranges_hash(ranges), total_stages, shard_rank, shard_count,
                               (uint32_t)std::max(1, ctx->k2_stages_per_item), diag_only ? 1u : 0u,
                               (ctx->k2_debug & 3) == 1 ? 1u : 0u};
    if (ctx->items.holds(rq)) return STORM_HIP_OK;
    std::vector<MfmaItem> items;
    if (int rc = plan_tile_sum(rq, ranges, items)) return rc;
    return ctx->items.put(ctx, rq, items.data(), items.size(), "K2: the item table", kItemsFloorBytes);
}

// The strip list of an all-pairs pass (plan_strips, storm_hip_plan.cpp), cached by its request: the context's shaping
// options, the shape and the shard.
static StripOptions strip_options_of(const storm_hip_ctx_t* ctx, int xcd_group, bool rows_form) {
    StripOptions o;
    o.max_run = ctx->k2_max_run;
    o.tail_run = ctx->k2_tail_run;
    o.tail_slices = ctx->k2_tail_slices;
    o.rows_form = rows_form;
    o.tail_auto = rows_form && !ctx->k2_tail_set;   // (the planner chooses the tail for one device's whole pass only)
    o.lpt_rounds = ctx->k2_lpt_rounds;
    o.shard_pairs = ctx->k2_shard_pairs != 0;
    o.n_cus = ctx->n_cus;
    o.xcd_group = xcd_group;
    o.persistent = ctx->k2_persistent != 0;
    o.one_slice_probe = (ctx->k2_debug & 16) != 0;
    return o;
}

static int ensure_strip_items(storm_hip_ctx_t* ctx, const std::vector<RowRange>& ranges,
                              uint32_t n_kslices, uint32_t shard_rank, uint32_t shard_count,
                              uint32_t a_tile, int xcd_group = 1, bool rows_form = false) {
    const StripRequest rq = strip_request(strip_options_of(ctx, xcd_group, rows_form), ranges, n_kslices, shard_rank, shard_count, a_tile);
    if (ctx->strips.holds(rq)) return STORM_HIP_OK;   // (k2_*_used are still this list's: nothing else writes them)
    ctx->strips.forget();   // (the queue bounds below are the new list's)
    std::vector<StripItem> items;
    StripChoice used;
    plan_strips(rq, ranges, items, ctx->strips.queue_base, ctx->strips.queue_count, &used);
    ctx->k2_max_run_used = used.max_run;
    ctx->k2_tail_run_used = used.tail_run;
    ctx->k2_tail_slices_used = used.tail_slices;
    if (items.size() >= (1ull << 31)) {
        set_error("K2s: %zu strip items exceed the grid limit", items.size());
        return STORM_HIP_EINVAL;
    }
    return ctx->strips.put(ctx, rq, items.data(), items.size(), "K2s: the strip items", kStripItemsFloorBytes);
}

// Row pitch of the FP4 shadow. Rows whose byte length is a multiple of a large power of two put
// every row block of a k-slice 2^15+ bytes apart, i.e. into a handful of L2 sets and memory
// channels; a few extra 128-byte lines per row break the pattern (strip kernel 0.866 -> 0.835 ms at
// the headline shape, its L2 misses 3.4 -> 0.86 GB per launch; 3 lines also suit the expansion's
// writes better than 1). k2_pitch_pad: -1 = that rule, otherwise the pad in bytes.
// The tile kernel wants the same pad once its tiles are launched in XCD groups
// (xcd_grouped_tiles): materialised matrix 1.72 ms dense, 1.56 ms with 384 B, 1.99 ms with 128 B
// (profiles/r02_e_matrix_order_pad.txt). In round 1's row-major tile order it had measured the
// other way round (1.96 dense, 2.25 padded).
static uint64_t shadow_pitch(const storm_hip_ctx_t* ctx, uint64_t row_bytes) {
    if (ctx->k2_pitch_pad >= 0) return row_bytes + (uint64_t)ctx->k2_pitch_pad;
    return row_bytes + (row_bytes % 1024 == 0 ? 384u : 0u);
}
// The FP4 shadow of at least `bytes`; a shadow that moves holds nothing ("keep_shadow").
static int ensure_shadow(storm_hip_ctx_t* ctx, size_t bytes, const char* what) {
    if (bytes > ctx->d_x4.capacity) memset(ctx->x4_key, 0, sizeof(ctx->x4_key));
    return ctx->d_x4.ensure(bytes, what);
}

// X: bit rows (stride_words per row), n_rows_src of them readable; the FP4 shadow gets
// n_rows_dst rows (a multiple of the A tile, rows >= n_rows_src zero). `strip_mode` selects the kernel.
int launch_pairw_mfma_ranges(storm_hip_ctx_t* ctx, const uint64_t* X, uint64_t stride_words,
                             uint64_t n_rows_src, uint64_t n_rows_dst,
                             const std::vector<RowRange>& ranges, uint32_t shard_rank,
                             uint32_t shard_count, int strip_mode, uint64_t* d_total,
                             uint64_t shadow_generation, uint32_t n_words_logical) {
    // shadow_generation != 0 identifies the content of X (dense matrix + its generation): with
    // "keep_shadow" an unchanged shadow of the same layout and shard is not rebuilt.
    // strip_mode: 0 = tile kernel, 1 = strips with 256-row A tiles, 2 = wide strips (512 rows;
    // n_rows_dst and every range start must then be multiples of 512)
    const bool strips = strip_mode != 0;
    const uint32_t a_tile = strip_mode == 2 ? 512u : (uint32_t)kStripATile;
    const uint64_t row_bytes = stride_words * 32;  // 64 bits -> 64 nibbles = 32 bytes
    // k-slices that hold data: the zero padding of the rows up to 64 words is never multiplied
    // (a 256-bit matrix is one slice, not sixteen)
    const uint32_t n_kslices = n_words_logical
                                   ? kStripFp4.kslices(n_words_logical)
                                   : (uint32_t)(row_bytes / kStripRowBytes);
    // HBM tiling along k: the FP4 shadow is 4 x the bits. When the whole of it would exceed the
    // context's budget ("k2_shadow_budget_mb") the strips run k-chunk by k-chunk over a compact
    // shadow of one chunk — expand chunk, multiply chunk, partial sums accumulate in the slots —
    // so the footprint is bounded whatever M * N is. Every chunk has the same number of slices
    // (the last one overhangs into zero columns), hence one work list serves all of them.
    const uint64_t rows_alloc = std::max<uint64_t>(n_rows_dst, kTile);
    uint32_t n_chunks = 1, chunk_slices = n_kslices;
    uint64_t shadow_row_bytes = row_bytes;
    if (strips) {
        uint64_t want = 1;  // chunks needed
        if (ctx->k2_shadow_budget_mb > 0) {
            const uint64_t budget = (uint64_t)ctx->k2_shadow_budget_mb << 20;
            const uint64_t full = rows_alloc * shadow_pitch(ctx, row_bytes);
            if (full > budget && n_kslices > 8) want = (full + budget - 1) / budget;
        }
        // the strips address a B stage (64 shadow rows) with 32-bit DMA offsets: a chunk's row pitch
        // stays below 2^26 bytes. Rows of more than 2^27 bits are therefore ALWAYS chunked (round 1
        // sent them to the popcount kernel at a fifth of the rate).
        constexpr uint32_t kDmaCapSlices = ((1u << 26) - 1024u) / kStripRowBytes / 8u * 8u;
        want = std::max<uint64_t>(want, ((uint64_t)n_kslices + kDmaCapSlices - 1) / kDmaCapSlices);
        if (want > 1) {
            chunk_slices = (uint32_t)(((uint64_t)n_kslices + want - 1) / want + 7u) / 8u * 8u;
            chunk_slices = std::min(chunk_slices, kDmaCapSlices);
            n_chunks = (n_kslices + chunk_slices - 1) / chunk_slices;
            shadow_row_bytes = (uint64_t)chunk_slices * kStripRowBytes;
        }
    }
    const uint64_t pitch = shadow_pitch(ctx, shadow_row_bytes);
    const size_t x4_bytes = (size_t)rows_alloc * pitch;
    if (n_rows_dst / kTile >= 65535) {
        set_error("K2: too many row blocks");
        return STORM_HIP_EINVAL;
    }
    if (int rc = ensure_shadow(ctx, x4_bytes, "K2: the FP4 shadow matrix")) return rc;
    const uint32_t total_stages = (uint32_t)(row_bytes / kStageBytes);
    if (strips) {
        ctx->items.forget();  // the strip items carry the diagonal tiles themselves: no sum-mode items
    } else if (int rc = ensure_items(ctx, ranges, total_stages, shard_rank, shard_count, false)) {
        return rc;
    }
    if (pitch * (uint64_t)(strips ? kStripBRows : kTile) >= (1ull << 32)) {
        set_error("K2: rows of %llu nibble bytes exceed the 32-bit DMA offsets; use variant 2",
                  (unsigned long long)shadow_row_bytes);
        return STORM_HIP_EINVAL;
    }
    if (strips)
        if (int rc = ensure_strip_items(ctx, ranges, chunk_slices, shard_rank, shard_count, a_tile))
            return rc;
    // accumulators are f32: a k-slice must stay below 2^24 bits
    if ((uint64_t)ctx->k2_stages_per_item * 128u >= (1u << 24)) {
        set_error("K2: k-slice too long for exact f32 accumulation");
        return STORM_HIP_EINVAL;
    }
    const uint32_t n_strip = strips ? ctx->strips.n : 0;
    const uint32_t n_tiles = ctx->items.n;   // the sum-mode list just ensured, or none
    const uint64_t key[4] = {(uint64_t)(uintptr_t)X, shadow_generation,
                             ((uint64_t)shard_rank << 32) | shard_count,
                             (pitch << 20) ^ (n_rows_dst << 2) ^ (uint64_t)strip_mode};
    const bool shadow_valid = ctx->keep_shadow && shadow_generation != 0 && n_chunks == 1 &&
                              !memcmp(key, ctx->x4_key, sizeof(key)) &&
                              (ctx->k2_debug >> 8) == 0;
    // what this shard expands: its own k-slices + the leftover slices (strips; within a chunk
    // the rule runs over the chunk's own slice numbers, as its work list does), or its own
    // k-groups (tile kernel)
    const ExpandOwn own = strips ? ExpandOwn{shard_rank, shard_count, 5u,
                                             ctx->k2_shard_pairs ? 0u   // pair-space ownership: every shard expands every column
                                                                 : strip_modulo_slices(chunk_slices, shard_count) / kOwnSlices}
                                 : ExpandOwn{shard_rank, shard_count, 7u, 0xffffffffu};
    const uint32_t nib = (ctx->k2_debug >> 8) ? (uint32_t)(ctx->k2_debug >> 8) & 15u : 2u;
    const uint64_t n_src = std::min(n_rows_src, n_rows_dst);
    for (uint32_t chunk = 0; chunk < n_chunks && (n_tiles > 0 || n_strip > 0); ++chunk) {
        if (!shadow_valid) {
            if (n_chunks == 1) {
                hipLaunchKernelGGL(expand_fp4_kernel,
                                   expand_grid(n_rows_dst, stride_words, expand_compact_halves(own, stride_words * 2)),
                                   dim3(256), 0, ctx->stream, X, stride_words, n_src, n_rows_dst,
                                   reinterpret_cast<uint4*>(ctx->d_x4.d), own, nib, pitch / 16);
            } else {
                const uint64_t h0 = (uint64_t)chunk * chunk_slices * 8u, h1 = h0 + (uint64_t)chunk_slices * 8u;
                hipLaunchKernelGGL(expand_fp4_kernel,
                                   expand_grid(n_rows_dst, stride_words, expand_compact_halves(own, h1 - h0)),
                                   dim3(256), 0, ctx->stream, X, stride_words, n_src, n_rows_dst,
                                   reinterpret_cast<uint4*>(ctx->d_x4.d), own, nib, pitch / 16, h0, h1, h0);
            }
        }
        STORM_HIP_TRY(hipGetLastError());
        if (n_chunks == 1) memcpy(ctx->x4_key, key, sizeof(key));
        else memset(ctx->x4_key, 0, sizeof(ctx->x4_key));
        if (n_strip > 0) {
            kernel_time_mark(ctx);
            const StripItem* sit = ctx->strips.d;
            const dim3 sgrid(n_strip), sblock(kStripThreads);
#ifdef STORM_HIP_PROBES   // the other forms of the strips (ring depths, 32x32x64, wide, persistent, timing probes, trace): tools build
            StripQueues queues;
            memcpy(queues.base, ctx->strips.queue_base, sizeof(queues.base));
            memcpy(queues.count, ctx->strips.queue_count, sizeof(queues.count));
            unsigned int* heads = reinterpret_cast<unsigned int*>(ctx->d_slots + kSlots);
            // persistent form: one workgroup per resident slot
            const dim3 pgrid(std::min<uint32_t>(n_strip, (uint32_t)ctx->n_cus * (strip_mode == 2 ? 2u : 4u)));
            // (the persistent form's queue heads are re-zeroed by the fold at the END of a pass: a
            //  k-chunked pass launches the strips several times in front of it, so it runs the plain
            //  form — found by the randomised soak, a second chunk saw exhausted queues)
            const bool persist = ctx->k2_persistent && n_chunks == 1;
            const int sel = strip_mode == 2 ? 100 + ctx->k2_ring
                                            : (persist && ctx->k2_ring == 4) ? 204
                                            : (persist && ctx->k2_ring == 18) ? 218
                                                                              : ctx->k2_ring;
            switch (sel) {  // ring depth: tuning probe
#include "../../tools/probes/strip_fp4_32_launch.hip"
                default:
                    if (ctx->k2_shape != 16)
                        hipLaunchKernelGGL(strip_fp4_kernel<kStripRingDefault>, sgrid, sblock,
                                           (size_t)ctx->k2_lds_pad, ctx->stream, ctx->d_x4, pitch, sit,
                                           ctx->d_slots);
                    else
                        hipLaunchKernelGGL(strip16_fp4_kernel<kStripRingDefault>, sgrid, sblock,
                                           (size_t)ctx->k2_lds_pad, ctx->stream, ctx->d_x4, pitch, sit,
                                           ctx->d_slots);
                    break;
            }
#else   // (the shipped library refuses the options that select the other forms)
            // k2_lds_pad: unused dynamic LDS, only to cap the workgroups per CU (tuning)
            hipLaunchKernelGGL(strip16_fp4_kernel<kStripRingDefault>, sgrid, sblock, (size_t)ctx->k2_lds_pad, ctx->stream,
                               ctx->d_x4, pitch, sit, ctx->d_slots);
#endif
            kernel_time_mark(ctx);
            STORM_HIP_TRY(hipGetLastError());
        }
        if (n_tiles > 0) {
            kernel_time_mark(ctx);
            const dim3 kgrid(n_tiles), block(kMfmaThreads);
            const MfmaItem* items = static_cast<const MfmaItem*>(ctx->items.recs());
            switch (ctx->k2_debug & 12) {  // 4 / 8: timing probes without DMA / without MFMA
#ifdef STORM_HIP_PROBES
                case 4:
                    hipLaunchKernelGGL(pairw_fp4_kernel<4>, kgrid, block, 0, ctx->stream, ctx->d_x4,
                                       pitch, items, ctx->d_slots);
                    break;
                case 8:
                    hipLaunchKernelGGL(pairw_fp4_kernel<8>, kgrid, block, 0, ctx->stream, ctx->d_x4,
                                       pitch, items, ctx->d_slots);
                    break;
#endif
                default:
                    hipLaunchKernelGGL(pairw_fp4_kernel<0>, kgrid, block, 0, ctx->stream, ctx->d_x4,
                                       pitch, items, ctx->d_slots);
                    break;
            }
            kernel_time_mark(ctx);
            STORM_HIP_TRY(hipGetLastError());
        }
    }
    if (n_tiles + n_strip > 0) {
        ctx->pass_report[0] |= strips ? STORM_HIP_RAN_FP4_STRIPS : STORM_HIP_RAN_FP4_TILES;
        ctx->pass_report[1] += ranges_word_pairs(ranges, n_words_logical ? n_words_logical : stride_words, shard_count);
    }
    ctx->last_info[0] = n_tiles + n_strip;
    ctx->last_info[1] = ctx->k2_stages_per_item;
    ctx->last_info[2] = n_chunks;
    ctx->last_info[3] = 0;
    return launch_fold_slots(ctx, d_total);
}

// Rectangular sum_{i in A, j in B} popcount(a_i & b_j) (STORM_wrapper_square, storm.c:153-171,
// with the reference's missing offset2 reset fixed) on the strip kernel: the FP4 shadow holds
// [A ; B], each padded to a multiple of 256 rows, and every A tile walks all of B's 64-row
// blocks with no diagonal phase.
int launch_square_mfma(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a,
                       const storm_hip_matrix_s* b, uint64_t* d_total) {
    const uint64_t stride_words = a->stride_words;
    const uint64_t row_bytes = stride_words * 32;
    const uint64_t pitch = shadow_pitch(ctx, row_bytes);
    const uint64_t rows_a = (a->n_rows + kStripATile - 1) / kStripATile * kStripATile;
    const uint64_t rows_b = (b->n_rows + kStripATile - 1) / kStripATile * kStripATile;
    const size_t x4_bytes = (size_t)(rows_a + rows_b) * pitch;
    if (pitch * (uint64_t)kStripBRows >= (1ull << 32) || (rows_a + rows_b) >= (1ull << 31)) {
        set_error("square (matrix cores): operand too large for the strip kernel's 32-bit offsets");
        return STORM_HIP_EINVAL;
    }
    if (int rc = ensure_shadow(ctx, x4_bytes, "square: the FP4 shadow")) return rc;
    memset(ctx->x4_key, 0, sizeof(ctx->x4_key));  // the shadow is about to hold [A ; B]
    const uint32_t n_kslices = (uint32_t)(row_bytes / kStripRowBytes);
    const uint32_t kMaxRun = (uint32_t)std::min(4096, ctx->k2_max_run > 0 ? ctx->k2_max_run : 128);   // (0 = auto: the rectangle has no tail problem)
    const uint32_t jb0 = (uint32_t)(rows_a / kStripBRows);
    const uint32_t jb1 = jb0 + (uint32_t)((b->n_rows + kStripBRows - 1) / kStripBRows);
    std::vector<StripItem> items;
    for (uint32_t ks = 0; ks < n_kslices; ++ks)
        for (uint32_t a_row0 = 0; a_row0 < a->n_rows; a_row0 += (uint32_t)kStripATile)
            for (uint32_t j0 = jb0; j0 < jb1; j0 += kMaxRun)
                items.push_back({a_row0, 0u, j0, std::min(jb1, j0 + kMaxRun), ks});
    if (items.size() >= (1ull << 31)) {
        set_error("square: %zu strip items exceed the grid limit", items.size());
        return STORM_HIP_EINVAL;
    }
    // (no key: the cached all-pairs list is gone and nobody asks for this one again)
    if (int rc = ctx->strips.put(ctx, std::nullopt, items.data(), items.size(), "square: the strip items", kStripItemsFloorBytes)) return rc;
    for (int side = 0; side < 2; ++side) {
        const storm_hip_matrix_s* m = side ? b : a;
        const uint64_t rows_dst = side ? rows_b : rows_a;
        const dim3 grid = expand_grid(rows_dst, stride_words);
        hipLaunchKernelGGL(expand_fp4_kernel, grid, dim3(256), 0, ctx->stream, m->d,
                           stride_words, std::min<uint64_t>(m->n_rows_pad, rows_dst), rows_dst,
                           reinterpret_cast<uint4*>(ctx->d_x4.d + (side ? rows_a * pitch : 0)),
                           kExpandAll, 2u, pitch / 16);
        STORM_HIP_TRY(hipGetLastError());
    }
#ifdef STORM_HIP_PROBES
    if (ctx->k2_shape != 16)
        hipLaunchKernelGGL(strip_fp4_kernel<kStripRingDefault>, dim3((uint32_t)items.size()),
                           dim3(kStripThreads), 0, ctx->stream, ctx->d_x4, pitch,
                           ctx->strips.recs(), ctx->d_slots);
    else
#endif
        hipLaunchKernelGGL(strip16_fp4_kernel<kStripRingDefault>, dim3((uint32_t)items.size()),
                           dim3(kStripThreads), 0, ctx->stream, ctx->d_x4, pitch,
                           ctx->strips.recs(), ctx->d_slots);
    STORM_HIP_TRY(hipGetLastError());
    ctx->last_info[0] = (uint32_t)items.size();
    return launch_fold_slots(ctx, d_total);
}

// Per-row set-bit counts for the OR / XOR epilogues: a scratch buffer kept in the context.
static int ensure_counts_scratch(storm_hip_ctx_t* ctx, size_t n, uint32_t** out) {
    if (int rc = ctx->d_counts.ensure(n * sizeof(uint32_t), "matrix output: the row-count scratch")) return rc;
    *out = ctx->d_counts;
    return STORM_HIP_OK;
}

// Clears the output window of the tiles whose k range is split over several items (same write
// predicate as pairw_fp4_kernel<., true>). Grid (cut tile, band of 16 rows), thread = column. (Until round 5 the grid ran over
// the PARTS and all but the first part of a tile returned at once: 2560 workgroups for 10 windows at 1024 rows, 8 us.)
__global__ __launch_bounds__(256) void zero_tiles_kernel(const MfmaItem* __restrict__ items, uint32_t first, OutWindow window) {
    const OutWindow w = window.loaded();
    const MfmaItem it = items[first + blockIdx.x];   // `first`: where the records of the cut tiles begin (behind all items)
    const uint32_t j = (uint32_t)it.J * kTile + threadIdx.x;
    if (!w.wants_col(j)) return;
    // blockIdx.y: band of 16 rows (one workgroup per tile took 16 us for the 92 windows of the
    // headline call: a serial walk down 256 rows)
    for (uint32_t r = blockIdx.y * 16u; r < blockIdx.y * 16u + 16u; ++r) {
        const uint32_t i = (uint32_t)it.I * kTile + r;
        if (w.writes_row(i, j)) *w.at(i, j) = 0;
    }
}

// [r5] Adds up the windows the k-parts of a tile wrote into `parts` (tilebits8_kernel / tilering_kernel with parts != nullptr)
// and writes the tile's counts — same write predicate as the tile kernels, OR / XOR from the row counts. Grid (k-part item,
// band of kReduceBand rows), thread = column; the tile's first part does the work, its parts follow it in the item list.
constexpr uint32_t kReduceBand = 2;   // rows per workgroup of reduce_parts_kernel
__global__ __launch_bounds__(256) void reduce_parts_kernel(const MfmaItem* __restrict__ items, uint32_t first, uint32_t n_items,
                                                           const uint32_t* __restrict__ parts, OutWindow window) {
    const OutWindow w = window.loaded();
    const uint32_t k = first + blockIdx.x;
    const MfmaItem it = items[k];
    if (it.stage0 != 0) return;
    uint32_t n_parts = 1;
    while (k + n_parts < n_items && items[k + n_parts].stage0 != 0) ++n_parts;   // (a tile's parts: stage0 ascending from 0)
    const uint32_t j = (uint32_t)it.J * kTile + threadIdx.x;
    if (!w.wants_col(j)) return;
    const uint32_t nj = w.nj(j);
    const uint32_t* src = parts + (uint64_t)blockIdx.x * (kTile * kTile) + threadIdx.x;
    // blockIdx.y: band of kReduceBand rows; the parts' loads of a row are independent: eight in flight
    for (uint32_t r = blockIdx.y * kReduceBand; r < blockIdx.y * kReduceBand + kReduceBand; ++r) {
        const uint32_t i = (uint32_t)it.I * kTile + r;
        if (w.writes_row(i, j)) {
            uint32_t c = 0;
            const uint32_t* row = src + r * (uint32_t)kTile;
            uint32_t p = 0;
            for (; p + 8u <= n_parts; p += 8u) {
                uint32_t v[8];
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) v[q] = row[(uint64_t)(p + q) * (kTile * kTile)];
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q) c += v[q];
            }
            for (; p < n_parts; ++p) c += row[(uint64_t)p * (kTile * kTile)];
            *w.at(i, j) = w.value(c, i, nj);
        }
    }
}

// Plans (plan_matrix_tiles, storm_hip_plan.cpp) and uploads the item table of a matrix-output launch, before the caller
// launches anything else, so that the one host wait for the pageable upload does not sit between the kernels.
// The table of the previous call is still on the device when this call asks for the same tiles cut the same way (a
// repeated call, the bands of one output): no upload, and no host wait in front of the kernels.
static int ensure_matrix_tiles(storm_hip_ctx_t* ctx, MatrixTilesRequest&& rq, MatrixPlan* plan) {
    rq.n_cus = (uint32_t)std::max(1, ctx->n_cus);
    rq.split = ctx->k2_matrix_split;
    rq.min_part = ctx->k2_matrix_min_part;
    if (ctx->items.holds(rq)) {
        *plan = ctx->items.matrix_plan;
        return STORM_HIP_OK;
    }
    std::vector<MfmaItem> items;
    plan_matrix_tiles(rq, items, plan);
    // the context's item buffer (shared with the tile kernel's sum mode and K2h, whose cached list is dropped here);
    // hipMalloc / hipFree per call would cost more than the kernel's tail
    ctx->items.matrix_plan = *plan;
    return ctx->items.put(ctx, std::move(rq), items.data(), items.size(), "matrix output: the item table", kItemsFloorBytes);
}

// Runs the 256 x 256 tile kernel that k2_tile_shape_eff names over the planned items, into the window w. `bits` (the
// default): the operands are the matrix rows themselves; otherwise (the FP4 forms) ops is the shadow, as one matrix, that
// the caller has just expanded in the tile layout. The kernel holds one workgroup per CU, so n tiles take ceil(n / CUs)
// rounds and a nearly empty last round costs a whole one (820 tiles on 256 CUs at the headline shape: 3.2 -> 4). The
// tiles of the last round are therefore cut along k into as many parts as fill the CUs; the parts add into a cleared
// window (or, option k2_matrix_parts, write windows of their own that reduce_parts_kernel adds up).
static int run_matrix_tiles(storm_hip_ctx_t* ctx, const MatrixPlan& plan, const TileOperands& ops, bool bits, const OutWindow& w) {
    if (!bits) memset(ctx->x4_key, 0, sizeof(ctx->x4_key));  // callers rebuilt the shadow in the tile layout
    const MfmaItem* d_items = static_cast<const MfmaItem*>(ctx->items.recs());
    // [r5] option k2_matrix_parts: the k-parts of the tile kernels that ship write their own windows and a second kernel
    // adds them up (no clearing, no atomics); otherwise — and for the other forms, and for part lists beyond 1 GiB of
    // windows — the parts add into the cleared output
    const uint32_t n_split = plan.n_items - plan.n_full;
    uint32_t* d_parts = nullptr;
    if (n_split && bits && (ctx->k2_tile_shape_eff == 2 || ctx->k2_tile_shape_eff == 5) && ctx->k2_matrix_parts &&
        (size_t)n_split * kTile * kTile * sizeof(uint32_t) <= ((size_t)1 << 30)) {
        const size_t need = (size_t)n_split * kTile * kTile * sizeof(uint32_t);
        if (ctx->d_parts.ensure(need, "matrix output: the k-parts' windows") == STORM_HIP_OK)
            d_parts = ctx->d_parts;   // (no memory for the windows: the atomics still work)
    }
    if (n_split && !d_parts)
        hipLaunchKernelGGL(zero_tiles_kernel, dim3(plan.n_cut, kTile / 16), dim3(256), 0, ctx->stream, d_items, plan.n_items, w);
    if (bits && ctx->k2_tile_shape_eff == 3 && timing_env()) {
        int nb = -1;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, tile16_bits_kernel, kTiThreads, kTiLdsBytes);
        fprintf(stderr, "[tile16_bits_kernel] workgroups per CU by the runtime's occupancy query: %d (LDS %u B)\n", nb, kTiLdsBytes);
    }
    if (bits && ctx->k2_tile_shape_eff == 3)
        hipLaunchKernelGGL(tile16_bits_kernel, dim3((plan.n_items + 7u) / 8u * 16u), dim3(kTiThreads), kTiLdsBytes, ctx->stream,
                           ops, d_items, plan.n_items, w, plan.n_full);
    else if (bits && ctx->k2_tile_shape_eff == 4)
        hipLaunchKernelGGL(tile32_bits_kernel, dim3((plan.n_items + 7u) / 8u * 16u), dim3(kTiThreads), kTiLdsBytes, ctx->stream,
                           ops, d_items, plan.n_items, w, plan.n_full);
    else if (bits && ctx->k2_tile_shape_eff == 5 && ctx->k2_ring_sync == 0)
        hipLaunchKernelGGL(tilering_kernel<false>, dim3(plan.n_items), dim3(kTrThreads), 0, ctx->stream, ops, d_items, w,
                           plan.n_full, d_parts);
    else if (bits && ctx->k2_tile_shape_eff == 5)
        hipLaunchKernelGGL(tilering_kernel<true>, dim3(plan.n_items), dim3(kTrThreads), 0, ctx->stream, ops, d_items, w,
                           plan.n_full, d_parts);
    else if (bits && ctx->k2_tile_shape_eff == 2)
        hipLaunchKernelGGL(tilebits8_kernel, dim3(plan.n_items), dim3(kMfmaThreads), 0, ctx->stream, ops, d_items, w,
                           plan.n_full, d_parts);
#ifdef STORM_HIP_PROBES
    else if (bits)
        hipLaunchKernelGGL(tilebits_kernel, dim3(plan.n_items), dim3(kTbThreads), 0, ctx->stream, ops, d_items, w, plan.n_full);
    else if (ctx->k2_tile_shape_eff == 16)
        hipLaunchKernelGGL(tile16_fp4_kernel, dim3(plan.n_items), dim3(kMfmaThreads), 0, ctx->stream, ops.xa, ops.pitch, d_items,
                           w, plan.n_full);
#endif
    else
        hipLaunchKernelGGL((pairw_fp4_kernel<0, true>), dim3(plan.n_items), dim3(kMfmaThreads), 0, ctx->stream, ops.xa, ops.pitch,
                           d_items, ctx->d_slots, w, plan.n_full);
    if (d_parts)
        hipLaunchKernelGGL(reduce_parts_kernel, dim3(n_split, kTile / kReduceBand), dim3(256), 0, ctx->stream, d_items, plan.n_full,
                           plan.n_items, d_parts, w);
    return hipGetLastError() == hipSuccess ? STORM_HIP_OK : STORM_HIP_EHIP;
}

// ---- what the materialised-output entry points share ----
// The limits of the tile kernels, under the entry point's name: 32-bit DMA offsets within a tile of `tile_rows` rows, and
// 16-bit row-block numbers in the item records. pitch_first: which of the two a call that exceeds both reports (each entry
// point keeps the order it had).
static int check_tile_limits(const char* entry, uint64_t pitch, uint64_t tile_rows, uint64_t row_blocks, bool pitch_first) {
    const bool blocks_bad = row_blocks > 65535u;
    const bool pitch_bad = pitch * tile_rows >= (1ull << 32);  // FP4 shadow: rows of 2^25 bits; bit operands: 2^27
    if (pitch_bad && (pitch_first || !blocks_bad))
        set_error("%s: rows of %llu operand bytes exceed the tile kernel's 32-bit DMA offsets", entry, (unsigned long long)pitch);
    else if (blocks_bad)
        set_error("%s: too many row blocks", entry);
    return pitch_bad || blocks_bad ? STORM_HIP_EINVAL : STORM_HIP_OK;
}

// (a report of its own: the per-pair output is no all-pairs pass)
static void report_tiles_out(storm_hip_ctx_t* ctx, uint64_t word_pairs) {
    ctx->pass_report[0] = STORM_HIP_RAN_TILES_OUT;
    ctx->pass_report[1] = word_pairs;
    ctx->pass_report[2] = ctx->pass_report[3] = 0;
}

// The per-row counts the OR / XOR epilogues need, per virtual row: a's rows and, with b, b's from virtual row rows_a on
// (n virtual rows in all). AND: none, *d_counts = null.
static int op_row_counts(storm_hip_ctx_t* ctx, int op, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint64_t rows_a,
                         uint64_t n, uint32_t** d_counts) {
    *d_counts = nullptr;
    if (op == STORM_HIP_OP_AND) return STORM_HIP_OK;
    int rc = ensure_counts_scratch(ctx, n, d_counts);
    if (rc == STORM_HIP_OK) rc = launch_row_counts(ctx, a, *d_counts);
    if (rc == STORM_HIP_OK && b) rc = launch_row_counts(ctx, b, *d_counts + rows_a);
    return rc;
}
static int op_row_counts(storm_hip_ctx_t* ctx, int op, const storm_hip_matrix_s* m, uint32_t** d_counts) {
    return op_row_counts(ctx, op, m, nullptr, 0, m->n_rows, d_counts);
}

// ---- K2h (tile128_kernel): 128 x 128 tiles for matrices of few 256 x 256 tiles, k-parts whose sums meet inside the launch ----
// Eligible: bit operands, and a 128-row window within the 32-bit buffer offsets. `tiles256` = what the 256 x 256
// decomposition would launch; k2_tile_shape = 6 forces, 0 takes K2h below k2_wave_below tiles.
static bool choose_tile128(const storm_hip_ctx_t* ctx, uint64_t tiles256, uint64_t pitch, bool bits) {
    if (!bits || pitch * 128u >= (1ull << 32)) return false;
    if (ctx->k2_tile_shape == 6) return true;
    return ctx->k2_tile_shape == 0 && tiles256 < (uint64_t)ctx->k2_wave_below;
}

// Plans the K2h list of the 128 x 128 tiles that hold a pair of the window (plan_tile128, storm_hip_plan.cpp; cached by its
// request while the same call repeats), uploads it and launches tile128_kernel in the window's form over total_stages
// 128-bit stages of k. value_bits = 2 (any form, no row counts): the rows hold 2-bit values and the kernel writes their
// dot products (tile128_kernel<false, 2>, or <true, 2> in the lag form); the list is planned with a chunk's weight of 9 x 256.
static int run_tile128(storm_hip_ctx_t* ctx, uint32_t total_stages, const TileOperands& ops, const OutWindow& w, uint32_t value_bits) {
    const uint32_t lag = w.form == OutForm::Lag ? w.lag : 0u;
    const uint32_t ia0 = w.i_lo / kThTile, ia1 = (w.n_rows + kThTile - 1) / kThTile;
    const uint32_t jb0 = w.j_base / kThTile, jb1 = (w.col_end() + kThTile - 1) / kThTile;
    if (int rc = check_tile_limits("pairw_matrix", 0, kThTile, std::max(ia1, jb1), false)) return rc;
    const Tile128Request rq = {ia0, ia1, jb0, jb1, w.rect() ? 0u : 1u, total_stages, (uint32_t)std::max(1, ctx->n_cus),
                               ctx->k2_part_slots, ctx->k2_part_min_chunks, ctx->k2_part_cost_diag,
                               ctx->k2_part_narrow != 0 ? 1u : 0u, lag, value_bits == 2u ? kThWeightDosage : kThWeightBits};
    if (!ctx->items.holds(rq)) {
        Tile128Plan plan;
        plan_tile128(rq, &plan);
        ctx->items.forget();
        // the parts' windows and the tiles' tickets (zero between launches: the part that ends a tile clears its ticket)
        if (int rc = ctx->d_parts.ensure((size_t)plan.n_windows * kThWindowWords * sizeof(uint32_t), "pairw_matrix: the k-parts' windows"))
            return rc;
        if (plan.n_tiles * sizeof(uint32_t) > ctx->d_tickets.capacity || ctx->tickets_dirty) {
            if (int rc = ctx->d_tickets.ensure(plan.n_tiles * sizeof(uint32_t), "pairw_matrix: the tiles' tickets", 4096 * sizeof(uint32_t)))
                return rc;
            STORM_HIP_TRY(hipMemsetAsync(ctx->d_tickets, 0, ctx->d_tickets.capacity, ctx->stream));
            ctx->tickets_dirty = false;
        }
        if (int rc = ctx->items.put(ctx, rq, plan.items.data(), plan.items.size(), "pairw_matrix: the item table", kItemsFloorBytes))
            return rc;
    } else if (ctx->tickets_dirty) {
        STORM_HIP_TRY(hipMemsetAsync(ctx->d_tickets, 0, ctx->d_tickets.capacity, ctx->stream));
        ctx->tickets_dirty = false;
    }
    const PartItem* d_items = static_cast<const PartItem*>(ctx->items.recs());
    const uint32_t n_parts = ctx->items.n;
    if (n_parts && w.form == OutForm::Lag && value_bits == 2u)
        hipLaunchKernelGGL((tile128_kernel<true, 2>), dim3(n_parts), dim3(kThThreads), 0, ctx->stream, ops, d_items, w,
                           ctx->d_parts, ctx->d_tickets);
    else if (n_parts && w.form == OutForm::Lag)
        hipLaunchKernelGGL(tile128_kernel<true>, dim3(n_parts), dim3(kThThreads), 0, ctx->stream, ops, d_items, w,
                           ctx->d_parts, ctx->d_tickets);
    else if (n_parts && value_bits == 2u)
        hipLaunchKernelGGL((tile128_kernel<false, 2>), dim3(n_parts), dim3(kThThreads), 0, ctx->stream, ops, d_items, w,
                           ctx->d_parts, ctx->d_tickets);
    else if (n_parts)
        hipLaunchKernelGGL(tile128_kernel<false>, dim3(n_parts), dim3(kThThreads), 0, ctx->stream, ops, d_items, w,
                           ctx->d_parts, ctx->d_tickets);
    if (hipGetLastError() != hipSuccess) {
        ctx->tickets_dirty = true;
        return STORM_HIP_EHIP;
    }
    return STORM_HIP_OK;   // (a failed wait marks the tickets as well: pair_matrix_out, storm_hip_internal.h)
}

// Materialised upper triangle: out[i * ld + j] = popcount(row_i & row_j) for i < j < n_rows
// (device pointer, uint32). One tile item per (I <= J) spanning all of k; f32 accumulation is
// exact for rows of fewer than 2^24 bits.
int launch_pairw_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int op, uint32_t* d_out,
                        uint64_t ld, uint64_t band_row0, uint64_t band_rows) {
    // band: only rows [band_row0, band_row0 + band_rows) of the triangle, written from output row 0
    const uint64_t band_end = std::min<uint64_t>(m->n_rows, band_row0 + band_rows);
    if (band_row0 >= band_end) return STORM_HIP_OK;
    ctx->k2_tile_shape_eff = (ctx->k2_tile_shape && ctx->k2_tile_shape != 6) ? ctx->k2_tile_shape : (m->sparse_origin ? 2 : 5);   // (6 = K2w, chosen below; not eligible: as 0)
    report_tiles_out(ctx, m->n_rows * (m->n_rows - (m->n_rows != 0)) / 2 * m->n_words);
    if (m->n_rows < 2) return STORM_HIP_OK;
    const uint64_t n_rows4 = (m->n_rows + kStripATile - 1) / kStripATile * kStripATile;
    const uint64_t row_bytes = m->stride_words * 32;
    // bit-operand kernel: the operands are the matrix rows themselves (no shadow, no expansion)
    const bool bits = ctx->k2_tile_shape_eff <= 5;
    const uint64_t pitch = bits ? m->stride_words * 8 : shadow_pitch(ctx, row_bytes);
    const size_t x4_bytes = bits ? 0 : (size_t)n_rows4 * pitch;
    if (int rc = check_tile_limits("pairw_matrix", pitch, kTile, n_rows4 / kTile + 1, false)) return rc;
    if (int rc = ensure_shadow(ctx, x4_bytes, "pairw_matrix: the FP4 shadow")) return rc;
    // stages of 128 bits; the bit kernels walk whole 512-bit chunks that hold DATA (the pitch's pad chunks — 8 of 136 at
    // the headline shape since round 4's pitch pad — are never multiplied)
    const uint32_t total_stages = bits ? (m->n_words + 7u) / 8u * 4u : (uint32_t)(row_bytes / kStageBytes);
    const uint32_t nT = (uint32_t)((m->n_rows + kTile - 1) / kTile);
    // [r6] few tiles: 128 x 128 tiles, cut along k where they are too few, the parts' sums meeting inside the launch
    // (tile128_kernel) instead of k-parts of 256 x 256 tiles that clear and atomically add into the output
    const uint64_t band_tiles = (uint64_t)((band_end + kTile - 1) / kTile - band_row0 / kTile);
    const uint64_t tiles256 = band_tiles * nT - (band_row0 / kTile) * band_tiles - band_tiles * (band_tiles - 1) / 2;
    const bool k2h = choose_tile128(ctx, tiles256, pitch, bits);
    int rc = STORM_HIP_OK;
    MatrixPlan plan;
    if (k2h) {
        ctx->k2_tile_shape_eff = 6;
    } else {
        // off-diagonal tiles first; the diagonal ones (half of their window is written) go last,
        // where run_matrix_tiles may cut them along k
        MatrixTilesRequest rq;
        rq.total_stages = total_stages;
        std::vector<std::pair<uint16_t, uint16_t>>& tiles = rq.tiles;
        const uint32_t t_lo = (uint32_t)(band_row0 / kTile), t_hi = (uint32_t)((band_end + kTile - 1) / kTile);
        // ... and last of all the tiles of a ragged last row block (few valid columns): with
        // tilebits8_kernel both kinds are short items, and the k-split of the last round then works on
        // the shortest ones
        const bool ragged = m->n_rows % kTile != 0 && m->n_rows % kTile <= 192 && nT > 1;
        const uint32_t nT_full = ragged ? nT - 1 : nT;
        xcd_grouped_tiles(t_lo, std::min(t_hi, nT_full), 0, nT_full, true, tiles);
        for (uint32_t i = t_lo; i < std::min(t_hi, nT_full); ++i) tiles.emplace_back((uint16_t)i, (uint16_t)i);
        if (ragged)
            for (uint32_t i = t_lo; i < t_hi; ++i) tiles.emplace_back((uint16_t)i, (uint16_t)(nT - 1));
        // what a tile costs next to a full one under tilebits8_kernel: a diagonal tile multiplies 5 of its
        // 8 block pairs per SIMD; a ragged one ceil(columns / 64) of 4 blocks per wave, but not below the
        // inflation work of its A operands (measured: 0.3)
        std::vector<float>& cost = rq.cost;
        if (ctx->k2_tile_shape_eff >= 2 && ctx->k2_tile_shape_eff <= 5) {
            // (tilering_kernel: a diagonal tile keeps its busiest SIMD at 12 of 16 block rows; a ragged column multiplies one
            //  block column in two of the eight waves but stores all of its images: options k2_ring_cost_*)
            const bool ring = ctx->k2_tile_shape_eff == 5;
            const float ragged_cost = ring ? std::max(ctx->k2_ring_cost_ragged / 100.0f, m->n_rows % kTile > 16 ? 1.0f : 0.0f)
                                           : std::max(ctx->k2_tile_cost_ragged / 100.0f, (float)((m->n_rows % kTile + 63) / 64) / 4.0f);
            for (const auto& t : tiles) {
                float c = t.first == t.second ? (ring ? ctx->k2_ring_cost_diag : ctx->k2_tile_cost_diag) / 100.0f : 1.0f;
                if (ragged && t.second == nT - 1) c *= ragged_cost;
                cost.push_back(c);
            }
        }
        rc = ensure_matrix_tiles(ctx, std::move(rq), &plan);
    }
    uint32_t* d_counts = nullptr;
    if (rc == STORM_HIP_OK) rc = op_row_counts(ctx, op, m, &d_counts);
    if (rc == STORM_HIP_OK) {
        // rows [band_row0, band_end) are written; the columns run over the whole matrix
        const OutWindow w = triangle_window(d_out, ld, band_row0, band_end, m->n_rows, d_counts, op);
        if (!bits) {
            const dim3 grid = expand_grid(n_rows4, m->stride_words);
            hipLaunchKernelGGL(expand_fp4_kernel, grid, dim3(256), 0, ctx->stream, m->d,
                               m->stride_words, std::min<uint64_t>(m->n_rows_pad, n_rows4), n_rows4,
                               reinterpret_cast<uint4*>(ctx->d_x4.d), kExpandAll, 2u, pitch / 16);
        }
        const TileOperands ops = bits ? operands_of(m->d, pitch, m->n_rows_pad) : operands_of(ctx->d_x4.d, pitch, n_rows4);
        rc = k2h ? run_tile128(ctx, total_stages, ops, w, 1u) : run_matrix_tiles(ctx, plan, ops, bits, w);
    }
    if (rc == STORM_HIP_EHIP) set_error("pairw_matrix: HIP failure");
    return rc;
}

// ---- the calls that have K2h alone: the lag layout and the rows of 2-bit values (the other output kernels know neither) ----
// the pairs within L rows of each other among the rows [0, r) of n: row i has min(L, n - 1 - i) of them (L = n - 1: all pairs)
static uint64_t pairs_below(uint64_t r, uint64_t n, uint64_t L) {
    const uint64_t full = std::min(r, n - L);            // rows with all L partners
    const uint64_t rest = r - full;                      // rows n - L + t, t < rest: L - t partners
    return full * L + rest * L - rest * (rest + 1) / 2;
}

// tile128_kernel over one matrix (b null) or over [A ; B] (B's virtual rows count on from w.j_base: A's rows padded to 256;
// equal n_words and strides) into the finished window w, under the entry point's name: the limits, what the call ran
// (k2_tile_shape_used: 6 = K2h on bits, 7 = on 2-bit values, value_bits 2), the report of the window's pairs, the rows'
// counts for `op` (one matrix; the dot products are AND: none), the launch. Queued.
static int launch_tile128(storm_hip_ctx_t* ctx, const char* entry, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, OutWindow w,
                          uint32_t value_bits, int op) {
    const uint64_t pitch = a->stride_words * 8, rows_a = b ? w.j_base : 0;
    if (int rc = check_tile_limits(entry, pitch, kThTile, (rows_a + (b ? b : a)->n_rows + kThTile - 1) / kThTile, true)) return rc;
    const uint64_t L = w.form == OutForm::Lag ? w.lag : w.n_cols - 1;   // (a triangle: every pair)
    const uint64_t pairs = w.rect() ? (uint64_t)w.n_rows * w.j_count : pairs_below(w.n_rows, w.n_cols, L) - pairs_below(w.i_lo, w.n_cols, L);
    ctx->k2_tile_shape_eff = value_bits == 2u ? 7 : 6;
    report_tiles_out(ctx, pairs * a->n_words);
    uint32_t* d_counts = nullptr;
    int rc = op_row_counts(ctx, op, a, &d_counts);
    w.row_counts = d_counts;
    const TileOperands ops = b ? operands_of(a->d, b->d, pitch, rows_a, std::min<uint64_t>(a->n_rows_pad, rows_a),
                                             std::min<uint64_t>(b->n_rows_pad, (b->n_rows + kThTile - 1) / kThTile * kThTile))
                               : operands_of(a->d, pitch, a->n_rows_pad);
    if (rc == STORM_HIP_OK) rc = run_tile128(ctx, (a->n_words + 7u) / 8u * 4u, ops, w, value_bits);
    if (rc == STORM_HIP_EHIP) set_error("%s: HIP failure", entry);
    return rc;
}

// The triangle's pairs within max_lag rows of each other, in the lag layout: out[(i - band_row0) * ld + (j - i - 1)] =
// popcount(row_i OP row_j) for band_row0 <= i < band_row0 + band_rows, i < j < n_rows, j - i <= L = min(max_lag, n_rows - 1)
// (device pointer, uint32, ld >= L); value_bits 2: sum_s v_i[s] v_j[s] of rows of 2-bit values instead. The tile list follows
// the diagonal; nothing outside the layout is written.
static int launch_lag(storm_hip_ctx_t* ctx, const char* entry, const storm_hip_matrix_s* m, int op, uint64_t max_lag, uint64_t band_row0,
                      uint64_t band_rows, uint32_t* d_out, uint64_t ld, uint32_t value_bits) {
    const uint64_t n = m->n_rows;
    const uint64_t band_end = std::min<uint64_t>(n, band_row0 + std::min<uint64_t>(band_rows, n));
    if (n < 2 || band_row0 >= band_end || max_lag == 0) return STORM_HIP_OK;
    return launch_tile128(ctx, entry, m, nullptr, lag_window(d_out, ld, band_row0, band_end, n, std::min<uint64_t>(max_lag, n - 1), nullptr, op),
                          value_bits, op);
}
int launch_pairw_lag_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int op, uint64_t max_lag, uint64_t band_row0,
                            uint64_t band_rows, uint32_t* d_out, uint64_t ld) {
    return launch_lag(ctx, "pairw_lag_matrix", m, op, max_lag, band_row0, band_rows, d_out, ld, 1u);
}
int launch_pairw_lag_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t max_lag, uint64_t band_row0,
                                   uint64_t band_rows, uint32_t* d_out, uint64_t ld) {
    return launch_lag(ctx, "pairw_lag_dosage_matrix", m, STORM_HIP_OP_AND, max_lag, band_row0, band_rows, d_out, ld, 2u);
}

// The dot products of rows of 2-bit values (storm_hip_pairw_dosage_matrix_device): out[i * ld + j] = sum_s v_i[s] v_j[s] for
// i < j < n_rows, value s of a row in bits 2 (s % 32), 2 (s % 32) + 1 of word s / 32 (device pointer, uint32).
int launch_pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint32_t* d_out, uint64_t ld) {
    const uint64_t n = m->n_rows;
    if (n < 2) return STORM_HIP_OK;
    return launch_tile128(ctx, "pairw_dosage_matrix", m, nullptr, triangle_window(d_out, ld, 0, n, n, nullptr, STORM_HIP_OP_AND), 2u,
                          STORM_HIP_OP_AND);
}

// The rectangle of two matrices of rows of 2-bit values (storm_hip_square_dosage_matrix_device): out[i * ld + j] =
// sum_s a_i[s] b_j[s] for every row i of A and j of B (device pointer, uint32, ld >= b->n_rows; equal n_words and strides).
int launch_square_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint32_t* d_out,
                                uint64_t ld) {
    if (a->n_rows == 0 || b->n_rows == 0) return STORM_HIP_OK;
    if (a->stride_words != b->stride_words || a->n_words != b->n_words) {
        set_error("square_dosage_matrix: rows of %u and %u words", a->n_words, b->n_words);
        return STORM_HIP_EINVAL;
    }
    const uint64_t rows_a = (a->n_rows + kTile - 1) / kTile * kTile;
    return launch_tile128(ctx, "square_dosage_matrix", a, b, rectangle_window(d_out, ld, a->n_rows, rows_a, b->n_rows, nullptr, STORM_HIP_OP_AND),
                          2u, STORM_HIP_OP_AND);
}

// Materialised rectangle: out[i * ld + j] = popcount(a_i OP b_j) for every row i of A and j of B
// (device pointer, uint32, ld >= b->n_rows): the tile kernel over the virtual rows [A ; B] (FP4 forms: a shadow holding them).
int launch_square_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a,
                         const storm_hip_matrix_s* b, int op, uint32_t* d_out, uint64_t ld) {
    if (a->n_rows == 0 || b->n_rows == 0) return STORM_HIP_OK;
    ctx->k2_tile_shape_eff = (ctx->k2_tile_shape && ctx->k2_tile_shape != 6) ? ctx->k2_tile_shape : ((a->sparse_origin && b->sparse_origin) ? 2 : 5);
    const uint64_t stride_words = a->stride_words;
    const uint64_t row_bytes = stride_words * 32;
    const bool bits = ctx->k2_tile_shape_eff <= 5 && b->stride_words == stride_words;
    const uint64_t pitch = bits ? stride_words * 8 : shadow_pitch(ctx, row_bytes);
    const uint64_t rows_a = (a->n_rows + kTile - 1) / kTile * kTile;
    const uint64_t rows_b = (b->n_rows + kTile - 1) / kTile * kTile;
    if (int rc = check_tile_limits("square_matrix", pitch, kTile, (rows_a + rows_b) / kTile + 1, false)) return rc;
    const size_t x4_bytes = bits ? 0 : (size_t)(rows_a + rows_b) * pitch;
    if (int rc = ensure_shadow(ctx, x4_bytes, "square_matrix: the FP4 shadow")) return rc;
    // (bit kernels: whole 512-bit chunks that hold DATA; the pitch's pad chunks are never multiplied)
    const uint32_t total_stages = bits ? (std::max(a->n_words, b->n_words) + 7u) / 8u * 4u : (uint32_t)(row_bytes / kStageBytes);
    const uint32_t ta = (uint32_t)(rows_a / kTile), tb = (uint32_t)(rows_b / kTile);
    const bool k2h = choose_tile128(ctx, (uint64_t)ta * tb, pitch, bits);   // [r6] few tiles: tile128_kernel
    int rc = STORM_HIP_OK;
    MatrixPlan plan;
    if (k2h) {
        ctx->k2_tile_shape_eff = 6;
    } else {
        MatrixTilesRequest rq;
        rq.total_stages = total_stages;
        xcd_grouped_tiles(0, ta, ta, ta + tb, false, rq.tiles);
        rc = ensure_matrix_tiles(ctx, std::move(rq), &plan);
    }
    uint32_t* d_counts = nullptr;  // per virtual row
    if (rc == STORM_HIP_OK) rc = op_row_counts(ctx, op, a, b, rows_a, rows_a + rows_b, &d_counts);
    if (rc == STORM_HIP_OK) {
        const OutWindow w = rectangle_window(d_out, ld, a->n_rows, rows_a, b->n_rows, d_counts, op);
        for (int side = 0; side < 2 && !bits; ++side) {
            const storm_hip_matrix_s* m = side ? b : a;
            const uint64_t rows_dst = side ? rows_b : rows_a;
            const dim3 grid = expand_grid(rows_dst, stride_words);
            hipLaunchKernelGGL(expand_fp4_kernel, grid, dim3(256), 0, ctx->stream, m->d,
                               stride_words, std::min<uint64_t>(m->n_rows_pad, rows_dst), rows_dst,
                               reinterpret_cast<uint4*>(ctx->d_x4.d + (side ? rows_a * pitch : 0)),
                               kExpandAll, 2u, pitch / 16);
        }
        const TileOperands ops = bits ? operands_of(a->d, b->d, pitch, rows_a, std::min<uint64_t>(a->n_rows_pad, rows_a),
                                                    std::min<uint64_t>(b->n_rows_pad, rows_b))
                                      : operands_of(ctx->d_x4.d, pitch, rows_a + rows_b);
        rc = k2h ? run_tile128(ctx, total_stages, ops, w, 1u) : run_matrix_tiles(ctx, plan, ops, bits, w);
    }
    if (rc == STORM_HIP_EHIP) set_error("square_matrix: HIP failure");
    return rc;
}

// The K2q work list of the last geometry (build_bitstream, storm_hip_plan.cpp), cached by its request.
static BitstreamRequest bitstream_request_of(const storm_hip_ctx_t* ctx, const std::vector<RowRange>& ranges, uint32_t n_kslices,
                                             uint32_t shard_rank, uint32_t shard_count, uint64_t pitch) {
    BitstreamShaping sh;
    sh.groups_per_cu = ctx->k2_stream_groups_per_cu;
    sh.min_piece = std::max(1, ctx->k2_stream_min_piece);
    sh.min_run = std::max(1, ctx->k2_stream_min_run);
    sh.w3_1 = ctx->k2_stream_w3_1;
    sh.w3_2 = ctx->k2_stream_w3_2;
    return bitstream_request(sh, ranges, n_kslices, shard_rank, shard_count, (uint32_t)std::max(1, ctx->n_cus), pitch);
}

static int ensure_bitstream(storm_hip_ctx_t* ctx, const std::vector<RowRange>& ranges, uint32_t n_kslices,
                            uint32_t shard_rank, uint32_t shard_count, uint64_t pitch) {
    const BitstreamRequest rq = bitstream_request_of(ctx, ranges, n_kslices, shard_rank, shard_count, pitch);
    if (ctx->bitfirst.holds(rq)) return STORM_HIP_OK;
    ctx->bitfirst.forget();   // (the segment table and the counters below change in front of the put)
    BitstreamPlan plan;
    build_bitstream(rq, ranges, plan);
    if (plan.bases.size() >= (1ull << 32) ||
        (!ranges.empty() && ranges.back().r1 * pitch / 64 + n_kslices >= (1ull << 32))) {
        set_error("K2q: the matrix is beyond the 32-bit stage addresses (64-byte units)");
        return STORM_HIP_EINVAL;
    }
    if (plan.max_stages > kBsMaxStages) {
        set_error("K2q: a workgroup of %u stages exceeds the exact range of its accumulators", plan.max_stages);
        return STORM_HIP_EINVAL;
    }
    const size_t seg_bytes = std::max<size_t>(plan.segs.size(), 1) * sizeof(BitSeg);
    // one device buffer: first[G + 1] | first_stage[G + 1] | bases[stages]
    std::vector<uint32_t> packed(plan.first);
    packed.insert(packed.end(), plan.first_stage.begin(), plan.first_stage.end());
    packed.insert(packed.end(), plan.bases.begin(), plan.bases.end());
    packed.push_back(0u);  // a trailing workgroup without stages reads bases[total stages] (bitstream_kernel: prep)
    // the segments travel in front of the stage tables, whose put waits for both
    if (int rc = ctx->d_bitsegs.ensure(seg_bytes, "K2q: the segment table")) return rc;
    if (upload_bytes(ctx, ctx->d_bitsegs, plan.segs.data(), plan.segs.size() * sizeof(BitSeg))) {
        set_error("K2q: the segment table: the copy to the device failed");
        return STORM_HIP_EHIP;
    }
    ctx->n_bit_groups = plan.groups;
    ctx->bit_stages = plan.stages;
    ctx->bit_max_stages = plan.max_stages;
    ctx->n_bit_segs = (uint32_t)plan.segs.size();
    return ctx->bitfirst.put(ctx, rq, packed.data(), packed.size(), "K2q: the workgroups' stage tables");
}

// One launch: the all-pairs total of every row range of a bit matrix (pitch in bytes, rows up to the
// next multiple of 256 behind every range readable and zero) into *d_total.
int launch_pairw_bitstream(storm_hip_ctx_t* ctx, const uint64_t* X, uint64_t pitch,
                           const std::vector<RowRange>& ranges, uint32_t n_kslices, uint32_t shard_rank,
                           uint32_t shard_count, uint64_t* d_total) {
    if (pitch * (uint64_t)kStripBRows >= (1ull << 32) || pitch % 64 != 0) {
        set_error("K2q: rows of %llu bytes are outside the bit-operand stream's 32-bit DMA offsets",
                  (unsigned long long)pitch);
        return STORM_HIP_EINVAL;
    }
    if (int rc = ensure_bitstream(ctx, ranges, n_kslices, shard_rank, shard_count, pitch)) return rc;
    ctx->pass_report[0] |= STORM_HIP_RAN_BITSTREAM;
    ctx->pass_report[1] += ranges_word_pairs(ranges, (uint64_t)n_kslices * 8u, shard_count);
    ctx->items.forget();
    ctx->last_info[0] = ctx->n_bit_groups;
    ctx->last_info[1] = ctx->bit_max_stages;
    ctx->last_info[2] = 1;
    ctx->last_info[3] = ctx->n_bit_segs;
    if (ctx->n_bit_groups == 0)   // (nothing to multiply: the fold of the empty slots writes the 0 — d_total may be the host mailbox)
        return launch_fold_slots(ctx, d_total);
    kernel_time_mark(ctx);
    const dim3 grid(ctx->n_bit_groups), block(kStripThreads);
#ifdef STORM_HIP_PROBES
    if (ctx->k2_ring == 18) {  // schedule trace (results stay correct)
        const size_t need = (size_t)ctx->n_bit_groups * 8 * sizeof(unsigned long long);
        if (int rc = ctx->d_trace.ensure(need, "K2q: the schedule trace")) return rc;
        ctx->trace_items = ctx->n_bit_groups;
        ctx->trace_is_stream = true;
        hipLaunchKernelGGL(bitstream_kernel<true>, grid, block, 0, ctx->stream,
                           reinterpret_cast<const uint8_t*>(X), pitch, ctx->d_bitsegs.d,
                           ctx->bitfirst.recs(),
                           ctx->bitfirst.recs() + 2 * ((size_t)ctx->n_bit_groups + 1),
                           ctx->bitfirst.recs() + ((size_t)ctx->n_bit_groups + 1), ctx->d_slots,
                           reinterpret_cast<unsigned long long*>(d_total), ctx->d_trace);
    } else
#endif
        hipLaunchKernelGGL(bitstream_kernel<false>, grid, block, 0, ctx->stream,
                           reinterpret_cast<const uint8_t*>(X), pitch, ctx->d_bitsegs.d,
                           ctx->bitfirst.recs(),
                           ctx->bitfirst.recs() + 2 * ((size_t)ctx->n_bit_groups + 1),
                           ctx->bitfirst.recs() + ((size_t)ctx->n_bit_groups + 1), ctx->d_slots,
                           reinterpret_cast<unsigned long long*>(d_total), (unsigned long long*)nullptr);
    kernel_time_mark(ctx);
    STORM_HIP_TRY(hipGetLastError());
    return STORM_HIP_OK;
}

#ifdef STORM_HIP_PROBES  // host side of K2w: ensure_bitwave, launch_pairw_bitwave: tools build (make probes)
#include "../../tools/probes/bitwave_launch.hip"
#endif  // STORM_HIP_PROBES

// K2b over arbitrary row ranges of a bit matrix X (pitch bytes per row, n_words of them hold data), in one of the K2b
// forms of the table (storm_hip_plan.h: kStripBits, kStripBitsWide, kStripRows). The rows of every range's last A tile
// beyond its r1 must be readable and zero in X. Dense container: the matrix; sparse container: the pool rows of its
// block columns.
int launch_pairw_bits_ranges(storm_hip_ctx_t* ctx, const uint8_t* X, uint64_t pitch,
                             const std::vector<RowRange>& ranges, const StripForm& form, uint32_t n_words, uint32_t shard_rank,
                             uint32_t shard_count, uint64_t* d_total, bool slots_hold_sums) {
    if (pitch * (uint64_t)kStripBRows >= (1ull << 32)) {
        set_error("K2b: rows of %llu bytes are beyond the strips' 32-bit DMA offsets", (unsigned long long)pitch);
        return STORM_HIP_EINVAL;
    }
    ctx->items.forget();  // the strip items carry the diagonal tiles themselves
    const uint32_t n_kslices = form.kslices(n_words);
    if (int rc = ensure_strip_items(ctx, ranges, n_kslices, shard_rank, shard_count, form.a_tile, form.xcd_group, form.rows_form()))
        return rc;
    const uint32_t n_strip = ctx->strips.n;
    ctx->k2_operands_used = form.operands_report;
    ctx->k2_strip_rows_used = form.rows_report;
    if (n_strip > 0) {
        ctx->pass_report[0] |= STORM_HIP_RAN_BIT_STRIPS;
        ctx->pass_report[1] += ranges_word_pairs(ranges, (uint64_t)n_kslices * form.slice_words(), shard_count);
    }
    ctx->last_info[0] = n_strip;
    ctx->last_info[1] = ctx->k2_stages_per_item;
    ctx->last_info[2] = 1;
    ctx->last_info[3] = 0;
    // the fold inside the launch (option k2_fold_inline: -1 = whenever the packed slot words cannot overflow, 0 = never:
    // a fold launch follows): arrivals per slot below 2^16, a slot's sum below 2^48 (StripForm::wave_sum_max)
    // ... and what it is worth depends on the launch: a short one (up to 4096 workgroups: N <= ~2000 at M = 65536) spends a
    // fifth of a pass in the fold launch and its gaps and uses 256 slots, one per polling thread (-1 = on for those); a long
    // one gains nothing (profiles/r05_c_fold_ab.jsonl) and keeps the fold launch unless the option is 1
    const uint32_t fold_slots = n_strip <= 4096u ? 256u : (uint32_t)kSlots;
    const bool fold_wanted = ctx->k2_fold_inline > 0 || (ctx->k2_fold_inline < 0 && n_strip <= 4096u);
    const uint64_t arrivals_per_slot = (uint64_t)n_strip * (uint64_t)form.waves / (uint64_t)fold_slots + 1u;
    // (slots_hold_sums: another kernel of this pass — the list-probe kernel — has added sums of unknown size: fold launch)
    const bool fold_inline = fold_wanted && !slots_hold_sums && n_strip > 0 && arrivals_per_slot < 65535u &&
                             arrivals_per_slot * form.wave_sum_max < (1ull << 48);   // (runs are capped at 4096 stages)
    if (n_strip > 0) {
        kernel_time_mark(ctx);
        const dim3 grid(n_strip), block(form.threads());
        unsigned long long* const fold_to = fold_inline ? reinterpret_cast<unsigned long long*>(d_total) : nullptr;
        if (form.kernel == StripKernel::Rows) {
            // where the rows end, for a pass that is one plain range from row 0 (the dense matrix, whole or sharded): the
            // kernel issues no MFMA for the zero rows behind r1 in whole fragments and blocks (storm_hip_plan.h)
            const bool plain = ranges.size() == 1 && ranges[0].r0 == 0 && ranges[0].a_end == 0 && ranges[0].back_from == ~0ull &&
                               ranges[0].r1 < (uint64_t)kStripRowsNoTrim;
            hipLaunchKernelGGL(strip16_rows_kernel, grid, block, (size_t)ctx->k2_lds_pad, ctx->stream, X, pitch, ctx->strips.recs(),
                               ctx->d_slots, fold_to, fold_slots, plain ? (uint32_t)ranges[0].r1 : kStripRowsNoTrim);
        } else if (form.kernel == StripKernel::BitsWide)
            hipLaunchKernelGGL(strip16_bits2_kernel, grid, block, (size_t)ctx->k2_lds_pad, ctx->stream, X, pitch, ctx->strips.recs(),
                               ctx->d_slots, fold_to, fold_slots);
        else
            hipLaunchKernelGGL(strip16_bits_kernel, grid, block, (size_t)ctx->k2_lds_pad, ctx->stream, X, pitch, ctx->strips.recs(),
                               ctx->d_slots, fold_to, fold_slots);
        kernel_time_mark(ctx);
        STORM_HIP_TRY(hipGetLastError());
    }
    return fold_inline ? STORM_HIP_OK : launch_fold_slots(ctx, d_total);
}

#ifdef STORM_HIP_PROBES
// k2_strip_operands = 1 (tools build): the strips on bit operands, one item per workgroup (stripbits_kernel)
static int launch_pairw_stripbits(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, const std::vector<RowRange>& ranges,
                                  uint32_t shard_rank, uint32_t shard_count, uint64_t* d_total) {
    ctx->items.forget();  // the strip items carry the diagonal tiles themselves
    if (int rc = ensure_strip_items(ctx, ranges, kStripBits.chunks(m->n_words), shard_rank, shard_count, kStripBits.a_tile))
        return rc;
    const uint32_t n_strip = ctx->strips.n;
    if (n_strip > 0) {
        kernel_time_mark(ctx);
        hipLaunchKernelGGL(stripbits_kernel, dim3(n_strip), dim3(kStripThreads), 0, ctx->stream,
                           reinterpret_cast<const uint8_t*>(m->d), m->stride_words * 8, ctx->strips.recs(), ctx->d_slots);
        kernel_time_mark(ctx);
        STORM_HIP_TRY(hipGetLastError());
    }
    ctx->last_info[0] = n_strip;
    ctx->last_info[1] = ctx->k2_stages_per_item;
    ctx->last_info[2] = 1;
    ctx->last_info[3] = 0;
    return launch_fold_slots(ctx, d_total);
}
#endif

// The all-pairs total of a matrix that is still in the CALLER's memory (STORM_wrapper_diag[_blocked], storm.c:132-150,
// :222-279: the raw-buffer entry points pay the transfer on every call — 82 MB at the headline shape, 1.5 ms in front of
// a 0.76 ms pass). The rows travel in panels of whole A tiles on a second stream; as soon as a panel has landed, K2b
// multiplies the pairs whose later row lies in it (RowRange::back_from: the panel's tiles stationary, all rows in front
// of them streaming past) while the next panel is on the bus. What stays exposed is the first panel's copy and the last
// panel's pairs. One fold at the end; the work lists of the panels stay on the device between calls.
static int pairw_bits_upload_queue(storm_hip_ctx_t* ctx, storm_hip_matrix_s* m, const uint64_t* host_rows,
                                   uint64_t src_stride_words, const StripForm& form, uint64_t* d_total);
int launch_pairw_bits_upload(storm_hip_ctx_t* ctx, storm_hip_matrix_s* m, const uint64_t* host_rows,
                             uint64_t src_stride_words, const StripForm& form, uint64_t* d_total) {
    const int rc = pairw_bits_upload_queue(ctx, m, host_rows, src_stride_words, form, d_total);
    if (rc != STORM_HIP_OK) {
        // a failure behind the first panel copy: the copies may still be reading the caller's rows (which the caller is about
        // to get back, and may free) and writing the matrix (which the caller of this function releases): drain both streams,
        // and disarm the mailbox this call was launched into
        if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        ctx->mail_armed = false;
    }
    return rc;
}
// (choose_pass has said "in panels" on `form`: the matrix's zero rows reach the form's A tile and its pitch the DMA offsets)
static int pairw_bits_upload_queue(storm_hip_ctx_t* ctx, storm_hip_matrix_s* m, const uint64_t* host_rows,
                                   uint64_t src_stride_words, const StripForm& form, uint64_t* d_total) {
    const uint64_t pitch = m->stride_words * 8;
    const uint64_t tiles = (m->n_rows + form.a_tile - 1) / form.a_tile;
    if (!ctx->copy_stream) STORM_HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    std::vector<PanelList>& lists = ctx->panel_lists;
    // The copies must not overtake what the context's stream still has to do to this matrix: storm_hip_matrix_create
    // zero-fills a fresh allocation ASYNCHRONOUSLY there, storm_hip_matrix_resize clears the rows a shrinking matrix gives
    // up (a first call on a new shape lost rows to that memset one time in six before this wait was here).
    if (lists.empty()) lists.resize(1);
    if (!lists[0].landed) STORM_HIP_TRY(hipEventCreateWithFlags(&lists[0].landed, hipEventDisableTiming));
    STORM_HIP_TRY(hipEventRecord(lists[0].landed, ctx->stream));
    STORM_HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, lists[0].landed, 0));
    // Panels of equal size, at most 8 and at least 4 tiles each: the last panel's pairs (~ 2 / panels of the pass) are what
    // the copies cannot cover, and short panels cost every item its prologue and every copy its set-up (shrinking the last
    // panels to 4, 3 and 2 tiles changed nothing at the headline shape — 1.87 ms either way: the pageable copy itself,
    // 44 - 48 GB/s, is the bound — and cost 6 % at 10000 x 524288).
    std::vector<uint64_t> first_tile;   // panel p = tiles [first_tile[p], first_tile[p + 1])
    {
        const uint64_t n = std::max<uint64_t>(1, std::min<uint64_t>(8, tiles / 4));
        for (uint64_t p = 0; p <= n; ++p) first_tile.push_back(tiles * p / n);
    }
    const uint64_t n_panels = first_tile.size() - 1;
    const uint32_t n_kslices = form.kslices(m->n_words);
    if (lists.size() < n_panels) lists.resize(n_panels);
    ctx->pass_report[0] |= STORM_HIP_RAN_BIT_STRIPS;
    ctx->pass_report[1] += ranges_word_pairs({{0, m->n_rows}}, (uint64_t)n_kslices * form.slice_words(), 1);
    ctx->k2_operands_used = form.operands_report;
    ctx->k2_strip_rows_used = form.rows_report;
    uint64_t n_total = 0;
    for (uint64_t p = 0; p < n_panels; ++p) {
        const uint64_t t0 = first_tile[p], t1 = first_tile[p + 1];
        if (t0 >= t1) continue;
        const uint64_t row0 = t0 * form.a_tile, row1 = std::min<uint64_t>(m->n_rows, t1 * form.a_tile);
        PanelList& l = lists[p];
        if (!l.landed) STORM_HIP_TRY(hipEventCreateWithFlags(&l.landed, hipEventDisableTiming));
        STORM_HIP_TRY(hipMemcpy2DAsync(m->d + row0 * m->stride_words, pitch, host_rows + row0 * src_stride_words,
                                       src_stride_words * 8, (size_t)m->n_words * 8, row1 - row0, hipMemcpyHostToDevice,
                                       ctx->copy_stream));
        STORM_HIP_TRY(hipEventRecord(l.landed, ctx->copy_stream));
        // (a fixed run length: a panel's list is short and all tail)
        StripOptions po = strip_options_of(ctx, form.xcd_group, form.rows_form());
        po.max_run = 128;
        po.shard_pairs = po.persistent = po.one_slice_probe = 0;
        RowRange rg{0, row1};
        rg.back_from = row0;
        const std::vector<RowRange> panel = {rg};
        const StripRequest rq = strip_request(po, panel, n_kslices, 0, 1, form.a_tile);
        if (!l.list.holds(rq)) {
            std::vector<StripItem> items;
            uint32_t qb[8], qc[8];
            plan_strips(rq, panel, items, qb, qc);
            if (items.size() >= (1ull << 31)) {
                set_error("pairw_dense_upload: %zu strip items exceed the grid limit", items.size());
                return STORM_HIP_EINVAL;
            }
            if (int rc = l.list.put(ctx, rq, items.data(), items.size(), "pairw_dense_upload: a panel's strip items", 1024 * sizeof(StripItem)))
                return rc;
        }
        STORM_HIP_TRY(hipStreamWaitEvent(ctx->stream, l.landed, 0));
        if (l.list.n) {
            hipLaunchKernelGGL(strip16_bits_kernel, dim3(l.list.n), dim3(form.threads()), (size_t)ctx->k2_lds_pad, ctx->stream,
                               reinterpret_cast<const uint8_t*>(m->d), pitch, l.list.recs(), ctx->d_slots,
                               (unsigned long long*)nullptr, (uint32_t)kSlots);
            STORM_HIP_TRY(hipGetLastError());
        }
        n_total += l.list.n;
    }
    ctx->last_info[0] = n_total;
    ctx->last_info[1] = ctx->k2_stages_per_item;
    ctx->last_info[2] = 1;
    ctx->last_info[3] = n_panels;
    return launch_fold_slots(ctx, d_total);
}

// The dense container's pass on the matrix cores, in the form choose_pass has named (storm_hip_plan.cpp).
int launch_pairw_mfma(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint32_t shard_rank,
                      uint32_t shard_count, const PassChoice& pass, uint64_t* d_total) {
    ctx->k2_operands_used = pass.operands_used;
    const uint64_t pitch = m->stride_words * 8;
    std::vector<RowRange> ranges;
    if (m->n_rows > 1) ranges.push_back({0, m->n_rows});
    switch (pass.kernel) {
    case PassKernel::Strips:   // the default: strips on bit operands over the matrix itself (no shadow, nothing to expand)
        return launch_pairw_bits_ranges(ctx, reinterpret_cast<const uint8_t*>(m->d), pitch, ranges, *pass.form, m->n_words,
                                        shard_rank, shard_count, d_total);
    case PassKernel::Bitstream:   // (k-slices of 512 bits that hold data: the zero padding of the rows is never multiplied)
        return launch_pairw_bitstream(ctx, m->d, pitch, ranges, kStripBits.chunks(m->n_words), shard_rank, shard_count, d_total);
#ifdef STORM_HIP_PROBES
    case PassKernel::ToolsBitwave:
        return launch_pairw_bitwave(ctx, m->d, pitch, ranges, kStripBits.chunks(m->n_words), shard_rank, shard_count, d_total);
    case PassKernel::ToolsStripBits:
        return launch_pairw_stripbits(ctx, m, ranges, shard_rank, shard_count, d_total);
#else
    case PassKernel::ToolsBitwave:
    case PassKernel::ToolsStripBits:
        set_error("k2_strip_operands = 1 (stripbits_kernel) is in the tools build only (`make probes`)");
        return STORM_HIP_EINVAL;
#endif
    default: {   // the FP4 kernels over the shadow
        const uint64_t tile = pass.strip_mode == 2 ? 512 : kStripATile;
        return launch_pairw_mfma_ranges(ctx, m->d, m->stride_words, m->n_rows_pad, (m->n_rows + tile - 1) / tile * tile, ranges,
                                        shard_rank, shard_count, pass.strip_mode, d_total, m->generation, m->n_words);
    }
    }
}

}  // namespace storm

#ifdef STORM_HIP_PROBES
// Tools build only: the in-kernel clock witness of the stamped kernels (STORM_CLOCK_BEGIN / _END above) since the last
// call: out = {sum of shader-clock ticks, sum of 100 MHz ticks, workgroups}; clears the counters. Current device.
extern "C" int storm_hip_probe_clock(uint64_t out[3]) {
    unsigned long long v[4] = {0, 0, 0, 0};
    if (hipDeviceSynchronize() != hipSuccess) return STORM_HIP_EINVAL;
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(storm::g_clock_probe), sizeof(v)) != hipSuccess) return STORM_HIP_EINVAL;
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
    const unsigned long long z[4] = {0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(storm::g_clock_probe), z, sizeof(z)) != hipSuccess) return STORM_HIP_EINVAL;
    return STORM_HIP_OK;
}
#endif
