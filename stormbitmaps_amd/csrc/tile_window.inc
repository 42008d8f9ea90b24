// tile_window.inc — the two records every materialised-output kernel takes by value: where the virtual rows of its item
// table live (TileOperands) and which window of the caller's buffer its counts go to (OutWindow). Included by
// storm_hip_mfma.hip inside namespace storm, ahead of every output kernel and probe fragment; design notes: DESIGN.md §4.

struct TileOperands {       // where the virtual rows of the item table live
    const uint8_t* xa;      // virtual rows [0, split): matrix A (or the only matrix)
    const uint8_t* xb;      // virtual rows [split, ..): matrix B
    uint64_t pitch;         // bytes per row of both
    uint32_t split;         // first virtual row of matrix B (0xffffffff: none)
    uint32_t rows_a, rows_b;  // allocated rows behind xa / xb (reads beyond return zero)

    // The tile of `height` rows from virtual row v0 on: its first row and the bytes of it that exist (the range of the
    // tile's buffer descriptor: rows beyond the allocation read as zero).
    __device__ __forceinline__ void tile_rows(uint32_t v0, uint32_t height, const uint8_t*& base, uint32_t& bytes) const {
        const bool second = v0 >= split;
        const uint32_t r0 = second ? v0 - split : v0;
        const uint32_t have = second ? rows_b : rows_a;
        const uint32_t rows = have > r0 ? min(have - r0, height) : 0u;
        base = (second ? xb : xa) + (uint64_t)r0 * pitch;
        bytes = rows * (uint32_t)pitch;
    }
};

// One matrix: virtual row = matrix row.
static TileOperands operands_of(const void* d, uint64_t pitch, uint64_t rows_allocated) {
    return {static_cast<const uint8_t*>(d), nullptr, pitch, 0xffffffffu, (uint32_t)std::min<uint64_t>(rows_allocated, 0xffffffffu), 0u};
}
// [A ; B]: B's virtual rows count on from `split` (A's rows padded to whole tiles); rows_a / rows_b = what exists of each
// within the virtual rows the items name.
static TileOperands operands_of(const void* da, const void* db, uint64_t pitch, uint64_t split, uint64_t rows_a, uint64_t rows_b) {
    return {static_cast<const uint8_t*>(da), static_cast<const uint8_t*>(db), pitch, (uint32_t)split, (uint32_t)rows_a, (uint32_t)rows_b};
}

// The window of the caller's buffer a launch writes, in virtual rows i (A side) and j (B side) of the item table:
//   Triangle  : pairs i < j < n_cols of one matrix, rows i_lo <= i < n_rows (a band), at out[(i - i_lo) * ld + j];
//   Rectangle : rows i_lo <= i < n_rows against the virtual rows j_base + [0, j_count) (B behind A), at
//               out[(i - i_lo) * ld + (j - j_base)];
//   Lag       : the triangle's pairs with j - i <= lag, at out[(i - i_lo) * ld + (j - i - 1)] (tile128_kernel<true> only).
// row_counts (per virtual row; null: AND) turns the AND count c of a pair into n_i + n_j - and_weight * c (OR: 1, XOR: 2).
enum class OutForm : uint32_t { Triangle, Rectangle, Lag };

struct OutWindow {
    uint32_t* out;
    uint64_t ld;
    const uint32_t* row_counts;
    uint32_t and_weight;
    uint32_t i_lo, n_rows;      // rows written
    uint32_t n_cols;            // Triangle, Lag: the matrix's row count
    uint32_t j_base, j_count;   // Rectangle: the columns' virtual rows (otherwise 0)
    uint32_t lag;               // Lag
    OutForm form;

    // The row counts as the kernels read them: nothing writes them while a launch runs, and the constant address space says
    // so (what `const __restrict__` on a kernel's parameter said: no store through `out` stands between two of their loads).
    typedef const __attribute__((address_space(4))) uint32_t* counts_ptr_t;
    __device__ __forceinline__ counts_ptr_t counts() const { return (counts_ptr_t)row_counts; }

    // Every kernel works on `const OutWindow w = window.loaded()`, never on its parameter: every field read once, into
    // registers. (Read where the members below use them, the fields of the by-value argument are loaded from the
    // kernel-argument segment again behind every branch: 600 scalar loads and as many waits in tile128_kernel's epilogue.)
    // It is the kernel's first statement — or, in tilering_kernel, whose k-loop leaves no register to spare, the epilogue's:
    // the few fields its prologue asks are read from the parameter there, in straight-line code.
    __device__ __forceinline__ OutWindow loaded() const {
        return {out, ld, row_counts, and_weight, i_lo, n_rows, n_cols, j_base, j_count, lag, form};
    }

    __host__ __device__ __forceinline__ bool rect() const { return form == OutForm::Rectangle; }
    // one past the last virtual row that is a column
    __host__ __device__ __forceinline__ uint32_t col_end() const { return rect() ? j_base + j_count : n_cols; }
    // is column j wanted
    __device__ __forceinline__ bool wants_col(uint32_t j) const {
        return rect() ? (j >= j_base && j - j_base < j_count) : j < n_cols;
    }
    // is (i, j) written, j being a wanted column (the kernels ask wants_col once per column and this per element).
    // kLag: the caller is instantiated for the Lag form (every other kernel sees the other two only)
    template <bool kLag = false>
    __device__ __forceinline__ bool writes_row(uint32_t i, uint32_t j) const {
        if constexpr (kLag) return i >= i_lo && i < n_rows && i < j && j - i <= lag;
        else return i >= i_lo && i < n_rows && (rect() || i < j);
    }
    // address of (i, j)
    template <bool kLag = false>
    __device__ __forceinline__ uint32_t* at(uint32_t i, uint32_t j) const {
        return &out[(uint64_t)(i - i_lo) * ld + (kLag ? j - i - 1u : j - j_base)];
    }
    // n_j of a column (0 where none is needed)
    __device__ __forceinline__ uint32_t nj(uint32_t j) const { return (row_counts && wants_col(j)) ? counts()[j] : 0u; }
    // value stored for AND count c at row i, given n_j
    __device__ __forceinline__ uint32_t value(uint32_t c, uint32_t i, uint32_t nj) const {
        return row_counts ? counts()[i] + nj - and_weight * c : c;
    }
    // ... added by an item that covers a part of k only (mod 2^32 throughout): the n_i + n_j term comes with the first part
    __device__ __forceinline__ uint32_t part_value(uint32_t c, uint32_t i, uint32_t nj, bool first) const {
        return row_counts ? (first ? counts()[i] + nj : 0u) - and_weight * c : c;
    }
    // does the block [i0, i0 + h) x [j0, j0 + w) lie wholly inside the window and, in a triangle, above the diagonal
    // (Triangle and Rectangle: what the kernels' 16-byte store paths ask)
    __device__ __forceinline__ bool covers(uint32_t i0, uint32_t h, uint32_t j0, uint32_t w) const {
        return i0 >= i_lo && i0 + h <= n_rows &&
               (rect() ? (j0 >= j_base && j0 - j_base + w <= j_count) : (j0 + w <= n_cols && i0 + h <= j0));
    }
};

static inline uint32_t and_weight_of(int op) { return op == STORM_HIP_OP_XOR ? 2u : 1u; }

// Rows [row0, row_end) of the triangle of a matrix of n rows. d_counts: per row, null for AND (and for dot products).
static OutWindow triangle_window(uint32_t* d_out, uint64_t ld, uint64_t row0, uint64_t row_end, uint64_t n, const uint32_t* d_counts, int op) {
    return {d_out, ld, d_counts, and_weight_of(op), (uint32_t)row0, (uint32_t)row_end, (uint32_t)n, 0u, 0u, 0u, OutForm::Triangle};
}
// Every row of A (rows_a of them, virtual rows from 0) against every row of B (rows_b, virtual rows from j_base).
static OutWindow rectangle_window(uint32_t* d_out, uint64_t ld, uint64_t rows_a, uint64_t j_base, uint64_t rows_b, const uint32_t* d_counts, int op) {
    return {d_out, ld, d_counts, and_weight_of(op), 0u, (uint32_t)rows_a, 0u, (uint32_t)j_base, (uint32_t)rows_b, 0u, OutForm::Rectangle};
}
// Rows [row0, row_end) of the triangle's pairs within `lag` rows of each other, in the lag layout.
static OutWindow lag_window(uint32_t* d_out, uint64_t ld, uint64_t row0, uint64_t row_end, uint64_t n, uint64_t lag, const uint32_t* d_counts, int op) {
    return {d_out, ld, d_counts, and_weight_of(op), (uint32_t)row0, (uint32_t)row_end, (uint32_t)n, 0u, 0u, (uint32_t)lag, OutForm::Lag};
}
