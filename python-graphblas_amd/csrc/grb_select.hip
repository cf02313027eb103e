// grb_select.hip -- GrB_select: C<Mask, replace> = accum(C, select(op, A, y)) and the vector form (C API 2.0 section 4.3.9; reference
// core/matrix.py:2597-2623, core/vector.py select -> GrB_Matrix_select_<T> / GrB_Vector_select_<T> / the _Scalar forms).
//
// The builtin index-unary operators that return BOOL keep the entry a(i, j) when   (k = the thunk as INT64, i + k in int64)
//   TRIL j <= i + k    TRIU j >= i + k    DIAG j == i + k    OFFDIAG j != i + k
//   COLLE j <= k       COLGT j > k        ROWLE i <= k       ROWGT i > k
//   VALUE{EQ,NE,GT,GE,LT,LE}_<T>   (T) a(i, j)  cmp  (T) y    -- both cast with cast_value; a comparison against NaN is false except NE
// A vector is a column: j = 0.
//
// Matrix kernel: ENTRY-parallel, independent of the row lengths -- an R-MAT row has 0 .. 10^5 entries.
//   1. flag   a wavefront takes consecutive blocks of 64 entries of d_col (/ d_val); it finds the row of its first entry by ONE search
//             in d_ptr and walks forward from there (64 row ends at a time through LDS); one 64-bit keep word per block (__ballot) and
//             its popcount, plain vector stores.  The positional operators never read the value stream.
//   2. scan   prim_exclusive_sum_i64 over the per-block popcounts
//   3. rows   Np[i] = prefix(Ap[i]),  prefix(p) = blocksum[p >> 6] + popc(keep[p >> 6] & below(p & 63)): no per-row counting, no atomics
//   4. fill   every kept entry writes column and value at prefix(p): coalesced reads, compacted writes, the order (sorted columns) kept
// Short cuts, all exact: ROWLE / ROWGT keep a contiguous range of entries (row pointers sliced, columns and values copied); a thunk
// that keeps everything or nothing is decided on the host.
#include <algorithm>

#include "grb_index_ops.hpp"  // Thunk, sel_pos / sel_val, the entry -> row walk (shared with grb_apply.hip)

namespace grb {

constexpr bool sel_needs_row(int op) { return op == SEL_TRIL || op == SEL_TRIU || op == SEL_DIAG || op == SEL_OFFDIAG; }

// ---- 1. flag pass ------------------------------------------------------------------------------------------------------
// keep[b] bit l = entry 64 b + l stays; bsum[b] = popc(keep[b]); bsum[nblocks] = 0 (the scan turns it into the total)
template <int OP, typename T>
__global__ void __launch_bounds__(256) k_select_flag(const int64_t *__restrict__ Ap, int64_t m, const int32_t *__restrict__ Aj, const T *__restrict__ Ax,
                                                     int a_iso, int64_t nnz, int64_t nblocks, int64_t k, T y, unsigned long long *__restrict__ keep,
                                                     int64_t *__restrict__ bsum)
{
    constexpr bool NEED_ROW = sel_needs_row(OP);
    constexpr bool IS_VALUE = OP >= SEL_VALUEEQ;
    __shared__ int64_t s_end[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * SEL_BPW;
    const int64_t b1 = b0 + SEL_BPW < nblocks ? b0 + SEL_BPW : nblocks;
    if (blockIdx.x == 0 && threadIdx.x == 0) bsum[nblocks] = 0;
    int64_t r = 0;  // (wave-uniform) the row of the first entry of the current block
    if constexpr (NEED_ROW) {
        if (b0 < b1) r = walk_first_row(Ap, m, b0 << 6);
    }
    for (int64_t b = b0; b < b1; b++) {
        const int64_t p = b << 6, e = p + lane;
        const bool active = e < nnz;
        int64_t row = r;
        if constexpr (NEED_ROW) row = walk_block_rows(Ap, m, nnz, p, lane, s_end[wave], r);
        bool pred = false;
        if (active) {
            if constexpr (IS_VALUE) pred = sel_val<OP, T>(Ax[a_iso ? 0 : e], y);
            else pred = sel_pos<OP>(row, (int64_t)Aj[e], k);
        }
        const unsigned long long word = __ballot(pred);
        if (lane == 0) {
            keep[b] = word;
            bsum[b] = __popcll(word);
        }
    }
}

// ---- 3. row pointers from the same prefix --------------------------------------------------------------------------------
__global__ void k_select_rowptr(const int64_t *__restrict__ Ap, int64_t m, int64_t nnz, int64_t nblocks, const unsigned long long *__restrict__ keep,
                                const int64_t *__restrict__ bsum, int64_t *__restrict__ Np)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const int64_t p = Ap[i];
    Np[i] = p >= nnz ? bsum[nblocks] : bsum[p >> 6] + __popcll(keep[p >> 6] & ((1ull << (p & 63)) - 1));
}

// ---- 4. fill pass: U = an unsigned integer of the value size (the values are moved, not read) ------------------------------------
template <typename U>
__global__ void k_select_fill(const int32_t *__restrict__ Aj, const U *__restrict__ Ax, int a_iso, int64_t nnz, const unsigned long long *__restrict__ keep,
                              const int64_t *__restrict__ bsum, int32_t *__restrict__ Nj, U *__restrict__ Nx)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const unsigned long long w = keep[e >> 6];
    const int l = (int)(e & 63);
    if (!((w >> l) & 1ull)) return;
    const int64_t pos = bsum[e >> 6] + __popcll(w & ((1ull << l) - 1));
    Nj[pos] = Aj[e];
    if (Nx) Nx[pos] = Ax[a_iso ? 0 : e];
}

// ROWLE / ROWGT: the kept entries are [lo, hi)
__global__ void k_select_rowslice(const int64_t *__restrict__ Ap, int64_t m, int64_t lo, int64_t hi, int64_t *__restrict__ Np)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    int64_t p = Ap[i];
    p = p < lo ? lo : (p > hi ? hi : p);
    Np[i] = p - lo;
}

// ---- vector form: one element-wise pass over values and presence words (the style of grb_vecops.hip) ---------------------------------
template <int OP, typename T>
__global__ void k_vselect(int64_t n, const T *__restrict__ val, const uint64_t *__restrict__ bits, int64_t k, T y, uint64_t *__restrict__ t_bits)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t g = i >> 6;
    bool pred = false;
    if (i < n && ((bits[g] >> lane) & 1ull)) {
        if constexpr (OP >= SEL_VALUEEQ) pred = sel_val<OP, T>(val[i], y);
        else pred = sel_pos<OP>(i, 0, k);
    }
    const unsigned long long b = __ballot(pred);
    if (lane == 0 && g < ((n + 63) >> 6)) t_bits[g] = b;
}

// (ROWLE / ROWGT of a matrix never reach the flag pass: they are a slice of the row pointers)
#define SEL_FOR_POS_FLAG(X) X(SEL_TRIL) X(SEL_TRIU) X(SEL_DIAG) X(SEL_OFFDIAG) X(SEL_COLLE) X(SEL_COLGT)
#define SEL_FOR_POS(X) SEL_FOR_POS_FLAG(X) X(SEL_ROWLE) X(SEL_ROWGT)
#define SEL_FOR_VAL(X) X(SEL_VALUEEQ) X(SEL_VALUENE) X(SEL_VALUEGT) X(SEL_VALUEGE) X(SEL_VALUELT) X(SEL_VALUELE)

template <typename TO>
static void launch_flag_value(int code, dim3 grid, const int64_t *Ap, int64_t m, const int32_t *Aj, const void *xs, int a_iso, int64_t nnz, int64_t nblocks,
                              TO y, unsigned long long *keep, int64_t *bsum)
{
    switch (code) {
#define SEL_CASE(OPC)                                                                                                                              \
    case OPC:                                                                                                                                      \
        hipLaunchKernelGGL((k_select_flag<OPC, TO>), grid, dim3(256), 0, ctx().stream, Ap, m, Aj, (const TO *)xs, a_iso, nnz, nblocks, (int64_t)0, y, \
                           keep, bsum);                                                                                                            \
        break;
        SEL_FOR_VAL(SEL_CASE)
#undef SEL_CASE
    default: fail(GrB_PANIC, "select: unknown operator code");
    }
}
template <typename TO>
static void launch_vselect_value(int code, dim3 grid, int64_t n, const void *xs, const uint64_t *bits, TO y, uint64_t *t_bits)
{
    switch (code) {
#define SEL_CASE(OPC)                                                                                                                  \
    case OPC:                                                                                                                          \
        hipLaunchKernelGGL((k_vselect<OPC, TO>), grid, dim3(256), 0, ctx().stream, n, (const TO *)xs, bits, (int64_t)0, y, t_bits);   \
        break;
        SEL_FOR_VAL(SEL_CASE)
#undef SEL_CASE
    default: fail(GrB_PANIC, "select: unknown operator code");
    }
}

// 1 = the thunk keeps every entry of an m x n matrix, -1 = none, 0 = depends on the entry.  After it, |k| < m + n for the operators
// that add: i + k cannot overflow
static int sel_trivial(int op, int64_t m, int64_t n, int64_t k)
{
    const bool off = k > n - 1 || k < -(m - 1);  // diagonal k does not cross the matrix
    switch (op) {
    case SEL_TRIL: return k >= n - 1 ? 1 : (k < -(m - 1) ? -1 : 0);
    case SEL_TRIU: return k <= -(m - 1) ? 1 : (k > n - 1 ? -1 : 0);
    case SEL_DIAG: return off ? -1 : 0;
    case SEL_OFFDIAG: return off ? 1 : 0;
    case SEL_COLLE: return k >= n - 1 ? 1 : (k < 0 ? -1 : 0);
    case SEL_COLGT: return k < 0 ? 1 : (k >= n - 1 ? -1 : 0);
    case SEL_ROWLE: return k >= m - 1 ? 1 : (k < 0 ? -1 : 0);
    case SEL_ROWGT: return k < 0 ? 1 : (k >= m - 1 ? -1 : 0);
    default: return 0;
    }
}

// T (of type `ctype`, fresh storage) = the entries of S the operator keeps.  full_values: one value per entry even when S is iso
// (the write rule reads one value per entry when it masks or accumulates)
static MatrixOwner select_build(GB_Matrix_opaque *S, const GB_IndexUnaryOp_opaque *op, const Thunk &th, int ctype, bool full_values)
{
    MatrixOwner Tm(matrix_new(type_of_code(ctype), S->nrows, S->ncols));
    if (S->nvals == 0) return Tm;
    const int code = op->op, stype = S->type->code;
    const int64_t m = (int64_t)S->nrows, n = (int64_t)S->ncols, nnz = S->nvals;
    const size_t ssize = S->type->size;
    const int64_t k = sel_is_value(code) ? 0 : thunk_as<int64_t>(th);
    const bool t_iso = S->iso && !full_values;
    const int a_iso = S->iso ? 1 : 0;
    const int trivial = sel_trivial(code, m, n, k);
    if (trivial < 0) return Tm;
    // the output: row pointers, columns, and the kept values (one when t_iso) moved in S's type; matrix_adopt casts them to C's type
    DevPtr<int64_t> Tp;
    DevPtr<int32_t> Tj;
    DevPtr<char> raw;
    auto alloc_out = [&](int64_t kept) {
        Tp.reset((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1)));
        Tj.reset((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)kept));
        raw.reset((char *)dev_alloc(ssize * (size_t)(t_iso ? 1 : kept)));
        if (t_iso) d2d(raw.p, S->d_val, ssize);
    };

    if (trivial > 0 || code == SEL_ROWLE || code == SEL_ROWGT) {
        // a contiguous range [lo, hi) of entries: slice the row pointers, copy columns and values
        int64_t lo = 0, hi = nnz;
        if (trivial == 0) {
            int64_t cut = 0;
            d2h(&cut, S->d_ptr + (k + 1), sizeof(int64_t));  // (0 <= k < m - 1 here)
            if (code == SEL_ROWLE) hi = cut;
            else lo = cut;
        }
        const int64_t kept = hi - lo;
        if (kept == 0) return Tm;
        alloc_out(kept);
        if (trivial > 0) d2d(Tp.p, S->d_ptr, sizeof(int64_t) * (size_t)(m + 1));
        else {
            hipLaunchKernelGGL(k_select_rowslice, grid1d(m + 1), dim3(256), 0, ctx().stream, (const int64_t *)S->d_ptr, m, lo, hi, Tp.p);
            ctx().stats.kernel_launches += 1;
        }
        d2d(Tj.p, S->d_col + lo, sizeof(int32_t) * (size_t)kept);
        if (!t_iso) {
            values_expanded(raw.p, (const char *)S->d_val + (a_iso ? 0 : ssize * (size_t)lo), a_iso, kept, ssize);
            ctx().stats.kernel_launches += a_iso;
        }
        matrix_adopt(Tm.get(), Tp.release(), Tj.release(), raw.release(), stype, kept, t_iso);
        GRB_HIP(hipGetLastError());
        return Tm;
    }

    // ---- the flag / scan / rows / fill passes ----
    const int64_t nblocks = ceil_div(nnz, 64);
    DevBuf<unsigned long long> keep((size_t)nblocks);
    DevBuf<int64_t> bsum((size_t)nblocks + 1);
    const dim3 fgrid((unsigned)ceil_div(nblocks, 4 * SEL_BPW)), fblock(256);
    const int64_t *Ap = S->d_ptr;
    const int32_t *Aj = S->d_col;
    if (!sel_is_value(code)) {
        switch (code) {
#define SEL_CASE(OPC)                                                                                                                              \
    case OPC:                                                                                                                                      \
        hipLaunchKernelGGL((k_select_flag<OPC, char>), fgrid, fblock, 0, ctx().stream, Ap, m, Aj, (const char *)nullptr, 0, nnz, nblocks, k, (char)0, \
                           keep.p, bsum.p);                                                                                                        \
        break;
            SEL_FOR_POS_FLAG(SEL_CASE)
#undef SEL_CASE
        default: fail(GrB_PANIC, "select: unknown operator code");
        }
    } else {
        // entry and thunk are compared in the operator's type: an operator of another type than the matrix's (A.select(">=", 2.5) on an
        // integer matrix) costs one cast pass over the values first (11 x 11 type pairs are not instantiated per operator)
        const int ot = op->type;
        DevPtr<char> xcast;
        const void *xs = values_as(S, ot, xcast);
        GRB_DISPATCH_TYPE(ot, TO, { launch_flag_value<TO>(code, fgrid, Ap, m, Aj, xs, a_iso, nnz, nblocks, thunk_as<TO>(th), keep.p, bsum.p); })
    }
    prim_exclusive_sum_i64(bsum.p, bsum.p, nblocks + 1);
    ctx().stats.kernel_launches += 2;
    int64_t kept = 0;
    d2h(&kept, bsum.p + nblocks, sizeof(int64_t));
    if (kept > 0) {
        alloc_out(kept);
        hipLaunchKernelGGL(k_select_rowptr, grid1d(m + 1), dim3(256), 0, ctx().stream, Ap, m, nnz, nblocks, (const unsigned long long *)keep.p,
                           (const int64_t *)bsum.p, Tp.p);
        GRB_DISPATCH_SIZE(ssize, U, hipLaunchKernelGGL((k_select_fill<U>), grid1d(nnz), dim3(256), 0, ctx().stream, Aj, (const U *)S->d_val, a_iso, nnz,
                                                       (const unsigned long long *)keep.p, (const int64_t *)bsum.p, Tj.p, (U *)(t_iso ? nullptr : raw.p)))
        ctx().stats.kernel_launches += 2;
        matrix_adopt(Tm.get(), Tp.release(), Tj.release(), raw.release(), stype, kept, t_iso);
    }
    GRB_HIP(hipGetLastError());
    return Tm;
}

static void check_select_op(const GB_IndexUnaryOp_opaque *op)
{
    if (!op) fail(GrB_NULL_POINTER, "GrB_select: the operator is NULL");
    if (!op_is_select(op->op))
        fail(GrB_DOMAIN_MISMATCH, std::string("GrB_select: ") + (op->name ? op->name : "the operator") +
                                      " does not return BOOL (an apply operator): select takes GrB_TRIL .. GrB_ROWGT and GrB_VALUE*_<T>");
}

static void matrix_select(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, const GB_IndexUnaryOp_opaque *op,
                          GB_Matrix_opaque *A, const Thunk &th, const GB_Descriptor_opaque *desc)
{
    require_init();
    check_matrix(C, "C");
    check_matrix(A, "A");
    if (Mask) check_matrix(Mask, "Mask");
    check_select_op(op);
    const Desc f = desc_of(desc);  // (T1 is ignored: there is no second input)
    const uint64_t in_rows = f.t0 ? A->ncols : A->nrows, in_cols = f.t0 ? A->nrows : A->ncols;
    if (C->nrows != in_rows || C->ncols != in_cols)
        fail(GrB_DIMENSION_MISMATCH, "GrB_select: output is " + std::to_string(C->nrows) + " x " + std::to_string(C->ncols) + ", the input " +
                                         (f.t0 ? "(transposed) " : "") + std::to_string(in_rows) + " x " + std::to_string(in_cols));
    check_mask_accum("GrB_select", C, Mask, accum);
    if (matrix_writes_nothing(C, Mask, f)) return;
    ctx().stats = GrX_Stats{};
    GB_Matrix_opaque *S = f.t0 ? matrix_transpose_cached(A) : A;
    matrix_finish(C, Mask, accum, select_build(S, op, th, C->type->code, Mask || accum), f, C == A);
    ctx().stats.out_nvals = C->nvals;
    if (ctx().blocking) sync_stream();
}

static void vector_select(GB_Vector_opaque *w, GB_Vector_opaque *mask, const GB_BinaryOp_opaque *accum, const GB_IndexUnaryOp_opaque *op,
                          GB_Vector_opaque *u, const Thunk &th, const GB_Descriptor_opaque *desc)
{
    require_init();
    check_select_op(op);
    const int code = op->op;
    // order-aware like the other element-wise operations: the positional operators need the natural index, the value ones any common order
    if (sel_is_value(code)) {
        check_vector_any(w, "w");
        check_vector_any(u, "u");
        if (mask) check_vector_any(mask, "mask");
    } else {
        check_vector(w, "w");
        check_vector(u, "u");
        if (mask) check_vector(mask, "mask");
    }
    const Desc f = desc_of(desc);
    if (w->n != u->n) fail(GrB_DIMENSION_MISMATCH, "GrB_select: output size " + std::to_string(w->n) + " does not match the input size " + std::to_string(u->n));
    check_vector_mask_accum("GrB_select", w, mask, accum);
    if (vector_writes_nothing(w, mask, f)) return;
    ctx().stats = GrX_Stats{};
    if (w->n == 0) return;
    if (sel_is_value(code)) {
        GB_Vector_opaque *vs[3] = {w, u, mask};
        (void)vectors_common_order(vs, 3);
    }
    const int64_t n = (int64_t)w->n;
    const size_t nwords = bits_words64((uint64_t)n);
    const int64_t threads = (int64_t)nwords * 64;
    DevBuf<uint64_t> t_bits(nwords);
    DevPtr<char> x_hold, t_hold;
    DevPtr<uint64_t> m_hold;
    if (!u->d_val) {
        GRB_HIP(hipMemsetAsync(t_bits.p, 0, nwords * 8, ctx().stream));
    } else if (!sel_is_value(code)) {
        // |k| beyond 2^62 decides like 2^62 (indices are below 2^40): i + k stays inside int64
        const int64_t lim = (int64_t)1 << 62;
        const int64_t k = std::max(-lim, std::min(lim, thunk_as<int64_t>(th)));
        switch (code) {
#define SEL_CASE(OPC)                                                                                                                       \
    case OPC:                                                                                                                               \
        hipLaunchKernelGGL((k_vselect<OPC, char>), grid1d(threads), dim3(256), 0, ctx().stream, n, (const char *)nullptr, (const uint64_t *)u->d_bits, k, \
                           (char)0, t_bits.p);                                                                                              \
        break;
            SEL_FOR_POS(SEL_CASE)
#undef SEL_CASE
        default: fail(GrB_PANIC, "select: unknown operator code");
        }
        ctx().stats.kernel_launches += 1;
    } else {
        const int ot = op->type;
        const void *xs = vector_values_as(u->d_val, u->type->code, ot, n, x_hold);
        GRB_DISPATCH_TYPE(ot, TO, { launch_vselect_value<TO>(code, grid1d(threads), n, xs, (const uint64_t *)u->d_bits, thunk_as<TO>(th), t_bits.p); })
        ctx().stats.kernel_launches += 1;
    }
    // t's values in w's type (a buffer of its own when w is u: the write rule works in place)
    const uint64_t *m_bits = vector_mask_words(mask, w, f.structure, m_hold);
    vector_ensure_storage(w);
    const void *tw = w->d_val;  // (u without entries: t_bits is zero, any array of w's type will do)
    if (w == u) {
        t_hold.reset((char *)dev_alloc(w->type->size * (size_t)n));
        d2d(t_hold.get(), u->d_val, w->type->size * (size_t)n);
        tw = t_hold.get();
    } else if (u->d_val) {
        tw = vector_values_as(u->d_val, u->type->code, w->type->code, n, t_hold);
    }
    vector_finish(w, tw, t_bits.p, m_bits, f, accum);
    GRB_HIP(hipGetLastError());
    if (ctx().blocking) sync_stream();
}

void preload_select() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_select_rowptr)); (void)hipGetLastError(); }

}  // namespace grb

using namespace grb;

extern "C" GrB_Info GrB_Matrix_select_Scalar(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op,
                                             const GrB_Matrix A, const GrB_Scalar y, const GrB_Descriptor desc)
{
    GRB_TRY
    check_matrix(C, "C");
    matrix_select(C, Mask, accum, op, A, thunk_of_scalar(y, "GrB_select"), desc);
    GRB_CATCH(errp(C))
}
extern "C" GrB_Info GrB_Vector_select_Scalar(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op,
                                             const GrB_Vector u, const GrB_Scalar y, const GrB_Descriptor desc)
{
    GRB_TRY
    check_vector_any(w, "w");
    vector_select(w, mask, accum, op, u, thunk_of_scalar(y, "GrB_select"), desc);
    GRB_CATCH(errp(w))
}

// every typed entry point accepts every select operator: y is cast to the operator's thunk type (python-graphblas passes its default
// thunk False through GrB_Matrix_select_BOOL with a positional operator)
#define DEF_SELECT_TYPED(NAME, ctype)                                                                                                            \
    extern "C" GrB_Info GrB_Matrix_select_##NAME(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op,       \
                                                 const GrB_Matrix A, ctype y, const GrB_Descriptor desc)                                         \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        matrix_select(C, Mask, accum, op, A, thunk_of<ctype>(TC_##NAME, y), desc);                                                               \
        GRB_CATCH(errp(C))                                                                                                                       \
    }                                                                                                                                            \
    extern "C" GrB_Info GrB_Vector_select_##NAME(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op,       \
                                                 const GrB_Vector u, ctype y, const GrB_Descriptor desc)                                         \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        vector_select(w, mask, accum, op, u, thunk_of<ctype>(TC_##NAME, y), desc);                                                               \
        GRB_CATCH(errp(w))                                                                                                                       \
    }
GRB_FOR_EACH_TYPE(DEF_SELECT_TYPED)
#undef DEF_SELECT_TYPED
