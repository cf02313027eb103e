// grb_apply.hip -- GrB_apply with a bound scalar or an index-unary operator: C<Mask, replace> = accum(C, T), T with the structure of A
// (of A' under GrB_DESC_T0; T1 is ignored), and the vector form (C API 2.0 section 4.3.8; reference core/matrix.py apply,
// core/vector.py apply -> GrB_{Matrix,Vector}_apply_{BinaryOp1st,BinaryOp2nd,IndexOp}_{<T>,Scalar}).  DESIGN.md section 4.9.
//
// The value of T at (i, j), X = the operator's type (entry and scalar are cast to it with cast_value), k = the thunk as INT64:
//   BinaryOp2nd   op((X) a, (X) s)        BinaryOp1st   op((X) s, (X) a)        -- X, or BOOL for GrB_EQ .. GrB_LE
//   IndexOp       ROWINDEX i + k    COLINDEX j + k    DIAGINDEX j - i + k       -- int64 arithmetic, then the operator's type
//                 GrB_TRIL .. GrB_ROWGT, GrB_VALUE*_<T>: the predicate GrB_select keeps an entry by (sel_pos / sel_val), as BOOL
// A vector is a column: j = 0.  T is cast to C's type by matrix_adopt when the two differ.
//
// Two matrix kernels, both bound by memory bandwidth:
//   by value     (bind-1st / bind-2nd, VALUE*) a pure stream over the nnz values: a lane moves 16 bytes of input per load
//                (16 / sizeof(X) values) where both arrays are 16-byte aligned, element by element otherwise and in the tail.  One
//                kernel per (operator, operator type): bind-1st is the flipped operator bound second (op(s, a) = op'(a, s)), a
//                comparison the VALUE* predicate of the same name, a matrix of another type one cast pass first (values_as).
//   by position  ENTRY-parallel: a wavefront takes consecutive blocks of 64 entries and finds their rows by the walk of k_select_flag
//                (walk_first_row / walk_block_rows, grb_index_ops.hpp); COLINDEX, COLLE / COLGT read d_col alone, ROWINDEX,
//                ROWLE / ROWGT the row alone.  The value stream is never read.
// The structure of T is a copy of A's row pointers and columns.  Short cuts, all exact: an empty A; SECOND, PAIR and ANY of (a, s)
// (ANY may return either operand: the scalar, every time) give an iso T of one value computed on the host, and so does an iso A
// under any by-value operator; none of them runs a value pass.
// GrX_last_stats: method 13 by value, 14 by position, 6 without a value pass; tiles = wavefront units; out_nvals = nnz(C).
#include <algorithm>

#include "grb_index_ops.hpp"

namespace grb {

// ---- the operators -----------------------------------------------------------------------------------------------------------
// A by-value operator code: a binary operator of OpCode computing op(a, s), or SEL_VALUE* (a cmp s -> BOOL).  A by-position one:
// SEL_TRIL .. SEL_ROWGT (-> BOOL) or APPLY_*INDEX.  The result type of operator OP over X:
template <int OP, typename X> struct ApplyOut {
    using type = typename std::conditional<(OP >= SEL_TRIL && OP <= SEL_VALUELE), bool, X>::type;
};
template <int OP, typename X> GRB_HD typename ApplyOut<OP, X>::type apply_val(X a, X s)
{
    if constexpr (OP >= SEL_VALUEEQ) return sel_val<OP, X>(a, s);
    else return apply_binop<X>(OP, a, s);
}
// (the index arithmetic wraps in int64 like the operator's own cast; the predicates get a thunk clamped to +-2^62 by the host)
template <int OP, typename TO> GRB_HD TO apply_pos(int64_t i, int64_t j, int64_t k)
{
    if constexpr (OP == APPLY_ROWINDEX) return cast_value<TO, int64_t>((int64_t)((uint64_t)i + (uint64_t)k));
    else if constexpr (OP == APPLY_COLINDEX) return cast_value<TO, int64_t>((int64_t)((uint64_t)j + (uint64_t)k));
    else if constexpr (OP == APPLY_DIAGINDEX) return cast_value<TO, int64_t>((int64_t)((uint64_t)j - (uint64_t)i + (uint64_t)k));
    else return sel_pos<OP>(i, j, k);
}
constexpr bool apply_needs_row(int op) { return !(op == APPLY_COLINDEX || op == SEL_COLLE || op == SEL_COLGT); }
constexpr bool apply_needs_col(int op) { return !(op == APPLY_ROWINDEX || op == SEL_ROWLE || op == SEL_ROWGT); }

// (SECOND and PAIR -- ANY is SECOND here -- never reach the matrix kernel: one value, computed by apply_one_value)
#define APPLY_FOR_STREAM(X)                                                                                                         \
    X(OP_FIRST) X(OP_PLUS) X(OP_MINUS) X(OP_RMINUS) X(OP_TIMES) X(OP_MIN) X(OP_MAX) X(OP_LOR) X(OP_LAND) X(OP_LXOR) X(OP_LXNOR)      \
    X(SEL_VALUEEQ) X(SEL_VALUENE) X(SEL_VALUEGT) X(SEL_VALUEGE) X(SEL_VALUELT) X(SEL_VALUELE)
#define APPLY_FOR_VAL(X) APPLY_FOR_STREAM(X) X(OP_SECOND) X(OP_PAIR)
#define APPLY_FOR_PRED(X) X(SEL_TRIL) X(SEL_TRIU) X(SEL_DIAG) X(SEL_OFFDIAG) X(SEL_COLLE) X(SEL_COLGT) X(SEL_ROWLE) X(SEL_ROWGT)
#define APPLY_FOR_INDEX(X) X(APPLY_ROWINDEX) X(APPLY_COLINDEX) X(APPLY_DIAGINDEX)

// ---- by value: a stream ---------------------------------------------------------------------------------------------------------
template <typename T, int N> struct alignas(sizeof(T) * N) ApplyPack {
    T v[N];
};

// A workgroup takes 256 V consecutive values, V = 16 / sizeof(X).  vec: thread t takes the V values from 256 V b + V t on -- one 16-byte
// load and one store of V results -- and the last, partial pack of the array element by element; else (an array that is not 16-byte
// aligned) it takes the values 256 V b + 256 q + t, q < V, one at a time, coalesced all the same.
template <int OP, typename X>
__global__ void __launch_bounds__(256) k_apply_val(const X *__restrict__ Ax, int64_t nnz, int vec, X s, typename ApplyOut<OP, X>::type *__restrict__ Tx)
{
    using TO = typename ApplyOut<OP, X>::type;
    constexpr int V = 16 / (int)sizeof(X);
    const int64_t base = (int64_t)blockIdx.x * (256 * V);
    if (vec) {
        const int64_t e0 = base + (int64_t)threadIdx.x * V;
        if (e0 + V <= nnz) {
            const ApplyPack<X, V> in = *reinterpret_cast<const ApplyPack<X, V> *>(Ax + e0);
            ApplyPack<TO, V> out;
#pragma unroll
            for (int q = 0; q < V; q++) out.v[q] = apply_val<OP, X>(in.v[q], s);
            *reinterpret_cast<ApplyPack<TO, V> *>(Tx + e0) = out;
        } else {
            for (int64_t e = e0; e < nnz; e++) Tx[e] = apply_val<OP, X>(Ax[e], s);
        }
    } else {
#pragma unroll
        for (int q = 0; q < V; q++) {
            const int64_t e = base + q * 256 + threadIdx.x;
            if (e < nnz) Tx[e] = apply_val<OP, X>(Ax[e], s);
        }
    }
}

// ---- by position: entry-parallel, the rows by the walk of k_select_flag -------------------------------------------------------------
template <int OP, typename TO>
__global__ void __launch_bounds__(256) k_apply_pos(const int64_t *__restrict__ Ap, int64_t m, const int32_t *__restrict__ Aj, int64_t nnz, int64_t nblocks,
                                                   int64_t k, TO *__restrict__ Tx)
{
    constexpr bool NEED_ROW = apply_needs_row(OP), NEED_COL = apply_needs_col(OP);
    __shared__ int64_t s_end[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * SEL_BPW;
    const int64_t b1 = b0 + SEL_BPW < nblocks ? b0 + SEL_BPW : nblocks;
    int64_t r = 0;  // (wave-uniform) the row of the first entry of the current block
    if constexpr (NEED_ROW) {
        if (b0 < b1) r = walk_first_row(Ap, m, b0 << 6);
    }
    for (int64_t b = b0; b < b1; b++) {
        const int64_t p = b << 6, e = p + lane;
        int64_t row = r;
        if constexpr (NEED_ROW) row = walk_block_rows(Ap, m, nnz, p, lane, s_end[wave], r);
        if (e < nnz) {
            int64_t j = 0;
            if constexpr (NEED_COL) j = (int64_t)Aj[e];
            Tx[e] = apply_pos<OP, TO>(row, j, k);
        }
    }
}

// ---- vector form: one element-wise pass over values and presence words (the style of k_vselect) -------------------------------------
// BY_VALUE: t = apply_val(val[i], s); else apply_pos(i, 0, k).  An absent element gets a zero nobody reads
template <int OP, typename X, bool BY_VALUE>
__global__ void k_vapply(int64_t n, const X *__restrict__ val, const uint64_t *__restrict__ bits, int64_t k, X s, typename ApplyOut<OP, X>::type *__restrict__ t_val)
{
    using TO = typename ApplyOut<OP, X>::type;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    TO t{};
    if ((bits[i >> 6] >> (i & 63)) & 1ull) {
        if constexpr (BY_VALUE) t = apply_val<OP, X>(val[i], s);
        else t = apply_pos<OP, TO>(i, 0, k);
    }
    t_val[i] = t;
}

// ---- what a call applies ---------------------------------------------------------------------------------------------------------
struct ApplySpec {
    bool by_value;
    int code;   // see above
    int xtype;  // by value: the type entry and scalar are cast to; by position: the type of T
    Thunk th;   // the bound scalar / the thunk
    int ttype() const { return (code >= SEL_TRIL && code <= SEL_VALUELE) ? (int)TC_BOOL : xtype; }
};

// op(a, s) when the scalar is bound second, op(s, a) = op'(a, s) when it is bound first
static ApplySpec spec_of_binop(const GB_BinaryOp_opaque *op, bool bind1st, const Thunk &th)
{
    if (!op) fail(GrB_NULL_POINTER, "GrB_apply: the operator is NULL");
    ApplySpec sp{true, 0, op->type, th};
    if (op_is_comparison(op->op)) {
        switch (op->op) {
        case OP_EQ: sp.code = SEL_VALUEEQ; break;
        case OP_NE: sp.code = SEL_VALUENE; break;
        case OP_GT: sp.code = bind1st ? SEL_VALUELT : SEL_VALUEGT; break;
        case OP_LT: sp.code = bind1st ? SEL_VALUEGT : SEL_VALUELT; break;
        case OP_GE: sp.code = bind1st ? SEL_VALUELE : SEL_VALUEGE; break;
        default: sp.code = bind1st ? SEL_VALUEGE : SEL_VALUELE; break;
        }
    } else {
        sp.code = canonical_op(op->type, op->op);  // (rejects the handle-only operators: GrB_DIV, GxB_POW, ...)
        if (bind1st) sp.code = flip_op(sp.code);
        if (sp.code == OP_ANY) sp.code = OP_SECOND;  // (ANY may return either operand: the bound scalar, every time)
    }
    return sp;
}
static ApplySpec spec_of_indexop(const GB_IndexUnaryOp_opaque *op, const Thunk &th)
{
    if (!op) fail(GrB_NULL_POINTER, "GrB_apply: the operator is NULL");
    if (!op_is_select(op->op) && !op_is_apply_index(op->op))
        fail(GrB_NOT_IMPLEMENTED, std::string("GrB_apply: ") + (op->name ? op->name : "the operator") + " is not implemented by libgrb_mi355x");
    ApplySpec sp{sel_is_value(op->op), op->op, op->type, th};
    if (!sp.by_value && op_is_select(op->op)) sp.xtype = TC_BOOL;
    return sp;
}
// the thunk of a positional operator: the predicates compare i + k with indices below 2^40, so |k| beyond 2^62 decides like 2^62 and
// i + k stays inside int64; ROWINDEX / COLINDEX / DIAGINDEX take k as it is (their sum wraps)
static int64_t position_thunk(const ApplySpec &sp)
{
    const int64_t k = thunk_as<int64_t>(sp.th), lim = (int64_t)1 << 62;
    return op_is_apply_index(sp.code) ? k : std::max(-lim, std::min(lim, k));
}

// t = op(a, s) for ONE entry, on the host; the bytes of t (in the operator's result type) go to `out`
template <typename X> static void apply_one_value(int code, X a, X s, unsigned char *out)
{
    switch (code) {
#define APPLY_CASE(OPC)                                        \
    case OPC: {                                                \
        const auto t = apply_val<OPC, X>(a, s);                \
        memcpy(out, &t, sizeof(t));                            \
    } break;
        APPLY_FOR_VAL(APPLY_CASE)
#undef APPLY_CASE
    default: fail(GrB_PANIC, "apply: unknown operator code");
    }
}
template <typename X> static void launch_apply_val(int code, dim3 grid, const void *xs, int64_t nnz, int vec, X s, void *out)
{
    switch (code) {
#define APPLY_CASE(OPC)                                                                                                                      \
    case OPC:                                                                                                                                \
        hipLaunchKernelGGL((k_apply_val<OPC, X>), grid, dim3(256), 0, ctx().stream, (const X *)xs, nnz, vec, s,                              \
                           (typename ApplyOut<OPC, X>::type *)out);                                                                          \
        break;
        APPLY_FOR_STREAM(APPLY_CASE)
#undef APPLY_CASE
    default: fail(GrB_PANIC, "apply: unknown operator code");
    }
}
template <typename X> static void launch_vapply_val(int code, int64_t n, const void *xs, const uint64_t *bits, X s, void *out)
{
    switch (code) {
#define APPLY_CASE(OPC)                                                                                                                      \
    case OPC:                                                                                                                                \
        hipLaunchKernelGGL((k_vapply<OPC, X, true>), grid1d(n), dim3(256), 0, ctx().stream, n, (const X *)xs, bits, (int64_t)0, s,          \
                           (typename ApplyOut<OPC, X>::type *)out);                                                                          \
        break;
        APPLY_FOR_VAL(APPLY_CASE)
#undef APPLY_CASE
    default: fail(GrB_PANIC, "apply: unknown operator code");
    }
}
// the by-position kernels: the predicates write BOOL, the index operators INT32 or INT64 (`ttype`)
static void launch_apply_pos(int code, int ttype, dim3 grid, const int64_t *Ap, int64_t m, const int32_t *Aj, int64_t nnz, int64_t nblocks, int64_t k,
                             void *out)
{
    switch (code) {
#define APPLY_CASE(OPC)                                                                                                                      \
    case OPC: hipLaunchKernelGGL((k_apply_pos<OPC, bool>), grid, dim3(256), 0, ctx().stream, Ap, m, Aj, nnz, nblocks, k, (bool *)out); break;
        APPLY_FOR_PRED(APPLY_CASE)
#undef APPLY_CASE
#define APPLY_CASE(OPC)                                                                                                                      \
    case OPC:                                                                                                                                \
        if (ttype == TC_INT32) hipLaunchKernelGGL((k_apply_pos<OPC, int32_t>), grid, dim3(256), 0, ctx().stream, Ap, m, Aj, nnz, nblocks, k, (int32_t *)out); \
        else hipLaunchKernelGGL((k_apply_pos<OPC, int64_t>), grid, dim3(256), 0, ctx().stream, Ap, m, Aj, nnz, nblocks, k, (int64_t *)out);  \
        break;
        APPLY_FOR_INDEX(APPLY_CASE)
#undef APPLY_CASE
    default: fail(GrB_PANIC, "apply: unknown operator code");
    }
}
static void launch_vapply_pos(int code, int ttype, int64_t n, const uint64_t *bits, int64_t k, void *out)
{
    const dim3 grid = grid1d(n);
    switch (code) {
#define APPLY_CASE(OPC)                                                                                                                      \
    case OPC:                                                                                                                                \
        hipLaunchKernelGGL((k_vapply<OPC, char, false>), grid, dim3(256), 0, ctx().stream, n, (const char *)nullptr, bits, k, (char)0, (bool *)out); \
        break;
        APPLY_FOR_PRED(APPLY_CASE)
#undef APPLY_CASE
#define APPLY_CASE(OPC)                                                                                                                      \
    case OPC:                                                                                                                                \
        if (ttype == TC_INT32)                                                                                                               \
            hipLaunchKernelGGL((k_vapply<OPC, int32_t, false>), grid, dim3(256), 0, ctx().stream, n, (const int32_t *)nullptr, bits, k, (int32_t)0, (int32_t *)out); \
        else                                                                                                                                 \
            hipLaunchKernelGGL((k_vapply<OPC, int64_t, false>), grid, dim3(256), 0, ctx().stream, n, (const int64_t *)nullptr, bits, k, (int64_t)0, (int64_t *)out); \
        break;
        APPLY_FOR_INDEX(APPLY_CASE)
#undef APPLY_CASE
    default: fail(GrB_PANIC, "apply: unknown operator code");
    }
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the values of T by value, in the operator's result type, into `raw`; true: T is iso (one value, no value pass)
template <typename X> static bool apply_values(const GB_Matrix_opaque *S, const ApplySpec &sp, DevPtr<char> &raw)
{
    const int code = sp.code;
    const int64_t nnz = S->nvals;
    const size_t osize = type_size(sp.ttype());
    const X s = thunk_as<X>(sp.th);
    if (S->iso || code == OP_SECOND || code == OP_PAIR) {
        X a{};
        if (S->iso) {  // A's one value, cast like every entry would be
            Thunk av{S->type->code, {0}};
            d2h(av.v, S->d_val, S->type->size);
            a = thunk_as<X>(av);
        }
        unsigned char one[8] = {0};
        apply_one_value<X>(code, a, s, one);
        raw.reset((char *)dev_alloc(osize));
        h2d(raw.p, one, osize);
        return true;
    }
    // entry and scalar meet in the operator's type: a matrix of another type costs one cast pass over the values first (11 x 11 type
    // pairs are not instantiated per operator)
    DevPtr<char> xcast;
    const void *xs = values_as(S, sp.xtype, xcast);
    ctx().stats.kernel_launches += xcast.p ? 1 : 0;
    raw.reset((char *)dev_alloc(osize * (size_t)nnz));
    constexpr int V = 16 / (int)sizeof(X);
    // (an adopted array -- GrX_Matrix_import_CSR_device without a copy -- starts wherever its owner put it)
    const int vec = aligned16(xs) && aligned16(raw.p) ? 1 : 0;
    const int64_t wgs = ceil_div(nnz, 256 * V);
    if (wgs > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
    launch_apply_val<X>(code, dim3((unsigned)wgs), xs, nnz, vec, s, raw.p);
    ctx().stats.kernel_launches += 1;
    ctx().stats.method = 13;
    ctx().stats.tiles = ceil_div(nnz, 64 * V);
    return false;
}

// T (of type `ctype`, fresh storage) = the operator applied to every entry of S.  full_values: one value per entry even when T could be
// iso (the write rule reads one value per entry when it masks or accumulates)
static MatrixOwner apply_build(GB_Matrix_opaque *S, const ApplySpec &sp, int ctype, bool full_values)
{
    MatrixOwner Tm(matrix_new(type_of_code(ctype), S->nrows, S->ncols));
    ctx().stats.method = 6;
    if (S->nvals == 0) return Tm;
    const int64_t m = (int64_t)S->nrows, nnz = S->nvals;
    // the structure of T is A's: a copy, matrix_adopt takes ownership
    DevPtr<int64_t> Tp((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1)));
    DevPtr<int32_t> Tj((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
    d2d(Tp.p, S->d_ptr, sizeof(int64_t) * (size_t)(m + 1));
    d2d(Tj.p, S->d_col, sizeof(int32_t) * (size_t)nnz);
    DevPtr<char> raw;
    bool t_iso = false;
    if (sp.by_value) {
        GRB_DISPATCH_TYPE(sp.xtype, X, { t_iso = apply_values<X>(S, sp, raw); })
    } else {
        const int64_t nblocks = ceil_div(nnz, 64), units = ceil_div(nblocks, SEL_BPW);
        const int64_t wgs = ceil_div(units, 4);
        if (wgs > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
        raw.reset((char *)dev_alloc(type_size(sp.ttype()) * (size_t)nnz));
        launch_apply_pos(sp.code, sp.ttype(), dim3((unsigned)wgs), S->d_ptr, m, S->d_col, nnz, nblocks, position_thunk(sp), raw.p);
        ctx().stats.kernel_launches += 1;
        ctx().stats.method = 14;
        ctx().stats.tiles = units;
    }
    matrix_adopt(Tm.get(), Tp.release(), Tj.release(), raw.release(), sp.ttype(), nnz, t_iso);
    if (full_values) matrix_expand_iso(Tm.get());
    GRB_HIP(hipGetLastError());
    return Tm;
}

// T (fresh, type `ctype`) = op(s, S) / op(S, s) for the binary operator `op` of type `ot` (a comparison gives BOOL), for the operations
// that end in a bound-scalar stream: the union with defaults against an empty operand (matrix_ewise_core, grb_mxm.hip)
MatrixOwner matrix_apply_bound(GB_Matrix_opaque *S, int op, int ot, bool bind1st, const Thunk &scalar, int ctype, bool full_values)
{
    const GB_BinaryOp_opaque bop{op, ot, "eWiseUnion"};
    return apply_build(S, spec_of_binop(&bop, bind1st, scalar), ctype, full_values);
}

static void matrix_apply(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, const ApplySpec &sp, GB_Matrix_opaque *A,
                         const GB_Descriptor_opaque *desc)
{
    require_init();
    check_matrix(C, "C");
    check_matrix(A, "A");
    if (Mask) check_matrix(Mask, "Mask");
    const Desc f = desc_of(desc);  // (T1 is ignored: there is no second input)
    const uint64_t in_rows = f.t0 ? A->ncols : A->nrows, in_cols = f.t0 ? A->nrows : A->ncols;
    if (C->nrows != in_rows || C->ncols != in_cols)
        fail(GrB_DIMENSION_MISMATCH, "GrB_apply: output is " + std::to_string(C->nrows) + " x " + std::to_string(C->ncols) + ", the input " +
                                         (f.t0 ? "(transposed) " : "") + std::to_string(in_rows) + " x " + std::to_string(in_cols));
    check_mask_accum("GrB_apply", C, Mask, accum);
    if (matrix_writes_nothing(C, Mask, f)) return;
    ctx().stats = GrX_Stats{};
    GB_Matrix_opaque *S = f.t0 ? matrix_transpose_cached(A) : A;
    matrix_finish(C, Mask, accum, apply_build(S, sp, C->type->code, Mask || accum), f, C == A);
    ctx().stats.out_nvals = C->nvals;
    if (ctx().blocking) sync_stream();
}

static void vector_apply(GB_Vector_opaque *w, GB_Vector_opaque *mask, const GB_BinaryOp_opaque *accum, const ApplySpec &sp, GB_Vector_opaque *u,
                         const GB_Descriptor_opaque *desc)
{
    require_init();
    // order-aware like the other element-wise operations: the positional operators need the natural index, the value ones any common order
    if (sp.by_value) {
        check_vector_any(w, "w");
        check_vector_any(u, "u");
        if (mask) check_vector_any(mask, "mask");
    } else {
        check_vector(w, "w");
        check_vector(u, "u");
        if (mask) check_vector(mask, "mask");
    }
    const Desc f = desc_of(desc);
    if (w->n != u->n) fail(GrB_DIMENSION_MISMATCH, "GrB_apply: output size " + std::to_string(w->n) + " does not match the input size " + std::to_string(u->n));
    check_vector_mask_accum("GrB_apply", w, mask, accum);
    if (vector_writes_nothing(w, mask, f)) return;
    ctx().stats = GrX_Stats{};
    if (w->n == 0) return;
    if (sp.by_value) {
        GB_Vector_opaque *vs[3] = {w, u, mask};
        (void)vectors_common_order(vs, 3);
    }
    const int64_t n = (int64_t)w->n;
    const size_t nwords = bits_words64((uint64_t)n);
    const int tt = sp.ttype(), wt = w->type->code;
    // t: u's presence bits (a copy: the write rule works in place and w may be u), the values in the operator's result type
    DevBuf<uint64_t> t_bits(nwords);
    DevBuf<char> t_val(type_size(tt) * (size_t)n);
    DevPtr<char> x_hold, t_hold;
    DevPtr<uint64_t> m_hold;
    if (!u->d_val) {
        GRB_HIP(hipMemsetAsync(t_bits.p, 0, nwords * 8, ctx().stream));
        GRB_HIP(hipMemsetAsync(t_val.p, 0, type_size(tt) * (size_t)n, ctx().stream));
    } else {
        d2d(t_bits.p, u->d_bits, nwords * 8);
        if (sp.by_value) {
            const void *xs = vector_values_as(u->d_val, u->type->code, sp.xtype, n, x_hold);
            GRB_DISPATCH_TYPE(sp.xtype, X, { launch_vapply_val<X>(sp.code, n, xs, t_bits.p, thunk_as<X>(sp.th), t_val.p); })
        } else {
            launch_vapply_pos(sp.code, tt, n, t_bits.p, position_thunk(sp), t_val.p);
        }
        ctx().stats.kernel_launches += 1;
    }
    const uint64_t *m_bits = vector_mask_words(mask, w, f.structure, m_hold);
    vector_finish(w, vector_values_as(t_val.p, tt, wt, n, t_hold), t_bits.p, m_bits, f, accum);
    GRB_HIP(hipGetLastError());
    if (ctx().blocking) sync_stream();
}

void preload_apply() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_apply_pos<APPLY_ROWINDEX, int64_t>)); (void)hipGetLastError(); }

}  // namespace grb

using namespace grb;

// ---- the _Scalar forms: an empty scalar is GrB_EMPTY_OBJECT, with its text on the output --------------------------------------------
extern "C" GrB_Info GrB_Matrix_apply_BinaryOp1st_Scalar(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op,
                                                        const GrB_Scalar x, const GrB_Matrix A, const GrB_Descriptor desc)
{
    GRB_TRY
    check_matrix(C, "C");
    matrix_apply(C, Mask, accum, spec_of_binop(op, true, thunk_of_scalar(x, "GrB_apply")), A, desc);
    GRB_CATCH(errp(C))
}
extern "C" GrB_Info GrB_Matrix_apply_BinaryOp2nd_Scalar(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op,
                                                        const GrB_Matrix A, const GrB_Scalar y, const GrB_Descriptor desc)
{
    GRB_TRY
    check_matrix(C, "C");
    matrix_apply(C, Mask, accum, spec_of_binop(op, false, thunk_of_scalar(y, "GrB_apply")), A, desc);
    GRB_CATCH(errp(C))
}
extern "C" GrB_Info GrB_Matrix_apply_IndexOp_Scalar(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op,
                                                    const GrB_Matrix A, const GrB_Scalar y, const GrB_Descriptor desc)
{
    GRB_TRY
    check_matrix(C, "C");
    matrix_apply(C, Mask, accum, spec_of_indexop(op, thunk_of_scalar(y, "GrB_apply")), A, desc);
    GRB_CATCH(errp(C))
}
extern "C" GrB_Info GrB_Vector_apply_BinaryOp1st_Scalar(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op,
                                                        const GrB_Scalar x, const GrB_Vector u, const GrB_Descriptor desc)
{
    GRB_TRY
    check_vector_any(w, "w");
    vector_apply(w, mask, accum, spec_of_binop(op, true, thunk_of_scalar(x, "GrB_apply")), u, desc);
    GRB_CATCH(errp(w))
}
extern "C" GrB_Info GrB_Vector_apply_BinaryOp2nd_Scalar(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op,
                                                        const GrB_Vector u, const GrB_Scalar y, const GrB_Descriptor desc)
{
    GRB_TRY
    check_vector_any(w, "w");
    vector_apply(w, mask, accum, spec_of_binop(op, false, thunk_of_scalar(y, "GrB_apply")), u, desc);
    GRB_CATCH(errp(w))
}
extern "C" GrB_Info GrB_Vector_apply_IndexOp_Scalar(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op,
                                                    const GrB_Vector u, const GrB_Scalar y, const GrB_Descriptor desc)
{
    GRB_TRY
    check_vector_any(w, "w");
    vector_apply(w, mask, accum, spec_of_indexop(op, thunk_of_scalar(y, "GrB_apply")), u, desc);
    GRB_CATCH(errp(w))
}

// every typed entry point accepts every operator: the scalar is cast to the operator's type (to INT64 for a positional one)
#define DEF_APPLY_TYPED(NAME, ctype)                                                                                                             \
    extern "C" GrB_Info GrB_Matrix_apply_BinaryOp1st_##NAME(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, \
                                                            ctype x, const GrB_Matrix A, const GrB_Descriptor desc)                              \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        check_matrix(C, "C");                                                                                                                    \
        matrix_apply(C, Mask, accum, spec_of_binop(op, true, thunk_of<ctype>(TC_##NAME, x)), A, desc);                                           \
        GRB_CATCH(errp(C))                                                                                                                       \
    }                                                                                                                                            \
    extern "C" GrB_Info GrB_Matrix_apply_BinaryOp2nd_##NAME(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, \
                                                            const GrB_Matrix A, ctype y, const GrB_Descriptor desc)                              \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        check_matrix(C, "C");                                                                                                                    \
        matrix_apply(C, Mask, accum, spec_of_binop(op, false, thunk_of<ctype>(TC_##NAME, y)), A, desc);                                          \
        GRB_CATCH(errp(C))                                                                                                                       \
    }                                                                                                                                            \
    extern "C" GrB_Info GrB_Matrix_apply_IndexOp_##NAME(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op, \
                                                        const GrB_Matrix A, ctype y, const GrB_Descriptor desc)                                  \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        check_matrix(C, "C");                                                                                                                    \
        matrix_apply(C, Mask, accum, spec_of_indexop(op, thunk_of<ctype>(TC_##NAME, y)), A, desc);                                               \
        GRB_CATCH(errp(C))                                                                                                                       \
    }                                                                                                                                            \
    extern "C" GrB_Info GrB_Vector_apply_BinaryOp1st_##NAME(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, \
                                                            ctype x, const GrB_Vector u, const GrB_Descriptor desc)                              \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        check_vector_any(w, "w");                                                                                                                \
        vector_apply(w, mask, accum, spec_of_binop(op, true, thunk_of<ctype>(TC_##NAME, x)), u, desc);                                           \
        GRB_CATCH(errp(w))                                                                                                                       \
    }                                                                                                                                            \
    extern "C" GrB_Info GrB_Vector_apply_BinaryOp2nd_##NAME(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, \
                                                            const GrB_Vector u, ctype y, const GrB_Descriptor desc)                              \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        check_vector_any(w, "w");                                                                                                                \
        vector_apply(w, mask, accum, spec_of_binop(op, false, thunk_of<ctype>(TC_##NAME, y)), u, desc);                                          \
        GRB_CATCH(errp(w))                                                                                                                       \
    }                                                                                                                                            \
    extern "C" GrB_Info GrB_Vector_apply_IndexOp_##NAME(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_IndexUnaryOp op, \
                                                        const GrB_Vector u, ctype y, const GrB_Descriptor desc)                                  \
    {                                                                                                                                            \
        GRB_TRY                                                                                                                                  \
        check_vector_any(w, "w");                                                                                                                \
        vector_apply(w, mask, accum, spec_of_indexop(op, thunk_of<ctype>(TC_##NAME, y)), u, desc);                                               \
        GRB_CATCH(errp(w))                                                                                                                       \
    }
GRB_FOR_EACH_TYPE(DEF_APPLY_TYPED)
#undef DEF_APPLY_TYPED
