// grb_kron.hip -- GrB_kronecker: C<Mask, replace> = accum(C, T), T = A (x) B under a binary operator (C API 2.0 section 4.3.11; reference
// core/matrix.py kronecker -> GrB_Matrix_kronecker_{BinaryOp,Monoid,Semiring}).  DESIGN.md section 4.11.
//
// T is (ma mb) x (na nb): T[ia mb + ib, ja nb + jb] = op((X) A[ia, ja], (X) B[ib, jb]) for every pair of stored entries, X = the
// operator's type (BOOL for GrB_EQ .. GrB_LE); A' / B' under GrB_DESC_T0 / T1; the _Semiring form takes the multiply operator.
//
// The structure has a closed form -- no count pass, no scan.  Row ia mb + ib of T holds lenA(ia) lenB(ib) entries, already sorted: the
// A entries of row ia in order, under each the B entries of row ib in order.  So
//     Tp[ia mb + ib] = Ap[ia] nnz(B) + lenA(ia) Bp[ib]            nnz(T) = nnz(A) nnz(B)
// and entry p of that row is A entry Ap[ia] + p / lenB(ib) with B entry Bp[ib] + p % lenB(ib), at column ja nb + jb.
//
// Two kernels: k_kron_ptr writes the ma mb + 1 row pointers; k_kron_fill is ordered by OUTPUT entry -- a wavefront takes SEL_BPW
// consecutive blocks of 64 entries of T, finds the row of its first entry by one search in Tp and walks on from there
// (walk_first_row / walk_block_rows, grb_index_ops.hpp), so that every block is 64 consecutive columns and 64 consecutive values:
// whole lines, whatever the row lengths of the operands are.  A and B are tiny beside T and are re-read from cache.
// Short cuts, all exact: an empty operand gives an empty T; PAIR, FIRST with an iso A, SECOND with an iso B and two iso operands give
// an iso T, its one value computed on the host and only the columns written (the structure-only instantiation of k_kron_fill).  ANY
// may return either operand of a pair: the first, every time -- it runs as FIRST.
// GrX_last_stats: method 20 when the value fill ran, 6 for the short cuts; tiles = wavefront units; out_nvals = nnz(C).
#include "grb_index_ops.hpp"

namespace grb {

// ---- the operators -------------------------------------------------------------------------------------------------------------
// An operator code of the fill: a binary operator of OpCode, or SEL_VALUE* for a comparison (a cmp b -> BOOL, the predicates of
// GrB_select).  KRON_STRUCTURE: no values at all.
constexpr int KRON_STRUCTURE = -2;
template <int OP, typename X> struct KronOut {
    using type = typename std::conditional<(OP >= SEL_VALUEEQ && OP <= SEL_VALUELE), bool, X>::type;
};
template <int OP, typename X> GRB_HD typename KronOut<OP, X>::type kron_val(X a, X b)
{
    if constexpr (OP >= SEL_VALUEEQ) return sel_val<OP, X>(a, b);
    else return apply_binop<X>(OP, a, b);
}
// (PAIR -- and ANY, which is FIRST here -- never reach the kernel with values: one value, computed by kron_one_value)
#define KRON_FOR_FILL(X)                                                                                                            \
    X(OP_FIRST) X(OP_SECOND) X(OP_PLUS) X(OP_MINUS) X(OP_RMINUS) X(OP_TIMES) X(OP_MIN) X(OP_MAX) X(OP_LOR) X(OP_LAND) X(OP_LXOR)     \
    X(OP_LXNOR) X(SEL_VALUEEQ) X(SEL_VALUENE) X(SEL_VALUEGT) X(SEL_VALUEGE) X(SEL_VALUELT) X(SEL_VALUELE)
#define KRON_FOR_VAL(X) KRON_FOR_FILL(X) X(OP_PAIR)

static int kron_code_of_comparison(int op)
{
    switch (op) {
    case OP_EQ: return SEL_VALUEEQ;
    case OP_NE: return SEL_VALUENE;
    case OP_GT: return SEL_VALUEGT;
    case OP_LT: return SEL_VALUELT;
    case OP_GE: return SEL_VALUEGE;
    default: return SEL_VALUELE;
    }
}

// ---- the row pointers ------------------------------------------------------------------------------------------------------------
__global__ void k_kron_ptr(const int64_t *__restrict__ Ap, const int64_t *__restrict__ Bp, int64_t ma, int64_t mb, int64_t nnzb, int64_t *__restrict__ Tp)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, rows = ma * mb;
    if (r > rows) return;
    if (r == rows) {
        Tp[r] = Ap[ma] * nnzb;
        return;
    }
    const int64_t ia = r / mb, ib = r - ia * mb;
    const int64_t a0 = Ap[ia];
    Tp[r] = a0 * nnzb + (Ap[ia + 1] - a0) * Bp[ib];
}

// n = q d + r, exact; with 32-bit arithmetic where both fit (the 64-bit division is a long software loop on the device)
__device__ __forceinline__ void kron_divmod(int64_t n, int64_t d, int64_t &q, int64_t &r)
{
    if ((((uint64_t)n | (uint64_t)d) >> 32) == 0) {
        const uint32_t qq = (uint32_t)n / (uint32_t)d;
        q = qq;
        r = (uint32_t)n - qq * (uint32_t)d;
    } else {
        q = n / d;
        r = n - q * d;
    }
}

// ---- the fill: entry-parallel over T, the rows by the walk of k_select_flag -----------------------------------------------------------
// a_step / b_step: 1, or 0 for an iso operand (its one value); OP == KRON_STRUCTURE writes the columns alone
template <int OP, typename X>
__global__ void __launch_bounds__(256) k_kron_fill(const int64_t *__restrict__ Tp, int64_t rows, int64_t mb, int64_t nb, const int64_t *__restrict__ Ap,
                                                   const int32_t *__restrict__ Aj, const X *__restrict__ Ax, int64_t a_step, const int64_t *__restrict__ Bp,
                                                   const int32_t *__restrict__ Bj, const X *__restrict__ Bx, int64_t b_step, int64_t nnz, int64_t nblocks,
                                                   int32_t *__restrict__ Tj, typename KronOut<OP, X>::type *__restrict__ Tx)
{
    __shared__ int64_t s_end[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * SEL_BPW;
    const int64_t b1 = b0 + SEL_BPW < nblocks ? b0 + SEL_BPW : nblocks;
    int64_t r = 0;  // (wave-uniform) the row of the first entry of the current block
    if (b0 < b1) r = walk_first_row(Tp, rows, b0 << 6);
    for (int64_t b = b0; b < b1; b++) {
        const int64_t p = b << 6, e = p + lane;
        const int64_t row = walk_block_rows(Tp, rows, nnz, p, lane, s_end[wave], r);
        if (e < nnz) {
            int64_t ia, ib, qa, qb;
            kron_divmod(row, mb, ia, ib);
            const int64_t bs = Bp[ib], lenb = Bp[ib + 1] - bs;  // (lenb > 0: the row holds entry e)
            kron_divmod(e - Tp[row], lenb, qa, qb);
            const int64_t ea = Ap[ia] + qa, eb = bs + qb;
            Tj[e] = (int32_t)((int64_t)Aj[ea] * nb + (int64_t)Bj[eb]);  // (below 2^31: checked by the host)
            if constexpr (OP != KRON_STRUCTURE) Tx[e] = kron_val<OP, X>(Ax[ea * a_step], Bx[eb * b_step]);
        }
    }
}

// t = op(a, b) for ONE pair, on the host; the bytes of t (in the operator's result type) go to `out`
template <typename X> static void kron_one_value(int code, X a, X b, unsigned char *out)
{
    switch (code) {
#define KRON_CASE(OPC)                                        \
    case OPC: {                                               \
        const auto t = kron_val<OPC, X>(a, b);                \
        memcpy(out, &t, sizeof(t));                           \
    } break;
        KRON_FOR_VAL(KRON_CASE)
#undef KRON_CASE
    default: fail(GrB_PANIC, "kronecker: unknown operator code");
    }
}

struct KronArgs {
    const int64_t *Tp, *Ap, *Bp;
    const int32_t *Aj, *Bj;
    int64_t rows, mb, nb, a_step, b_step, nnz, nblocks;
    int32_t *Tj;
};
template <typename X> static void launch_kron_fill(int code, dim3 grid, const KronArgs &k, const void *Ax, const void *Bx, void *out)
{
    switch (code) {
#define KRON_CASE(OPC)                                                                                                                       \
    case OPC:                                                                                                                                \
        hipLaunchKernelGGL((k_kron_fill<OPC, X>), grid, dim3(256), 0, ctx().stream, k.Tp, k.rows, k.mb, k.nb, k.Ap, k.Aj, (const X *)Ax,      \
                           k.a_step, k.Bp, k.Bj, (const X *)Bx, k.b_step, k.nnz, k.nblocks, k.Tj, (typename KronOut<OPC, X>::type *)out);     \
        break;
        KRON_FOR_FILL(KRON_CASE)
#undef KRON_CASE
    default: fail(GrB_PANIC, "kronecker: unknown operator code");
    }
}

// M's first stored value (its one value when iso), cast to X like every entry would be
template <typename X> static X kron_first_value(const GB_Matrix_opaque *M)
{
    Thunk v{M->type->code, {0}};
    d2h(v.v, M->d_val, M->type->size);
    return thunk_as<X>(v);
}

// T (fresh, of the operator's result type `tt`) = A (x) B under operator `code` over type `ot`
static MatrixOwner kron_build(GB_Matrix_opaque *A, GB_Matrix_opaque *B, int code, int ot, int tt, uint64_t t_rows, uint64_t t_cols)
{
    MatrixOwner Tm(matrix_new(type_of_code(tt), t_rows, t_cols));
    ctx().stats.method = 6;
    if (A->nvals == 0 || B->nvals == 0) return Tm;
    if (t_cols > 0x7fffffffull) fail(GrB_NOT_IMPLEMENTED, "matrices with entries need ncols < 2^31 (int32 column indices)");
    int64_t nnz = 0;
    if (__builtin_mul_overflow(A->nvals, B->nvals, &nnz) || nnz > INT64_MAX / 16)
        fail(GrB_OUT_OF_MEMORY, "kronecker: the product of " + std::to_string(A->nvals) + " and " + std::to_string(B->nvals) + " entries does not fit");
    if (t_rows >= (uint64_t)INT64_MAX / 16) fail(GrB_OUT_OF_MEMORY, "kronecker: " + std::to_string(t_rows) + " row pointers do not fit");
    const int64_t ma = (int64_t)A->nrows, mb = (int64_t)B->nrows, rows = (int64_t)t_rows;
    if (code == OP_ANY) code = OP_FIRST;  // (ANY may return either operand: the first, every time)
    const bool t_iso = (A->iso && B->iso) || code == OP_PAIR || (code == OP_FIRST && A->iso) || (code == OP_SECOND && B->iso);
    const size_t osize = type_size(tt);
    DevPtr<int64_t> Tp((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(rows + 1)));
    DevPtr<int32_t> Tj((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
    DevPtr<char> raw((char *)dev_alloc(osize * (size_t)(t_iso ? 1 : nnz)));
    hipLaunchKernelGGL(k_kron_ptr, grid1d(rows + 1), dim3(256), 0, ctx().stream, (const int64_t *)A->d_ptr, (const int64_t *)B->d_ptr, ma, mb, B->nvals,
                       Tp.p);
    const int64_t nblocks = ceil_div(nnz, 64), units = ceil_div(nblocks, SEL_BPW);
    const int64_t wgs = ceil_div(units, 4);
    if (wgs > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
    KronArgs k{Tp.p, A->d_ptr, B->d_ptr, A->d_col, B->d_col, rows, mb, (int64_t)B->ncols, A->iso ? 0 : 1, B->iso ? 0 : 1, nnz, nblocks, Tj.p};
    if (t_iso) {
        unsigned char one[8] = {0};
        GRB_DISPATCH_TYPE(ot, X, { kron_one_value<X>(code, kron_first_value<X>(A), kron_first_value<X>(B), one); })
        h2d(raw.p, one, osize);
        hipLaunchKernelGGL((k_kron_fill<KRON_STRUCTURE, char>), dim3((unsigned)wgs), dim3(256), 0, ctx().stream, k.Tp, k.rows, k.mb, k.nb, k.Ap, k.Aj,
                           (const char *)nullptr, k.a_step, k.Bp, k.Bj, (const char *)nullptr, k.b_step, k.nnz, k.nblocks, k.Tj, (char *)nullptr);
    } else {
        // the operands meet in the operator's type: an operand of another type costs one cast pass over its values first
        DevPtr<char> a_cast, b_cast;
        const void *Ax = values_as(A, ot, a_cast), *Bx = values_as(B, ot, b_cast);
        ctx().stats.kernel_launches += (a_cast.p ? 1 : 0) + (b_cast.p ? 1 : 0);
        GRB_DISPATCH_TYPE(ot, X, { launch_kron_fill<X>(code, dim3((unsigned)wgs), k, Ax, Bx, raw.p); })
        ctx().stats.method = 20;
    }
    ctx().stats.kernel_launches += 2;
    ctx().stats.tiles = units;
    matrix_adopt(Tm.get(), Tp.release(), Tj.release(), raw.release(), tt, nnz, t_iso);
    GRB_HIP(hipGetLastError());
    return Tm;
}

// `op_in` / `ot`: the operator's code and type
static void matrix_kron_core(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, int op_in, int ot, GB_Matrix_opaque *A,
                             GB_Matrix_opaque *B, const GB_Descriptor_opaque *desc)
{
    const Desc f = desc_of(desc);
    const uint64_t a_rows = f.t0 ? A->ncols : A->nrows, a_cols = f.t0 ? A->nrows : A->ncols;
    const uint64_t b_rows = f.t1 ? B->ncols : B->nrows, b_cols = f.t1 ? B->nrows : B->ncols;
    uint64_t t_rows = 0, t_cols = 0;
    const bool fits = !__builtin_mul_overflow(a_rows, b_rows, &t_rows) && !__builtin_mul_overflow(a_cols, b_cols, &t_cols);
    if (!fits || C->nrows != t_rows || C->ncols != t_cols)
        fail(GrB_DIMENSION_MISMATCH, "kronecker: output is " + std::to_string(C->nrows) + " x " + std::to_string(C->ncols) + ", the product of " +
                                         std::to_string(a_rows) + " x " + std::to_string(a_cols) + " and " + std::to_string(b_rows) + " x " +
                                         std::to_string(b_cols) + (fits ? " is " + std::to_string(t_rows) + " x " + std::to_string(t_cols) : " is beyond 2^64"));
    check_mask_accum("kronecker", C, Mask, accum);
    const bool cmp = op_is_comparison(op_in);
    const int code = cmp ? kron_code_of_comparison(op_in) : canonical_op(ot, op_in);  // (rejects the handle-only operators: GrB_DIV, GxB_POW, ...)
    const int tt = cmp ? (int)TC_BOOL : ot;
    ctx().stats = GrX_Stats{};
    if (matrix_writes_nothing(C, Mask, f)) return;
    GB_Matrix_opaque *Ae = f.t0 ? matrix_transpose_cached(A) : A;
    GB_Matrix_opaque *Be = f.t1 ? matrix_transpose_cached(B) : B;
    MatrixOwner Tm = kron_build(Ae, Be, code, ot, tt, t_rows, t_cols);
    matrix_retype(Tm.get(), tt, C->type->code);  // T in the output type
    if (Mask || accum) matrix_expand_iso(Tm.get());  // (the write rule reads one value per entry when it masks or accumulates)
    matrix_finish(C, Mask, accum, std::move(Tm), f, C == A || C == B);
    ctx().stats.out_nvals = C->nvals;
    if (ctx().blocking) sync_stream();
}

void preload_kron() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_kron_ptr)); (void)hipGetLastError(); }

}  // namespace grb

using namespace grb;

// the _Semiring form takes the multiply operator, as eWiseMult does (C API 2.0 section 4.3.11)
#define GRB_MATRIX_KRON(FUNC, HANDLE, CODE)                                                                                       \
    extern "C" GrB_Info FUNC(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const HANDLE op, const GrB_Matrix A, \
                             const GrB_Matrix B, const GrB_Descriptor desc)                                                      \
    {                                                                                                                             \
        GRB_TRY                                                                                                                   \
        require_init();                                                                                                           \
        check_matrix(C, "C");                                                                                                     \
        if (Mask) check_matrix(Mask, "Mask");                                                                                     \
        check_matrix(A, "A");                                                                                                     \
        check_matrix(B, "B");                                                                                                     \
        if (!op) fail(GrB_NULL_POINTER, "kronecker: operator is NULL");                                                           \
        matrix_kron_core(C, Mask, accum, op->CODE, op->type, A, B, desc);                                                        \
        GRB_CATCH(errp(C))                                                                                                        \
    }
GRB_MATRIX_KRON(GrB_Matrix_kronecker_BinaryOp, GrB_BinaryOp, op)
GRB_MATRIX_KRON(GrB_Matrix_kronecker_Monoid, GrB_Monoid, op)
GRB_MATRIX_KRON(GrB_Matrix_kronecker_Semiring, GrB_Semiring, mult)
#undef GRB_MATRIX_KRON
