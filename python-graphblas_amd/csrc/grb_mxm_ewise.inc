// grb_mxm_ewise.inc -- T = A (op) B element-wise on two matrices with sorted CSR rows: over the UNION of the patterns (eWiseAdd: an
// entry one side alone holds passes through) or their INTERSECTION (eWiseMult), a WAVEFRONT per unit (part of grb_mxm.hip; DESIGN.md
// section 4.6).
//
// Reference: graphblas/core/matrix.py ewise_add / ewise_mult -> GrB_Matrix_eWiseAdd_* / GrB_Matrix_eWiseMult_* (C API 2.0 sections
// 4.3.4 / 4.3.5); the vector form is ewise_core of grb_vecops.hip, whose semantics these follow.
//
// The two-list case of the merge of grb_mxm_write.inc, with its helpers and its unit tables as they are:
//   * a unit is a row, or -- for rows with more than WR_LONG entries in A and B together -- a (row, column piece) pair;
//   * per step lane l loads entry l of the next chunk of A(i,:) and of B(i,:); the step's BOUND is the smaller last-loaded column
//     over the lists that still have unloaded entries; every A entry up to the bound finds its partner in the B chunk by a 6-step
//     search in LDS (and reads the partner's value there), every B entry up to the bound learns the same way whether A holds it;
//   * an emitted entry's position = emitted entries of its own list before it + emitted entries of the other list below its column
//     -- two popcounts of ballots; no atomics;
//   * counts per unit -> one scan -> the same walk fills.
// An iso operand is read as its single value.  Comparison operators write BOOL (k_ewise_cmp of grb_vecops.hip is the vector precedent).
// The union WITH DEFAULTS (GxB_Matrix_eWiseUnion; DESIGN.md section 4.12) is the same walk and the same count: only the fill differs --
// an entry of A alone is op(a, beta), an entry of B alone op(alpha, b), where eWiseAdd passes a and b through.
// LDS: 2 column chunks + 1 value chunk per wavefront = 2 KiB + 256 sizeof(T) per workgroup (k_mat_write_wave: 3 KiB + 256 sizeof(T)).
#pragma once

struct EwiseArgs {
    const int64_t *Ap;
    const int32_t *Aj;
    const void *Ax;
    int a_iso;
    const int64_t *Bp;
    const int32_t *Bj;
    const void *Bx;
    int b_iso;
    int op;                // canonical binary operator, or a comparison code (CMP kernels)
    // units (k_write_units_per_row / k_write_unit_rows of the write rule)
    const int64_t *ubase;  // first unit of every row (m + 1)
    const int32_t *urow;   // the row of every unit
    int64_t n_units;
    int piece_cols;        // columns per piece of a cut row
    int64_t *ucount;       // count pass: entries the unit emits
    const int64_t *uoff;   // fill pass: where the unit writes
    int32_t *Tj;
    void *Tx;
    // REGION kernels (GrB_assign without an accumulator, grb_assign.hip): an entry of A alone is dropped when its row is selected
    // (rinv == nullptr: every row) and its column lies in the assigned columns (jbits == nullptr: the range [jlo, jhi))
    const int32_t *rinv;
    const unsigned long long *jbits;
    int jlo, jhi;
    // DEFS kernels (GxB_Matrix_eWiseUnion): the value that stands in for the absent A entry / B entry, in the operator's type
    alignas(8) unsigned char alpha[8], beta[8];
};

template <typename T>
__device__ __forceinline__ bool ewise_compare(int op, T a, T b)
{
    switch (op) {
    case OP_EQ: return a == b;
    case OP_NE: return a != b;
    case OP_GT: return a > b;
    case OP_LT: return a < b;
    case OP_GE: return a >= b;
    default: return a <= b;
    }
}

// T: the operator's type (both operands are in it); CMP: `op` is a comparison and the result BOOL; REGION: the assign flavour of the
// union (EwiseArgs::rinv); DEFS: the union with defaults (EwiseArgs::alpha / beta; fill pass only)
template <typename T, bool UNION, bool FILL, bool CMP, bool REGION = false, bool DEFS = false>
__global__ __launch_bounds__(256) void k_mat_ewise_wave(const EwiseArgs a)
{
    using TO = typename std::conditional<CMP, bool, T>::type;
    constexpr int COL_END = 0x7fffffff;
    __shared__ int s_a[4][64], s_b[4][64];
    __shared__ T s_bv[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t unit = (int64_t)blockIdx.x * 4 + wv;
    if (unit >= a.n_units) return;  // (uniform over the wavefront)
    const int64_t row = a.urow[unit];
    const int64_t u0 = a.ubase[row], pieces = a.ubase[row + 1] - u0;
    int64_t pa = a.Ap[row], ea = a.Ap[row + 1], pb = a.Bp[row], eb = a.Bp[row + 1];
    if (pieces > 1) {  // this wavefront's column piece of a long row
        const int64_t piece = unit - u0;
        const int64_t c_lo = piece * a.piece_cols, c_hi = c_lo + a.piece_cols;
        const int k_lo = (int)c_lo, k_hi = (piece == pieces - 1 || c_hi >= COL_END) ? COL_END : (int)c_hi;
        pa = wave_lower_bound(a.Aj, pa, ea, k_lo, lane);
        ea = wave_lower_bound(a.Aj, pa, ea, k_hi, lane);
        pb = wave_lower_bound(a.Bj, pb, eb, k_lo, lane);
        eb = wave_lower_bound(a.Bj, pb, eb, k_hi, lane);
    }
    const T *Ax = (const T *)a.Ax, *Bx = (const T *)a.Bx;
    TO *Tx = (TO *)a.Tx;
    int *sa = s_a[wv], *sb = s_b[wv];
    T *sbv = s_bv[wv];
    const int op = a.op;
    T alpha = (T)0, beta = (T)0;
    if constexpr (DEFS) {
        __builtin_memcpy(&alpha, a.alpha, sizeof(T));
        __builtin_memcpy(&beta, a.beta, sizeof(T));
    }
    bool row_in = false;  // (REGION, wave-uniform) the row is one of the assigned rows
    if constexpr (REGION) row_in = a.rinv ? a.rinv[row] >= 0 : true;
    int64_t out = FILL ? a.uoff[unit] : 0, cnt = 0;
    // (the intersection is complete as soon as one list is: what the other still holds has no partner)
    while (UNION ? (pa < ea || pb < eb) : (pa < ea && pb < eb)) {
        // ---- the next chunk of both lists
        const bool a_in = pa + lane < ea, b_in = pb + lane < eb;
        const int aj = a_in ? a.Aj[pa + lane] : COL_END, bj = b_in ? a.Bj[pb + lane] : COL_END;
        T av = (T)0, bv = (T)0;
        if (FILL && a_in) av = Ax[a.a_iso ? 0 : pa + lane];
        if (FILL && b_in) bv = Bx[a.b_iso ? 0 : pb + lane];
        sa[lane] = aj;
        sb[lane] = bj;
        sbv[lane] = bv;
        // the step's bound: the smaller last-loaded column over the lists with entries still unloaded (v_readlane, as in k_mat_write_wave)
        const int last_a = ea - pa > 64 ? __builtin_amdgcn_readlane(aj, 63) : COL_END, last_b = eb - pb > 64 ? __builtin_amdgcn_readlane(bj, 63) : COL_END;
        const int bound = last_a < last_b ? last_a : last_b;
        mw_sync();
        const bool use_a = a_in && aj <= bound, use_b = b_in && bj <= bound;
        bool emit_a = false, emit_b = false;
        TO za = (TO)0, zb = (TO)0;
        int lb_b = 0, lb_a = 0;
        // ---- A entries: partner in the B chunk
        if (use_a) {
            lb_b = chunk_lower_bound(sb, aj);
            const bool hb = lb_b < 64 && sb[lb_b] == aj;
            emit_a = UNION || hb;
            if constexpr (REGION) {
                if (!hb && row_in && (a.jbits ? ((a.jbits[aj >> 6] >> (aj & 63)) & 1ull) != 0 : (aj >= a.jlo && aj < a.jhi))) emit_a = false;
            }
            if (FILL) {
                if (hb) {
                    if constexpr (CMP) za = ewise_compare<T>(op, av, sbv[lb_b]);
                    else za = apply_binop<T>(op, av, sbv[lb_b]);
                } else if constexpr (DEFS) {
                    if constexpr (CMP) za = ewise_compare<T>(op, av, beta);
                    else za = apply_binop<T>(op, av, beta);
                } else {
                    za = cast_value<TO, T>(av);
                }
            }
        }
        // ---- B entries without a partner in A
        if (UNION && use_b) {
            lb_a = chunk_lower_bound(sa, bj);
            emit_b = !(lb_a < 64 && sa[lb_a] == bj);
            if constexpr (DEFS) {
                if constexpr (CMP) zb = ewise_compare<T>(op, alpha, bv);
                else zb = apply_binop<T>(op, alpha, bv);
            } else {
                zb = cast_value<TO, T>(bv);
            }
        }
        const unsigned long long e_a = __ballot(emit_a), e_b = __ballot(emit_b);
        if (FILL) {
            const unsigned long long mine = bits_below(lane);
            if (emit_a) {
                const int64_t o = out + cnt + __popcll(e_a & mine) + __popcll(e_b & bits_below(lb_b));
                a.Tj[o] = aj;
                Tx[o] = za;
            }
            if (emit_b) {
                const int64_t o = out + cnt + __popcll(e_b & mine) + __popcll(e_a & bits_below(lb_a));
                a.Tj[o] = bj;
                Tx[o] = zb;
            }
        }
        cnt += __popcll(e_a) + __popcll(e_b);
        pa += __popcll(__ballot(use_a));
        pb += __popcll(__ballot(use_b));
        mw_sync();
    }
    if (!FILL && lane == 0) a.ucount[unit] = cnt;
}

template <typename T>
static void launch_ewise_fill(bool is_add, bool cmp, dim3 grid, const EwiseArgs &ea, bool region = false, bool defs = false)
{
    const dim3 block(256);
    if (defs) {
        if (cmp) hipLaunchKernelGGL((k_mat_ewise_wave<T, true, true, true, false, true>), grid, block, 0, ctx().stream, ea);
        else hipLaunchKernelGGL((k_mat_ewise_wave<T, true, true, false, false, true>), grid, block, 0, ctx().stream, ea);
    } else if (region) {
        hipLaunchKernelGGL((k_mat_ewise_wave<T, true, true, false, true>), grid, block, 0, ctx().stream, ea);
    } else if (is_add) {
        if (cmp) hipLaunchKernelGGL((k_mat_ewise_wave<T, true, true, true>), grid, block, 0, ctx().stream, ea);
        else hipLaunchKernelGGL((k_mat_ewise_wave<T, true, true, false>), grid, block, 0, ctx().stream, ea);
    } else {
        if (cmp) hipLaunchKernelGGL((k_mat_ewise_wave<T, false, true, true>), grid, block, 0, ctx().stream, ea);
        else hipLaunchKernelGGL((k_mat_ewise_wave<T, false, true, false>), grid, block, 0, ctx().stream, ea);
    }
}

// T (fresh storage, type `tt`) = A (op) B; Ax / Bx: the operands' values in the operator's type `ot` (one value when iso); both
// operands hold entries (or, an empty one, at least its row pointers).  reg: the assign flavour of the union.  defs: the union with
// defaults -- alpha, then beta, 8 bytes each, in type `ot`
static MatrixOwner ewise_merge(GB_Matrix_opaque *A, const void *Ax, GB_Matrix_opaque *B, const void *Bx, int ot, int tt, int op, bool is_add, bool cmp,
                               const MergeRegion *reg = nullptr, const unsigned char *defs = nullptr)
{
    MatrixOwner Tm(matrix_new(type_of_code(tt), A->nrows, A->ncols));
    const int64_t m = (int64_t)A->nrows;
    EwiseArgs ea{};
    ea.Ap = A->d_ptr; ea.Aj = A->d_col; ea.Ax = Ax; ea.a_iso = A->iso ? 1 : 0;
    ea.Bp = B->d_ptr; ea.Bj = B->d_col; ea.Bx = Bx; ea.b_iso = B->iso ? 1 : 0;
    ea.op = op;
    if (reg) { ea.rinv = reg->rinv; ea.jbits = reg->jbits; ea.jlo = (int)reg->jlo; ea.jhi = (int)reg->jhi; }
    if (defs) { memcpy(ea.alpha, defs, 8); memcpy(ea.beta, defs + 8, 8); }
    const UnitTable ut = unit_table(ea.Ap, ea.Bp, m, (int64_t)A->ncols);
    if (ut.n_units == 0) {
        ctx().stats.kernel_launches += 2;
        return Tm;
    }
    int64_t nnzT = 0;
    DevBuf<int64_t> uoff(ut.n_units + 1, true);
    ea.ubase = ut.ubase.p; ea.urow = ut.urow.p; ea.n_units = ut.n_units; ea.piece_cols = ut.piece_cols; ea.ucount = uoff.p;
    const dim3 grid = ut.grid(), block(256);
    // (the count pass reads no value: one instantiation per pattern rule)
    if (reg) hipLaunchKernelGGL((k_mat_ewise_wave<uint8_t, true, false, false, true>), grid, block, 0, ctx().stream, ea);
    else if (is_add) hipLaunchKernelGGL((k_mat_ewise_wave<uint8_t, true, false, false>), grid, block, 0, ctx().stream, ea);
    else hipLaunchKernelGGL((k_mat_ewise_wave<uint8_t, false, false, false>), grid, block, 0, ctx().stream, ea);
    prim_exclusive_sum_i64(uoff.p, uoff.p, ut.n_units + 1);
    d2h(&nnzT, uoff.p + ut.n_units, sizeof(int64_t));
    ctx().stats.kernel_launches += 5;
    if (nnzT) {
        Tm->d_ptr = (int64_t *)dev_alloc(sizeof(int64_t) * (m + 1));
        unit_table_rowptr(ut, uoff.p, m, Tm->d_ptr);
        Tm->d_col = (int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnzT);
        Tm->d_val = dev_alloc(type_size(tt) * (size_t)nnzT);
        ea.uoff = uoff.p; ea.Tj = Tm->d_col; ea.Tx = Tm->d_val;
        GRB_DISPATCH_TYPE(ot, TO, { launch_ewise_fill<TO>(is_add, cmp, grid, ea, reg != nullptr, defs != nullptr); })
        ctx().stats.kernel_launches += 2;
    }
    Tm->nvals = nnzT;
    GRB_HIP(hipGetLastError());
    sync_stream();  // (the unit tables are released at the end of this scope)
    return Tm;
}

// T = the entries of S as eWiseAdd passes them through when the other operand is empty: cast to the operator's type `ot`, to the
// element-wise result type `tt`, then to `ctype`.  full_values: one value per entry even when S is iso (the write rule reads one value
// per entry of T when it masks or accumulates)
static MatrixOwner ewise_pass_through(GB_Matrix_opaque *S, int ot, int tt, int ctype, bool full_values)
{
    MatrixOwner Tm(matrix_cast_copy(S, ot));
    matrix_retype(Tm.get(), ot, tt);
    matrix_retype(Tm.get(), tt, ctype);
    if (full_values) matrix_expand_iso(Tm.get());
    GRB_HIP(hipGetLastError());
    return Tm;
}

// Z (fresh storage, C's type, one value per entry) = the union of C and S, `op` where both hold an entry; S is in C's type.  With `reg`
// (GrB_assign without an accumulator: op = SECOND) an entry of C alone inside the region is dropped.  DESIGN.md section 4.10
MatrixOwner matrix_merge_region(GB_Matrix_opaque *C, GB_Matrix_opaque *S, int op, const MergeRegion *reg)
{
    const int ct = C->type->code;
    if (C->nvals == 0 || (S->nvals == 0 && !reg)) {
        MatrixOwner Z(matrix_cast_copy(C->nvals ? C : S, ct));
        matrix_expand_iso(Z.get());
        return Z;
    }
    matrix_rowptr(S);
    return ewise_merge(C, C->d_val, S, S->d_val, ct, ct, op, true, false, reg);
}
