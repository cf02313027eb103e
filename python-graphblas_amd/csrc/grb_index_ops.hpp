// grb_index_ops.hpp -- what GrB_select (grb_select.hip) and GrB_apply (grb_apply.hip) share: the thunk of a call, the arithmetic of the
// builtin index-unary operators, and the walk that gives every entry of a CSR matrix its row without reading one row pointer per entry.
#pragma once
#include "grb_internal.hpp"
#include "grb_ops.hpp"

namespace grb {

struct Thunk {  // the scalar of a select / apply call: its type and its bytes
    int type;
    unsigned char v[8];
};
template <typename X> static Thunk thunk_of(int type, X x)
{
    Thunk t{type, {0}};
    memcpy(t.v, &x, sizeof(X));
    return t;
}
template <typename D> static D thunk_as(const Thunk &t)
{
    D out{};
    GRB_DISPATCH_TYPE(t.type, TY, {
        TY y;
        memcpy(&y, t.v, sizeof(TY));
        out = cast_value<D, TY>(y);
    })
    return out;
}
// `who` prefixes the error text ("GrB_select", "GrB_apply")
static inline Thunk thunk_of_scalar(const GB_Scalar_opaque *y, const char *who)
{
    if (!y) fail(GrB_NULL_POINTER, std::string(who) + ": the thunk scalar is NULL");
    if (y->magic != MAGIC_SCALAR)
        fail(y->magic == MAGIC_FREED ? GrB_UNINITIALIZED_OBJECT : GrB_INVALID_OBJECT, std::string(who) + ": the thunk is not a valid GrB_Scalar");
    if (!y->has) fail(GrB_EMPTY_OBJECT, std::string(who) + ": the thunk scalar is empty");
    Thunk t{y->type->code, {0}};
    memcpy(t.v, y->value, sizeof(t.v));
    return t;
}

// T (fresh storage, type `ctype`) = op(scalar, S) (bind1st) or op(S, scalar) for a binary operator code `op` of type `ot`, by the
// bound-scalar stream of GrB_apply (grb_apply.hip); full_values: one value per entry even when T could be iso
MatrixOwner matrix_apply_bound(GB_Matrix_opaque *S, int op, int ot, bool bind1st, const Thunk &scalar, int ctype, bool full_values);

template <int OP> GRB_HD bool sel_pos(int64_t i, int64_t j, int64_t k)
{
    switch (OP) {
    case SEL_TRIL: return j <= i + k;
    case SEL_TRIU: return j >= i + k;
    case SEL_DIAG: return j == i + k;
    case SEL_OFFDIAG: return j != i + k;
    case SEL_COLLE: return j <= k;
    case SEL_COLGT: return j > k;
    case SEL_ROWLE: return i <= k;
    default: return i > k;
    }
}
template <int OP, typename T> GRB_HD bool sel_val(T a, T y)
{
    switch (OP) {
    case SEL_VALUEEQ: return a == y;
    case SEL_VALUENE: return a != y;
    case SEL_VALUEGT: return a > y;
    case SEL_VALUEGE: return a >= y;
    case SEL_VALUELT: return a < y;
    default: return a <= y;
    }
}

// the lanes of ONE wavefront exchange data through LDS (the same three steps as mw_sync of grb_mxm.hip)
__device__ __forceinline__ void sel_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int SEL_BPW = 8;  // blocks of 64 entries a wavefront walks: one search in d_ptr per 512 entries

// ---- the entry -> row walk of a wavefront over consecutive blocks of 64 entries -------------------------------------------------
// walk_first_row: the row r of entry p0, Ap[r] <= p0 < Ap[r + 1], by ONE search (Ap[0] = 0 and Ap[m] = nnz bracket every entry).
__device__ __forceinline__ int64_t walk_first_row(const int64_t *__restrict__ Ap, int64_t m, int64_t p0)
{
    int64_t lo = 0, hi = m;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (Ap[mid] <= p0) lo = mid;
        else hi = mid;
    }
    return lo;
}
// walk_block_rows: the row of entry e = p + lane of the block [p, p + 64), given r = the row of entry p (wave-uniform):
//   row(e) = r + #{rows r' >= r whose end Ap[r' + 1] <= e}, 64 row ends at a time through `s_end` (64 words of LDS of this wavefront),
// counted by a search in LDS.  Every lane of the wavefront calls; r becomes the row of the block's last entry, where the next block
// walks on from.
__device__ __forceinline__ int64_t walk_block_rows(const int64_t *__restrict__ Ap, int64_t m, int64_t nnz, int64_t p, int lane, int64_t *s_end, int64_t &r)
{
    const int64_t e = p + lane;
    const int64_t e_last = p + 63 < nnz ? p + 63 : nnz - 1;
    int64_t row = r;
    for (int64_t base = r + 1;; base += 64) {
        const int64_t idx = base + lane;
        s_end[lane] = idx <= m ? Ap[idx] : INT64_MAX;
        sel_sync();
        int c = 0;
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
            if (s_end[c + step - 1] <= e) c += step;
        if (c == 63 && s_end[63] <= e) c = 64;
        row += c;
        const int64_t last = s_end[63];
        sel_sync();
        if (last > e_last) break;
    }
    r = __shfl(row, 63);
    return row;
}

}  // namespace grb
