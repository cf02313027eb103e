// grb_diag.hip -- diagonals in both directions (reference core/vector.py diag -> GrB_Matrix_diag,
// core/matrix.py diag -> GxB_Vector_diag):
//   GrB_Matrix_diag   C (new, square, order n + |k|, v's type) with v on its k-th diagonal: C(i, i + k) = v(i), k >= 0; C(i - k, i) = v(i), k < 0
//   GxB_Vector_diag   v = the k-th diagonal of A, cast to v's type: v(i) = A(i, i + k), k >= 0; A(i - k, i), k < 0
//
// vector -> matrix.  A vector is values + 64-bit presence words, and row r0 + i of C holds one entry or none, so the whole CSR follows
// from the words: the popcount of every word (k_diag_popc), ONE exclusive sum over the ceil(n / 64) counts, and a fill with a wavefront
// per word (k_diag_fill) in which lane l writes Cp[r0 + 64 w + l] = base[w] + popc(word & below(l)) for its row, present or not, and --
// its bit set -- the column c0 + i and the value at that position (r0 = max(-k, 0), c0 = max(k, 0)).  The |k| rows before the
// diagonal's first row (k < 0) get 0, the rows behind its last one (k > 0) and Cp[order] the entry count: |k| + 1 stores by the same
// launch.  No pass over rows, no atomics.
//
// matrix -> vector.  One lane per position of the diagonal (k_diag_extract): a search for the wanted column in [Ap[r], Ap[r + 1]), the
// value where the entry was found (an iso A: its one value), the presence word of 64 positions by __ballot from lane 0.  The length of
// v IS the diagonal's, so every word of v is written and the bits at and above the length stay clear (GrB_Vector_resize copies whole
// words).  A of another type than v: the diagonal is gathered in A's type and cast once (len values, not nnz).
// GrX_last_stats: method 23 (GrB_Matrix_diag) / 24 (GxB_Vector_diag), 6 when nothing ran on the device; tiles = wavefronts.
#include <algorithm>

#include "grb_internal.hpp"
#include "grb_ops.hpp"

namespace grb {

// counts[w] = entries of presence word w; counts[nwords] = 0 (the exclusive sum leaves the total there)
__global__ void k_diag_popc(const uint64_t *__restrict__ bits, int64_t nwords, int64_t *__restrict__ counts)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w <= nwords) counts[w] = w < nwords ? (int64_t)__popcll(bits[w]) : 0;
}

// U: the unsigned integer of the value size (values are moved, not read).  base: the exclusive sum of k_diag_popc's counts
template <typename U>
__global__ __launch_bounds__(256) void k_diag_fill(const uint64_t *__restrict__ bits, const U *__restrict__ val, int64_t n, int64_t nwords, int64_t k,
                                                   const int64_t *__restrict__ base, int64_t *__restrict__ Cp, int32_t *__restrict__ Cj, U *__restrict__ Cx)
{
    const int lane = threadIdx.x & 63;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, w = tid >> 6;
    const int64_t ak = k < 0 ? -k : k, r0 = k < 0 ? ak : 0, c0 = k > 0 ? ak : 0;
    if (w < nwords) {
        const uint64_t word = bits[w];
        const int64_t i = (w << 6) + lane;
        if (i < n) {
            const int64_t o = base[w] + __popcll(word & ((1ull << lane) - 1ull));
            Cp[r0 + i] = o;
            if ((word >> lane) & 1ull) {
                Cj[o] = (int32_t)(c0 + i);
                Cx[o] = val[i];
            }
        }
    }
    // the rows outside the diagonal's, and the end of the array: Cp has n + |k| + 1 words
    const int64_t nnz = base[nwords], nth = (int64_t)gridDim.x * 256;
    for (int64_t e = tid; e <= ak; e += nth) {
        if (k >= 0) Cp[n + e] = nnz;
        else if (e < ak) Cp[e] = 0;
        else Cp[n + ak] = nnz;
    }
}

template <typename U>
__global__ __launch_bounds__(256) void k_diag_extract(const int64_t *__restrict__ Ap, const int32_t *__restrict__ Aj, const U *__restrict__ Ax, int iso,
                                                      int64_t len, int64_t k, U *__restrict__ out, uint64_t *__restrict__ bits, int64_t nwords)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, w = i >> 6;
    if (w >= nwords) return;  // (uniform over the wavefront)
    bool has = false;
    if (i < len) {
        const int64_t r = i + (k < 0 ? -k : 0);
        const int32_t c = (int32_t)(i + (k > 0 ? k : 0));
        const int64_t hi = Ap[r + 1];
        const int64_t p = lower_bound<int32_t>(Aj, Ap[r], hi, c);
        U x = (U)0;
        if (p < hi && Aj[p] == c) {
            has = true;
            x = Ax[iso ? 0 : p];
        }
        out[i] = x;  // (an absent position gets a zero nobody reads)
    }
    const unsigned long long b = __ballot(has);
    if (lane == 0) bits[w] = b;
}

static dim3 wave_grid(int64_t waves)
{
    const int64_t g = ceil_div(waves, 4);
    if (g > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
    return dim3((unsigned)(g > 0 ? g : 1));
}

static MatrixOwner matrix_of_diag(GB_Vector_opaque *v, int64_t k)
{
    const uint64_t ak = k < 0 ? (uint64_t)(-(k + 1)) + 1 : (uint64_t)k;
    if (ak > GrB_INDEX_MAX || v->n + ak > GrB_INDEX_MAX + 1) fail(GrB_INVALID_VALUE, "GrB_Matrix_diag: the order n + |k| exceeds GrB_INDEX_MAX + 1");
    const uint64_t order = v->n + ak;
    const int64_t nv = vector_nvals(v);
    // (as every matrix with entries: int32 column indices)
    if (nv && order > 0x7fffffffull) fail(GrB_NOT_IMPLEMENTED, "matrices with entries need ncols < 2^31 (int32 column indices)");
    MatrixOwner C(matrix_new(v->type, order, order));
    ctx().stats = GrX_Stats{};
    ctx().stats.method = 6;
    if (nv == 0) return C;
    const int64_t n = (int64_t)v->n, nwords = (int64_t)bits_words64(v->n);
    DevBuf<int64_t> base(nwords + 1);
    hipLaunchKernelGGL(k_diag_popc, grid1d(nwords + 1), dim3(256), 0, ctx().stream, (const uint64_t *)v->d_bits, nwords, base.p);
    prim_exclusive_sum_i64(base.p, base.p, nwords + 1);
    C->d_ptr = (int64_t *)dev_alloc(sizeof(int64_t) * (order + 1));
    C->d_col = (int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nv);
    C->d_val = dev_alloc(v->type->size * (size_t)nv);
    // a wavefront per word -- or, a short vector far off the main diagonal, enough wavefronts for the |k| + 1 outside stores of Cp (the
    // loop over them strides by the grid; 32 wavefronts per CU are plenty for a store stream)
    const int64_t edge_waves = std::min<int64_t>(ceil_div((int64_t)ak + 1, 64), (int64_t)ctx().num_cus * 32);
    const dim3 grid = wave_grid(std::max(nwords, edge_waves));
    GRB_DISPATCH_SIZE(v->type->size, U, {
        hipLaunchKernelGGL((k_diag_fill<U>), grid, dim3(256), 0, ctx().stream, (const uint64_t *)v->d_bits, (const U *)v->d_val, n, nwords, k,
                           (const int64_t *)base.p, C->d_ptr, C->d_col, (U *)C->d_val);
    })
    C->nvals = nv;
    ctx().stats.method = 23;
    ctx().stats.kernel_launches = 3;
    ctx().stats.tiles = (int64_t)grid.x * 4;
    ctx().stats.out_nvals = nv;
    GRB_HIP(hipGetLastError());
    sync_stream();  // (`base` is released at the end of this scope)
    return C;
}

static void vector_of_diag(GB_Vector_opaque *v, GB_Matrix_opaque *A, int64_t k)
{
    const int64_t m = (int64_t)A->nrows, n = (int64_t)A->ncols;
    int64_t len = 0;
    if (k >= 0 && k < n) len = std::min(m, n - k);
    else if (k < 0 && k > -m) len = std::min(m + k, n);
    if ((int64_t)v->n != len)
        fail(GrB_DIMENSION_MISMATCH, "GxB_Vector_diag: diagonal " + std::to_string(k) + " of a " + std::to_string(m) + " x " + std::to_string(n) + " matrix has length " +
                                         std::to_string(len) + ", the output " + std::to_string(v->n));
    ctx().stats = GrX_Stats{};
    ctx().stats.method = 6;
    ctx().stats.out_nvals = -1;
    if (len == 0 || A->nvals == 0) {  // v's old entries go, none come
        vector_release_storage(v);
        return;
    }
    vector_ensure_storage(v);
    const int at = A->type->code, vt = v->type->code;
    const int64_t nwords = (int64_t)bits_words64((uint64_t)len);
    DevPtr<char> gathered;  // the diagonal in A's type, when that is not v's
    void *out = v->d_val;
    if (at != vt) {
        gathered.reset((char *)dev_alloc(A->type->size * (size_t)len));
        out = gathered.p;
    }
    GRB_DISPATCH_SIZE(A->type->size, U, {
        hipLaunchKernelGGL((k_diag_extract<U>), wave_grid(nwords), dim3(256), 0, ctx().stream, (const int64_t *)A->d_ptr, (const int32_t *)A->d_col,
                           (const U *)A->d_val, A->iso ? 1 : 0, len, k, (U *)out, v->d_bits, nwords);
    })
    if (at != vt) cast_array(vt, v->d_val, at, gathered.p, len);
    v->nvals = -1;
    ctx().stats.method = 24;
    ctx().stats.kernel_launches = at != vt ? 2 : 1;
    ctx().stats.tiles = nwords;
    GRB_HIP(hipGetLastError());
    if (ctx().blocking) sync_stream();
}

void preload_diag() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_diag_popc)); (void)hipGetLastError(); }

}  // namespace grb

using namespace grb;

extern "C" GrB_Info GrB_Matrix_diag(GrB_Matrix *C, const GrB_Vector v, int64_t k)
{
    GRB_TRY
    if (!C) fail(GrB_NULL_POINTER, "GrB_Matrix_diag: output pointer is NULL");
    require_init();
    check_vector(v, "v");
    *C = matrix_of_diag(v, k).release();
    GRB_CATCH((std::string *)nullptr)
}

extern "C" GrB_Info GxB_Vector_diag(GrB_Vector v, const GrB_Matrix A, int64_t k, const GrB_Descriptor desc)
{
    GRB_TRY
    require_init();
    check_vector(v, "v");
    check_matrix(A, "A");
    (void)desc;  // (accepted and ignored: a transposed input is -k on the caller's side)
    vector_of_diag(v, A, k);
    GRB_CATCH(errp(v))
}
