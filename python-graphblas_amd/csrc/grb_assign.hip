// grb_assign.hip -- GrB_Matrix_assign: C<Mask, replace>(I, J) = accum(C(I, J), A), its scalar forms GrB_Matrix_assign_<T> / _Scalar,
// GrB_Row_assign / GrB_Col_assign, GrB_Matrix_setElement_<T> / _Scalar and GrB_Matrix_removeElement (C API 2.0 sections 4.3.7.2 - 4.3.7.6,
// 4.2.4.8 / 4.2.4.9; reference core/matrix.py __setitem__ / Updater -> C(mask, accum)[I, J] << A).
//
// GrB_assign, not GxB_subassign: the mask has C's shape.  Two steps:
//   1. Z = C;  Z(I, J) = accum ? accum(C(I, J), A) : A  -- without an accumulator the positions of I x J that A leaves empty lose theirs;
//   2. C<Mask, replace> = Z over the whole of C, no accumulator (matrix_finish; without a mask C takes Z's storage).
// Z is a fresh matrix, so C may alias A or the mask, and every check runs before anything in C changes.
//
// Stages of the matrix form:
//   index lists   I and J on the device once, bounds-checked there; inverse tables  int32 rinv[nrows(C)], jinv[ncols(C)]  (-1 = not selected)
//                 by fill + scatter.  A repeated index is undefined in the specification; here it is DETECTED: after the scatter every k
//                 reads inv[L[k]] back, a mismatch raises GrB_INVALID_VALUE.  The host classifies J in the pass that copies it:
//                   method 15  J is GrB_ALL or a run lo, lo + 1, ...     column + lo
//                   method 16  J strictly increasing                     J[column], the order of a row is kept
//                   method 17  any other J                               J[column], then one radix sort of  row << 32 | column  and a gather
//   placement     S'(I[i], J[j]) = A(i, j) in CSR over nrows(C) rows: row lengths through rinv, one exclusive sum, an entry-parallel copy
//                 in units of ASG_UNIT entries of S' -- one search per unit in the scanned lengths, then the entry -> row walk of
//                 grb_index_ops.hpp, 64 entries at a time (no unit table, no thread walks a row).  Values move as 1 / 2 / 4 / 8-byte words;
//                 an iso A stays iso
//   region merge  Z = the two-list wavefront merge of C(r, :) and S'(r, :) per unit of the UnitTable (grb_mxm_ewise.inc): with an
//                 accumulator it IS eWiseAdd(C, S', accum); without, S' wins and an entry of C alone is dropped iff its row is selected
//                 and its column is in J (a range test for method 15, else a bitmap of ncols bits)
//   finish        matrix_finish(C, Mask, nullptr, Z)
// The scalar form never materialises ni * nj values:
//   method 18  a non-complemented mask: Z matters only where the mask is true, so S' = the mask's entries with a row in I, a column in J
//              and (valued mask) a true value -- entry-parallel flag / scan / fill -- as an iso pattern with the scalar
//   method 19  no mask, or a complemented one: the dense region rows I x sorted J as an iso pattern (4 ni nj bytes of columns; answered
//              with GrB_OUT_OF_MEMORY before anything is allocated when they do not fit the free device memory)
//   then Z = eWiseAdd(C, S', accum or SECOND): the region is dense, nothing is deleted.
//   method  6  short cuts: ni = 0 or nj = 0 (Z = C; the write rule still runs), GrB_ALL x GrB_ALL without mask or accumulator (a cast copy)
// GrB_Row_assign / GrB_Col_assign (the mask is a VECTOR over the row / column; replace touches that row / column only): the row / column
// of C as a vector (GrB_Col_extract), the existing GrB_Vector_assign on it, the vector back as a 1 x n / n x 1 matrix through the matrix
// form.  setElement = the scalar form with one index each; removeElement = the matrix form with an empty 1 x 1 A: both cost O(nnz(C)).
// GrX_last_stats: method as above, tiles = the placement's (or the filter's / the dense fill's) wavefront units, out_nvals = nnz(C).
#include <algorithm>
#include <vector>

#include "grb_index_ops.hpp"

extern "C" const uint64_t *GrB_ALL;

namespace grb {

constexpr int ASG_UNIT = 2048;  // entries of S' a wavefront places (32 blocks of 64: one search in the row pointers per unit)

// ---- index lists -------------------------------------------------------------------------------------------------------------------------
// flags[0]: an index at or beyond the dimension
__global__ void k_asg_check(const uint64_t *__restrict__ L, int64_t n, uint64_t dim, int *flags)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && L[k] >= dim) flags[0] = 1;
}
// inv[L[k]] = k (inv was filled with -1; of a repeated index one writer stays)
__global__ void k_asg_scatter(const uint64_t *__restrict__ L, int64_t n, uint64_t dim, int32_t *__restrict__ inv)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && L[k] < dim) inv[L[k]] = (int32_t)k;
}
// flags[1]: some k does not find itself in the table -- another position of the list holds the same index
__global__ void k_asg_readback(const uint64_t *__restrict__ L, int64_t n, uint64_t dim, const int32_t *__restrict__ inv, int *flags)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && L[k] < dim && inv[L[k]] != (int32_t)k) flags[1] = 1;
}
// bits: bit c = column c is selected (inv[c] >= 0); a word per wavefront, no atomics
__global__ void k_asg_bitmap(const int32_t *__restrict__ inv, int64_t n, unsigned long long *__restrict__ bits)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long w = __ballot(c < n && inv[c] >= 0);
    if ((threadIdx.x & 63) == 0 && (c >> 6) < ((n + 63) >> 6)) bits[c >> 6] = w;
}

// one index list of a call: its device copy, its class and its inverse table
struct AsgList {
    const uint64_t *h = nullptr;  // the caller's list; nullptr: GrB_ALL
    int64_t n = 0;                // indices it selects
    int64_t dim = 0;              // the dimension it indexes
    bool run = true, increasing = true;
    int64_t lo = 0;               // first index of a run
    DevPtr<uint64_t> d;           // the list on the device
    DevPtr<int32_t> inv;          // dim entries: position in the list, -1 = not selected (nullptr: GrB_ALL, or a run of columns)
    DevPtr<unsigned long long> bits;  // (columns, on demand) bit per index: selected
    bool all() const { return h == nullptr; }
    bool is_run() const { return !h || run; }
};

static const uint64_t *asg_host_list(const uint64_t *L, const char *who, const char *what)
{
    if (!L) fail(GrB_NULL_POINTER, std::string(who) + ": the index list " + what + " is NULL");
    return L == GrB_ALL ? nullptr : L;
}

// need_inv: the inverse table is wanted even for a run (rows always; columns only to find a repeated index)
static void asg_list_build(AsgList &L, const uint64_t *host, uint64_t n, uint64_t dim, bool need_inv, const char *who, const char *what)
{
    L.h = host;
    L.dim = (int64_t)dim;
    L.n = host ? (int64_t)n : (int64_t)dim;
    if (!host) return;
    if (n >= (1ull << 31)) fail(GrB_NOT_IMPLEMENTED, std::string(who) + ": index lists of 2^31 or more entries are outside this library's path");
    if (n == 0) return;
    L.lo = (int64_t)host[0];
    for (uint64_t k = 1; k < n; k++) {
        L.run = L.run && host[k] == host[0] + k;
        L.increasing = L.increasing && host[k] > host[k - 1];
    }
    L.d.reset((uint64_t *)dev_alloc(sizeof(uint64_t) * (size_t)n));
    h2d(L.d.p, host, sizeof(uint64_t) * (size_t)n);
    DevBuf<int> flags(2, true);
    const int64_t N = (int64_t)n;
    hipLaunchKernelGGL(k_asg_check, grid1d(N), dim3(256), 0, ctx().stream, (const uint64_t *)L.d.p, N, dim, flags.p);
    ctx().stats.kernel_launches += 1;
    if ((need_inv || !L.run) && dim > 0) {
        L.inv.reset((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)dim));
        GRB_HIP(hipMemsetAsync(L.inv.p, 0xff, sizeof(int32_t) * (size_t)dim, ctx().stream));
        hipLaunchKernelGGL(k_asg_scatter, grid1d(N), dim3(256), 0, ctx().stream, (const uint64_t *)L.d.p, N, dim, L.inv.p);
        hipLaunchKernelGGL(k_asg_readback, grid1d(N), dim3(256), 0, ctx().stream, (const uint64_t *)L.d.p, N, dim, (const int32_t *)L.inv.p, flags.p);
        ctx().stats.kernel_launches += 3;
    }
    int hflags[2] = {0, 0};
    d2h(hflags, flags.p, sizeof(hflags));
    if (hflags[0]) fail(GrB_INDEX_OUT_OF_BOUNDS, std::string(who) + ": an index of the list " + what + " is outside the matrix");
    if (hflags[1])
        fail(GrB_INVALID_VALUE, std::string(who) + ": the index list " + what + " holds an index more than once (undefined in the specification; this library rejects it)");
}

static void asg_list_bitmap(AsgList &L)
{
    const size_t words = bits_words64((uint64_t)L.dim);
    L.bits.reset((unsigned long long *)dev_alloc(sizeof(unsigned long long) * std::max<size_t>(words, 1)));
    hipLaunchKernelGGL(k_asg_bitmap, grid1d((int64_t)words * 64), dim3(256), 0, ctx().stream, (const int32_t *)L.inv.p, L.dim, L.bits.p);
    ctx().stats.kernel_launches += 1;
}

// the region I x J as the merge and the mask filter test it
static MergeRegion asg_region(AsgList &I, AsgList &J)
{
    MergeRegion reg{};
    reg.rinv = I.all() ? nullptr : I.inv.p;
    if (J.is_run()) {
        reg.jbits = nullptr;
        reg.jlo = J.all() ? 0 : J.lo;
        reg.jhi = reg.jlo + J.n;
    } else {
        if (!J.bits) asg_list_bitmap(J);
        reg.jbits = J.bits.p;
    }
    return reg;
}

// ---- placement ------------------------------------------------------------------------------------------------------------------------
// len[r] = entries of the row of S that lands on row r of C (len[m] = 0: the scan turns it into the total)
__global__ void k_asg_rowlen(const int64_t *__restrict__ Sp, const int32_t *__restrict__ rinv, int64_t m, int64_t *__restrict__ len)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > m) return;
    int64_t n = 0;
    if (r < m) {
        const int64_t a = rinv ? (int64_t)rinv[r] : r;
        if (a >= 0) n = Sp[a + 1] - Sp[a];
    }
    len[r] = n;
}

// entry e of S' (row r of C, found by the walk) is entry Sp[a] + (e - Pp[r]) of row a = rinv[r] of S.  KEYS: the columns come out in any
// order, so the entry is written as a sort key  r << 32 | column  with e as its payload instead (method 17)
template <bool KEYS, typename U>
__global__ void __launch_bounds__(256) k_asg_place(const int64_t *__restrict__ Sp, const int32_t *__restrict__ Sj, const U *__restrict__ Sx,
                                                   const int32_t *__restrict__ rinv, const int64_t *__restrict__ Pp, int64_t m, int64_t nnz,
                                                   int64_t nunits, const uint64_t *__restrict__ J, int32_t jlo, int32_t *__restrict__ Tj,
                                                   U *__restrict__ Tx, uint64_t *__restrict__ key, uint32_t *__restrict__ pay)
{
    __shared__ int64_t s_end[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= nunits) return;  // (uniform over the wavefront)
    const int64_t p0 = u * ASG_UNIT, p1 = p0 + ASG_UNIT < nnz ? p0 + ASG_UNIT : nnz;
    int64_t r = walk_first_row(Pp, m, p0);
    for (int64_t p = p0; p < p1; p += 64) {
        const int64_t e = p + lane;
        const int64_t row = walk_block_rows(Pp, m, nnz, p, lane, s_end[wave], r);
        if (e < p1) {
            const int64_t a = rinv ? (int64_t)rinv[row] : row;
            const int64_t src = Sp[a] + (e - Pp[row]);
            const int32_t c = Sj[src];
            const int32_t col = J ? (int32_t)J[c] : c + jlo;
            if constexpr (KEYS) {
                key[e] = ((uint64_t)row << 32) | (uint64_t)(uint32_t)col;
                pay[e] = (uint32_t)e;
            } else {
                Tj[e] = col;
            }
            if (Tx) Tx[e] = Sx[src];
        }
    }
}

template <typename U>
__global__ void k_asg_gather(const uint64_t *__restrict__ key, const uint32_t *__restrict__ pay, const U *__restrict__ Vx, int64_t n,
                             int32_t *__restrict__ Tj, U *__restrict__ Tx)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    Tj[q] = (int32_t)(key[q] & 0xffffffffull);
    if (Tx) Tx[q] = Vx[pay[q]];
}

static dim3 asg_unit_grid(int64_t nunits, const char *who)
{
    if (nunits > (int64_t)UINT32_MAX * 4) fail(GrB_NOT_IMPLEMENTED, std::string(who) + ": more than 2^34 units");
    return dim3((unsigned)std::max<int64_t>(1, ceil_div(nunits, 4)));
}

// S' (fresh storage, type `ctype`, the shape of C) with S'(I[i], J[j]) = S(i, j); S holds entries
static MatrixOwner assign_place(GB_Matrix_opaque *S, AsgList &I, AsgList &J, uint64_t c_rows, uint64_t c_cols, int ctype)
{
    const int64_t m = (int64_t)c_rows, nnz = S->nvals;
    const size_t ssize = S->type->size;
    const bool iso = S->iso;
    ctx().stats.method = J.is_run() ? 15 : (J.increasing ? 16 : 17);
    const bool keys = ctx().stats.method == 17;
    if (keys && nnz >= (1ll << 32))
        fail(GrB_NOT_IMPLEMENTED, "GrB_Matrix_assign: an unsorted column list that places 2^32 or more entries (" + std::to_string(nnz) +
                                      ") is outside this library's path: sort the list, or assign in pieces");
    MatrixOwner Tm(matrix_new(type_of_code(ctype), c_rows, c_cols));
    DevPtr<int64_t> Pp((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1)));
    const int32_t *rinv = I.all() ? nullptr : I.inv.p;
    hipLaunchKernelGGL(k_asg_rowlen, grid1d(m + 1), dim3(256), 0, ctx().stream, (const int64_t *)S->d_ptr, rinv, m, Pp.p);
    prim_exclusive_sum_i64(Pp.p, Pp.p, m + 1);
    const int64_t nunits = ceil_div(nnz, ASG_UNIT);
    ctx().stats.tiles = nunits;
    const dim3 ugrid = asg_unit_grid(nunits, "GrB_Matrix_assign");
    DevPtr<int32_t> Tj((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
    DevPtr<char> raw((char *)dev_alloc(ssize * (size_t)(iso ? 1 : nnz)));
    if (iso) d2d(raw.p, S->d_val, ssize);
    const uint64_t *Jd = J.is_run() ? nullptr : J.d.p;
    const int32_t jlo = (int32_t)(J.all() ? 0 : J.lo);
    if (!keys) {
        GRB_DISPATCH_SIZE(ssize, U, hipLaunchKernelGGL((k_asg_place<false, U>), ugrid, dim3(256), 0, ctx().stream, (const int64_t *)S->d_ptr,
                                              (const int32_t *)S->d_col, (const U *)S->d_val, rinv, (const int64_t *)Pp.p, m, nnz, nunits, Jd, jlo, Tj.p,
                                              (U *)(iso ? nullptr : raw.p), (uint64_t *)nullptr, (uint32_t *)nullptr))
        ctx().stats.kernel_launches += 3;
    } else {
        DevBuf<uint64_t> key((size_t)nnz), key_s((size_t)nnz);
        DevBuf<uint32_t> pay((size_t)nnz), pay_s((size_t)nnz);
        DevBuf<char> vx(iso ? 0 : ssize * (size_t)nnz);
        GRB_DISPATCH_SIZE(ssize, U, hipLaunchKernelGGL((k_asg_place<true, U>), ugrid, dim3(256), 0, ctx().stream, (const int64_t *)S->d_ptr,
                                              (const int32_t *)S->d_col, (const U *)S->d_val, rinv, (const int64_t *)Pp.p, m, nnz, nunits, Jd, jlo,
                                              (int32_t *)nullptr, (U *)(iso ? nullptr : vx.p), key.p, pay.p))
        int rbits = 0;
        while ((1ll << rbits) < m) rbits++;
        prim_sort_pairs_u64_u32((const uint64_t *)key.p, key_s.p, (const uint32_t *)pay.p, pay_s.p, nnz, 32 + rbits);
        GRB_DISPATCH_SIZE(ssize, U, hipLaunchKernelGGL((k_asg_gather<U>), grid1d(nnz), dim3(256), 0, ctx().stream, (const uint64_t *)key_s.p,
                                              (const uint32_t *)pay_s.p, (const U *)vx.p, nnz, Tj.p, (U *)(iso ? nullptr : raw.p)))
        ctx().stats.kernel_launches += 5;
        sync_stream();  // (the sort's buffers are released at the end of this scope)
    }
    matrix_adopt(Tm.get(), Pp.release(), Tj.release(), raw.release(), S->type->code, nnz, iso);
    GRB_HIP(hipGetLastError());
    return Tm;
}

// ---- the scalar form's patterns ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool asg_value_true(const void *Mx, int m_type, int m_iso, int64_t p)
{
    const int64_t q = m_iso ? 0 : p;
    switch (m_type) {
    case TC_BOOL: case TC_INT8: case TC_UINT8: return ((const uint8_t *)Mx)[q] != 0;
    case TC_INT16: case TC_UINT16: return ((const uint16_t *)Mx)[q] != 0;
    case TC_INT32: case TC_UINT32: return ((const uint32_t *)Mx)[q] != 0;
    case TC_INT64: case TC_UINT64: return ((const uint64_t *)Mx)[q] != 0;
    case TC_FP32: return ((const float *)Mx)[q] != 0.0f;
    default: return ((const double *)Mx)[q] != 0.0;
    }
}

// method 18, flag pass over the mask's entries (the shape of k_select_flag): keep[b] bit l = entry 64 b + l of the mask is true, its row is
// selected and its column is; bsum[b] = popc(keep[b]); bsum[nblocks] = 0
template <bool NEED_ROW>
__global__ void __launch_bounds__(256) k_asg_mask_flag(const int64_t *__restrict__ Mp, int64_t m, const int32_t *__restrict__ Mj, const void *__restrict__ Mx,
                                                       int m_type, int m_iso, int structure, int64_t nnz, int64_t nblocks, MergeRegion reg,
                                                       unsigned long long *__restrict__ keep, int64_t *__restrict__ bsum)
{
    __shared__ int64_t s_end[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * SEL_BPW;
    const int64_t b1 = b0 + SEL_BPW < nblocks ? b0 + SEL_BPW : nblocks;
    if (blockIdx.x == 0 && threadIdx.x == 0) bsum[nblocks] = 0;
    int64_t r = 0;
    if constexpr (NEED_ROW) {
        if (b0 < b1) r = walk_first_row(Mp, m, b0 << 6);
    }
    for (int64_t b = b0; b < b1; b++) {
        const int64_t p = b << 6, e = p + lane;
        int64_t row = r;
        if constexpr (NEED_ROW) row = walk_block_rows(Mp, m, nnz, p, lane, s_end[wave], r);
        bool pred = false;
        if (e < nnz) {
            const int32_t c = Mj[e];
            pred = reg.jbits ? ((reg.jbits[c >> 6] >> (c & 63)) & 1ull) != 0 : (c >= reg.jlo && c < reg.jhi);
            if constexpr (NEED_ROW) pred = pred && reg.rinv[row] >= 0;
            if (pred && !structure) pred = asg_value_true(Mx, m_type, m_iso, e);
        }
        const unsigned long long word = __ballot(pred);
        if (lane == 0) {
            keep[b] = word;
            bsum[b] = __popcll(word);
        }
    }
}
__global__ void k_asg_mask_rowptr(const int64_t *__restrict__ Mp, int64_t m, int64_t nnz, int64_t nblocks, const unsigned long long *__restrict__ keep,
                                  const int64_t *__restrict__ bsum, int64_t *__restrict__ Np)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const int64_t p = Mp[i];
    Np[i] = p >= nnz ? bsum[nblocks] : bsum[p >> 6] + __popcll(keep[p >> 6] & ((1ull << (p & 63)) - 1));
}
__global__ void k_asg_mask_fill(const int32_t *__restrict__ Mj, int64_t nnz, const unsigned long long *__restrict__ keep, const int64_t *__restrict__ bsum,
                                int32_t *__restrict__ Nj)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const unsigned long long w = keep[e >> 6];
    const int l = (int)(e & 63);
    if ((w >> l) & 1ull) Nj[bsum[e >> 6] + __popcll(w & ((1ull << l) - 1))] = Mj[e];
}

// method 19: the dense region.  len[r] = nj for a selected row; the columns of every selected row are the sorted list
__global__ void k_asg_dense_rowlen(const int32_t *__restrict__ rinv, int64_t m, int64_t nj, int64_t *__restrict__ len)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > m) return;
    len[r] = (r < m && (!rinv || rinv[r] >= 0)) ? nj : 0;
}
__global__ void k_asg_iota(int64_t n, uint32_t *__restrict__ pos)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) pos[k] = (uint32_t)k;
}
// a wavefront per (selected row, chunk of ASG_UNIT columns): copies the chunk of the sorted list (sJ == nullptr: jlo, jlo + 1, ...)
__global__ void __launch_bounds__(256) k_asg_dense_fill(const uint64_t *__restrict__ sJ, int64_t jlo, int64_t nj, int64_t chunks, int64_t nunits,
                                                        int32_t *__restrict__ Tj)
{
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= nunits) return;
    const int64_t q = u / chunks, k0 = (u - q * chunks) * ASG_UNIT, k1 = k0 + ASG_UNIT < nj ? k0 + ASG_UNIT : nj;
    for (int64_t k = k0 + lane; k < k1; k += 64) Tj[q * nj + k] = (int32_t)(sJ ? (int64_t)sJ[k] : jlo + k);
}

// P (fresh, iso, C's type, the value `x`) = the pattern the scalar is assigned to
static MatrixOwner scalar_pattern_dense(GB_Matrix_opaque *C, AsgList &I, AsgList &J, const void *x)
{
    const int64_t m = (int64_t)C->nrows, ni = I.n, nj = J.n;
    ctx().stats.method = 19;
    MatrixOwner P(matrix_new(C->type, C->nrows, C->ncols));
    // (ni, nj < 2^31: the product fits 62 bits)
    size_t free_b = 0, total_b = 0;
    GRB_HIP(hipMemGetInfo(&free_b, &total_b));
    if ((uint64_t)ni * (uint64_t)nj > (uint64_t)free_b / 4)
        fail(GrB_OUT_OF_MEMORY, "GrB_Matrix_assign: the scalar would be assigned to " + std::to_string(ni) + " x " + std::to_string(nj) +
                                    " positions, whose column indices alone do not fit the free device memory; assign under a mask, or in pieces");
    const int64_t nnz = ni * nj;
    DevPtr<int64_t> Pp((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1)));
    hipLaunchKernelGGL(k_asg_dense_rowlen, grid1d(m + 1), dim3(256), 0, ctx().stream, (const int32_t *)(I.all() ? nullptr : I.inv.p), m, nj, Pp.p);
    prim_exclusive_sum_i64(Pp.p, Pp.p, m + 1);
    ctx().stats.kernel_launches += 2;
    // the sorted list: a run needs none, an increasing list is its own
    DevBuf<uint64_t> sJ(J.is_run() || J.increasing ? 0 : (size_t)nj);
    const uint64_t *sj = nullptr;
    if (!J.is_run()) {
        if (J.increasing) sj = J.d.p;
        else {
            DevBuf<uint32_t> iota((size_t)nj), perm((size_t)nj);
            int cbits = 1;
            while (cbits < 63 && (1ll << cbits) < (int64_t)C->ncols) cbits++;
            hipLaunchKernelGGL(k_asg_iota, grid1d(nj), dim3(256), 0, ctx().stream, nj, iota.p);
            prim_sort_pairs_u64_u32((const uint64_t *)J.d.p, sJ.p, (const uint32_t *)iota.p, perm.p, nj, cbits);
            ctx().stats.kernel_launches += 2;
            sync_stream();
            sj = sJ.p;
        }
    }
    const int64_t chunks = ceil_div(nj, ASG_UNIT), nunits = ni * chunks;
    ctx().stats.tiles = nunits;
    DevPtr<int32_t> Tj((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
    hipLaunchKernelGGL(k_asg_dense_fill, asg_unit_grid(nunits, "GrB_Matrix_assign"), dim3(256), 0, ctx().stream, sj, J.all() ? (int64_t)0 : J.lo, nj, chunks,
                       nunits, Tj.p);
    ctx().stats.kernel_launches += 1;
    DevPtr<char> one((char *)dev_alloc(8));
    h2d(one.p, x, C->type->size);
    matrix_adopt(P.get(), Pp.release(), Tj.release(), one.release(), C->type->code, nnz, true);
    GRB_HIP(hipGetLastError());
    sync_stream();
    return P;
}

static MatrixOwner scalar_pattern_mask(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, bool structure, AsgList &I, AsgList &J, const void *x)
{
    const int64_t m = (int64_t)C->nrows, nnz = Mask->nvals;
    ctx().stats.method = 18;
    MatrixOwner P(matrix_new(C->type, C->nrows, C->ncols));
    if (nnz == 0) return P;
    DevPtr<int64_t> Pp((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1)));
    DevPtr<int32_t> Tj;
    int64_t kept = 0;
    if (I.all() && J.all() && structure) {
        // the mask's structure IS the pattern: no filter
        kept = nnz;
        d2d(Pp.p, Mask->d_ptr, sizeof(int64_t) * (size_t)(m + 1));
        Tj.reset((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
        d2d(Tj.p, Mask->d_col, sizeof(int32_t) * (size_t)nnz);
    } else {
        const MergeRegion reg = asg_region(I, J);
        const int64_t nblocks = ceil_div(nnz, 64), nunits = ceil_div(nblocks, SEL_BPW);
        ctx().stats.tiles = nunits;
        DevBuf<unsigned long long> keep((size_t)nblocks);
        DevBuf<int64_t> bsum((size_t)nblocks + 1);
        const dim3 grid = asg_unit_grid(nunits, "GrB_Matrix_assign");
        if (reg.rinv)
            hipLaunchKernelGGL((k_asg_mask_flag<true>), grid, dim3(256), 0, ctx().stream, (const int64_t *)Mask->d_ptr, m, (const int32_t *)Mask->d_col,
                               (const void *)Mask->d_val, Mask->type->code, Mask->iso ? 1 : 0, structure ? 1 : 0, nnz, nblocks, reg, keep.p, bsum.p);
        else
            hipLaunchKernelGGL((k_asg_mask_flag<false>), grid, dim3(256), 0, ctx().stream, (const int64_t *)Mask->d_ptr, m, (const int32_t *)Mask->d_col,
                               (const void *)Mask->d_val, Mask->type->code, Mask->iso ? 1 : 0, structure ? 1 : 0, nnz, nblocks, reg, keep.p, bsum.p);
        prim_exclusive_sum_i64(bsum.p, bsum.p, nblocks + 1);
        d2h(&kept, bsum.p + nblocks, sizeof(int64_t));
        ctx().stats.kernel_launches += 2;
        if (kept > 0) {
            Tj.reset((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)kept));
            hipLaunchKernelGGL(k_asg_mask_rowptr, grid1d(m + 1), dim3(256), 0, ctx().stream, (const int64_t *)Mask->d_ptr, m, nnz, nblocks,
                               (const unsigned long long *)keep.p, (const int64_t *)bsum.p, Pp.p);
            hipLaunchKernelGGL(k_asg_mask_fill, grid1d(nnz), dim3(256), 0, ctx().stream, (const int32_t *)Mask->d_col, nnz, (const unsigned long long *)keep.p,
                               (const int64_t *)bsum.p, Tj.p);
            ctx().stats.kernel_launches += 2;
        }
        GRB_HIP(hipGetLastError());
        sync_stream();  // (keep / bsum are released at the end of this scope)
    }
    if (kept > 0) {
        DevPtr<char> one((char *)dev_alloc(8));
        h2d(one.p, x, C->type->size);
        matrix_adopt(P.get(), Pp.release(), Tj.release(), one.release(), C->type->code, kept, true);
    }
    return P;
}

// ---- the calls --------------------------------------------------------------------------------------------------------------------------
// the last two steps of every form: Z = merge(C, S'), C<Mask, replace> = Z
static void assign_finish(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, GB_Matrix_opaque *Sp, const MergeRegion *reg, Desc f)
{
    const int op = accum ? canonical_op(C->type->code, accum->op) : (int)OP_SECOND;
    MatrixOwner Z = matrix_merge_region(C, Sp, op, accum ? nullptr : reg);
    matrix_finish(C, Mask, nullptr, std::move(Z), f, true);
    ctx().stats.out_nvals = C->nvals;
    sync_stream();  // (the index lists were host arrays borrowed for the call)
}

// Z = C: nothing is assigned, the write rule still runs (replace under a mask still deletes)
static void assign_nothing(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, Desc f)
{
    ctx().stats.method = 6;
    if (Mask) {
        MatrixOwner Z(matrix_cast_copy(C, C->type->code));
        matrix_expand_iso(Z.get());
        matrix_finish(C, Mask, nullptr, std::move(Z), f, true);
    }
    ctx().stats.out_nvals = C->nvals;
    sync_stream();
}

static void matrix_assign(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, GB_Matrix_opaque *A, const uint64_t *Ih, uint64_t ni,
                          const uint64_t *Jh, uint64_t nj, const GB_Descriptor_opaque *desc)
{
    const char *who = "GrB_Matrix_assign";
    require_init();
    check_matrix(C, "C");
    check_matrix(A, "A");
    if (Mask) check_matrix(Mask, "Mask");
    Ih = asg_host_list(Ih, who, "I");
    Jh = asg_host_list(Jh, who, "J");
    const Desc f = desc_of(desc);
    const uint64_t a_rows = f.t0 ? A->ncols : A->nrows, a_cols = f.t0 ? A->nrows : A->ncols;
    const uint64_t want_rows = Ih ? ni : C->nrows, want_cols = Jh ? nj : C->ncols;
    if (a_rows != want_rows || a_cols != want_cols)
        fail(GrB_DIMENSION_MISMATCH, std::string(who) + ": the input is " + std::to_string(a_rows) + " x " + std::to_string(a_cols) + ", the index lists select " +
                                         std::to_string(want_rows) + " x " + std::to_string(want_cols));
    check_mask_accum(who, C, Mask, accum);
    if (accum) canonical_op(C->type->code, accum->op);  // (an operator no kernel implements is rejected before anything runs)
    ctx().stats = GrX_Stats{};
    AsgList I, J;
    asg_list_build(I, Ih, ni, C->nrows, true, who, "I");
    asg_list_build(J, Jh, nj, C->ncols, false, who, "J");
    if (matrix_writes_nothing(C, Mask, f)) return;
    if (C->nrows == 0 || C->ncols == 0) return;
    if (I.n == 0 || J.n == 0) return assign_nothing(C, Mask, f);
    GB_Matrix_opaque *S = f.t0 ? matrix_transpose_cached(A) : A;
    const int ctype = C->type->code;
    if (I.all() && J.all() && !Mask && !accum) {
        ctx().stats.method = 6;
        MatrixOwner Z(matrix_cast_copy(S, ctype));
        matrix_finish(C, nullptr, nullptr, std::move(Z), f, true);
        ctx().stats.out_nvals = C->nvals;
        sync_stream();
        return;
    }
    MatrixOwner Sp;
    if (S->nvals == 0) {
        ctx().stats.method = J.is_run() ? 15 : (J.increasing ? 16 : 17);
        Sp.reset(matrix_new(C->type, C->nrows, C->ncols));
    } else {
        Sp = assign_place(S, I, J, C->nrows, C->ncols, ctype);
    }
    MergeRegion reg{};
    if (!accum) reg = asg_region(I, J);
    assign_finish(C, Mask, accum, Sp.get(), &reg, f);
}

// x: the scalar's bytes in C's type
static void matrix_assign_scalar(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, const void *x, const uint64_t *Ih, uint64_t ni,
                                 const uint64_t *Jh, uint64_t nj, const GB_Descriptor_opaque *desc, const char *who)
{
    if (Mask) check_matrix(Mask, "Mask");
    Ih = asg_host_list(Ih, who, "I");
    Jh = asg_host_list(Jh, who, "J");
    const Desc f = desc_of(desc);
    check_mask_accum(who, C, Mask, accum);
    if (accum) canonical_op(C->type->code, accum->op);
    ctx().stats = GrX_Stats{};
    AsgList I, J;
    asg_list_build(I, Ih, ni, C->nrows, true, who, "I");
    asg_list_build(J, Jh, nj, C->ncols, false, who, "J");
    if (matrix_writes_nothing(C, Mask, f)) return;
    if (C->nrows == 0 || C->ncols == 0) return;
    if (I.n == 0 || J.n == 0) return assign_nothing(C, Mask, f);
    // (a non-complemented mask bounds what of Z the write rule reads by its own true entries)
    MatrixOwner P = (Mask && !f.comp) ? scalar_pattern_mask(C, Mask, f.structure, I, J, x) : scalar_pattern_dense(C, I, J, x);
    assign_finish(C, Mask, accum, P.get(), nullptr, f);
}

template <typename X>
static void matrix_assign_typed(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, X x, const uint64_t *I, uint64_t ni, const uint64_t *J,
                                uint64_t nj, const GB_Descriptor_opaque *desc, const char *who)
{
    require_init();
    check_matrix(C, "C");
    unsigned char v[8] = {0};
    GRB_DISPATCH_TYPE(C->type->code, TC, {
        const TC c = cast_value<TC, X>(x);
        memcpy(v, &c, sizeof(TC));
    })
    matrix_assign_scalar(C, Mask, accum, v, I, ni, J, nj, desc, who);
}

template <typename X>
static void matrix_set_element(GB_Matrix_opaque *C, X x, uint64_t i, uint64_t j)
{
    require_init();
    check_matrix(C, "C");
    if (i >= C->nrows || j >= C->ncols)
        fail(GrB_INVALID_INDEX, "setElement: (" + std::to_string(i) + ", " + std::to_string(j) + ") is outside a matrix of " + std::to_string(C->nrows) + " x " +
                                    std::to_string(C->ncols));
    matrix_assign_typed<X>(C, nullptr, nullptr, x, &i, 1, &j, 1, nullptr, "GrB_Matrix_setElement");
}

static void matrix_remove_element(GB_Matrix_opaque *C, uint64_t i, uint64_t j)
{
    require_init();
    check_matrix(C, "C");
    if (i >= C->nrows || j >= C->ncols)
        fail(GrB_INVALID_INDEX, "removeElement: (" + std::to_string(i) + ", " + std::to_string(j) + ") is outside a matrix of " + std::to_string(C->nrows) + " x " +
                                    std::to_string(C->ncols));
    if (C->nvals == 0) return;
    MatrixOwner E(matrix_new(C->type, 1, 1));
    matrix_assign(C, nullptr, nullptr, E.get(), &i, 1, &j, 1, nullptr);
}

// ---- row / column assign: through the vector form ---------------------------------------------------------------------------------------------
// words[w] = popc of presence word w (words[nwords] = 0)
__global__ void k_asg_vec_count(const uint64_t *__restrict__ bits, int64_t nwords, int64_t *__restrict__ wsum)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w <= nwords) wsum[w] = w < nwords ? __popcll(bits[w]) : 0;
}
// the vector's entries as the row of a 1 x n matrix (COL = false) or the column of an n x 1 matrix (COL = true: Tp has n + 1 pointers)
template <bool COL, typename U>
__global__ void k_asg_vec_fill(const U *__restrict__ val, const uint64_t *__restrict__ bits, const int64_t *__restrict__ wsum, int64_t n,
                               int64_t *__restrict__ Tp, int32_t *__restrict__ Tj, U *__restrict__ Tx)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > n) return;
    const int64_t nwords = (n + 63) >> 6;
    const int64_t pos = e == n ? wsum[nwords] : wsum[e >> 6] + __popcll(bits[e >> 6] & ((1ull << (e & 63)) - 1));
    if (COL) Tp[e] = pos;
    else if (e == 0) { Tp[0] = 0; Tp[1] = wsum[nwords]; }
    if (e < n && ((bits[e >> 6] >> (e & 63)) & 1ull)) {
        Tj[pos] = COL ? 0 : (int32_t)e;
        Tx[pos] = val[e];
    }
}

static MatrixOwner vector_as_matrix(GB_Vector_opaque *w, bool col)
{
    const int64_t n = (int64_t)w->n;
    MatrixOwner W(matrix_new(w->type, col ? w->n : 1, col ? 1 : w->n));
    if (!w->d_val || n == 0) return W;
    const int64_t nwords = (int64_t)bits_words64(w->n);
    DevBuf<int64_t> wsum((size_t)nwords + 1);
    hipLaunchKernelGGL(k_asg_vec_count, grid1d(nwords + 1), dim3(256), 0, ctx().stream, (const uint64_t *)w->d_bits, nwords, wsum.p);
    prim_exclusive_sum_i64(wsum.p, wsum.p, nwords + 1);
    int64_t nv = 0;
    d2h(&nv, wsum.p + nwords, sizeof(int64_t));
    if (nv == 0) return W;
    DevPtr<int64_t> Tp((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)((col ? n : 1) + 1)));
    DevPtr<int32_t> Tj((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nv));
    DevPtr<char> Tx((char *)dev_alloc(w->type->size * (size_t)nv));
    GRB_DISPATCH_SIZE(w->type->size, U, {
        if (col) hipLaunchKernelGGL((k_asg_vec_fill<true, U>), grid1d(n + 1), dim3(256), 0, ctx().stream, (const U *)w->d_val, (const uint64_t *)w->d_bits,
                                    (const int64_t *)wsum.p, n, Tp.p, Tj.p, (U *)Tx.p);
        else hipLaunchKernelGGL((k_asg_vec_fill<false, U>), grid1d(n + 1), dim3(256), 0, ctx().stream, (const U *)w->d_val, (const uint64_t *)w->d_bits,
                                (const int64_t *)wsum.p, n, Tp.p, Tj.p, (U *)Tx.p);
    })
    matrix_adopt(W.get(), Tp.release(), Tj.release(), Tx.release(), w->type->code, nv, false);
    GRB_HIP(hipGetLastError());
    sync_stream();
    return W;
}

struct VectorOwner {
    GB_Vector_opaque *v = nullptr;
    ~VectorOwner() { if (v) vector_free(v); }
};

// a step that runs through a vector entry point: its error text moves to C
static void asg_vector_step(GrB_Info rc, GB_Vector_opaque *w)
{
    if (rc != GrB_SUCCESS) fail(rc, w->err);
}

// row = true: C(i, J) ; row = false: C(I, j).  `idx` is the row / column, `L` the list along it
static void rowcol_assign(GB_Matrix_opaque *C, GB_Vector_opaque *mask, const GB_BinaryOp_opaque *accum, GB_Vector_opaque *u, uint64_t idx, const uint64_t *L,
                          uint64_t nl, const GB_Descriptor_opaque *desc, bool row)
{
    const char *who = row ? "GrB_Row_assign" : "GrB_Col_assign";
    require_init();
    check_matrix(C, "C");
    check_vector(u, "u");
    if (mask) check_vector(mask, "mask");
    if (!L) fail(GrB_NULL_POINTER, std::string(who) + ": the index list is NULL");
    const uint64_t dim = row ? C->nrows : C->ncols, len = row ? C->ncols : C->nrows;
    if (idx >= dim)
        fail(GrB_INVALID_INDEX, std::string(who) + (row ? ": row " : ": column ") + std::to_string(idx) + " is outside a matrix of " + std::to_string(C->nrows) +
                                    " x " + std::to_string(C->ncols));
    if (mask && mask->n != len) fail(GrB_DIMENSION_MISMATCH, std::string(who) + ": the mask has " + std::to_string(mask->n) + " elements, the " + (row ? "row " : "column ") + std::to_string(len));
    // 1. the row / column of C as a vector
    VectorOwner w;
    w.v = vector_new(C->type, len);
    GB_Descriptor_opaque d_ext{};
    d_ext.t0 = row;
    asg_vector_step(GrB_Col_extract(w.v, nullptr, nullptr, C, GrB_ALL, len, idx, &d_ext), w.v);
    // 2. the vector form on it, with the caller's mask, accumulator, list and descriptor
    asg_vector_step(GrB_Vector_assign(w.v, mask, const_cast<GB_BinaryOp_opaque *>(accum), u, L, nl, const_cast<GB_Descriptor_opaque *>(desc)), w.v);
    // 3. back as a 1 x n / n x 1 matrix, unmasked
    check_vector(w.v, "w");
    MatrixOwner W = vector_as_matrix(w.v, !row);
    if (row) matrix_assign(C, nullptr, nullptr, W.get(), &idx, 1, GrB_ALL, C->ncols, nullptr);
    else matrix_assign(C, nullptr, nullptr, W.get(), GrB_ALL, C->nrows, &idx, 1, nullptr);
}

void preload_assign() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_asg_rowlen)); (void)hipGetLastError(); }

}  // namespace grb

using namespace grb;

extern "C" GrB_Info GrB_Matrix_assign(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni,
                                      const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc)
{
    GRB_TRY
    matrix_assign(C, Mask, accum, A, I, ni, J, nj, desc);
    GRB_CATCH(errp(C))
}

extern "C" GrB_Info GrB_Row_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const GrB_Index *J,
                                   GrB_Index nj, const GrB_Descriptor desc)
{
    GRB_TRY
    rowcol_assign(C, mask, accum, u, i, J, nj, desc, true);
    GRB_CATCH(errp(C))
}

extern "C" GrB_Info GrB_Col_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index *I, GrB_Index ni,
                                   GrB_Index j, const GrB_Descriptor desc)
{
    GRB_TRY
    rowcol_assign(C, mask, accum, u, j, I, ni, desc, false);
    GRB_CATCH(errp(C))
}

extern "C" GrB_Info GrB_Matrix_removeElement(GrB_Matrix C, GrB_Index i, GrB_Index j)
{
    GRB_TRY
    matrix_remove_element(C, i, j);
    GRB_CATCH(errp(C))
}

// a GrB_Scalar handed to a matrix entry point: through the typed form of the same entry point (as the vector forms, grb_surface.hip)
static void asg_check_scalar(const GB_Scalar_opaque *s)
{
    if (!s) fail(GrB_NULL_POINTER, "s is NULL");
    if (s->magic != MAGIC_SCALAR) fail(s->magic == MAGIC_FREED ? GrB_UNINITIALIZED_OBJECT : GrB_INVALID_OBJECT, "s is not a valid GrB_Scalar");
}
template <typename FI, typename FU, typename FD>
static GrB_Info asg_scalar_dispatch(const GB_Scalar_opaque *s, FI as_int64, FU as_uint64, FD as_double)
{
    const int tc = s->type->code;
    if (tc == TC_UINT64) {
        uint64_t q = 0;
        memcpy(&q, s->value, 8);
        return as_uint64(q);
    }
    if (tc == TC_FP32 || tc == TC_FP64) {
        double d = 0;
        GRB_DISPATCH_TYPE(tc, TS, {
            TS v;
            memcpy(&v, s->value, sizeof(TS));
            d = cast_value<double, TS>(v);
        })
        return as_double(d);
    }
    int64_t q = 0;
    GRB_DISPATCH_TYPE(tc, TS, {
        TS v;
        memcpy(&v, s->value, sizeof(TS));
        q = cast_value<int64_t, TS>(v);
    })
    return as_int64(q);
}

extern "C" GrB_Info GrB_Matrix_assign_Scalar(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Scalar s, const GrB_Index *I,
                                             GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc)
{
    GRB_TRY
    check_matrix(C, "C");
    asg_check_scalar(s);
    if (!s->has) fail(GrB_NOT_IMPLEMENTED, "assign of an EMPTY scalar (deleting the selected entries) is outside this library's path");
    return asg_scalar_dispatch(
        s, [&](int64_t q) { return GrB_Matrix_assign_INT64(C, Mask, accum, q, I, ni, J, nj, desc); },
        [&](uint64_t q) { return GrB_Matrix_assign_UINT64(C, Mask, accum, q, I, ni, J, nj, desc); },
        [&](double d) { return GrB_Matrix_assign_FP64(C, Mask, accum, d, I, ni, J, nj, desc); });
    GRB_CATCH(errp(C))
}

extern "C" GrB_Info GrB_Matrix_setElement_Scalar(GrB_Matrix C, const GrB_Scalar s, GrB_Index i, GrB_Index j)
{
    GRB_TRY
    check_matrix(C, "C");
    asg_check_scalar(s);
    if (!s->has) return GrB_Matrix_removeElement(C, i, j);  // (C API 2.0: an empty scalar removes the element)
    return asg_scalar_dispatch(
        s, [&](int64_t q) { return GrB_Matrix_setElement_INT64(C, q, i, j); }, [&](uint64_t q) { return GrB_Matrix_setElement_UINT64(C, q, i, j); },
        [&](double d) { return GrB_Matrix_setElement_FP64(C, d, i, j); });
    GRB_CATCH(errp(C))
}

#define DEF_ASSIGN_TYPED(NAME, ctype)                                                                                                                   \
    extern "C" GrB_Info GrB_Matrix_assign_##NAME(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, ctype x, const GrB_Index *I, GrB_Index ni, \
                                                 const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc)                                            \
    {                                                                                                                                                   \
        GRB_TRY                                                                                                                                         \
        matrix_assign_typed<ctype>(C, Mask, accum, x, I, ni, J, nj, desc, "GrB_Matrix_assign");                                                         \
        GRB_CATCH(errp(C))                                                                                                                              \
    }                                                                                                                                                   \
    extern "C" GrB_Info GrB_Matrix_setElement_##NAME(GrB_Matrix C, ctype x, GrB_Index i, GrB_Index j)                                                   \
    {                                                                                                                                                   \
        GRB_TRY                                                                                                                                         \
        matrix_set_element<ctype>(C, x, i, j);                                                                                                          \
        GRB_CATCH(errp(C))                                                                                                                              \
    }
GRB_FOR_EACH_TYPE(DEF_ASSIGN_TYPED)
#undef DEF_ASSIGN_TYPED
