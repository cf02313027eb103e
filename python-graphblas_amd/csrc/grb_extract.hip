// grb_extract.hip -- GrB_Matrix_extract: C<Mask, replace> = accum(C, A(I, J)), GrB_Col_extract: w<mask, replace> = accum(w, A(I, j)) and
// GrB_Matrix_extractElement_<T> (C API 2.0 sections 4.3.6.2 / 4.3.6.3 / 4.2.4.10; reference core/matrix.py:3020-3090 -> A[I, J],
// A[I, j], A[i, J], A[i, j]).
//
// Matrix kernel: T(i', j') = S(I[i'], J[j']), S = A or its cached transpose (T0).  `I` is only ever a gather of
// rows -- any order, any repetition.  The host classifies `J` in the one pass that copies it:
//   method  9  J is GrB_ALL or a run lo, lo + 1, ...: the wanted entries of a source row are ONE segment of it (two searches in its sorted
//              columns, none for GrB_ALL); the count pass reads no entry; the fill copies the segment, column - lo
//   method 10  J strictly increasing, looked up in a table  int32 jinv[ncols]  (-1 = not selected)
//   method 11  J strictly increasing, looked up by a binary search in the device copy of J
//   method 12  any other J (unsorted, duplicates): J sorted with its positions; an entry is emitted once per occurrence of its column, as
//              key  i' << 32 | j'  with its emit position as payload; one radix sort orders every row; one gather
//   method  6  short cuts decided on the host: an empty result, or GrB_ALL x GrB_ALL (a cast copy)
// The house shape of select / eWise: count -> one exclusive sum -> fill, no atomics.  Work is cut into UNITS that do not depend on the row
// lengths: the part of a source row the call can select from (narrowed to [min J, max J] by two searches), in chunks of EXT_UNIT entries;
// a wavefront takes a unit 64 entries at a time (coalesced reads, __ballot + popcount positions, contiguous writes).  Output rows come
// out with sorted columns.  Table or search (methods 10 / 11) is a byte count, see extract_build.
#include <algorithm>
#include <vector>

#include "grb_internal.hpp"
#include "grb_ops.hpp"

extern "C" const uint64_t *GrB_ALL;

namespace grb {

constexpr int EXT_UNIT = 8192;  // entries of a unit

// an index of a list at or beyond the dimension it indexes raises the flag
__global__ void k_ext_check(const uint64_t *__restrict__ L, int64_t n, uint64_t dim, int *oob)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && L[k] >= dim) *oob = 1;
}

// ---- rows: per output row the segment [seg[i], seg[i] + len[i]) of S's entries the call can select from, and its units -----------------
// NARROW: only the entries with a column in [clo, chi).  len[ni] = units[ni] = 0: the scans turn them into the totals
template <bool NARROW>
__global__ void k_ext_rowseg(const int64_t *__restrict__ Sp, const int32_t *__restrict__ Sj, int64_t m, const uint64_t *__restrict__ I, int64_t ni,
                             int64_t clo, int64_t chi, int64_t *__restrict__ seg, int64_t *__restrict__ len, int64_t *__restrict__ units)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > ni) return;
    int64_t a = 0, b = 0;
    if (i < ni) {
        const uint64_t r = I ? I[i] : (uint64_t)i;
        if (r < (uint64_t)m) {
            a = Sp[r];
            b = Sp[r + 1];
            if constexpr (NARROW) {
                a = lower_bound<int32_t>(Sj, a, b, (int32_t)clo);
                b = chi > INT32_MAX ? b : lower_bound<int32_t>(Sj, a, b, (int32_t)chi);
            }
        }
        seg[i] = a;
    }
    len[i] = b - a;
    units[i] = (b - a + EXT_UNIT - 1) / EXT_UNIT;
}

// what a wavefront works on: unit u = chunk (u - ubase[i]) of output row i, the last i with ubase[i] <= u
struct ExtUnit {
    int64_t row, src, n, off;  // output row, first source entry, entries, offset of the chunk in the row's segment
};
__device__ __forceinline__ ExtUnit ext_unit(int64_t u, const int64_t *__restrict__ ubase, int64_t ni, const int64_t *__restrict__ seg,
                                            const int64_t *__restrict__ lpre)
{
    int64_t lo = 0, hi = ni;  // ubase[0] = 0 <= u < ubase[ni]
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ubase[mid] <= u) lo = mid;
        else hi = mid;
    }
    ExtUnit w;
    w.row = lo;
    w.off = (u - ubase[lo]) * EXT_UNIT;
    const int64_t rest = lpre[lo + 1] - lpre[lo] - w.off;
    w.n = rest < EXT_UNIT ? rest : EXT_UNIT;
    w.src = seg[lo] + w.off;
    return w;
}

// ---- method 9: copy the segment.  U = an unsigned integer of the value size (the values are moved, not read) -------------------------------
template <typename U>
__global__ void __launch_bounds__(256) k_ext_copy(const int32_t *__restrict__ Sj, const U *__restrict__ Sx, int a_iso, const int64_t *__restrict__ seg,
                                                  const int64_t *__restrict__ lpre, const int64_t *__restrict__ ubase, int64_t ni, int64_t nunits,
                                                  int32_t clo, int32_t *__restrict__ Tj, U *__restrict__ Tx)
{
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= nunits) return;
    const ExtUnit w = ext_unit(u, ubase, ni, seg, lpre);
    const int64_t dst = lpre[w.row] + w.off;
    for (int64_t k = lane; k < w.n; k += 64) {
        Tj[dst + k] = Sj[w.src + k] - clo;
        if (Tx) Tx[dst + k] = Sx[a_iso ? 0 : w.src + k];
    }
}

// ---- methods 10 / 11: J strictly increasing --------------------------------------------------------------------------------------------
__global__ void k_ext_jinv(const uint64_t *__restrict__ J, int64_t nj, int64_t ncols, int32_t *__restrict__ jinv)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nj && J[k] < (uint64_t)ncols) jinv[J[k]] = (int32_t)k;
}

// TABLE: jinv[col], else a search of col in J.  FILL = false: ucount[u] = selected entries of the unit (ucount[nunits] = 0);
// FILL = true: the same walk writes them from upos[u] on
template <bool TABLE, bool FILL, typename U>
__global__ void __launch_bounds__(256) k_ext_pick(const int32_t *__restrict__ Sj, const U *__restrict__ Sx, int a_iso, const int64_t *__restrict__ seg,
                                                  const int64_t *__restrict__ lpre, const int64_t *__restrict__ ubase, int64_t ni, int64_t nunits,
                                                  const int32_t *__restrict__ jinv, const uint64_t *__restrict__ J, int64_t nj,
                                                  int64_t *__restrict__ upos, int32_t *__restrict__ Tj, U *__restrict__ Tx)
{
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if constexpr (!FILL)
        if (blockIdx.x == 0 && threadIdx.x == 0) upos[nunits] = 0;
    if (u >= nunits) return;
    const ExtUnit w = ext_unit(u, ubase, ni, seg, lpre);
    int64_t pos = FILL ? upos[u] : 0;
    for (int64_t k0 = 0; k0 < w.n; k0 += 64) {  // (wave-uniform trip count)
        const int64_t k = k0 + lane;
        int32_t jn = -1;
        if (k < w.n) {
            const int32_t col = Sj[w.src + k];
            if constexpr (TABLE) jn = jinv[col];
            else {
                const int64_t p = lower_bound<uint64_t>(J, 0, nj, (uint64_t)col);
                if (p < nj && J[p] == (uint64_t)col) jn = (int32_t)p;
            }
        }
        const unsigned long long word = __ballot(jn >= 0);
        if constexpr (FILL) {
            if (jn >= 0) {
                const int64_t p = pos + __popcll(word & ((1ull << lane) - 1));
                Tj[p] = jn;
                if (Tx) Tx[p] = Sx[a_iso ? 0 : w.src + k];
            }
        }
        pos += __popcll(word);
    }
    if constexpr (!FILL)
        if (lane == 0) upos[u] = pos;
}

// Tp[i] = position of the first unit of row i (i = 0 .. ni)
__global__ void k_ext_rowptr(const int64_t *__restrict__ ubase, const int64_t *__restrict__ upos, int64_t ni, int64_t *__restrict__ Tp)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= ni) Tp[i] = upos[ubase[i]];
}

// ---- method 12: any J.  sJ = the columns of J ascending, perm[t] = the position in J of sJ[t] --------------------------------------------------
__global__ void k_ext_iota(int64_t nj, uint32_t *__restrict__ pos)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nj) pos[k] = (uint32_t)k;
}

// an entry of column c is emitted once per occurrence of c in J: the run [lb, ub) of c in sJ.  FILL = false counts; FILL = true emits, 64
// at a time: emit slot s of a block of 64 entries belongs to the first lane whose inclusive count exceeds s (a search over the lanes), so
// a wavefront's writes are contiguous whatever the multiplicities are
template <bool FILL, typename U>
__global__ void __launch_bounds__(256) k_ext_dup(const int32_t *__restrict__ Sj, const U *__restrict__ Sx, int a_iso, const int64_t *__restrict__ seg,
                                                 const int64_t *__restrict__ lpre, const int64_t *__restrict__ ubase, int64_t ni, int64_t nunits,
                                                 const uint64_t *__restrict__ sJ, const uint32_t *__restrict__ perm, int64_t nj,
                                                 int64_t *__restrict__ upos, uint64_t *__restrict__ key, uint32_t *__restrict__ pay, U *__restrict__ Vx)
{
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if constexpr (!FILL)
        if (blockIdx.x == 0 && threadIdx.x == 0) upos[nunits] = 0;
    if (u >= nunits) return;
    const ExtUnit w = ext_unit(u, ubase, ni, seg, lpre);
    int64_t pos = FILL ? upos[u] : 0;
    for (int64_t k0 = 0; k0 < w.n; k0 += 64) {
        const int64_t k = k0 + lane;
        int64_t lb = 0, mult = 0;
        if (k < w.n) {
            const uint64_t col = (uint64_t)Sj[w.src + k];
            lb = lower_bound<uint64_t>(sJ, 0, nj, col);
            mult = lower_bound<uint64_t>(sJ, lb, nj, col + 1) - lb;
        }
        int64_t incl = mult;  // inclusive sum over the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t t = __shfl_up(incl, (unsigned)d);
            if (lane >= d) incl += t;
        }
        const int64_t total = __shfl(incl, 63);
        if constexpr (FILL) {
            const int64_t excl = incl - mult;
            for (int64_t s0 = 0; s0 < total; s0 += 64) {
                const int64_t s = s0 + lane;
                int from = 0;  // lanes with incl <= s
                for (int step = 32; step > 0; step >>= 1) {
                    const int64_t v = __shfl(incl, from + step - 1);
                    if (v <= s) from += step;
                }
                const int64_t lb_from = __shfl(lb, from), excl_from = __shfl(excl, from);
                if (s < total) {
                    const int64_t p = pos + s;
                    key[p] = ((uint64_t)w.row << 32) | (uint64_t)perm[lb_from + (s - excl_from)];
                    pay[p] = (uint32_t)p;
                    if (Vx) Vx[p] = Sx[a_iso ? 0 : w.src + k0 + from];
                }
            }
        }
        pos += total;
    }
    if constexpr (!FILL)
        if (lane == 0) upos[u] = pos;
}

template <typename U>
__global__ void k_ext_gather(const uint64_t *__restrict__ key, const uint32_t *__restrict__ pay, const U *__restrict__ Vx, int64_t n,
                             int32_t *__restrict__ Tj, U *__restrict__ Tx)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    Tj[q] = (int32_t)(key[q] & 0xffffffffull);
    if (Tx) Tx[q] = Vx[pay[q]];
}

// ---- column / row / element -----------------------------------------------------------------------------------------------------------
// t(k) = S(I[k], j), or with ROW  t(k) = S(j, I[k]): one search in a sorted row per k (I == nullptr: k itself)
template <typename U>
__global__ void k_ext_col(const int64_t *__restrict__ Sp, const int32_t *__restrict__ Sj, const U *__restrict__ Sx, int a_iso, int row_form, int64_t j,
                          const uint64_t *__restrict__ I, int64_t n, uint64_t dim, U *__restrict__ t_val, uint64_t *__restrict__ t_bits, int *oob)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool has = false;
    if (k < n) {
        const uint64_t idx = I ? I[k] : (uint64_t)k;
        if (idx >= dim) *oob = 1;
        else {
            const int64_t row = row_form ? j : (int64_t)idx;
            const int32_t col = (int32_t)(row_form ? (int64_t)idx : j);
            const int64_t e = Sp[row + 1], p = lower_bound<int32_t>(Sj, Sp[row], e, col);
            if (p < e && Sj[p] == col) {
                has = true;
                t_val[k] = Sx[a_iso ? 0 : p];
            }
        }
    }
    const unsigned long long b = __ballot(has);
    if ((threadIdx.x & 63) == 0 && (k >> 6) < ((n + 63) >> 6)) t_bits[k >> 6] = b;
}

// t = row `row` of S as a vector: a thread per entry (the presence words are shared: atomicOr, as k_assign_scatter)
template <typename U>
__global__ void k_ext_rowscatter(const int32_t *__restrict__ Sj, const U *__restrict__ Sx, int a_iso, int64_t e0, int64_t e1, U *__restrict__ t_val,
                                 unsigned long long *__restrict__ t_bits)
{
    const int64_t e = e0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= e1) return;
    const int32_t c = Sj[e];
    t_val[c] = Sx[a_iso ? 0 : e];
    atomicOr(&t_bits[c >> 6], 1ull << (c & 63));
}

// one wavefront: a 64-way search of column j in row i; out[0] = found, out[1] = the value's bytes
template <typename U>
__global__ void __launch_bounds__(64) k_ext_element(const int64_t *__restrict__ Sp, const int32_t *__restrict__ Sj, const U *__restrict__ Sx, int a_iso,
                                                    int64_t i, int32_t j, unsigned long long *__restrict__ out)
{
    const int lane = threadIdx.x;
    int64_t lo = Sp[i], hi = Sp[i + 1];
    while (hi - lo > 64) {  // (wave-uniform) keep the piece whose first column is the last one <= j
        const int64_t step = (hi - lo + 63) >> 6, p = lo + lane * step;
        const unsigned long long le = __ballot(p < hi && Sj[p] <= j);
        const int c = __popcll(le);
        if (c == 0) {
            hi = lo;
            break;
        }
        lo += (c - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    const int64_t p = lo + lane;
    const unsigned long long hit = __ballot(p < hi && Sj[p] == j);
    if (lane == 0) {
        unsigned long long v = 0;
        if (hit) v = (unsigned long long)Sx[a_iso ? 0 : lo + (__ffsll(hit) - 1)];
        out[0] = hit ? 1ull : 0ull;
        out[1] = v;
    }
}

static void ext_check_flag(int *d_flag, const char *what)
{
    int h = 0;
    d2h(&h, d_flag, sizeof(int));
    if (h) fail(GrB_INDEX_OUT_OF_BOUNDS, std::string(what) + ": an index of a list is outside the matrix");
}

// T (of type `ctype`, fresh storage, ni x nj) = S(I, J).  I / J == nullptr: GrB_ALL.  full_values: one value per entry even when S is iso
// (the write rule reads one value per entry when it masks or accumulates)
static MatrixOwner extract_build(GB_Matrix_opaque *S, const uint64_t *I, uint64_t ni, const uint64_t *J, uint64_t nj, int ctype, bool full_values)
{
    const int64_t m = (int64_t)S->nrows, n = (int64_t)S->ncols;
    if (!I) ni = (uint64_t)m;
    if (!J) nj = (uint64_t)n;
    if (ni >= (1ull << 31) || nj >= (1ull << 31)) fail(GrB_NOT_IMPLEMENTED, "GrB_Matrix_extract: index lists of 2^31 or more entries are outside this library's path");
    // ---- J in one pass: a run lo, lo + 1, ...?  strictly increasing?  its smallest and largest column
    bool run = true, increasing = true;
    uint64_t jmin = 0, jmax = 0;
    if (J && nj) {
        jmin = jmax = J[0];
        for (uint64_t k = 1; k < nj; k++) {
            run = run && J[k] == J[0] + k;
            increasing = increasing && J[k] > J[k - 1];
            jmin = std::min(jmin, J[k]);
            jmax = std::max(jmax, J[k]);
        }
    }
    // ---- the lists on the device, their indices checked there; one flag comes back
    DevBuf<uint64_t> dI(I ? (size_t)ni : 0), dJ(J ? (size_t)nj : 0);
    if ((I && ni) || (J && nj)) {
        DevBuf<int> oob(1, true);
        if (I && ni) {
            h2d(dI.p, I, sizeof(uint64_t) * (size_t)ni);
            hipLaunchKernelGGL(k_ext_check, grid1d((int64_t)ni), dim3(256), 0, ctx().stream, (const uint64_t *)dI.p, (int64_t)ni, (uint64_t)m, oob.p);
            ctx().stats.kernel_launches += 1;
        }
        if (J && nj) {
            h2d(dJ.p, J, sizeof(uint64_t) * (size_t)nj);
            hipLaunchKernelGGL(k_ext_check, grid1d((int64_t)nj), dim3(256), 0, ctx().stream, (const uint64_t *)dJ.p, (int64_t)nj, (uint64_t)n, oob.p);
            ctx().stats.kernel_launches += 1;
        }
        ext_check_flag(oob.p, "GrB_Matrix_extract");
    }
    const int stype = S->type->code;
    const size_t ssize = S->type->size;
    const bool t_iso = S->iso && !full_values;
    const int a_iso = S->iso ? 1 : 0;
    // ---- short cuts
    if (ni == 0 || nj == 0 || S->nvals == 0) {
        ctx().stats.method = 6;
        return MatrixOwner(matrix_new(type_of_code(ctype), ni, nj));
    }
    if (!I && !J) {
        ctx().stats.method = 6;
        MatrixOwner Tm(matrix_cast_copy(S, ctype));
        if (full_values) matrix_expand_iso(Tm.get());
        ctx().stats.out_nvals = Tm->nvals;
        return Tm;
    }
    const int method_run = (!J || run) ? 1 : 0;
    MatrixOwner Tm(matrix_new(type_of_code(ctype), ni, nj));
    const int64_t *Sp = S->d_ptr;
    const int32_t *Sj = S->d_col;
    const int64_t NI = (int64_t)ni, NJ = (int64_t)nj;
    // ---- rows: segment, length and units of every output row; the two sums
    const int64_t clo = J ? (int64_t)jmin : 0, chi = J ? (int64_t)jmax + 1 : n;  // the columns the call can select from: [clo, chi)
    const bool narrow = clo > 0 || chi < n;
    DevBuf<int64_t> seg((size_t)NI), lpre((size_t)NI + 1), ubase((size_t)NI + 1);
    const uint64_t *Ip = I ? dI.p : nullptr;
    if (narrow)
        hipLaunchKernelGGL((k_ext_rowseg<true>), grid1d(NI + 1), dim3(256), 0, ctx().stream, Sp, Sj, m, Ip, NI, clo, chi, seg.p, lpre.p, ubase.p);
    else
        hipLaunchKernelGGL((k_ext_rowseg<false>), grid1d(NI + 1), dim3(256), 0, ctx().stream, Sp, Sj, m, Ip, NI, clo, chi, seg.p, lpre.p, ubase.p);
    prim_exclusive_sum_i64(lpre.p, lpre.p, NI + 1);
    prim_exclusive_sum_i64(ubase.p, ubase.p, NI + 1);
    ctx().stats.kernel_launches += 3;
    int64_t E = 0, nunits = 0;  // entries the call can select from, units
    d2h(&E, lpre.p + NI, sizeof(int64_t));
    d2h(&nunits, ubase.p + NI, sizeof(int64_t));
    ctx().stats.tiles = nunits;
    if (nunits > (int64_t)UINT32_MAX * 4) fail(GrB_NOT_IMPLEMENTED, "GrB_Matrix_extract: more than 2^34 units");
    const dim3 ugrid((unsigned)std::max<int64_t>(1, ceil_div(nunits, 4)));
    int64_t kept = 0;
    DevPtr<int64_t> Tp;
    DevPtr<int32_t> Tj;
    DevPtr<char> raw;  // the kept values (one when t_iso) in S's type
    auto alloc_out = [&](int64_t nnz) {
        Tj.reset((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
        raw.reset((char *)dev_alloc(ssize * (size_t)(t_iso ? 1 : nnz)));
        if (t_iso) d2d(raw.p, S->d_val, ssize);
    };
    if (method_run) {
        // ---- method 9: the segments ARE the output rows
        ctx().stats.method = 9;
        kept = E;
        if (kept > 0) {
            alloc_out(kept);
            GRB_DISPATCH_SIZE(ssize, U, hipLaunchKernelGGL((k_ext_copy<U>), ugrid, dim3(256), 0, ctx().stream, Sj, (const U *)S->d_val, a_iso, (const int64_t *)seg.p,
                                                  (const int64_t *)lpre.p, (const int64_t *)ubase.p, NI, nunits, (int32_t)clo, Tj.p,
                                                  (U *)(t_iso ? nullptr : raw.p)))
            ctx().stats.kernel_launches += 1;
            Tp.reset(lpre.release());
        }
    } else if (nunits > 0) {
        DevBuf<int64_t> upos((size_t)nunits + 1);
        Tp.reset((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(NI + 1)));
        if (increasing) {
            // ---- methods 10 / 11.  The table costs 4 * ncols bytes (written once, read at random); it is taken when that is no more than
            // the (4 + sizeof T) * E bytes of columns and values the call reads anyway, so it never more than doubles the traffic.  A byte
            // count, not a timing
            const bool table = 4 * n <= (int64_t)(4 + ssize) * E;
            ctx().stats.method = table ? 10 : 11;
            DevBuf<int32_t> jinv(table ? (size_t)n : 0);
            if (table) {
                GRB_HIP(hipMemsetAsync(jinv.p, 0xff, sizeof(int32_t) * (size_t)n, ctx().stream));
                hipLaunchKernelGGL(k_ext_jinv, grid1d(NJ), dim3(256), 0, ctx().stream, (const uint64_t *)dJ.p, NJ, n, jinv.p);
                ctx().stats.kernel_launches += 2;
            }
#define EXT_PICK(TABLE, FILL, U, TJ, TX)                                                                                                              \
hipLaunchKernelGGL((k_ext_pick<TABLE, FILL, U>), ugrid, dim3(256), 0, ctx().stream, Sj, (const U *)S->d_val, a_iso, (const int64_t *)seg.p,          \
                   (const int64_t *)lpre.p, (const int64_t *)ubase.p, NI, nunits, (const int32_t *)jinv.p, (const uint64_t *)dJ.p, NJ, upos.p, TJ, TX)
            if (table) EXT_PICK(true, false, uint8_t, (int32_t *)nullptr, (uint8_t *)nullptr);
            else EXT_PICK(false, false, uint8_t, (int32_t *)nullptr, (uint8_t *)nullptr);
            prim_exclusive_sum_i64(upos.p, upos.p, nunits + 1);
            ctx().stats.kernel_launches += 2;
            d2h(&kept, upos.p + nunits, sizeof(int64_t));
            if (kept > 0) {
                alloc_out(kept);
                hipLaunchKernelGGL(k_ext_rowptr, grid1d(NI + 1), dim3(256), 0, ctx().stream, (const int64_t *)ubase.p, (const int64_t *)upos.p, NI, Tp.p);
                GRB_DISPATCH_SIZE(ssize, U, {
                    U *tx = (U *)(t_iso ? nullptr : raw.p);
                    if (table) EXT_PICK(true, true, U, Tj.p, tx);
                    else EXT_PICK(false, true, U, Tj.p, tx);
                })
                ctx().stats.kernel_launches += 2;
            }
#undef EXT_PICK
        } else {
            // ---- method 12
            ctx().stats.method = 12;
            int cbits = 1;
            while (cbits < 63 && (1ll << cbits) < n) cbits++;
            DevBuf<uint64_t> sJ((size_t)NJ);
            DevBuf<uint32_t> iota((size_t)NJ), perm((size_t)NJ);
            hipLaunchKernelGGL(k_ext_iota, grid1d(NJ), dim3(256), 0, ctx().stream, NJ, iota.p);
            prim_sort_pairs_u64_u32((const uint64_t *)dJ.p, sJ.p, (const uint32_t *)iota.p, perm.p, NJ, cbits);
#define EXT_DUP(FILL, U, KEY, PAY, VX)                                                                                                               \
hipLaunchKernelGGL((k_ext_dup<FILL, U>), ugrid, dim3(256), 0, ctx().stream, Sj, (const U *)S->d_val, a_iso, (const int64_t *)seg.p,                \
                   (const int64_t *)lpre.p, (const int64_t *)ubase.p, NI, nunits, (const uint64_t *)sJ.p, (const uint32_t *)perm.p, NJ, upos.p, KEY, PAY, VX)
            EXT_DUP(false, uint8_t, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint8_t *)nullptr);
            prim_exclusive_sum_i64(upos.p, upos.p, nunits + 1);
            ctx().stats.kernel_launches += 4;
            d2h(&kept, upos.p + nunits, sizeof(int64_t));
            if (kept >= (1ll << 32))
                fail(GrB_NOT_IMPLEMENTED, "GrB_Matrix_extract: an unsorted or repeating column list that selects 2^32 or more entries (" +
                                              std::to_string(kept) + ") is outside this library's path: sort the list, or extract in pieces");
            if (kept > 0) {
                alloc_out(kept);
                hipLaunchKernelGGL(k_ext_rowptr, grid1d(NI + 1), dim3(256), 0, ctx().stream, (const int64_t *)ubase.p, (const int64_t *)upos.p, NI, Tp.p);
                DevBuf<uint64_t> key((size_t)kept), key_s((size_t)kept);
                DevBuf<uint32_t> pay((size_t)kept), pay_s((size_t)kept);
                DevBuf<char> vx(t_iso ? 0 : ssize * (size_t)kept);
                GRB_DISPATCH_SIZE(ssize, U, EXT_DUP(true, U, key.p, pay.p, (U *)(t_iso ? nullptr : vx.p)))
                int rbits = 0;
                while ((1ll << rbits) < NI) rbits++;
                prim_sort_pairs_u64_u32((const uint64_t *)key.p, key_s.p, (const uint32_t *)pay.p, pay_s.p, kept, 32 + rbits);
                GRB_DISPATCH_SIZE(ssize, U, hipLaunchKernelGGL((k_ext_gather<U>), grid1d(kept), dim3(256), 0, ctx().stream, (const uint64_t *)key_s.p,
                                                      (const uint32_t *)pay_s.p, (const U *)vx.p, kept, Tj.p, (U *)(t_iso ? nullptr : raw.p)))
                ctx().stats.kernel_launches += 4;
            }
#undef EXT_DUP
        }
    } else {
        ctx().stats.method = increasing ? 11 : 12;  // (nothing to select from: no unit, no table)
    }
    if (kept > 0) matrix_adopt(Tm.get(), Tp.release(), Tj.release(), raw.release(), stype, kept, t_iso);
    ctx().stats.out_nvals = kept;
    GRB_HIP(hipGetLastError());
    return Tm;
}

static const uint64_t *ext_list(const uint64_t *L, const char *what)
{
    if (!L) fail(GrB_NULL_POINTER, std::string("GrB_extract: the index list ") + what + " is NULL");
    return L == GrB_ALL ? nullptr : L;
}

static void matrix_extract(GB_Matrix_opaque *C, GB_Matrix_opaque *Mask, const GB_BinaryOp_opaque *accum, GB_Matrix_opaque *A, const uint64_t *I,
                           uint64_t ni, const uint64_t *J, uint64_t nj, const GB_Descriptor_opaque *desc)
{
    require_init();
    check_matrix(C, "C");
    check_matrix(A, "A");
    if (Mask) check_matrix(Mask, "Mask");
    I = ext_list(I, "I");
    J = ext_list(J, "J");
    const Desc f = desc_of(desc);
    const uint64_t in_rows = f.t0 ? A->ncols : A->nrows, in_cols = f.t0 ? A->nrows : A->ncols;
    const uint64_t out_rows = I ? ni : in_rows, out_cols = J ? nj : in_cols;
    if (C->nrows != out_rows || C->ncols != out_cols)
        fail(GrB_DIMENSION_MISMATCH, "GrB_Matrix_extract: output is " + std::to_string(C->nrows) + " x " + std::to_string(C->ncols) + ", the index lists select " +
                                         std::to_string(out_rows) + " x " + std::to_string(out_cols));
    check_mask_accum("GrB_Matrix_extract", C, Mask, accum);
    if (matrix_writes_nothing(C, Mask, f)) return;
    ctx().stats = GrX_Stats{};
    GB_Matrix_opaque *S = f.t0 ? matrix_transpose_cached(A) : A;
    MatrixOwner Tm = extract_build(S, I, ni, J, nj, C->type->code, Mask || accum);
    const int64_t t_nvals = Tm->nvals;
    matrix_finish(C, Mask, accum, std::move(Tm), f, C == A);
    ctx().stats.out_nvals = t_nvals;  // (nnz(T), not nnz(C))
    sync_stream();  // (the index lists were host arrays borrowed for the call)
}

static void col_extract(GB_Vector_opaque *w, GB_Vector_opaque *mask, const GB_BinaryOp_opaque *accum, GB_Matrix_opaque *A, const uint64_t *I, uint64_t ni,
                        uint64_t j, const GB_Descriptor_opaque *desc)
{
    require_init();
    check_vector(w, "w");
    check_matrix(A, "A");
    if (mask) check_vector(mask, "mask");
    I = ext_list(I, "I");
    const Desc f = desc_of(desc);
    const bool row_form = f.t0;  // t(k) = A(j, I[k]) instead of A(I[k], j)
    const uint64_t dim = row_form ? A->ncols : A->nrows, jdim = row_form ? A->nrows : A->ncols;
    const uint64_t n = I ? ni : dim;
    if (w->n != n) fail(GrB_DIMENSION_MISMATCH, "GrB_Col_extract: the output has " + std::to_string(w->n) + " elements, the index list selects " + std::to_string(n));
    check_vector_mask_accum("GrB_Col_extract", w, mask, accum);
    if (j >= jdim)
        fail(GrB_INVALID_INDEX, std::string("GrB_Col_extract: ") + (row_form ? "row " : "column ") + std::to_string(j) + " is outside a matrix of " +
                                    std::to_string(A->nrows) + " x " + std::to_string(A->ncols));
    if (vector_writes_nothing(w, mask, f)) return;
    ctx().stats = GrX_Stats{};
    if (n == 0) return;
    const int at = A->type->code;
    const size_t asize = A->type->size, nwords = bits_words64(n);
    DevBuf<char> t_val(asize * (size_t)n);
    DevBuf<uint64_t> t_bits(nwords, true);
    DevBuf<uint64_t> dI(I ? (size_t)n : 0);
    DevBuf<int> oob(1, true);
    if (I) h2d(dI.p, I, sizeof(uint64_t) * (size_t)n);
    const int a_iso = A->iso ? 1 : 0;
    // every index, in order: a whole row of A (the row form), or of the transpose when it is already cached (the column form)
    GB_Matrix_opaque *R = I ? nullptr : (row_form ? A : A->tr);
    // (GrX_Stats.method, as for the matrix form: 9 = a whole row is copied, 11 = a search per element)
    ctx().stats.method = R ? 9 : 11;
    if (A->nvals == 0) {
        if (I) {
            hipLaunchKernelGGL(k_ext_check, grid1d((int64_t)n), dim3(256), 0, ctx().stream, (const uint64_t *)dI.p, (int64_t)n, dim, oob.p);
            ctx().stats.kernel_launches += 1;
        }
    } else if (R) {
        int64_t e[2] = {0, 0};
        d2h(e, R->d_ptr + j, 2 * sizeof(int64_t));
        if (e[1] > e[0]) {
            GRB_DISPATCH_SIZE(asize, U, hipLaunchKernelGGL((k_ext_rowscatter<U>), grid1d(e[1] - e[0]), dim3(256), 0, ctx().stream, (const int32_t *)R->d_col,
                                                  (const U *)R->d_val, R->iso ? 1 : 0, e[0], e[1], (U *)t_val.p, (unsigned long long *)t_bits.p))
            ctx().stats.kernel_launches += 1;
        }
    } else {
        GRB_DISPATCH_SIZE(asize, U, hipLaunchKernelGGL((k_ext_col<U>), grid1d((int64_t)nwords * 64), dim3(256), 0, ctx().stream, (const int64_t *)A->d_ptr,
                                              (const int32_t *)A->d_col, (const U *)A->d_val, a_iso, row_form ? 1 : 0, (int64_t)j,
                                              (const uint64_t *)(I ? dI.p : nullptr), (int64_t)n, dim, (U *)t_val.p, t_bits.p, oob.p))
        ctx().stats.kernel_launches += 1;
    }
    if (I) ext_check_flag(oob.p, "GrB_Col_extract");
    DevPtr<char> t_hold;
    DevPtr<uint64_t> m_hold;
    const uint64_t *m_bits = vector_mask_words(mask, w, f.structure, m_hold);
    vector_finish(w, vector_values_as(t_val.p, at, w->type->code, (int64_t)n, t_hold), t_bits.p, m_bits, f, accum);
    GRB_HIP(hipGetLastError());
    sync_stream();
}

// found: the entry's bytes (A's type) in v
static bool matrix_element(GB_Matrix_opaque *A, uint64_t i, uint64_t j, unsigned char v[8])
{
    if (i >= A->nrows || j >= A->ncols)
        fail(GrB_INVALID_INDEX, "extractElement: (" + std::to_string(i) + ", " + std::to_string(j) + ") is outside a matrix of " + std::to_string(A->nrows) +
                                    " x " + std::to_string(A->ncols));
    if (A->nvals == 0) return false;
    DevBuf<unsigned long long> out(2);
    GRB_DISPATCH_SIZE(A->type->size, U, hipLaunchKernelGGL((k_ext_element<U>), dim3(1), dim3(64), 0, ctx().stream, (const int64_t *)A->d_ptr, (const int32_t *)A->d_col,
                                                  (const U *)A->d_val, A->iso ? 1 : 0, (int64_t)i, (int32_t)j, out.p))
    unsigned long long h[2] = {0, 0};
    d2h(h, out.p, sizeof(h));
    memcpy(v, &h[1], 8);  // (little endian: the value's bytes come first)
    return h[0] != 0;
}

template <typename T>
static GrB_Info matrix_extract_element(T *x, GB_Matrix_opaque *A, uint64_t i, uint64_t j)
{
    if (!x) fail(GrB_NULL_POINTER, "extractElement: output pointer is NULL");
    unsigned char v[8];
    if (!matrix_element(A, i, j, v)) return GrB_NO_VALUE;
    GRB_DISPATCH_TYPE(A->type->code, TA, {
        TA a;
        memcpy(&a, v, sizeof(TA));
        *x = cast_value<T, TA>(a);
    })
    return GrB_SUCCESS;
}

void preload_extract() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_ext_rowptr)); (void)hipGetLastError(); }

}  // namespace grb

using namespace grb;

extern "C" GrB_Info GrB_Matrix_extract(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni,
                                       const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc)
{
    GRB_TRY
    matrix_extract(C, Mask, accum, A, I, ni, J, nj, desc);
    GRB_CATCH(errp(C))
}

extern "C" GrB_Info GrB_Col_extract(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni,
                                    GrB_Index j, const GrB_Descriptor desc)
{
    GRB_TRY
    col_extract(w, mask, accum, A, I, ni, j, desc);
    GRB_CATCH(errp(w))
}

#define DEF_EXTRACT_ELEMENT(NAME, ctype)                                                                               \
    extern "C" GrB_Info GrB_Matrix_extractElement_##NAME(ctype *x, const GrB_Matrix A, GrB_Index i, GrB_Index j)       \
    {                                                                                                                  \
        GRB_TRY                                                                                                        \
        require_init();                                                                                                \
        check_matrix(A, "A");                                                                                          \
        return matrix_extract_element<ctype>(x, A, i, j);                                                              \
        GRB_CATCH(errp(A))                                                                                             \
    }
GRB_FOR_EACH_TYPE(DEF_EXTRACT_ELEMENT)
#undef DEF_EXTRACT_ELEMENT
