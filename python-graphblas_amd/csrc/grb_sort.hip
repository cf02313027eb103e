// grb_sort.hip -- GxB_Matrix_sort / GxB_Vector_sort: the entries of every row ordered by value (reference
// core/ss/matrix.py:3983-4048, core/ss/vector.py:1559-1620), and GrX_Matrix_reverse_rows, the row reversal ss.compactify(reverse=True)
// needs behind it.
//
//   C(i, r) = the r-th value of row i of A in the order of op (GrB_LT_<T> ascending, GrB_GT_<T> descending), cast A -> C directly
//   P(i, r) = the column that value had in A;    both at columns 0 .. len_i - 1, row pointers those of A
// Ties go to the smaller original column under both operators; -0.0 and +0.0 tie; NaNs tie with each other and come after every
// number under BOTH operators (the library's own answer: the backend's comparator is no strict weak order on NaN).
//
// The sort item of an entry is (key, q): q its position inside its row -- a CSR row is in column order, so q is also the tie-break --
// and key the value, cast to the operator's type, as order-preserving unsigned bits (32 wide for 1-, 2- and 4-byte types, 64 for
// 8-byte types): sign flipped for signed integers, the sign-dependent flip for floats with -0.0 made +0.0, the bits complemented
// under GT.  "Number or NaN" is folded into the same word: NaN takes the all-ones key under both operators, which no number maps to
// (the largest number key is that of +inf ascending / -inf descending, 0xff80.. / 0xfff0..).  After the sort P = Aj[start + q] and
// C = Ax[start + q]: a direct gather, the key is never turned back into a value.
//
// Rows go down one of three paths by their length (k_sort_classify: a count pass, then an append pass into one row list):
//   lane groups   len <= SORT_WAVE_MAX = 64: W lanes per row, 64 / W rows per wavefront, W in {4, 16, 64} by length, short slots padded
//                 with a sentinel above every real item; a bitonic network in registers over __shfl_xor (k_sort_lanes)
//   LDS           len <= SORT_LDS_MAX = 4096: one workgroup of 256 per row, the items in LDS, bitonic over the next power of two
//                 (k_sort_lds)
//   radix         longer rows (the hubs): their entries gathered into one array, a stable radix sort on the key with the gathered
//                 position as payload, a second stable pass on the row's ordinal among the long rows over only the bits that ordinal
//                 needs; stability is the tie-break (k_sort_gather, k_sort_ordkeys, k_sort_long_fill)
// Every path writes an output entry once: column r, P, and the value moved in A's type (cast to C's type afterwards when they differ).
// The vector form compacts the present entries into one segment and runs the same paths on it.
#include <algorithm>

#include "grb_internal.hpp"
#include "grb_ops.hpp"

namespace grb {

constexpr int64_t SORT_WAVE_MAX = 64;
// LDS budget of k_sort_lds: an item is a key of up to 8 bytes and a 4-byte position, 12 bytes; MI355X has 160 KiB of LDS per CU and a
// workgroup may take 64 KiB.  4096 items = 48 KiB (32 KiB with 4-byte keys): three (five) workgroups of 256 per CU.  8192 items would
// be 96 KiB -- one workgroup per CU, and more than a workgroup may take.  So SORT_LDS_MAX is the largest power of two that keeps at
// least two workgroups per CU.
constexpr int64_t SORT_LDS_MAX = 4096;
enum { SORT_W4 = 0, SORT_W16, SORT_W64, SORT_LDS, SORT_RADIX, SORT_NCLS };

static int64_t g_sort_last[3] = {0, 0, 0};

template <typename TO> struct SortKey { using K = typename std::conditional<sizeof(TO) == 8, uint64_t, uint32_t>::type; };

// the value as order-preserving unsigned bits; desc: the order of GT
template <typename TO>
__device__ __forceinline__ typename SortKey<TO>::K sort_key(TO v, bool desc)
{
    using K = typename SortKey<TO>::K;
    K k;
    if constexpr (std::is_same<TO, bool>::value) k = v ? 1u : 0u;
    else if constexpr (std::is_same<TO, float>::value) {
        if (v != v) return ~(K)0;
        const uint32_t u = v == 0.0f ? 0u : __builtin_bit_cast(uint32_t, v);
        k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    } else if constexpr (std::is_same<TO, double>::value) {
        if (v != v) return ~(K)0;
        const uint64_t u = v == 0.0 ? 0ull : __builtin_bit_cast(uint64_t, v);
        k = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    } else if constexpr (std::is_signed<TO>::value) {
        if constexpr (sizeof(TO) == 8) k = (uint64_t)v ^ 0x8000000000000000ull;
        else k = (uint32_t)(int32_t)v ^ 0x80000000u;
    } else k = (K)v;
    return desc ? (K)~k : k;
}

template <typename K> struct SortItem {
    K key;
    uint32_t q;
};
template <typename K> __device__ __forceinline__ bool item_less(const SortItem<K> &a, const SortItem<K> &b)
{
    return a.key < b.key || (a.key == b.key && a.q < b.q);
}
constexpr uint32_t SORT_PAD_Q = 0xffffffffu;  // (a real position is below 2^31: the padding item lies above every real one)

// what every path reads and writes.  Aj == nullptr (the vector form): P gets the position q itself
struct SortIO {
    const int64_t *Ap;
    const int32_t *Aj;
    const void *Ax;  // the values that are moved, in A's type
    int vsize, a_iso;
    int32_t *Tj;     // output columns (one array; the second output gets a copy)
    int64_t *Px;     // nullptr: no P
    void *Cx;        // nullptr: no C, or an iso C
};

// output entry o of a row that starts at `start` takes position r and the source entry start + q
__device__ __forceinline__ void sort_emit(const SortIO &io, int64_t start, int64_t r, int64_t q)
{
    const int64_t o = start + r, s = start + q;
    if (io.Tj) io.Tj[o] = (int32_t)r;
    if (io.Px) io.Px[o] = io.Aj ? (int64_t)io.Aj[s] : q;
    if (io.Cx) {
        switch (io.vsize) {
        case 1: ((uint8_t *)io.Cx)[o] = ((const uint8_t *)io.Ax)[s]; break;
        case 2: ((uint16_t *)io.Cx)[o] = ((const uint16_t *)io.Ax)[s]; break;
        case 4: ((uint32_t *)io.Cx)[o] = ((const uint32_t *)io.Ax)[s]; break;
        default: ((uint64_t *)io.Cx)[o] = ((const uint64_t *)io.Ax)[s]; break;
        }
    }
}

__device__ __forceinline__ int sort_class(int64_t len)
{
    return len <= 4 ? SORT_W4 : (len <= 16 ? SORT_W16 : (len <= SORT_WAVE_MAX ? SORT_W64 : (len <= SORT_LDS_MAX ? SORT_LDS : SORT_RADIX)));
}

// ---- rows by class: FILL = false counts (cnt[c] += rows of class c; empty rows take no part), FILL = true appends row i to its
//      class's piece of `rows` (off[c] + a slot from the cursor cnt[c]); one atomic per wavefront and class -----------------------------
template <bool FILL>
__global__ void __launch_bounds__(256) k_sort_classify(const int64_t *__restrict__ Ap, int64_t m, unsigned int *__restrict__ cnt,
                                                       const int64_t *__restrict__ off, int32_t *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int cls = -1;
    if (i < m) {
        const int64_t len = Ap[i + 1] - Ap[i];
        if (len > 0) cls = sort_class(len);
    }
    for (int c = 0; c < SORT_NCLS; c++) {
        const unsigned long long mask = __ballot(cls == c);
        if (!mask) continue;  // (uniform over the wavefront)
        const int leader = __ffsll(mask) - 1;
        unsigned int base = 0;
        if (lane == leader) base = atomicAdd(&cnt[c], (unsigned int)__popcll(mask));
        if constexpr (FILL) {
            base = __shfl(base, leader);
            if (cls == c) rows[off[c] + base + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)i;
        }
    }
}

// ---- lane groups: W lanes per row, the bitonic network in registers -------------------------------------------------------------------
template <typename TO, int W>
__global__ void __launch_bounds__(256) k_sort_lanes(SortIO io, const TO *__restrict__ xs, const int32_t *__restrict__ rows, int64_t nrows, bool desc)
{
    using K = typename SortKey<TO>::K;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, grp = gid / W;
    const int sub = (int)(threadIdx.x & (W - 1));
    const bool valid = grp < nrows;
    int64_t start = 0, len = 0;
    if (valid) {
        const int64_t row = rows[grp];
        start = io.Ap[row];
        len = io.Ap[row + 1] - start;
    }
    SortItem<K> it{~(K)0, SORT_PAD_Q};
    if (sub < len) {
        it.key = sort_key<TO>(xs[io.a_iso ? 0 : start + sub], desc);
        it.q = (uint32_t)sub;
    }
    // (every lane of the wavefront takes part in every exchange; a partner lane ^ j stays inside the group of W)
#pragma unroll
    for (int k = 2; k <= W; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            SortItem<K> other;
            if constexpr (sizeof(K) == 8) other.key = (K)__shfl_xor((unsigned long long)it.key, j);
            else other.key = (K)__shfl_xor((unsigned int)it.key, j);
            other.q = __shfl_xor(it.q, j);
            const bool take_min = ((sub & j) == 0) == ((sub & k) == 0);
            if (take_min ? item_less(other, it) : item_less(it, other)) it = other;
        }
    }
    if (sub < len) sort_emit(io, start, sub, it.q);
}

// ---- LDS: one workgroup per row -------------------------------------------------------------------------------------------------------
// Keys and positions are two arrays, so a compare-exchange reads consecutive words per wavefront: partners j >= 64 apart are read
// conflict-free; below, a wavefront's 64 pairs fall into 2 j-strided runs per 2 j words, the usual bitonic 2-way conflict
template <typename TO>
__global__ void __launch_bounds__(256) k_sort_lds(SortIO io, const TO *__restrict__ xs, const int32_t *__restrict__ rows, bool desc)
{
    using K = typename SortKey<TO>::K;
    __shared__ K s_key[SORT_LDS_MAX];
    __shared__ uint32_t s_q[SORT_LDS_MAX];
    const int tid = threadIdx.x;
    const int64_t row = rows[blockIdx.x];
    const int64_t start = io.Ap[row];
    const int len = (int)(io.Ap[row + 1] - start);  // (<= SORT_LDS_MAX by its class)
    int N = 128;
    while (N < len) N <<= 1;
    for (int i = tid; i < N; i += 256) {
        if (i < len) {
            s_key[i] = sort_key<TO>(xs[io.a_iso ? 0 : start + i], desc);
            s_q[i] = (uint32_t)i;
        } else {
            s_key[i] = ~(K)0;
            s_q[i] = SORT_PAD_Q;
        }
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (N >> 1); t += 256) {
                const int a = 2 * t - (t & (j - 1)), b = a + j;  // (j a power of two: (t / j) * 2 j + t % j)
                const SortItem<K> x{s_key[a], s_q[a]}, y{s_key[b], s_q[b]};
                const bool up = (a & k) == 0;
                if (up ? item_less(y, x) : item_less(x, y)) {
                    s_key[a] = y.key; s_q[a] = y.q;
                    s_key[b] = x.key; s_q[b] = x.q;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < len; i += 256) sort_emit(io, start, i, s_q[i]);
}

// ---- radix: the long rows --------------------------------------------------------------------------------------------------------------
// glen[o] = entries of long row o; glen[nlong] = 0 (the exclusive sum leaves the total there)
__global__ void k_sort_long_lens(const int64_t *__restrict__ Ap, const int32_t *__restrict__ rows, int64_t nlong, int64_t *__restrict__ glen)
{
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o <= nlong) glen[o] = o < nlong ? Ap[rows[o] + 1] - Ap[rows[o]] : 0;
}
// a workgroup per long row: key, gathered position and ordinal of every entry
template <typename TO>
__global__ void __launch_bounds__(256) k_sort_gather(SortIO io, const TO *__restrict__ xs, const int32_t *__restrict__ rows, const int64_t *__restrict__ goff,
                                                     bool desc, typename SortKey<TO>::K *__restrict__ gkey, uint32_t *__restrict__ gpos, uint32_t *__restrict__ gord)
{
    const int64_t o = blockIdx.x, start = io.Ap[rows[o]], g0 = goff[o], len = goff[o + 1] - g0;
    for (int64_t t = threadIdx.x; t < len; t += 256) {
        gkey[g0 + t] = sort_key<TO>(xs[io.a_iso ? 0 : start + t], desc);
        gpos[g0 + t] = (uint32_t)(g0 + t);
        gord[g0 + t] = (uint32_t)o;
    }
}
__global__ void k_sort_ordkeys(const uint32_t *__restrict__ gpos, const uint32_t *__restrict__ gord, int64_t G, uint32_t *__restrict__ okey)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < G) okey[i] = gord[gpos[i]];
}
// slot i of the twice-sorted order belongs to the row of its source (the rows keep their lengths and their order)
__global__ void k_sort_long_fill(SortIO io, const int32_t *__restrict__ rows, const int64_t *__restrict__ goff, const uint32_t *__restrict__ gpos,
                                 const uint32_t *__restrict__ gord, int64_t G)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    const int64_t g = gpos[i], o = gord[g], g0 = goff[o];
    sort_emit(io, io.Ap[rows[o]], i - g0, g - g0);
}

// ---- the three paths over the m segments of io.Ap ---------------------------------------------------------------------------------------
template <typename TO>
static void sort_segments_typed(const SortIO &io, const void *xs_, int64_t m, bool desc, const int32_t *rows, const int64_t *cnt, const int64_t *off)
{
    using K = typename SortKey<TO>::K;
    const TO *xs = (const TO *)xs_;
    hipStream_t st = ctx().stream;
    auto wave_blocks = [](int64_t nrows, int W) {
        const int64_t g = ceil_div(nrows * W, 256);
        if (g > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
        return dim3((unsigned)g);
    };
    if (cnt[SORT_W4]) hipLaunchKernelGGL((k_sort_lanes<TO, 4>), wave_blocks(cnt[SORT_W4], 4), dim3(256), 0, st, io, xs, rows + off[SORT_W4], cnt[SORT_W4], desc);
    if (cnt[SORT_W16]) hipLaunchKernelGGL((k_sort_lanes<TO, 16>), wave_blocks(cnt[SORT_W16], 16), dim3(256), 0, st, io, xs, rows + off[SORT_W16], cnt[SORT_W16], desc);
    if (cnt[SORT_W64]) hipLaunchKernelGGL((k_sort_lanes<TO, 64>), wave_blocks(cnt[SORT_W64], 64), dim3(256), 0, st, io, xs, rows + off[SORT_W64], cnt[SORT_W64], desc);
    if (cnt[SORT_LDS]) hipLaunchKernelGGL((k_sort_lds<TO>), dim3((unsigned)cnt[SORT_LDS]), dim3(256), 0, st, io, xs, rows + off[SORT_LDS], desc);
    ctx().stats.kernel_launches += (cnt[SORT_W4] > 0) + (cnt[SORT_W16] > 0) + (cnt[SORT_W64] > 0) + (cnt[SORT_LDS] > 0);
    const int64_t nlong = cnt[SORT_RADIX];
    if (nlong) {
        const int32_t *lrows = rows + off[SORT_RADIX];
        DevBuf<int64_t> goff((size_t)nlong + 1);
        hipLaunchKernelGGL(k_sort_long_lens, grid1d(nlong + 1), dim3(256), 0, st, io.Ap, lrows, nlong, goff.p);
        prim_exclusive_sum_i64(goff.p, goff.p, nlong + 1);
        int64_t G = 0;
        d2h(&G, goff.p + nlong, sizeof(int64_t));
        if (G >= 0xffffffffll) fail(GrB_NOT_IMPLEMENTED, "GxB_sort: the rows beyond the in-core limit hold 2^32 entries or more");
        DevBuf<K> gkey((size_t)G), gkey2((size_t)G);
        DevBuf<uint32_t> gpos((size_t)G), gpos2((size_t)G), gord((size_t)G);
        hipLaunchKernelGGL((k_sort_gather<TO>), dim3((unsigned)nlong), dim3(256), 0, st, io, xs, lrows, (const int64_t *)goff.p, desc, gkey.p, gpos.p, gord.p);
        if constexpr (sizeof(K) == 8) prim_sort_pairs_u64_u32_bits(gkey.p, gkey2.p, gpos.p, gpos2.p, G, 0, 64);
        else prim_sort_pairs_u32_u32_bits(gkey.p, gkey2.p, gpos.p, gpos2.p, G, 0, 32);
        const uint32_t *order = gpos2.p;
        int obits = 0;
        while (((int64_t)1 << obits) < nlong) obits++;
        DevBuf<uint32_t> okey((size_t)(obits ? G : 1)), okey2((size_t)(obits ? G : 1));
        if (obits) {  // (one long row: the first pass is the answer)
            hipLaunchKernelGGL(k_sort_ordkeys, grid1d(G), dim3(256), 0, st, (const uint32_t *)gpos2.p, (const uint32_t *)gord.p, G, okey.p);
            prim_sort_pairs_u32_u32_bits(okey.p, okey2.p, gpos2.p, gpos.p, G, 0, obits);
            order = gpos.p;
        }
        hipLaunchKernelGGL(k_sort_long_fill, grid1d(G), dim3(256), 0, st, io, lrows, (const int64_t *)goff.p, order, (const uint32_t *)gord.p, G);
        ctx().stats.kernel_launches += obits ? 8 : 5;
        GRB_HIP(hipGetLastError());
        sync_stream();  // (the temporaries of this scope are released at its end)
    }
    (void)m;
}

// classifies the m segments, runs the paths, records GrX_sort_last
static void sort_segments(const SortIO &io, const void *xs, int ot, int64_t m, bool desc)
{
    hipStream_t st = ctx().stream;
    DevBuf<unsigned int> cnt_d(2 * SORT_NCLS, true);
    hipLaunchKernelGGL((k_sort_classify<false>), grid1d(m), dim3(256), 0, st, io.Ap, m, cnt_d.p, (const int64_t *)nullptr, (int32_t *)nullptr);
    unsigned int cnt_h[SORT_NCLS];
    d2h(cnt_h, cnt_d.p, sizeof(cnt_h));
    int64_t cnt[SORT_NCLS], off[SORT_NCLS + 1];
    off[0] = 0;
    for (int c = 0; c < SORT_NCLS; c++) {
        cnt[c] = cnt_h[c];
        off[c + 1] = off[c] + cnt[c];
    }
    DevBuf<int32_t> rows((size_t)off[SORT_NCLS]);
    DevBuf<int64_t> off_d(SORT_NCLS);
    h2d(off_d.p, off, sizeof(int64_t) * SORT_NCLS);
    hipLaunchKernelGGL((k_sort_classify<true>), grid1d(m), dim3(256), 0, st, io.Ap, m, cnt_d.p + SORT_NCLS, (const int64_t *)off_d.p, rows.p);
    ctx().stats.kernel_launches += 2;
    GRB_DISPATCH_TYPE(ot, TO, { sort_segments_typed<TO>(io, xs, m, desc, rows.p, cnt, off); })
    g_sort_last[0] = m - cnt[SORT_LDS] - cnt[SORT_RADIX];  // (rows without an entry count here: they take no lane)
    g_sort_last[1] = cnt[SORT_LDS];
    g_sort_last[2] = cnt[SORT_RADIX];
    GRB_HIP(hipGetLastError());
    sync_stream();  // (`rows` and the counters are released at the end of this scope)
}

// LT / GT in `desc`, or the error the operator earns
static bool sort_op_desc(const GB_BinaryOp_opaque *op, const char *who)
{
    if (!op) fail(GrB_NULL_POINTER, std::string(who) + ": the operator is NULL");
    if (op->op == OP_LT || op->op == OP_GT) return op->op == OP_GT;
    const std::string name = op->name ? op->name : "the operator";
    if (op_is_comparison(op->op) || op->type == TC_BOOL)
        fail(GrB_NOT_IMPLEMENTED, std::string(who) + ": " + name + " is not implemented as a sort order: GrB_LT_<T> (ascending) and GrB_GT_<T> (descending) are");
    fail(GrB_DOMAIN_MISMATCH, std::string(who) + ": " + name + " does not return BOOL: a sort takes GrB_LT_<T> or GrB_GT_<T>");
}
static void sort_check_perm_type(int code, const char *who, const char *what)
{
    if (code != TC_INT64 && code != TC_UINT64) fail(GrB_DOMAIN_MISMATCH, std::string(who) + ": " + what + " must be INT64 or UINT64");
}

// TC / TP (fresh, S's shape, types ctype / ptype; either may be unwanted: -1) = the rowwise sort of S
static void sort_build(GB_Matrix_opaque *S, int ot, bool desc, int ctype, int ptype, MatrixOwner &TC, MatrixOwner &TP)
{
    if (ctype >= 0) TC.reset(matrix_new(type_of_code(ctype), S->nrows, S->ncols));
    if (ptype >= 0) TP.reset(matrix_new(type_of_code(ptype), S->nrows, S->ncols));
    g_sort_last[0] = (int64_t)S->nrows;
    g_sort_last[1] = g_sort_last[2] = 0;
    if (S->nvals == 0) return;
    const int64_t m = (int64_t)S->nrows, nnz = S->nvals;
    const size_t ssize = S->type->size;
    const bool c_iso = S->iso;
    DevPtr<char> xcast;
    const void *xs = values_as(S, ot, xcast);
    DevPtr<int32_t> Tj((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
    DevPtr<int64_t> Px;
    DevPtr<char> raw;
    if (ptype >= 0) Px.reset((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)nnz));
    if (ctype >= 0) {
        raw.reset((char *)dev_alloc(ssize * (size_t)(c_iso ? 1 : nnz)));
        if (c_iso) d2d(raw.p, S->d_val, ssize);
    }
    SortIO io{S->d_ptr, S->d_col, S->d_val, (int)ssize, S->iso ? 1 : 0, Tj.p, Px.p, (ctype >= 0 && !c_iso) ? (void *)raw.p : nullptr};
    sort_segments(io, xs, ot, m, desc);
    auto rowptr_copy = [&]() {
        int64_t *p = (int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1));
        d2d(p, S->d_ptr, sizeof(int64_t) * (size_t)(m + 1));
        return p;
    };
    if (ctype >= 0 && ptype >= 0) {
        DevPtr<int32_t> Tj2((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
        d2d(Tj2.p, Tj.p, sizeof(int32_t) * (size_t)nnz);
        DevPtr<int64_t> p2(rowptr_copy());
        matrix_adopt(TP.get(), p2.release(), Tj2.release(), Px.release(), ptype, nnz, false);
    } else if (ptype >= 0) {
        DevPtr<int64_t> p2(rowptr_copy());
        matrix_adopt(TP.get(), p2.release(), Tj.release(), Px.release(), ptype, nnz, false);
    }
    if (ctype >= 0) {
        DevPtr<int64_t> p1(rowptr_copy());
        matrix_adopt(TC.get(), p1.release(), Tj.release(), raw.release(), S->type->code, nnz, c_iso);
    }
}

// the transpose of T as a fresh matrix of T's type (the columnwise sort: outputs of the transpose's rowwise sort, turned back)
static MatrixOwner sort_transposed(MatrixOwner &T)
{
    return MatrixOwner(matrix_cast_copy(matrix_transpose_cached(T.get()), T->type->code));
}

static void matrix_sort(GB_Matrix_opaque *C, GB_Matrix_opaque *P, const GB_BinaryOp_opaque *op, GB_Matrix_opaque *A, const GB_Descriptor_opaque *desc)
{
    const char *who = "GxB_Matrix_sort";
    require_init();
    if (!C && !P) fail(GrB_NULL_POINTER, std::string(who) + ": C and P are both NULL");
    if (C) check_matrix(C, "C");
    if (P) check_matrix(P, "P");
    check_matrix(A, "A");
    const bool gt = sort_op_desc(op, who);
    if (P) sort_check_perm_type(P->type->code, who, "P");
    for (GB_Matrix_opaque *X : {C, P})
        if (X && (X->nrows != A->nrows || X->ncols != A->ncols))
            fail(GrB_DIMENSION_MISMATCH, std::string(who) + ": " + (X == C ? "C" : "P") + " is " + std::to_string(X->nrows) + " x " + std::to_string(X->ncols) +
                                             ", A " + std::to_string(A->nrows) + " x " + std::to_string(A->ncols));
    const bool t0 = desc && desc->t0;  // (every other field is ignored: no mask, no accumulator, no replace)
    ctx().stats = GrX_Stats{};
    ctx().stats.method = 27;
    GB_Matrix_opaque *S = t0 ? matrix_transpose_cached(A) : A;
    MatrixOwner TC, TP;
    sort_build(S, op->type, gt, C ? C->type->code : -1, P ? P->type->code : -1, TC, TP);
    if (t0) {
        if (C) TC = sort_transposed(TC);
        if (P) TP = sort_transposed(TP);
    }
    // both outputs are built before either is written: C, P and A may alias one another
    const Desc plain;
    if (C) matrix_finish(C, nullptr, nullptr, std::move(TC), plain, C == A);
    if (P) matrix_finish(P, nullptr, nullptr, std::move(TP), plain, P == A);
    ctx().stats.out_nvals = C ? C->nvals : P->nvals;
    if (ctx().blocking) sync_stream();
}

// ---- vector form -------------------------------------------------------------------------------------------------------------------------
template <typename U>
__global__ void k_vsort_compact(const U *__restrict__ val, const uint64_t *__restrict__ idx, int64_t nv, U *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nv) out[i] = val[idx[i]];
}
// sorted position r takes the compacted entry perm[r]: its value (cv, may be nullptr) and its original index
template <typename U>
__global__ void k_vsort_finish(const int64_t *__restrict__ perm, const U *__restrict__ cv, const uint64_t *__restrict__ idx, int64_t nv, U *__restrict__ wv,
                               uint64_t *__restrict__ pv)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nv) return;
    const int64_t q = perm[r];
    if (wv) wv[r] = cv[q];
    if (pv) pv[r] = idx[q];
}
// presence of the first nv positions
__global__ void k_vsort_bits(uint64_t *__restrict__ bits, int64_t nwords, int64_t nv)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    const int64_t lo = w << 6;
    bits[w] = nv >= lo + 64 ? ~0ull : (nv > lo ? ((1ull << (nv - lo)) - 1ull) : 0ull);
}

static void vector_take_prefix(GB_Vector_opaque *w, int src_type, const void *src, int64_t nv)
{
    vector_ensure_storage(w);
    cast_array(w->type->code, w->d_val, src_type, src, nv);
    const int64_t nwords = (int64_t)bits_words64(w->n);
    hipLaunchKernelGGL(k_vsort_bits, grid1d(nwords), dim3(256), 0, ctx().stream, w->d_bits, nwords, nv);
    w->nvals = nv;
}

static void vector_sort(GB_Vector_opaque *w, GB_Vector_opaque *p, const GB_BinaryOp_opaque *op, GB_Vector_opaque *u, const GB_Descriptor_opaque *desc)
{
    const char *who = "GxB_Vector_sort";
    require_init();
    if (!w && !p) fail(GrB_NULL_POINTER, std::string(who) + ": w and p are both NULL");
    if (w) check_vector(w, "w");
    if (p) check_vector(p, "p");
    check_vector(u, "u");
    const bool gt = sort_op_desc(op, who);
    if (p) sort_check_perm_type(p->type->code, who, "p");
    for (GB_Vector_opaque *x : {w, p})
        if (x && x->n != u->n)
            fail(GrB_DIMENSION_MISMATCH, std::string(who) + ": " + (x == w ? "w" : "p") + " has size " + std::to_string(x->n) + ", u " + std::to_string(u->n));
    (void)desc;
    ctx().stats = GrX_Stats{};
    ctx().stats.method = 28;
    ctx().stats.out_nvals = -1;
    uint64_t *idx_raw = nullptr;
    const int64_t nv = vector_index_list(u, &idx_raw);
    DevPtr<uint64_t> idx(idx_raw);
    g_sort_last[0] = 1;
    g_sort_last[1] = g_sort_last[2] = 0;
    if (nv == 0) {
        if (w) vector_release_storage(w);
        if (p) vector_release_storage(p);
        return;
    }
    if (nv > 0x7fffffffll) fail(GrB_NOT_IMPLEMENTED, std::string(who) + ": vectors with 2^31 entries or more");
    hipStream_t st = ctx().stream;
    const int ut = u->type->code, ot = op->type;
    const size_t usize = u->type->size;
    // one segment: the present values compacted (in u's type, and in the operator's when that is another), the segment's two bounds
    DevBuf<char> cv(usize * (size_t)nv);
    GRB_DISPATCH_SIZE(usize, U, hipLaunchKernelGGL((k_vsort_compact<U>), grid1d(nv), dim3(256), 0, st, (const U *)u->d_val, (const uint64_t *)idx.p, nv, (U *)cv.p))
    DevPtr<char> xcast;
    const void *xs = cv.p;
    if (ot != ut) {
        xcast.reset((char *)dev_alloc(type_size(ot) * (size_t)nv));
        cast_array(ot, xcast.p, ut, cv.p, nv);
        xs = xcast.p;
    }
    DevBuf<int64_t> seg(2), perm((size_t)nv);
    const int64_t bounds[2] = {0, nv};
    h2d(seg.p, bounds, sizeof(bounds));
    SortIO io{seg.p, nullptr, nullptr, (int)usize, 0, nullptr, perm.p, nullptr};
    sort_segments(io, xs, ot, 1, gt);
    // the outputs in buffers of their own first: w and p may be u
    DevBuf<char> wv(usize * (size_t)(w ? nv : 1));
    DevBuf<uint64_t> pv((size_t)(p ? nv : 1));
    GRB_DISPATCH_SIZE(usize, U, hipLaunchKernelGGL((k_vsort_finish<U>), grid1d(nv), dim3(256), 0, st, (const int64_t *)perm.p, (const U *)cv.p, (const uint64_t *)idx.p,
                                                   nv, (U *)(w ? wv.p : nullptr), p ? pv.p : nullptr))
    if (w) vector_take_prefix(w, ut, wv.p, nv);
    if (p) vector_take_prefix(p, p->type->code, pv.p, nv);
    ctx().stats.kernel_launches += 2 + (w ? 2 : 0) + (p ? 2 : 0);
    GRB_HIP(hipGetLastError());
    sync_stream();  // (the temporaries of this scope are released at its end)
}

// ---- row reversal ------------------------------------------------------------------------------------------------------------------------
// a wavefront per row: the values of the row in reverse order over the row's own pattern
template <typename U>
__global__ void __launch_bounds__(256) k_reverse_rows(const int64_t *__restrict__ Ap, int64_t m, const U *__restrict__ Ax, U *__restrict__ out)
{
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (row >= m) return;
    const int64_t start = Ap[row], end = Ap[row + 1];
    for (int64_t e = start + (threadIdx.x & 63); e < end; e += 64) out[e] = Ax[start + (end - 1 - e)];
}

static void matrix_reverse_rows(GB_Matrix_opaque *C, GB_Matrix_opaque *A)
{
    require_init();
    check_matrix(C, "C");
    check_matrix(A, "A");
    if (C->nrows != A->nrows || C->ncols != A->ncols)
        fail(GrB_DIMENSION_MISMATCH, "GrX_Matrix_reverse_rows: C is " + std::to_string(C->nrows) + " x " + std::to_string(C->ncols) + ", A " +
                                         std::to_string(A->nrows) + " x " + std::to_string(A->ncols));
    ctx().stats = GrX_Stats{};
    MatrixOwner T(matrix_new(C->type, A->nrows, A->ncols));
    if (A->nvals) {
        const int64_t m = (int64_t)A->nrows, nnz = A->nvals;
        const size_t ssize = A->type->size;
        DevPtr<int64_t> Tp((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1)));
        DevPtr<int32_t> Tj((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)nnz));
        DevPtr<char> raw((char *)dev_alloc(ssize * (size_t)(A->iso ? 1 : nnz)));
        d2d(Tp.p, A->d_ptr, sizeof(int64_t) * (size_t)(m + 1));
        d2d(Tj.p, A->d_col, sizeof(int32_t) * (size_t)nnz);
        if (A->iso) d2d(raw.p, A->d_val, ssize);
        else {
            const int64_t g = ceil_div(m, 4);
            if (g > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
            GRB_DISPATCH_SIZE(ssize, U, hipLaunchKernelGGL((k_reverse_rows<U>), dim3((unsigned)g), dim3(256), 0, ctx().stream, (const int64_t *)A->d_ptr, m,
                                                           (const U *)A->d_val, (U *)raw.p))
            ctx().stats.kernel_launches += 1;
        }
        matrix_adopt(T.get(), Tp.release(), Tj.release(), raw.release(), A->type->code, nnz, A->iso);
    }
    matrix_finish(C, nullptr, nullptr, std::move(T), Desc{}, C == A);
    ctx().stats.out_nvals = C->nvals;
    GRB_HIP(hipGetLastError());
    if (ctx().blocking) sync_stream();
}

// ... and of a vector: the values of its entries in reverse order over its own pattern
template <typename U>
__global__ void k_reverse_vector(const U *__restrict__ val, const uint64_t *__restrict__ idx, int64_t nv, U *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nv) out[idx[i]] = val[idx[nv - 1 - i]];
}

static void vector_reverse(GB_Vector_opaque *w, GB_Vector_opaque *u)
{
    require_init();
    check_vector(w, "w");
    check_vector(u, "u");
    if (w->n != u->n) fail(GrB_DIMENSION_MISMATCH, "GrX_Vector_reverse: w has size " + std::to_string(w->n) + ", u " + std::to_string(u->n));
    ctx().stats = GrX_Stats{};
    ctx().stats.out_nvals = -1;
    uint64_t *idx_raw = nullptr;
    const int64_t nv = vector_index_list(u, &idx_raw);
    DevPtr<uint64_t> idx(idx_raw);
    if (nv == 0) {
        vector_release_storage(w);
        return;
    }
    const size_t usize = u->type->size;
    DevBuf<char> tmp(usize * (size_t)u->n, true);  // (w may be u)
    GRB_DISPATCH_SIZE(usize, U, hipLaunchKernelGGL((k_reverse_vector<U>), grid1d(nv), dim3(256), 0, ctx().stream, (const U *)u->d_val, (const uint64_t *)idx.p, nv,
                                                   (U *)tmp.p))
    vector_ensure_storage(w);
    cast_array(w->type->code, w->d_val, u->type->code, tmp.p, (int64_t)u->n);
    if (w != u) d2d(w->d_bits, u->d_bits, bits_words64(u->n) * sizeof(uint64_t));
    w->nvals = nv;
    ctx().stats.kernel_launches += 1;
    GRB_HIP(hipGetLastError());
    sync_stream();  // (`tmp` is released at the end of this scope)
}

void preload_sort() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_sort_long_lens)); (void)hipGetLastError(); }

}  // namespace grb

using namespace grb;

extern "C" GrB_Info GxB_Matrix_sort(GrB_Matrix C, GrB_Matrix P, GrB_BinaryOp op, const GrB_Matrix A, const GrB_Descriptor desc)
{
    GRB_TRY
    matrix_sort(C, P, op, A, desc);
    GRB_CATCH(errp(C) ? errp(C) : errp(P))
}
extern "C" GrB_Info GxB_Vector_sort(GrB_Vector w, GrB_Vector p, GrB_BinaryOp op, const GrB_Vector u, const GrB_Descriptor desc)
{
    GRB_TRY
    vector_sort(w, p, op, u, desc);
    GRB_CATCH(errp(w) ? errp(w) : errp(p))
}
extern "C" GrB_Info GrX_Matrix_reverse_rows(GrB_Matrix C, const GrB_Matrix A)
{
    GRB_TRY
    matrix_reverse_rows(C, A);
    GRB_CATCH(errp(C))
}
extern "C" GrB_Info GrX_Vector_reverse(GrB_Vector w, const GrB_Vector u)
{
    GRB_TRY
    vector_reverse(w, u);
    GRB_CATCH(errp(w))
}
extern "C" GrB_Info GrX_sort_limits(int64_t *wave_max, int64_t *lds_max)
{
    if (!wave_max || !lds_max) return GrB_NULL_POINTER;
    *wave_max = SORT_WAVE_MAX;
    *lds_max = SORT_LDS_MAX;
    return GrB_SUCCESS;
}
extern "C" GrB_Info GrX_sort_last(int64_t rows_by_path[3])
{
    if (!rows_by_path) return GrB_NULL_POINTER;
    for (int k = 0; k < 3; k++) rows_by_path[k] = g_sort_last[k];
    return GrB_SUCCESS;
}
