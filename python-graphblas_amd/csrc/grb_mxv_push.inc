// Part of grb_mxv.hip (included there, inside namespace grb): push-direction SpMSpV kernels
// ---------------------------------------------------------------------------------------------------
// push direction (SpMSpV): few entries in u.  T(j) = (+)_{k in u} mult(u_k, P(k,j)) where P's ROWS are indexed
// like u (P = A for vxm, A' for mxv).  The work -- all entries of the rows selected by u -- is cut into equal
// chunks over the prefix sum of those rows' lengths (hub rows in the frontier are shared by many threads);
// products land in a dense accumulator by native global atomics, restricted to positions the mask admits.
// ---------------------------------------------------------------------------------------------------
constexpr int PUSH_CHUNK = 8;  // consecutive work items per thread

__global__ void k_push_degrees(const uint64_t *idx, int64_t f, const int64_t *rowptr, int64_t *deg)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < f) {
        const int64_t k = (int64_t)idx[i];
        deg[i] = rowptr[k + 1] - rowptr[k];
    } else if (i == f) deg[i] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void k_push(const uint64_t *idx, int64_t f, const int64_t *pre /* f+1 */, int64_t work,
                                              const int64_t *rowptr, const int32_t *col, const T *aval, int a_iso,
                                              const T *u_val, int monoid, int mult, int need_a, int need_u,
                                              const uint64_t *m_bits, int has_mask, int m_comp,
                                              typename Widen<T>::type *t_val, unsigned long long *t_bits)
{
    using W = typename Widen<T>::type;
    const int64_t x0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PUSH_CHUNK;
    if (x0 >= work) return;
    // the frontier entry owning work item x0: last i with pre[i] <= x0
    int64_t lo = 0, hi = f;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (pre[mid] <= x0) lo = mid;
        else hi = mid;
    }
    int64_t i = lo;
    int64_t k = (int64_t)idx[i];
    int64_t next = pre[i + 1];
    int64_t p = rowptr[k] + (x0 - pre[i]);
    T uk = need_u ? u_val[k] : (T)0;
    const int64_t x1 = x0 + PUSH_CHUNK < work ? x0 + PUSH_CHUNK : work;
    for (int64_t x = x0; x < x1; x++) {
        while (x >= next) {  // move to the next frontier entry (rows of length 0 are skipped)
            i++;
            k = (int64_t)idx[i];
            next = pre[i + 1];
            p = rowptr[k];
            uk = need_u ? u_val[k] : (T)0;
        }
        const int j = col[p];
        bool ok = true;
        if (has_mask) {
            ok = (m_bits[j >> 6] >> (j & 63)) & 1ull;
            if (m_comp) ok = !ok;
        }
        if (ok) {
            const T av = need_a ? aval[a_iso ? 0 : p] : (T)0;
            const W prod = (W)apply_binop<T>(mult, uk, av);
            if (monoid == OP_ANY) t_val[j] = prod;
            else atomic_combine<W>(&t_val[j], prod, monoid);
            atomicOr(&t_bits[j >> 6], 1ull << (j & 63));
        }
        p++;
    }
}

template <typename W>
__global__ void k_fill_w(W *p, int64_t n, W v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---------------------------------------------------------------------------------------------------
// Thin frontiers (round 4): everything proportional to the WORK, nothing to the size of the vectors but one bitmap.
// ---------------------------------------------------------------------------------------------------
// The dense path above fills an accumulator of n values, casts it and runs the write rule over all n positions -- 0.17 ms for a
// frontier of THREE vertices at scale 22, behind three host round trips (entry count, frontier list, work).  Here:
//   k_push_frontier  one pass over the presence words of u: the frontier's positions appended to a list (any order: the monoids are
//                    commutative), its rows cut into chunks of 1024 entries appended to a work queue, fcount / work / chunks counted
//                    by atomics -- ONE host read decides push or pull and sizes nothing (the kernels below stride over the queue);
//   k_push_pass<0>   every admitted product stores the monoid's identity at its output position (all writers store the same value);
//   k_push_pass<1>   every admitted product goes to its position with one native atomic;
//   k_push_pass<2>   the first product to claim a position in a bitmap applies the write rule there: accum(w, t) or t.
// Entries of w that the rule deletes (replace outside the mask, no accumulator inside it) go by a pass over the presence WORDS
// (k_rows_tail's table).  A wavefront takes a chunk: hub rows in the frontier are shared by many wavefronts.  The operands may be
// in a matrix's vertex order (grb_mxv_order.inc): `in_map` turns a frontier position into the row of P, `out_map` a column of P
// into the output position -- a traversal that alternates push and pull never converts a vector.
constexpr int PUSH_Q = 1024;  // entries per work item
struct PushThin {
    const uint64_t *u_bits;
    int64_t n_in, n_out;
    const int32_t *in_map, *out_map;
    const int64_t *rowptr;
    const int32_t *col;
    const void *aval;
    int a_iso;
    const void *u_val;
    int monoid, mult, need_a, need_u;
    const uint64_t *m_bits;
    int has_mask, m_comp;
    uint32_t *f_list;
    int64_t f_cap;
    uint64_t *chunks;
    int64_t c_cap;
    unsigned long long *counters;  // [0] frontier entries, [1] work (entries of their rows), [2] chunks
    unsigned long long *counters_next;  // the next call's counters (the context keeps two sets): zeroed here, so that no call starts with a memset
    void *t_val;                   // n_out accumulators (widened semiring type): only marked positions are ever read
    unsigned long long *done_bits;
    // write rule
    void *w_val;
    unsigned long long *w_bits;
    int accum;
};

// exclusive prefix of v over the wavefront; *total = the wavefront's sum
__device__ __forceinline__ long long push_wave_excl(long long v, long long *total)
{
    long long inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const long long t = __shfl_up(inc, off);
        if ((int)(threadIdx.x & 63) >= off) inc += t;
    }
    *total = __shfl(inc, 63);
    return inc - v;
}
// (a thread per presence word; the three counters take ONE atomic per wavefront each: with one per frontier entry a frontier of 2 x 10^5
//  entries -- still "thin" at scale 24 -- spent 0.7 ms serialised on three addresses)
__global__ void k_push_frontier(const PushThin a)
{
    const int64_t wd = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (wd < 3) a.counters_next[wd] = 0ull;  // (last read by the host two calls ago)
    const uint64_t word = wd < ((a.n_in + 63) >> 6) ? a.u_bits[wd] : 0ull;
    if (__ballot(word != 0ull) == 0ull) return;  // (wave-uniform)
    // my entries: count, chunks and work
    long long my_cnt = __popcll(word), my_chunks = 0, my_work = 0;
    for (uint64_t bits = word; bits; bits &= bits - 1) {
        const int64_t pos = (wd << 6) + (__ffsll((long long)bits) - 1);
        const int64_t row = a.in_map ? (int64_t)a.in_map[pos] : pos;
        const int64_t len = a.rowptr[row + 1] - a.rowptr[row];
        my_work += len;
        my_chunks += (len + PUSH_Q - 1) / PUSH_Q;
    }
    long long tot_cnt, tot_chunks, tot_work;
    const long long off_cnt = push_wave_excl(my_cnt, &tot_cnt), off_chunks = push_wave_excl(my_chunks, &tot_chunks);
    (void)push_wave_excl(my_work, &tot_work);
    long long base_cnt = 0, base_chunks = 0;
    if (lane == 0) {
        base_cnt = (long long)atomicAdd(&a.counters[0], (unsigned long long)tot_cnt);
        base_chunks = (long long)atomicAdd(&a.counters[2], (unsigned long long)tot_chunks);
        atomicAdd(&a.counters[1], (unsigned long long)tot_work);
    }
    base_cnt = __shfl(base_cnt, 0);
    base_chunks = __shfl(base_chunks, 0);
    int64_t i = base_cnt + off_cnt, c0 = base_chunks + off_chunks;
    for (uint64_t bits = word; bits; bits &= bits - 1, i++) {
        if (i >= a.f_cap) break;  // (not thin after all: the host reads the count and takes another path)
        const int64_t pos = (wd << 6) + (__ffsll((long long)bits) - 1);
        a.f_list[i] = (uint32_t)pos;
        const int64_t row = a.in_map ? (int64_t)a.in_map[pos] : pos;
        const int64_t nch = (a.rowptr[row + 1] - a.rowptr[row] + PUSH_Q - 1) / PUSH_Q;
        for (int64_t c = 0; c < nch; c++, c0++)
            if (c0 < a.c_cap) a.chunks[c0] = ((uint64_t)i << 32) | (uint64_t)c;
    }
}

// one work item (a chunk of a frontier row) by the calling wavefront.  SMALL: the passes run inside ONE workgroup (k_push_small) --
// pass 0 also clears the word of the claim bitmap it will use (no memset of n / 8 bytes for three vertices), pass 2 reads what the
// atomics of pass 1 left in L2, not a line of its own L1.
template <typename T, int PASS, bool SMALL>
__device__ __forceinline__ void push_chunk(const PushThin &a, int64_t q, int lane)
{
    using W = typename Widen<T>::type;
    W *t_val = (W *)a.t_val;
    T *w_val = (T *)a.w_val;
    const uint64_t ch = a.chunks[q];
    const int64_t pos = (int64_t)a.f_list[ch >> 32];
    const int64_t row = a.in_map ? (int64_t)a.in_map[pos] : pos;
    const int64_t p0 = a.rowptr[row] + (int64_t)(uint32_t)ch * PUSH_Q;
    const int64_t pe = a.rowptr[row + 1], p1 = p0 + PUSH_Q < pe ? p0 + PUSH_Q : pe;
    const T uk = (PASS == 1 && a.need_u) ? ((const T *)a.u_val)[pos] : (T)0;
    for (int64_t p = p0 + lane; p < p1; p += 64) {
        const int64_t jc = a.col[p];
        const int64_t j = a.out_map ? (int64_t)a.out_map[jc] : jc;
        const unsigned long long bit = 1ull << (j & 63);
        if (a.has_mask) {
            bool ok = (a.m_bits[j >> 6] >> (j & 63)) & 1ull;
            if (a.m_comp) ok = !ok;
            if (!ok) continue;
        }
        if constexpr (PASS == 0) {
            t_val[j] = acc_seed<T, W>(a.monoid);
            if constexpr (SMALL) a.done_bits[j >> 6] = 0ull;  // (every writer of a word stores the same value)
        } else if constexpr (PASS == 1) {
            const T av = a.need_a ? ((const T *)a.aval)[a.a_iso ? 0 : p] : (T)0;
            const W prod = (W)apply_binop<T>(a.mult, uk, av);
            if (a.monoid == OP_ANY) t_val[j] = prod;
            else atomic_combine<W>(&t_val[j], prod, a.monoid);
        } else {
            const unsigned long long old = atomicOr(&a.done_bits[j >> 6], bit);
            if (old & bit) continue;  // (another product of this position applies the rule)
            W tw;
            unsigned long long wword;
            if constexpr (SMALL) {
                __atomic_load(&t_val[j], &tw, __ATOMIC_RELAXED);
                __atomic_load(&a.w_bits[j >> 6], &wword, __ATOMIC_RELAXED);
            } else {
                tw = t_val[j];
                wword = a.w_bits[j >> 6];
            }
            const T t = from_acc<T, W>(tw);
            const bool old_has = (wword >> (j & 63)) & 1ull;
            w_val[j] = (a.accum >= 0 && old_has) ? apply_binop<T>(a.accum, w_val[j], t) : t;
            if (!old_has) atomicOr(&a.w_bits[j >> 6], bit);
        }
    }
}

template <typename T, int PASS>
__global__ __launch_bounds__(256) void k_push_pass(const PushThin a, int64_t n_chunks)
{
    const int lane = threadIdx.x & 63;
    const int64_t wv0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwv = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t q = wv0; q < n_chunks; q += nwv) push_chunk<T, PASS, false>(a, q, lane);
}

// A handful of vertices (at most PUSH_SMALL_CHUNKS work items): the three passes as phases of ONE workgroup, the entries of w the write
// rule deletes taken from the frontier list when w IS the frontier (the level step q<!visited, replace> = q A) or skipped when w is
// known to be empty -- frontier kernel, one host read, this kernel.
constexpr int PUSH_SMALL_CHUNKS = 64, PUSH_SMALL_BLOCK = 1024;
template <typename T>
__global__ __launch_bounds__(PUSH_SMALL_BLOCK) void k_push_small(const PushThin a, int64_t n_chunks, int64_t fcount, int clear_frontier, int replace)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NWV = PUSH_SMALL_BLOCK / 64;
    for (int64_t q = wave; q < n_chunks; q += NWV) push_chunk<T, 0, true>(a, q, lane);
    __threadfence();
    __syncthreads();
    for (int64_t q = wave; q < n_chunks; q += NWV) push_chunk<T, 1, true>(a, q, lane);
    if (clear_frontier)  // k_push_words' table on the words that hold an entry of w (idempotent: a word may be visited by several entries)
        for (int64_t i = threadIdx.x; i < fcount; i += PUSH_SMALL_BLOCK) {
            const int64_t g = (int64_t)a.f_list[i] >> 6;
            const unsigned long long actw = a.has_mask ? (a.m_comp ? ~a.m_bits[g] : a.m_bits[g]) : ~0ull;
            const unsigned long long keep = a.accum >= 0 ? (replace ? actw : ~0ull) : (replace ? 0ull : ~actw);
            atomicAnd(&a.w_bits[g], keep);
        }
    __threadfence();
    __syncthreads();
    for (int64_t q = wave; q < n_chunks; q += NWV) push_chunk<T, 2, true>(a, q, lane);
}

// presence words of w before the products are applied: what the write rule deletes (see k_rows_tail: the same table, over all words)
__global__ void k_push_words(unsigned long long *w_bits, const uint64_t *m_bits, int has_mask, int m_comp, int accum, int replace, int64_t nwords)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nwords) return;
    const uint64_t actw = has_mask ? (m_comp ? ~m_bits[g] : m_bits[g]) : ~0ull;
    const uint64_t oldw = w_bits[g];
    w_bits[g] = accum >= 0 ? (replace ? (oldw & actw) : oldw) : (replace ? 0ull : (oldw & ~actw));
}
