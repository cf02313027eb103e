// grb_mxv_posn.hip -- GrB_mxv / GrB_vxm over a semiring whose multiply is POSITIONAL (GxB_FIRSTI .. GxB_SECONDJ1): the product reads
// indices, never values.  DESIGN.md section 4.13.  The BFS parent step  q<!parent, replace> = q' ANY.SECONDI A  is what it is for.
//
// z = mult(A(i,k), B(k,j)):  FIRSTI i   FIRSTJ k   SECONDI k   SECONDJ j,  the ...1 forms one more; int64 arithmetic, then the semiring's
// type (INT32 / INT64).  With u as the n x 1 column of mxv and the 1 x n row of vxm, per output o and inner index k:
//               FIRSTI   FIRSTJ   SECONDI   SECONDJ
//   mxv           o        k         k         0
//   vxm           0        k         k         o
// so every operator is one of OUTER (o), INNER (k), ZERO, plus an offset of 0 or 1 (pos_kind).  Monoids: MIN, MAX, ANY, PLUS.
//
// The kernels run on the plain CSR arrays (the pull layouts of grb_mxv.hip re-code the columns: the natural index is gone there), with
// the vectors in natural order, build T = dense values + presence words in the semiring's type and end in vector_finish.
//   pull  k_posn_pull over S (rows = outputs): a LANE GROUP of G = 4 / 8 / 16 / 64 lanes per row (G from the mean row length, the grid
//         from the row count alone), G consecutive columns per step, the operand's presence bit, one __ballot.  Column lists are sorted:
//         INNER under MIN / ANY ends at the first set lane, under MAX the row is walked from its end; OUTER / ZERO under MIN / MAX / ANY
//         only ask whether the intersection is empty (the same early exit); PLUS reads the whole row (popcounts; INNER: a group
//         reduction).  Rows the mask does not admit are skipped before any load; a full operand skips the bit tests.
//   push  k_posn_push over P (rows = inner indices), from the list of u's entries: ENTRY-parallel over the concatenated rows of the
//         frontier (a scan of their lengths, one search per 64 entries: walk_first_row / walk_block_rows), so a hub row is spread over
//         many wavefronts.  An admitted entry combines into t[j] by one atomic (MIN / MAX / PLUS) or a plain store (ANY: every writer
//         stores a valid answer) and sets the presence bit by atomicOr.
// Direction: the push_mode option with the numbers it has for the other semirings (0 never; 1 when u has fewer than n/64 entries and
// its rows' entries x 128 <= nnz; 2 whenever P is at hand); a transpose that is not cached is never built for a push.
// GrX_last_stats: method 25 pull, 26 push, 6 an operand without entries; tiles = wavefront units; flops = nnz(S) / the frontier's entries.
#include <algorithm>

#include "grb_index_ops.hpp"

namespace grb {

enum PosKind : int { PK_OUTER = 0, PK_INNER = 1, PK_ZERO = 2 };

static int pos_kind(int mult, bool vxm)
{
    switch ((mult - POS_FIRSTI) >> 1) {
    case 0: return vxm ? PK_ZERO : PK_OUTER;   // FIRSTI: the row of the first operand
    case 3: return vxm ? PK_OUTER : PK_ZERO;   // SECONDJ: the column of the second operand
    default: return PK_INNER;                  // FIRSTJ, SECONDI
    }
}

template <typename TS>
__global__ void k_posn_fill(TS *__restrict__ t, int64_t n, TS v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[i] = v;
}

__global__ void k_posn_degrees(const uint64_t *__restrict__ idx, int64_t f, const int64_t *__restrict__ rowptr, int64_t *__restrict__ deg)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < f) {
        const int64_t k = (int64_t)idx[i];
        deg[i] = rowptr[k + 1] - rowptr[k];
    } else if (i == f) deg[i] = 0;
}

// ---- pull: a group of G lanes per row of S; every lane of the wavefront runs every step (the ballots are wave-wide) -------------------
template <typename TS, int G>
__global__ void __launch_bounds__(256) k_posn_pull(const int64_t *__restrict__ Sp, const int32_t *__restrict__ Sj, int64_t m,
                                                   const uint64_t *__restrict__ u_bits /* nullptr: u is full */, const uint64_t *__restrict__ m_bits,
                                                   int m_comp, int mon, int kind, int off, TS *__restrict__ t_val, unsigned long long *__restrict__ t_bits)
{
    constexpr int RPW = 64 / G;  // rows of a wavefront
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t row = wave * RPW + lane / G;
    bool active = row < m;
    if (active && m_bits) active = (int)((m_bits[row >> 6] >> (row & 63)) & 1) != m_comp;  // (pruning only: the write rule decides)
    int64_t start = 0, end = 0;
    if (active) {
        start = Sp[row];
        end = Sp[row + 1];
        active = end > start;
    }
    const bool sum = mon == OP_PLUS;
    const bool back = mon == OP_MAX && kind == PK_INNER;  // the largest column first
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1);
    int64_t acc = 0;     // PLUS over INNER: this lane's share of the sum of the columns
    int64_t cnt = 0;     // PLUS: entries of the intersection so far (the same in every lane of the group)
    int64_t found = -1;  // MIN / MAX / ANY: the column the row ended at
    for (int64_t c = 0; __any(active); c += G) {
        const int64_t e = back ? end - 1 - c - gl : start + c + gl;
        const bool valid = active && (back ? e >= start : e < end);
        const int32_t col = valid ? Sj[e] : -1;
        const bool hit = valid && (!u_bits || ((u_bits[col >> 6] >> (col & 63)) & 1));
        const unsigned long long gb = (__ballot(hit) >> gbase) & gmask;
        const int32_t first_col = __shfl(col, gbase + (gb ? __ffsll(gb) - 1 : 0));
        if (active) {
            if (sum) {
                cnt += __popcll(gb);
                if (hit) acc += col;
            } else if (gb) {
                found = first_col;
                active = false;
            }
            if (c + G >= end - start) active = false;
        }
    }
    if (sum && kind == PK_INNER) {
#pragma unroll
        for (int s = G >> 1; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
    }
    const bool has = sum ? cnt > 0 : found >= 0;
    if (gl == 0 && has) {
        const int64_t o = kind == PK_OUTER ? row + off : (int64_t)off;
        int64_t z;
        if (sum) z = kind == PK_INNER ? (int64_t)((uint64_t)acc + (uint64_t)cnt * (uint64_t)off) : (int64_t)((uint64_t)cnt * (uint64_t)o);
        else z = kind == PK_INNER ? found + off : o;
        t_val[row] = cast_value<TS, int64_t>(z);
        atomicOr(&t_bits[row >> 6], 1ull << (row & 63));
    }
}

// ---- push: entry-parallel over the concatenated rows of the frontier (pre = the exclusive scan of their lengths, pre[fcount] = work) ----
template <typename TS>
__global__ void __launch_bounds__(256) k_posn_push(const uint64_t *__restrict__ idx, int64_t fcount, const int64_t *__restrict__ pre, int64_t work,
                                                   int64_t nblocks, const int64_t *__restrict__ Pp, const int32_t *__restrict__ Pj,
                                                   const uint64_t *__restrict__ m_bits, int m_comp, int mon, int kind, int off, TS *t_val,
                                                   unsigned long long *t_bits)
{
    __shared__ int64_t s_end[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * SEL_BPW;
    const int64_t b1 = b0 + SEL_BPW < nblocks ? b0 + SEL_BPW : nblocks;
    int64_t r = 0;  // (wave-uniform) the frontier position of the first entry of the current block
    if (b0 < b1) r = walk_first_row(pre, fcount, b0 << 6);
    for (int64_t b = b0; b < b1; b++) {
        const int64_t p = b << 6, e = p + lane;
        const int64_t fpos = walk_block_rows(pre, fcount, work, p, lane, s_end[wave], r);
        if (e < work) {
            const int64_t k = (int64_t)idx[fpos];
            const int64_t j = (int64_t)Pj[Pp[k] + (e - pre[fpos])];
            if (!m_bits || (int)((m_bits[j >> 6] >> (j & 63)) & 1) != m_comp) {
                const int64_t z = kind == PK_INNER ? k + off : (kind == PK_OUTER ? j + off : (int64_t)off);
                const TS v = cast_value<TS, int64_t>(z);
                if (mon == OP_ANY) t_val[j] = v;
                else atomic_combine<TS>(&t_val[j], v, mon);
                const unsigned long long bit = 1ull << (j & 63);
                if (!(t_bits[j >> 6] & bit)) atomicOr(&t_bits[j >> 6], bit);  // (a bit only ever goes from 0 to 1: a stale 0 costs one more atomic)
            }
        }
    }
}

template <typename TS>
static int64_t launch_posn_pull(GB_Matrix_opaque *S, const uint64_t *u_bits, const uint64_t *m_bits, bool comp, int mon, int kind, int off, void *t_val,
                                uint64_t *t_bits)
{
    const int64_t m = (int64_t)S->nrows;
    const int64_t mean = S->nvals / m;  // (m > 0: checked by the caller)
    const int G = mean <= 4 ? 4 : (mean <= 8 ? 8 : (mean <= 16 ? 16 : 64));
    const int64_t waves = ceil_div(m, 64 / G), wgs = ceil_div(waves, 4);
    if (wgs > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
#define POSN_PULL(GW)                                                                                                                      \
    hipLaunchKernelGGL((k_posn_pull<TS, GW>), dim3((unsigned)wgs), dim3(256), 0, ctx().stream, matrix_rowptr(S), (const int32_t *)S->d_col, m, u_bits, \
                       m_bits, comp ? 1 : 0, mon, kind, off, (TS *)t_val, (unsigned long long *)t_bits)
    switch (G) {
    case 4: POSN_PULL(4); break;
    case 8: POSN_PULL(8); break;
    case 16: POSN_PULL(16); break;
    default: POSN_PULL(64); break;
    }
#undef POSN_PULL
    return waves;
}

template <typename TS>
static TS posn_identity(int mon)
{
    return mon == OP_MIN ? type_max<TS>() : (mon == OP_MAX ? type_lowest<TS>() : (TS)0);
}

void mxv_positional(GB_Vector_opaque *w, GB_Vector_opaque *mask, const GB_BinaryOp_opaque *accum, const GB_Semiring_opaque *sr,
                    GB_Matrix_opaque *A, GB_Vector_opaque *u, bool vxm, Desc f)
{
    check_vector(w, "w");
    if (mask) check_vector(mask, "mask");
    check_vector(u, "u");
    // the matrix as multiplied: M = A, or A' under T0 (mxv) / T1 (vxm).  mxv pulls over M and pushes over M', vxm the other way round
    const bool tr = vxm ? f.t1 : f.t0;
    const uint64_t m_rows = tr ? A->ncols : A->nrows, m_cols = tr ? A->nrows : A->ncols;
    const uint64_t n_inner = vxm ? m_rows : m_cols, n_outer = vxm ? m_cols : m_rows;
    check_mxv_sizes(n_inner, n_outer, w, mask, accum, u);
    ctx().stats = GrX_Stats{};
    ctx().stats.method = 25;
    ctx().stats.long_kernel = -1;
    ctx().stats.cold_tile_mode = -1;
    ctx().stats.flops = A->nvals;
    ctx().stats.out_nvals = -1;
    const int64_t n_out = (int64_t)w->n;
    if (n_out == 0) return;
    if (vector_writes_nothing(w, mask, f)) return;
    const int st = sr->type;
    if (!op_is_positional(sr->mult) || (st != TC_INT32 && st != TC_INT64)) fail(GrB_PANIC, "mxv/vxm: not a positional semiring (internal error)");
    const int mon = canonical_op(st, sr->monoid);
    if (mon != OP_MIN && mon != OP_MAX && mon != OP_ANY && mon != OP_PLUS)
        fail(GrB_NOT_IMPLEMENTED, std::string("mxv/vxm: the positional operator ") + pos_op_name(sr->mult) + " is implemented under the MIN, MAX, ANY and PLUS monoids only");
    if (accum) (void)canonical_op(w->type->code, accum->op);  // (an accumulator without a kernel is rejected before the short cut below)
    const int kind = pos_kind(sr->mult, vxm), off = (sr->mult - POS_FIRSTI) & 1;
    DevPtr<uint64_t> m_hold;
    const uint64_t *m_bits = vector_mask_words(mask, w, f.structure, m_hold);

    // ---- an operand without entries: T is empty, only the write rule remains ----
    const int64_t nv = vector_nvals(u);
    if (A->nvals == 0 || nv == 0) {
        ctx().stats.method = 6;
        if (w->nvals == 0) return;
        if (!mask && !accum) {
            vector_release_storage(w);
            return;
        }
        vector_ensure_storage(w);
        DevBuf<uint64_t> t_bits(bits_words64(w->n), true);
        vector_finish(w, w->d_val, t_bits.p, m_bits, f, accum);
        ctx().stats.kernel_launches += 1;
        if (ctx().blocking) sync_stream();
        return;
    }

    // ---- direction ----
    GB_Matrix_opaque *P = vxm ? (tr ? A->tr : A) : (tr ? A : A->tr);  // rows indexed like u; nullptr: a transpose that is not cached
    bool push = false;
    int64_t work = 0, fcount = 0;
    DevPtr<uint64_t> idx;
    DevPtr<int64_t> pre;
    if (P && ctx().push_mode != 0 && (ctx().push_mode == 2 || nv * 64 < (int64_t)u->n)) {
        uint64_t *d_idx = nullptr;
        fcount = vector_index_list(u, &d_idx);
        idx.reset(d_idx);
        pre.reset((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(fcount + 1)));
        hipLaunchKernelGGL(k_posn_degrees, grid1d(fcount + 1), dim3(256), 0, ctx().stream, (const uint64_t *)idx.get(), fcount, matrix_rowptr(P), pre.get());
        prim_exclusive_sum_i64(pre.get(), pre.get(), fcount + 1);
        d2h(&work, pre.get() + fcount, sizeof(int64_t));
        ctx().stats.kernel_launches += 4;
        push = ctx().push_mode == 2 || work * 128 <= P->nvals;
    }

    // ---- T: dense values + presence in the semiring's type ----
    DevBuf<char> t_val((size_t)n_out * type_size(st));
    DevBuf<uint64_t> t_bits(bits_words64((uint64_t)n_out), true);
    if (push) {
        ctx().stats.method = 26;
        ctx().stats.flops = work;
        if (work > 0) {
            const int64_t nblocks = ceil_div(work, 64), units = ceil_div(nblocks, SEL_BPW), wgs = ceil_div(units, 4);
            if (wgs > 0x7fffffff) fail(GrB_NOT_IMPLEMENTED, "problem too large for one launch");
            if (st == TC_INT32) {
                hipLaunchKernelGGL((k_posn_fill<int32_t>), grid1d(n_out), dim3(256), 0, ctx().stream, (int32_t *)t_val.p, n_out, posn_identity<int32_t>(mon));
                hipLaunchKernelGGL((k_posn_push<int32_t>), dim3((unsigned)wgs), dim3(256), 0, ctx().stream, (const uint64_t *)idx.get(), fcount, (const int64_t *)pre.get(), work,
                                   nblocks, matrix_rowptr(P), (const int32_t *)P->d_col, m_bits, f.comp ? 1 : 0, mon, kind, off, (int32_t *)t_val.p, (unsigned long long *)t_bits.p);
            } else {
                hipLaunchKernelGGL((k_posn_fill<int64_t>), grid1d(n_out), dim3(256), 0, ctx().stream, (int64_t *)t_val.p, n_out, posn_identity<int64_t>(mon));
                hipLaunchKernelGGL((k_posn_push<int64_t>), dim3((unsigned)wgs), dim3(256), 0, ctx().stream, (const uint64_t *)idx.get(), fcount, (const int64_t *)pre.get(), work,
                                   nblocks, matrix_rowptr(P), (const int32_t *)P->d_col, m_bits, f.comp ? 1 : 0, mon, kind, off, (int64_t *)t_val.p, (unsigned long long *)t_bits.p);
            }
            ctx().stats.kernel_launches += 2;
            ctx().stats.tiles = units;
        }
    } else {
        GB_Matrix_opaque *S = vxm ? (tr ? A : matrix_transpose_cached(A)) : (tr ? matrix_transpose_cached(A) : A);  // rows = outputs
        const uint64_t *u_bits = nv == (int64_t)u->n ? nullptr : (const uint64_t *)u->d_bits;
        const int64_t waves = st == TC_INT32 ? launch_posn_pull<int32_t>(S, u_bits, m_bits, f.comp, mon, kind, off, t_val.p, t_bits.p)
                                             : launch_posn_pull<int64_t>(S, u_bits, m_bits, f.comp, mon, kind, off, t_val.p, t_bits.p);
        ctx().stats.method = 25;
        ctx().stats.flops = S->nvals;
        ctx().stats.kernel_launches += 1;
        ctx().stats.tiles = waves;
    }

    // ---- T in w's type, then the write rule (in place on w; u == w is safe: u was read above, in stream order) ----
    DevPtr<char> t_hold;
    const void *tw = vector_values_as(t_val.p, st, w->type->code, n_out, t_hold);
    vector_finish(w, tw, t_bits.p, m_bits, f, accum);
    ctx().stats.kernel_launches += tw == t_val.p ? 1 : 2;  // (the write rule, and the cast in front of it)
    GRB_HIP(hipGetLastError());
    if (ctx().blocking) sync_stream();
}

void preload_mxv_posn() { hipFuncAttributes at; (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_posn_degrees)); (void)hipGetLastError(); }

}  // namespace grb
