// grb_mxm_write.inc -- the GraphBLAS write rule  C<M, replace> = accum(C, T)  on sorted CSR rows, a WAVEFRONT per unit
// (part of grb_mxm.hip).
//
// Reference: the write rule every masked / accumulated call ends with -- graphblas/core/matrix.py:2264-2331 builds the
// expression, core/base.py:192-263 (`Updater`) carries mask / accum / replace into the C call; the C API 2.0 section 3.5.4
// semantics are restated by oracle/grb_oracle.c (grbo_mat_write).
//
// Round 1-2 walked the three sorted lists (C_old(i,:), T(i,:), M(i,:)) entry by entry with one THREAD per row, twice (count,
// fill): the rows of a product hold 10^4 entries on average and 10^5..10^6 in the hub rows, so the call ended on a handful of
// threads -- 1.6 s of a 1.77 s call at R-MAT scale 20 (9.7 G entries in T).  Here
//   * a unit is a row, or -- for rows with more than WR_LONG entries in C_old and T together -- a (row, column piece) pair: the
//     pieces of a row are found by 64-ary searches of the piece's first column in the three lists, so a hub row is merged by up
//     to 256 wavefronts side by side;
//   * a wavefront merges 64 entries of each list per step: lane l loads entry l of the next chunk of C_old, T and M; the step's
//     BOUND is the smallest last-loaded column over the lists that still have unloaded entries -- every loaded entry up to the
//     bound is final (nothing unloaded can be smaller); each T entry finds its partner in the C chunk and its mask entry in the M
//     chunk by a 6-step search in LDS, each C entry its partner in the T chunk; the output position of an emitted entry is the
//     number of emitted entries of its own list before it plus the emitted C-only (resp. T) entries below its column -- two
//     popcounts of ballots;
//   * counts per unit -> one scan -> the same walk writes.
#pragma once

constexpr int64_t WR_LONG = 8192;  // entries of C_old(i,:) + T(i,:) above which a row is cut into column pieces
constexpr int WR_MAX_PIECES = 256;

struct WriteArgs {
    int64_t m;
    const int64_t *Cp;
    const int32_t *Cj;
    const void *Cx;
    int c_iso;
    const int64_t *Tp;
    const int32_t *Tj;
    const void *Tx;
    const int64_t *Mp;
    const int32_t *Mj;
    const void *Mx;
    int m_type, m_iso, has_mask, m_struct, m_comp, accum, replace;
    // units
    const int64_t *ubase;  // first unit of every row (m + 1)
    const int32_t *urow;   // the row of every unit
    int64_t n_units;
    int piece_cols;        // columns per piece of a cut row
    int64_t *ucount;       // count pass: entries the unit emits
    const int64_t *uoff;   // fill pass: where the unit writes
    int32_t *Nj;
    void *Nx;
};

// units per row: 0 for a row with nothing in C_old and T, `pieces` for a long one, else 1
__global__ void k_write_units_per_row(const int64_t *Cp, const int64_t *Tp, int64_t m, int pieces, int64_t *upr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    if (i == m) { upr[i] = 0; return; }
    const int64_t len = (Cp ? Cp[i + 1] - Cp[i] : 0) + (Tp[i + 1] - Tp[i]);
    upr[i] = len == 0 ? 0 : (len > WR_LONG ? pieces : 1);
}
__global__ void k_write_unit_rows(const int64_t *ubase, int64_t m, int32_t *urow)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    for (int64_t u = ubase[i]; u < ubase[i + 1]; u++) urow[u] = (int32_t)i;
}
__global__ void k_write_rowptr(const int64_t *ubase, const int64_t *uoff, int64_t m, int64_t *Np)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= m) Np[i] = uoff[ubase[i]];
}

// The unit table of a merge of two sorted lists per row (the write rule: C_old and T; eWise: A and B), shared by both kernels
struct UnitTable {
    DevPtr<int64_t> ubase;  // first unit of every row (m + 1)
    DevPtr<int32_t> urow;   // the row of every unit (nullptr without units)
    int64_t n_units = 0;
    int piece_cols = 0;     // columns per piece of a cut row
    dim3 grid() const { return dim3((unsigned)ceil_div(n_units, 4)); }  // a wavefront per unit, four to a workgroup
};
// units of the m rows of the lists with row pointers Xp (nullptr: an empty list) and Yp over `ncols` columns: two launches, three
// when there are units (the callers count them)
static UnitTable unit_table(const int64_t *Xp, const int64_t *Yp, int64_t m, int64_t ncols)
{
    UnitTable ut;
    const int pieces = (int)std::min<int64_t>(WR_MAX_PIECES, std::max<int64_t>(1, ceil_div(ncols, (int64_t)16384)));
    ut.piece_cols = (int)std::min<int64_t>(0x7fffffff, ceil_div(ncols, (int64_t)pieces));
    ut.ubase.reset((int64_t *)dev_alloc(sizeof(int64_t) * (size_t)(m + 1)));
    hipLaunchKernelGGL(k_write_units_per_row, dim3((unsigned)ceil_div(m + 1, 256)), dim3(256), 0, ctx().stream, Xp, Yp, m, pieces, ut.ubase.p);
    prim_exclusive_sum_i64(ut.ubase.p, ut.ubase.p, m + 1);
    d2h(&ut.n_units, ut.ubase.p + m, sizeof(int64_t));
    if (ut.n_units > 0) {
        ut.urow.reset((int32_t *)dev_alloc(sizeof(int32_t) * (size_t)ut.n_units));
        hipLaunchKernelGGL(k_write_unit_rows, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, ctx().stream, (const int64_t *)ut.ubase.p, m, ut.urow.p);
    }
    return ut;
}
// Np[i] = where row i's first unit writes: uoff = the exclusive sum of the units' counts
static void unit_table_rowptr(const UnitTable &ut, const int64_t *uoff, int64_t m, int64_t *Np)
{
    hipLaunchKernelGGL(k_write_rowptr, dim3((unsigned)ceil_div(m + 1, 256)), dim3(256), 0, ctx().stream, (const int64_t *)ut.ubase.p, uoff, m, Np);
}

// first position p in [lo, hi) with a[p] >= key (hi if none), searched by the whole wavefront: 64 probes per round trip
__device__ __forceinline__ int64_t wave_lower_bound(const int32_t *a, int64_t lo, int64_t hi, int key, int lane)
{
    while (hi - lo > 64) {
        const int64_t step = (hi - lo + 63) >> 6;
        const int64_t p = lo + (int64_t)lane * step;
        const bool below = p < hi && a[p] < key;
        const int k = __popcll(__ballot(below));  // (sorted: the first k probes are below the key)
        if (k == 0) return lo;
        const int64_t nlo = lo + (int64_t)(k - 1) * step + 1, nhi = lo + (int64_t)k * step;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    const int64_t p = lo + lane;
    return lo + __popcll(__ballot(p < hi && a[p] < key));
}

__device__ __forceinline__ bool mask_entry_true(const void *Mx, int m_type, int m_iso, int64_t p)
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

// number of the 64 sorted values of `s` that are below `key` (padding = INT_MAX, never below a valid column)
__device__ __forceinline__ int chunk_lower_bound(const int *s, int key)
{
    int lo = 0;
#pragma unroll
    for (int st = 32; st > 0; st >>= 1)
        if (s[lo + st - 1] < key) lo += st;
    return lo + (lo < 64 && s[lo] < key ? 1 : 0);  // (lo <= 63 here: the last step settles entry 63)
}

__device__ __forceinline__ unsigned long long bits_below(int x) { return x >= 64 ? ~0ull : ((1ull << x) - 1ull); }

template <typename T, bool FILL>
__global__ __launch_bounds__(256) void k_mat_write_wave(const WriteArgs a)
{
    constexpr int COL_END = 0x7fffffff;
    __shared__ int s_c[4][64], s_t[4][64], s_m[4][64];
    __shared__ T s_cv[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t unit = (int64_t)blockIdx.x * 4 + wv;
    if (unit >= a.n_units) return;  // (uniform over the wavefront)
    const int64_t row = a.urow[unit];
    const int64_t u0 = a.ubase[row], pieces = a.ubase[row + 1] - u0;
    int64_t pc = a.Cp ? a.Cp[row] : 0, ec = a.Cp ? a.Cp[row + 1] : 0, pt = a.Tp[row], et = a.Tp[row + 1];
    int64_t pm = a.has_mask ? a.Mp[row] : 0, em = a.has_mask ? a.Mp[row + 1] : 0;
    if (pieces > 1) {  // this wavefront's column piece of a long row
        const int64_t piece = unit - u0;
        const int64_t c_lo = piece * a.piece_cols, c_hi = c_lo + a.piece_cols;
        const int k_lo = (int)c_lo, k_hi = (piece == pieces - 1 || c_hi >= COL_END) ? COL_END : (int)c_hi;
        pc = wave_lower_bound(a.Cj, pc, ec, k_lo, lane);
        ec = wave_lower_bound(a.Cj, pc, ec, k_hi, lane);
        pt = wave_lower_bound(a.Tj, pt, et, k_lo, lane);
        et = wave_lower_bound(a.Tj, pt, et, k_hi, lane);
        if (a.has_mask) {
            pm = wave_lower_bound(a.Mj, pm, em, k_lo, lane);
            em = wave_lower_bound(a.Mj, pm, em, k_hi, lane);
        }
    }
    const T *Cx = (const T *)a.Cx, *Tx = (const T *)a.Tx;
    T *Nx = (T *)a.Nx;
    int *sc = s_c[wv], *st = s_t[wv], *sm = s_m[wv];
    T *scv = s_cv[wv];
    const int accum = a.accum;
    const bool keep_old = !a.replace;
    int64_t out = FILL ? a.uoff[unit] : 0, cnt = 0;
    while (pc < ec || pt < et) {
        // ---- the next chunk of every list
        const bool c_in = pc + lane < ec, t_in = pt + lane < et, m_in = pm + lane < em;
        const int cj = c_in ? a.Cj[pc + lane] : COL_END, tj = t_in ? a.Tj[pt + lane] : COL_END;
        const int mj = m_in ? a.Mj[pm + lane] : COL_END;
        T cv = (T)0, tv = (T)0;
        if (FILL && c_in) cv = Cx[a.c_iso ? 0 : pc + lane];
        if (FILL && t_in) tv = Tx[pt + lane];
        bool m_true = m_in;
        if (m_in && !a.m_struct) m_true = mask_entry_true(a.Mx, a.m_type, a.m_iso, pm + lane);
        sc[lane] = cj;
        st[lane] = tj;
        sm[lane] = m_true ? mj : (m_in ? -1 - mj : COL_END);  // (a false mask entry keeps its place in the order under a negative code)
        scv[lane] = cv;
        // the step's bound: the smallest last-loaded column over the lists with entries still unloaded
        // (v_readlane, not __shfl: a ds_bpermute is a round trip through the LDS pipeline in the middle of the step's dependent chain)
        const int last_c = ec - pc > 64 ? __builtin_amdgcn_readlane(cj, 63) : COL_END, last_t = et - pt > 64 ? __builtin_amdgcn_readlane(tj, 63) : COL_END;
        const int last_m = em - pm > 64 ? __builtin_amdgcn_readlane(mj, 63) : COL_END;
        int bound = last_c < last_t ? last_c : last_t;
        bound = last_m < bound ? last_m : bound;
        mw_sync();
        const bool use_c = c_in && cj <= bound, use_t = t_in && tj <= bound;
        // ---- T entries: partner in the C chunk, mask entry in the M chunk
        bool emit_t = false, emit_c = false;
        T zt = (T)0, zc = (T)0;
        int lb_c = 0, lb_t = 0;
        auto mask_allows = [&](int j) {
            if (!a.has_mask) return true;
            // the mask chunk holds |code| in column order: search by column, then look at the sign
            int lo = 0;
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const int v = sm[lo + s - 1];
                if ((v < 0 ? -1 - v : v) < j) lo += s;
            }
            if (lo < 64) {
                const int v = sm[lo];
                if ((v < 0 ? -1 - v : v) < j) lo++;
            }
            bool mk = false;
            if (lo < 64) mk = sm[lo] == j;  // (present and true; a false entry holds -1 - j)
            return a.m_comp ? !mk : mk;
        };
        if (use_t) {
            lb_c = chunk_lower_bound(sc, tj);
            const bool hc = lb_c < 64 && sc[lb_c] == tj;
            if (mask_allows(tj)) {
                emit_t = true;
                if (FILL) zt = (accum >= 0 && hc) ? apply_binop<T>(accum, scv[lb_c], tv) : tv;
            } else if (keep_old && hc) {
                emit_t = true;
                if (FILL) zt = scv[lb_c];
            }
        }
        // ---- C entries without a partner in T
        if (use_c) {
            lb_t = chunk_lower_bound(st, cj);
            const bool ht = lb_t < 64 && st[lb_t] == cj;
            if (!ht) {
                emit_c = mask_allows(cj) ? accum >= 0 : keep_old;
                zc = cv;
            }
        }
        const unsigned long long e_t = __ballot(emit_t), e_c = __ballot(emit_c);
        if (FILL) {
            const unsigned long long mine = bits_below(lane);
            if (emit_t) {
                const int64_t o = out + cnt + __popcll(e_t & mine) + __popcll(e_c & bits_below(lb_c));
                a.Nj[o] = tj;
                Nx[o] = zt;
            }
            if (emit_c) {
                const int64_t o = out + cnt + __popcll(e_c & mine) + __popcll(e_t & bits_below(lb_t));
                a.Nj[o] = cj;
                Nx[o] = zc;
            }
        }
        cnt += __popcll(e_t) + __popcll(e_c);
        pc += __popcll(__ballot(use_c));
        pt += __popcll(__ballot(use_t));
        pm += __popcll(__ballot(m_in && mj <= bound));
        mw_sync();
    }
    if (!FILL && lane == 0) a.ucount[unit] = cnt;
}
