// Part of grb_mxv.hip (included there, inside namespace grb): k_mxv_seams (tile seams of the merge-path kernel) and the general vector write rule
// One wavefront per tile whose first row began in earlier tiles: fold the carries of tiles
// [t_s, tile) with the tile's own first partial and apply the write rule for that row.
template <typename T, int TILE>
__global__ __launch_bounds__(PULL_BLOCK) void k_mxv_seams(const PullArgs a)
{
    using W = typename Widen<T>::type;
    const int lane = threadIdx.x & 63;
    const int64_t seam_blocks = (a.n_tiles + PULL_BLOCK / 64 - 1) / (PULL_BLOCK / 64);
    if ((int64_t)blockIdx.x >= seam_blocks) {  // the workgroups behind the seam ones: one thread per long row
        const int64_t slot = ((int64_t)blockIdx.x - seam_blocks) * PULL_BLOCK + threadIdx.x;
        if (slot < a.n_long_epi) long_row_write<T>(a, slot);
        return;
    }
    const int64_t tile = (int64_t)blockIdx.x * (PULL_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;  // wave-uniform
    const unsigned char flag = a.first_has[tile];
    if (!(flag & 2)) return;  // wave-uniform
    const int monoid = a.monoid;
    const int64_t row = a.tile_row[tile];
    const int64_t t_s = (row + a.rowptr[row]) / TILE;
    const W *cv = (const W *)a.carry_val;
    W acc = pull_seed<T, W>(a, monoid);
    int has = 0;
    for (int64_t t = t_s + lane; t < tile; t += 64) {
        if (a.carry_has[t]) {
            acc = has ? apply_binop<W>(monoid, acc, cv[t]) : cv[t];
            has = 1;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const W o = __shfl_down(acc, off);
        const int oh = __shfl_down(has, off);
        if (oh) {
            acc = has ? apply_binop<W>(monoid, acc, o) : o;
            has = 1;
        }
    }
    if (lane == 0) {
        if (flag & 1) {
            const W f = ((const W *)a.first_val)[tile];
            acc = has ? apply_binop<W>(monoid, acc, f) : f;
            has = 1;
        }
        bool mact = true;
        if (a.has_mask) {
            mact = (((const uint32_t *)a.m_bits)[row >> 5] >> (row & 31)) & 1u;
            if (a.m_comp) mact = !mact;
        }
        const bool old_has = (a.w_old_bits[row >> 6] >> (row & 63)) & 1ull;
        const T old_val = old_has ? ((const T *)a.w_old_val)[row] : (T)0;
        const bool new_has = write_rule_row<T>(a, row, mact, old_has, old_val, has != 0, from_acc<T, W>(acc));
        const unsigned long long bit = 1ull << (row & 63);
        if (new_has) atomicOr((unsigned long long *)&a.w_new_bits[row >> 6], bit);
        else atomicAnd((unsigned long long *)&a.w_new_bits[row >> 6], ~bit);
    }
}

// (monoid, PAIR) over a full operand: the product of a row is the fold of (row length) ones -- its length for PLUS, its parity
// for LXOR, 1 for every other monoid -- present iff the row has an entry.  One thread per row, the wavefront writes the row
// group's presence word; no entry of the matrix is read.
template <typename T>
__global__ void k_mxv_rowlen(const PullArgs a)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t g = row >> 6;
    bool new_has = false;
    if (row < a.m) {
        const int64_t len = a.rowptr[row + 1] - a.rowptr[row];
        bool mact = true;
        if (a.has_mask) {
            mact = (a.m_bits[g] >> lane) & 1ull;
            if (a.m_comp) mact = !mact;
        }
        const bool old_has = (a.w_old_bits[g] >> lane) & 1ull;
        T old_val = (T)0;
        if (old_has && (a.accum >= 0 || a.fresh)) old_val = ((const T *)a.w_old_val)[row];
        T t = (T)1;
        if (a.monoid == OP_PLUS) t = (T)len;
        else if (a.monoid == OP_LXOR) t = (T)(len & 1);
        new_has = write_rule_row<T>(a, row, mact, old_has, old_val, len > 0, t);
    }
    const unsigned long long nb = __ballot(new_has);
    if (lane == 0 && g < (a.m + 63) >> 6) a.w_new_bits[g] = nb;
}

// General (unfused) write rule: w<mask,replace> = accum(w, (TW) t), t of another type.
template <typename TW>
__global__ void k_vec_write(int64_t n, const TW *w_old_val, const uint64_t *w_old_bits, TW *w_new_val,
                            uint64_t *w_new_bits, const TW *t_val, const uint64_t *t_bits, const uint64_t *m_bits,
                            int has_mask, int m_comp, int accum, int replace, int fresh)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one wavefront = one presence word
    const int lane = threadIdx.x & 63;
    const int64_t g = row >> 6;
    const int64_t nwords = (n + 63) >> 6;
    bool new_has = false;
    if (row < n) {
        bool mact = true;
        if (has_mask) {
            mact = (m_bits[g] >> lane) & 1ull;
            if (m_comp) mact = !mact;
        }
        const bool old_has = (w_old_bits[g] >> lane) & 1ull;
        const bool t_has = (t_bits[g] >> lane) & 1ull;
        if (!mact) {
            new_has = replace ? false : old_has;
            if (new_has && fresh) w_new_val[row] = w_old_val[row];
        } else if (accum >= 0) {
            if (old_has && t_has) { w_new_val[row] = apply_binop<TW>(accum, w_old_val[row], t_val[row]); new_has = true; }
            else if (old_has) { if (fresh) w_new_val[row] = w_old_val[row]; new_has = true; }
            else if (t_has) { w_new_val[row] = t_val[row]; new_has = true; }
        } else if (t_has) { w_new_val[row] = t_val[row]; new_has = true; }
    }
    const unsigned long long nb = __ballot(new_has);
    if (lane == 0 && g < nwords) w_new_bits[g] = nb;
}

// w<m_bits (^comp), replace> = accum(w, t), in place, t of w's type
static void vector_write_rule(GB_Vector_opaque *w, const void *t_val, const uint64_t *t_bits, const uint64_t *m_bits, bool comp, int accum,
                              bool replace)
{
    GRB_DISPATCH_TYPE(w->type->code, TW, {
        const int64_t nthreads = (int64_t)bits_words64(w->n) * 64;
        hipLaunchKernelGGL((k_vec_write<TW>), dim3((unsigned)ceil_div(nthreads, 256)), dim3(256), 0, ctx().stream, (int64_t)w->n,
                           (const TW *)w->d_val, (const uint64_t *)w->d_bits, (TW *)w->d_val, w->d_bits, (const TW *)t_val, t_bits,
                           m_bits, m_bits ? 1 : 0, comp ? 1 : 0, accum, replace ? 1 : 0, 0);
    })
}

// the last step of every vector operation (DESIGN.md section 4.8)
void vector_finish(GB_Vector_opaque *w, const void *t_val, const uint64_t *t_bits, const uint64_t *m_bits, Desc f, const GB_BinaryOp_opaque *accum)
{
    vector_ensure_storage(w);
    vector_write_rule(w, t_val, t_bits, m_bits, f.comp, accum ? canonical_op(w->type->code, accum->op) : -1, f.replace);
    w->nvals = -1;
}
