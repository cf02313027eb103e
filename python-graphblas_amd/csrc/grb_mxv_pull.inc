// Part of grb_mxv.hip (included there, inside namespace grb): k_mxv_pull -- merge-path pull SpMV tiles (matrices without the long/short row split)
// BOOL operand whose presence and value share a word (PullArgs::u_pv): xp / xv of N codes from one gather each; a code of
// -1 (nothing to gather) is out of range and reads 0 = absent
template <int N>
__device__ __forceinline__ void bool_pv_gather(__amdgpu_buffer_rsrc_t pv_rs, const int (&cc)[N], bool (&xp)[N], bool (&xv)[N])
{
    uint32_t pw[N];
#pragma unroll
    for (int i = 0; i < N; i++) pw[i] = buf_load<uint32_t>(pv_rs, (unsigned)(cc[i] >> 4) * 4u);
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int sh = (cc[i] & 15) * 2;
        xp[i] = (pw[i] >> sh) & 1u;
        xv[i] = (pw[i] >> (sh + 1)) & 1u;
    }
}

template <typename T, int MONOID_CT, int MULT_CT, int IPT>
__global__ __launch_bounds__(PULL_BLOCK) void k_mxv_pull(const PullArgs a)
{
    using W = typename Widen<T>::type;
    constexpr int TILE = PULL_BLOCK * IPT;
    static_assert(IPT % 4 == 0, "IPT must be a multiple of 4 (16-byte loads)");
    // LDS holds only per-ROW state (row-start marks, row accumulators): the tile's column indices and values
    // go straight from HBM into the registers of the thread that consumes them (IPT consecutive entries).
    __shared__ __attribute__((aligned(16))) unsigned short s_head[TILE + 8];
    // (+64: per-lane scratch slots that absorb the "nothing to emit" case of the branch-free fold)
    __shared__ W s_tval[TILE + 1 + 64];
    __shared__ unsigned char s_thas[TILE + 1 + 64];
    __shared__ unsigned int s_act[TILE / 32 + 3];
    __shared__ int s_any;
    __shared__ int s_wave_last[PULL_BLOCK / 64];

    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const T *aval = (const T *)a.aval;
    const bool need_aval = a.need_aval != 0, need_uval = a.need_uval != 0;
    const bool has_mask = a.has_mask != 0;
    const bool stage_vals = need_aval && !a.a_iso;
    const bool need_old = (a.accum >= 0) || a.fresh;
    PHASE_STAMP(0);

    // ---- tile coordinates -------------------------------------------------------------------------------------
    const int64_t i0 = a.tile_row[tile], i1 = a.tile_row[tile + 1];
    const int64_t total = a.m + a.nnz;
    const int64_t d0 = tile * (int64_t)TILE;
    const int64_t d1 = d0 + TILE < total ? d0 + TILE : total;
    const int64_t j0 = d0 - i0;
    const int nrows_t = (int)(i1 - i0);  // rows whose end falls inside this tile (slot nrows_t = the row still open)
    const int nnz_t = (int)((d1 - i1) - j0);
    const int base = tid * IPT;  // my IPT consecutive entries of the tile
    EARLY_EXIT(1);

    // ---- issue every HBM load of the tile now: my entries (16-byte buffer loads; the descriptor ends at the
    //      end of the arrays, out-of-range parts read 0), my row's bounds, mask word, old w of my first rows ----
    const int64_t left = a.nnz - j0;
    const __amdgpu_buffer_rsrc_t crs = make_rsrc(a.col + j0, left * 4);
    const __amdgpu_buffer_rsrc_t vrs = make_rsrc(aval + (a.a_iso ? 0 : j0), stage_vals ? left * (int64_t)sizeof(T) : 0);
    const bool whole = left >= TILE + 4;  // 16-byte loads never straddle the end of the arrays
    int creg[IPT];
    T vreg[IPT];
#pragma unroll
    for (int q = 0; q < IPT / 4; q++) {
        const unsigned k = (unsigned)(base + q * 4);
        if (whole && !(GRB_DBG(a, 2))) {
            // (non-temporal streaming, aux 2, measured 2-3 % slower than default-policy loads: debug flag 64 selects it)
            const auto c4 = (GRB_DBG(a, 64)) ? __builtin_amdgcn_raw_buffer_load_b128(crs, k * 4u, 0, 2)
                                         : __builtin_amdgcn_raw_buffer_load_b128(crs, k * 4u, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; i++) creg[q * 4 + i] = (int)c4[i];
            if constexpr (sizeof(T) == 4) {
                const auto v4 = (GRB_DBG(a, 64)) ? __builtin_amdgcn_raw_buffer_load_b128(vrs, k * 4u, 0, 2)
                                             : __builtin_amdgcn_raw_buffer_load_b128(vrs, k * 4u, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; i++) vreg[q * 4 + i] = __builtin_bit_cast(T, (unsigned int)v4[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) vreg[q * 4 + i] = buf_load<T>(vrs, (k + i) * (unsigned)sizeof(T));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                creg[q * 4 + i] = (GRB_DBG(a, 2)) ? (int)((k + i) & 1023) : buf_load<int>(crs, (k + i) * 4u);
                vreg[q * 4 + i] = (GRB_DBG(a, 2)) ? (T)1 : buf_load<T>(vrs, (k + i) * (unsigned)sizeof(T));
            }
        }
    }
    int64_t my_rs = 0, my_re = 0;
    if (tid <= nrows_t && i0 + tid < a.m) {
        my_rs = a.rowptr[i0 + tid];
        my_re = a.rowptr[i0 + tid + 1];
    }
    const int64_t rs0_64 = (i0 < a.m ? a.rowptr[i0] : a.nnz) - j0;  // start of row i0 relative to the tile
    const int abase = (int)(i0 & 31);  // bit of row i0 inside s_act[0]
    const int64_t last_row = i1 < a.m ? i1 : a.m - 1;
    const int nw = has_mask ? (int)((last_row >> 5) - (i0 >> 5)) + 1 : 0;
    const uint32_t mword = (tid < nw) ? ((const uint32_t *)a.m_bits)[(i0 >> 5) + tid] : 0u;
    const int64_t pre_g = (i0 >> 6) + wave;
    const int64_t pre_row = (pre_g << 6) + lane;
    uint64_t pre_word = 0;
    T pre_val = (T)0;
    if ((pre_g << 6) < a.m) {
        pre_word = a.w_old_bits[pre_g];
        if (need_old && pre_row < a.m) pre_val = ((const T *)a.w_old_val)[pre_row];
    }
    const T iso_v = (a.a_iso && need_aval) ? aval[0] : (T)0;
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t xbits_rs = make_rsrc(a.u_bits, a.u_full ? 0 : ((a.x_len + 63) >> 6) * 8);
    const __amdgpu_buffer_rsrc_t xvbits_rs = make_rsrc(a.u_valbits, a.u_valbits ? ((a.x_len + 63) >> 6) * 8 : 0);
    const __amdgpu_buffer_rsrc_t xpv_rs = make_rsrc(a.u_pv, a.u_pv ? ((a.x_len + 15) >> 4) * 4 : 0);
    PHASE_STAMP(1);
    EARLY_EXIT(2);

    // ---- LDS: row accumulators at the monoid identity, row-start marks cleared -----------------------------------
    for (int k = tid; k <= nrows_t; k += PULL_BLOCK) {
        s_tval[k] = pull_seed<T, W>(a, monoid);
        s_thas[k] = 0;
    }
    for (int k = tid * 8; k < TILE + 8; k += PULL_BLOCK * 8) *(uint4 *)&s_head[k] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) s_any = has_mask ? 0 : 1;
    __syncthreads();
    EARLY_EXIT(3);
    // ---- active-row words for rows i0 .. min(i1, m-1); mark the entry at which each non-empty row starts ----------
    for (int k = tid; k < nw; k += PULL_BLOCK) {
        uint32_t w = (k == tid) ? mword : ((const uint32_t *)a.m_bits)[(i0 >> 5) + k];
        if (a.m_comp) w = ~w;
        s_act[k] = w;
        const int64_t base_row = ((i0 >> 5) + k) << 5;
        uint32_t in = 0xffffffffu;  // restrict to [i0, last_row] for the "anything to do" test
        if (base_row < i0) in &= 0xffffffffu << (int)(i0 - base_row);
        if (base_row + 31 > last_row) in &= 0xffffffffu >> (int)(base_row + 31 - last_row);
        if (w & in) s_any = 1;
    }
    for (int k = tid; k <= nrows_t && i0 + k < a.m; k += PULL_BLOCK) {
        const int64_t rs = (k == tid) ? my_rs : a.rowptr[i0 + k];
        const int64_t re = (k == tid) ? my_re : a.rowptr[i0 + k + 1];
        const int64_t start = rs - j0;
        if (start >= 0 && start < nnz_t && rs < re) s_head[start] = (unsigned short)(k + 1);  // local row + 1
    }
    __syncthreads();
    PHASE_STAMP(2);
    EARLY_EXIT(4);
    const bool any_active = s_any != 0;

#define ROW_ACTIVE(r) (!has_mask || ((s_act[(abase + (r)) >> 5] >> ((abase + (r)) & 31)) & 1u))

    if (any_active) {
        // ---- local row (encoded k+1) of each of my entries: row starts inside my chunk, else the last start
        //      seen by earlier lanes (wavefront max-scan by shuffles) / earlier wavefronts (LDS) -------------------
        int h[IPT];
        if constexpr (IPT == 8) {
            const uint4 v = *(const uint4 *)&s_head[base];
            h[0] = v.x & 0xffff; h[1] = v.x >> 16; h[2] = v.y & 0xffff; h[3] = v.y >> 16;
            h[4] = v.z & 0xffff; h[5] = v.z >> 16; h[6] = v.w & 0xffff; h[7] = v.w >> 16;
        } else {
#pragma unroll
            for (int i = 0; i < IPT; i++) h[i] = s_head[base + i];
        }
        int lastk = 0;
#pragma unroll
        for (int i = 0; i < IPT; i++) lastk = h[i] ? h[i] : lastk;  // marks increase along the tile: last = max
        const int incl = wave_inclusive_max_nonneg(lastk);
        const int excl = wave_lane_below(incl, 0);
        if (lane == 63) s_wave_last[wave] = incl;
        __syncthreads();
        PHASE_STAMP(3);
        EARLY_EXIT(5);
        int e = 1;  // the tile's first entries belong to row i0
        for (int x = 0; x < wave; x++) e = e > s_wave_last[x] ? e : s_wave_last[x];
        e = e > excl ? e : excl;

        // ---- classify: column to gather, or -1 (past the tile end / masked-out row: the gather reads nothing) --------
        int ek[IPT], cc[IPT];
#pragma unroll
        for (int i = 0; i < IPT; i++) {
            e = h[i] ? h[i] : e;
            ek[i] = e;
            cc[i] = (base + i < nnz_t && ROW_ACTIVE(e - 1)) ? creg[i] : -1;
        }
        if (GRB_DBG(a, 16384 | 32768)) {  // diagnostic: fold every gather into the first 2^19 / 2^15 entries of the image
            const int gmask = (GRB_DBG(a, 16384)) ? 0x7ffff : 0x7fff;
#pragma unroll
            for (int i = 0; i < IPT; i++) cc[i] = cc[i] >= 0 ? (cc[i] & gmask) : -1;
        }
        // ---- gathers: presence words, then values -- IPT independent random accesses in flight per lane --------------
        bool xp[IPT];
        T xv[IPT];
        bool pv_done = false;
        if constexpr (std::is_same<T, bool>::value) {
            if (a.u_pv && !(GRB_DBG(a, 1))) {  // presence and value from one word
                bool_pv_gather<IPT>(xpv_rs, cc, xp, xv);
                pv_done = true;
            }
        }
        if (pv_done) {
        } else if (a.u_full || (GRB_DBG(a, 1))) {
#pragma unroll
            for (int i = 0; i < IPT; i++) xp[i] = cc[i] >= 0;
        } else {
            uint32_t bw[IPT];
#pragma unroll
            for (int i = 0; i < IPT; i++) bw[i] = buf_load<uint32_t>(xbits_rs, (unsigned)(cc[i] >> 5) * 4u);
#pragma unroll
            for (int i = 0; i < IPT; i++) xp[i] = (bw[i] >> (cc[i] & 31)) & 1u;
        }
        if (pv_done) {
        } else if (need_uval && !(GRB_DBG(a, 1))) {
            if constexpr (std::is_same<T, bool>::value) {
                // BOOL values travel bit-packed (2 MiB at scale 24, its hot head L1-resident) instead of one byte each
                uint32_t vw[IPT];
#pragma unroll
                for (int i = 0; i < IPT; i++) vw[i] = buf_load<uint32_t>(xvbits_rs, xp[i] ? (unsigned)(cc[i] >> 5) * 4u : 0xfffffff8u);
#pragma unroll
                for (int i = 0; i < IPT; i++) xv[i] = (vw[i] >> (cc[i] & 31)) & 1u;
            } else {
#pragma unroll
                for (int i = 0; i < IPT; i++) xv[i] = buf_load<T>(xval_rs, xp[i] ? (unsigned)cc[i] * (unsigned)sizeof(T) : 0xfffffff8u);
            }
        } else {
#pragma unroll
            for (int i = 0; i < IPT; i++) xv[i] = (T)(cc[i] & 7);
        }
        PHASE_STAMP(4);

        // ---- segmented fold of my chunk, straight-line: a segment ends where the next entry starts a row (or at the
        //      end of the chunk) and is emitted with ONE LDS atomic into its row's accumulator ------------------------
        T acc = (T)0;
        bool has = false;
#pragma unroll
        for (int i = 0; i < IPT; i++) {
            const T av = need_aval ? (a.a_iso ? iso_v : vreg[i]) : (T)0;
            const T prod = apply_binop<T>(mult, av, xv[i]);
            const bool keep = has && (i > 0) && (h[i] == 0);
            acc = xp[i] ? (keep ? apply_binop<T>(monoid, acc, prod) : prod) : (keep ? acc : (T)0);
            has = xp[i] || keep;
            const bool seg_end = (i == IPT - 1) ? true : (h[i + 1] != 0);
            // emit without a branch: a finished segment goes to its row's accumulator, anything else to this
            // lane's scratch slot (accumulators start at the monoid identity, so one atomic is right whether or
            // not other threads share the row; "any" just stores)
            const int k = (seg_end && has) ? ek[i] - 1 : TILE + 1 + lane;
            if (monoid == OP_ANY || (GRB_DBG(a, 16))) s_tval[k] = (W)acc;
            else atomic_combine<W>(&s_tval[k], (W)acc, monoid);
            s_thas[k] = 1;
        }
    }
    __syncthreads();
    PHASE_STAMP(5);
    EARLY_EXIT(6);

    // ---- epilogue: rows this tile owns, 64 consecutive rows per wavefront -----------------------------------------
    const bool started_earlier = (i0 < a.m) && (rs0_64 < 0);
    const int own_lo = (started_earlier && nrows_t > 0) ? 1 : 0;
    const int64_t row_lo = i0 + own_lo, row_hi = i1;  // [row_lo, row_hi)
    if (row_lo < row_hi && !(GRB_DBG(a, 4))) {
        const int64_t g_first = row_lo >> 6, g_last = (row_hi - 1) >> 6;
        for (int64_t g = g_first + wave; g <= g_last; g += PULL_BLOCK / 64) {
            const int64_t row = (g << 6) + lane;
            bool owned = row >= row_lo && row < row_hi;
            if (a.long_bits) owned = owned && !((a.long_bits[g] >> lane) & 1ull);  // long rows belong to k_mxv_long
            const uint64_t oldw = (g == pre_g) ? pre_word : a.w_old_bits[g];
            const bool old_has = (oldw >> lane) & 1ull;
            bool new_has = false;
            if (owned) {
                const int k = (int)(row - i0);
                const bool mact = ROW_ACTIVE(k);
                T old_val = pre_val;
                if (g != pre_g && need_old && old_has) old_val = ((const T *)a.w_old_val)[row];
                new_has = write_rule_row<T>(a, row, mact, old_has, old_val, s_thas[k] != 0, from_acc<T, W>(s_tval[k]));
            }
            const unsigned long long nb = __ballot(owned && new_has);
            const unsigned long long om = __ballot(owned);
            if (lane == 0) {
                if (om == ~0ull) a.w_new_bits[g] = nb;
                else {
                    atomicAnd((unsigned long long *)&a.w_new_bits[g], ~om);
                    if (nb) atomicOr((unsigned long long *)&a.w_new_bits[g], nb);
                }
            }
        }
    }
#undef ROW_ACTIVE
    PHASE_STAMP(6);

    // ---- seams: the row still open at the tile end, and a first row that began in an earlier tile ------------------
    if (tid == 0) {
        a.carry_has[tile] = s_thas[nrows_t];
        ((W *)a.carry_val)[tile] = s_tval[nrows_t];
        const bool se = started_earlier && nrows_t > 0;
        a.first_has[tile] = se ? (unsigned char)(2 | (s_thas[0] ? 1 : 0)) : (unsigned char)0;
        ((W *)a.first_val)[tile] = s_tval[0];
    }
    PHASE_STAMP(7);
}
