// Part of grb_mxv.hip (included there, inside namespace grb): k_mxv_rows -- one wavefront per 64 rows for the short rows of a split matrix + the write rule of every row
// ---------------------------------------------------------------------------------------------------
// Short rows of a split matrix (every row below split_min_len entries; the long rows are empty here): one WAVEFRONT per
// 64 consecutive rows = one word of the presence bitmap.  Nothing is shared between wavefronts: no workgroup barrier, no
// tile table, no seams.  The group's entries are contiguous in the CSR arrays and are consumed in windows of 64 x 8
// entries -- each lane takes 8 consecutive entries straight into registers (16-byte loads), the row of each entry
// comes from row-start marks in LDS plus a wavefront max-scan, products are folded per lane and every finished
// segment goes to its row's LDS accumulator with one LDS atomic (as in k_mxv_pull).  The epilogue applies the write
// rule to the 64 rows with coalesced loads and stores and writes the whole presence word; long rows of the group take
// their product from k_mxv_long's per-row accumulators.
// ---------------------------------------------------------------------------------------------------
#ifndef GRB_ROWS_BLOCK
#define GRB_ROWS_BLOCK 128  // (measured 64 / 128 / 256 / 512 / 1024 threads: 0.936 / 0.936 / 0.948 / 1.02 / 1.10 ms per masked call -- a block holds its CU slot until its slowest wavefront is done)
#endif
constexpr int ROWS_BLOCK = GRB_ROWS_BLOCK;
#ifndef GRB_ROWS_EPL
#define GRB_ROWS_EPL 4
#endif
constexpr int ROWS_EPL = GRB_ROWS_EPL;

// one group of 64 rows, by one wavefront; mark / acc / has are the wavefront's LDS scratch
// `head` / `head_n`: the first head_n entries (non-BOOL: values; BOOL: 32-bit words of value bits or of (presence, value) pairs)
// of the operand image kept in LDS by the caller -- gathers of those codes bypass the vector-memory path (0.7 instead of ~5 us
// per million, DESIGN.md section 4.1); nullptr / 0 = no head.
template <typename T, int MONOID_CT, int MULT_CT>
__device__ __forceinline__ void rows_group(const PullArgs &a, int64_t g, int lane, unsigned char *mark,
                                           typename Widen<T>::type *acc_slots, unsigned char *has_slots,
                                           const uint32_t *head = nullptr, int head_n = 0)
{
    using W = typename Widen<T>::type;
    constexpr int EPL = ROWS_EPL, WIN = 64 * EPL;
    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const T *aval = (const T *)a.aval;
    const bool need_aval = a.need_aval != 0, need_uval = a.need_uval != 0;
    const bool stage_vals = need_aval && !a.a_iso;
    const bool need_old = (a.accum >= 0) || a.fresh;
    const int64_t row = (g << 6) + lane;
    const bool in = row < a.m;

    // ---- everything the group needs from HBM is requested up front: row bounds, mask / presence / long-row words, old w
    const int64_t p0 = a.rowptr[in ? row : a.m], p1 = a.rowptr[in ? row + 1 : a.m];
    uint64_t actw = a.has_mask ? (a.m_comp ? ~a.m_bits[g] : a.m_bits[g]) : ~0ull;
    const uint64_t longw = a.long_bits ? a.long_bits[g] : 0ull;
    const uint64_t oldw = a.w_old_bits[g];
    const bool old_has = in && ((oldw >> lane) & 1ull);
    const T old_val = (need_old && in) ? ((const T *)a.w_old_val)[row] : (T)0;  // (not waiting for the presence word)
    const bool is_long = (longw >> lane) & 1ull;
    int long_slot = 0;
    if (longw) long_slot = a.long_prefix[g] + __popcll(longw & ((1ull << lane) - 1ull));
    bool t_has = false;
    W t_acc = pull_seed<T, W>(a, monoid);
    if (is_long) {
        t_has = a.tl_has[long_slot] != 0;
        t_acc = acc_from_stored<W>(((const W *)a.tl_val)[long_slot], a.tl_ord != 0);
    }
    const T iso_v = (a.a_iso && need_aval) ? aval[0] : (T)0;
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t xbits_rs = make_rsrc(a.u_bits, a.u_full ? 0 : ((a.x_len + 63) >> 6) * 8);
    const __amdgpu_buffer_rsrc_t xvbits_rs = make_rsrc(a.u_valbits, a.u_valbits ? ((a.x_len + 63) >> 6) * 8 : 0);
    const __amdgpu_buffer_rsrc_t xpv_rs = make_rsrc(a.u_pv, a.u_pv ? ((a.x_len + 15) >> 4) * 4 : 0);

    const int64_t gbase = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(p0 >> 32), 0) << 32) |
                                    (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p0, 0));
    const int rel = (int)(p0 - gbase), len = (int)(p1 - p0);
    const int total = __builtin_amdgcn_readlane(rel + len, 63);  // entries of the group (< 64 * split_min_len)

    // (floating-point MIN / MAX accumulators are kept in their order-preserving unsigned form: the fold's LDS atomic is then a native
    //  ds_min_u32 / ds_max_u32 -- atomicMin on a float in LDS compiles to a read, a compare and a compare-and-swap LOOP, four of
    //  them per group and lane)
    const bool acc_ord = acc_is_ordered<W>(monoid);
    acc_slots[lane] = acc_to_stored<W>(pull_seed<T, W>(a, monoid), acc_ord);
    acc_slots[64 + lane] = acc_to_stored<W>(pull_seed<T, W>(a, monoid), acc_ord);
    has_slots[lane] = 0;
    has_slots[64 + lane] = 0;

    const int64_t left = a.nnz - gbase;  // entries from the group's first to the end of the arrays
    const __amdgpu_buffer_rsrc_t crs = make_rsrc(a.col + gbase, left * 4);
    const __amdgpu_buffer_rsrc_t vrs = make_rsrc(aval + (a.a_iso ? 0 : gbase), stage_vals ? left * (int64_t)sizeof(T) : 0);
    const bool any_active = (actw & ~longw) != 0;  // (a group without an active short row reads none of its entries)

    // my EPL consecutive entries of the window at `wbase` (16-byte loads where they cannot straddle the end of the arrays)
    // (a full operand whose values the multiply does not read -- the row reductions -- needs no column index at all)
    const bool no_cols = a.u_full && !need_uval && !(GRB_DBG(a, 524288));
    auto load_window = [&](int wbase, int (&cr)[EPL], T (&vr)[EPL]) {
        const int e0 = wbase + lane * EPL;
        const bool whole = left >= (int64_t)wbase + WIN + 4;
        if (no_cols) {
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                cr[i] = 0;
                vr[i] = (T)0;
            }
            if (!stage_vals) return;
#pragma unroll
            for (int q = 0; q < EPL / 4; q++) {
                const unsigned k = (unsigned)(e0 + q * 4);
                if constexpr (sizeof(T) == 4) {
                    if (whole) {
                        const auto v4 = __builtin_amdgcn_raw_buffer_load_b128(vrs, k * 4u, 0, 0);
#pragma unroll
                        for (int i = 0; i < 4; i++) vr[q * 4 + i] = __builtin_bit_cast(T, (unsigned int)v4[i]);
                        continue;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; i++) vr[q * 4 + i] = buf_load<T>(vrs, (k + i) * (unsigned)sizeof(T));
            }
            return;
        }
#pragma unroll
        for (int q = 0; q < EPL / 4; q++) {
            const unsigned k = (unsigned)(e0 + q * 4);
            if (whole) {
                const auto c4 = (GRB_DBG(a, 64)) ? __builtin_amdgcn_raw_buffer_load_b128(crs, k * 4u, 0, 2)
                                             : __builtin_amdgcn_raw_buffer_load_b128(crs, k * 4u, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; i++) cr[q * 4 + i] = (int)c4[i];
                if constexpr (sizeof(T) == 4) {
                    const auto v4 = (GRB_DBG(a, 64)) ? __builtin_amdgcn_raw_buffer_load_b128(vrs, k * 4u, 0, 2)
                                                 : __builtin_amdgcn_raw_buffer_load_b128(vrs, k * 4u, 0, 0);
#pragma unroll
                    for (int i = 0; i < 4; i++) vr[q * 4 + i] = __builtin_bit_cast(T, (unsigned int)v4[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) vr[q * 4 + i] = buf_load<T>(vrs, (k + i) * (unsigned)sizeof(T));
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    cr[q * 4 + i] = buf_load<int>(crs, (k + i) * 4u);
                    vr[q * 4 + i] = buf_load<T>(vrs, (k + i) * (unsigned)sizeof(T));
                }
            }
        }
    };
    // the next window's entries are requested before the current window's gathers: one HBM round trip less per window
    int cnext[EPL];
    T vnext[EPL];
    if (total > 0 && any_active) load_window(0, cnext, vnext);
    for (int wbase = 0; wbase < total && any_active; wbase += WIN) {
        const int e0 = wbase + lane * EPL;  // my EPL consecutive entries of the group
        int creg[EPL];
        T vreg[EPL];
#pragma unroll
        for (int i = 0; i < EPL; i++) {
            creg[i] = cnext[i];
            vreg[i] = vnext[i];
        }
        if (wbase + WIN < total && !(GRB_DBG(a, 131072))) load_window(wbase + WIN, cnext, vnext);
        else if (wbase + WIN < total) {  // (diagnostic: no prefetch -- the load waits here)
            load_window(wbase + WIN, cnext, vnext);
            __builtin_amdgcn_s_waitcnt(0);
        }
        // ---- row of each entry: marks where rows start inside the window, max-scan across the wavefront -------------
        using MarkWord = typename std::conditional<EPL == 8, uint64_t, uint32_t>::type;  // my EPL marks in one LDS access
        *(MarkWord *)&mark[lane * EPL] = 0;
        wave_sync();
        if (len > 0 && rel >= wbase && rel < wbase + WIN) mark[rel - wbase] = (unsigned char)(lane + 1);
        const unsigned long long before = __ballot(len > 0 && rel <= wbase);  // rows begun at or before the window start
        const int carry_in = 64 - __clzll(before);                            // (1 + the last of them; never 0 inside a group)
        wave_sync();
        const uint64_t mk = *(const MarkWord *)&mark[lane * EPL];
        int h[EPL];
#pragma unroll
        for (int i = 0; i < EPL; i++) h[i] = (int)((mk >> (8 * i)) & 0xffu);
        int lastk = 0;
#pragma unroll
        for (int i = 0; i < EPL; i++) lastk = h[i] ? h[i] : lastk;  // marks increase along the window: last = max
        const int incl = wave_inclusive_max_nonneg(lastk);  // (in the vector ALU: seven ds_bpermute round trips sat here, between the entries and their gathers)
        int e = wave_lane_below(incl, 0);
        e = e > carry_in ? e : carry_in;
        // ---- classify: column to gather, or -1 (past the group's end / masked-out row: the gather reads nothing) -----
        int ek[EPL], cc[EPL];
#pragma unroll
        for (int i = 0; i < EPL; i++) {
            e = h[i] ? h[i] : e;
            ek[i] = e;
            cc[i] = (e0 + i < total && ((actw >> (e - 1)) & 1ull)) ? creg[i] : -1;
        }
        if (GRB_DBG(a, 16384 | 32768)) {  // diagnostic: fold every gather into the first 2^19 / 2^15 entries of the image
            const int gmask = (GRB_DBG(a, 16384)) ? 0x7ffff : 0x7fff;
#pragma unroll
            for (int i = 0; i < EPL; i++) cc[i] = cc[i] >= 0 ? (cc[i] & gmask) : -1;
        }
        // ---- gathers: presence words, then values -- EPL independent random accesses in flight per lane --------------
        bool xp[EPL];
        T xv[EPL];
        bool pv_done = false;
        if constexpr (std::is_same<T, bool>::value) {
            if (a.u_pv && !(GRB_DBG(a, 1))) {  // presence and value from one word
                bool_pv_gather<EPL>(xpv_rs, cc, xp, xv);
                pv_done = true;
            }
        }
        if (pv_done) {
        } else if (a.u_full || (GRB_DBG(a, 1))) {
#pragma unroll
            for (int i = 0; i < EPL; i++) xp[i] = cc[i] >= 0;
        } else {
            uint32_t bw[EPL];
#pragma unroll
            for (int i = 0; i < EPL; i++) bw[i] = buf_load<uint32_t>(xbits_rs, (unsigned)(cc[i] >> 5) * 4u);
#pragma unroll
            for (int i = 0; i < EPL; i++) xp[i] = (bw[i] >> (cc[i] & 31)) & 1u;
        }
        if (pv_done) {
        } else if (need_uval && !(GRB_DBG(a, 1))) {
            if constexpr (std::is_same<T, bool>::value) {
                uint32_t vw[EPL];
#pragma unroll
                for (int i = 0; i < EPL; i++) vw[i] = buf_load<uint32_t>(xvbits_rs, (xp[i] && (cc[i] >> 5) >= head_n) ? (unsigned)(cc[i] >> 5) * 4u : 0xfffffff8u);
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    uint32_t w32 = vw[i];
                    if (head_n > 0) {
                        const bool res = xp[i] && (cc[i] >> 5) < head_n;
                        uint32_t lw = head[res ? (cc[i] >> 5) : 0];
                        GRB_PIN(lw);
                        w32 = res ? lw : w32;
                    }
                    xv[i] = (w32 >> (cc[i] & 31)) & 1u;
                }
            } else {
                T xg[EPL];
#pragma unroll
                for (int i = 0; i < EPL; i++) xg[i] = buf_gather<T>(xval_rs, (xp[i] && cc[i] >= head_n) ? (unsigned)cc[i] * (unsigned)sizeof(T) : 0xfffffff8u);
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    xv[i] = xg[i];
                    if (head_n > 0) {
                        const bool res = xp[i] && cc[i] < head_n;
                        T xl;
                        if constexpr (sizeof(T) == 8) {
                            uint64_t w64 = ((const uint64_t *)head)[res ? cc[i] : 0];
                            GRB_PIN(w64);
                            xl = __builtin_bit_cast(T, w64);
                        } else {
                            uint32_t w32 = head[res ? cc[i] : 0];
                            GRB_PIN(w32);
                            if constexpr (sizeof(T) == 4) xl = __builtin_bit_cast(T, w32);
                            else xl = (T)w32;
                        }
                        xv[i] = res ? xl : xg[i];
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < EPL; i++) xv[i] = (T)(cc[i] & 7);
        }
        // ---- segmented fold of my entries, straight-line: a segment ends where the next entry starts a row (or at the
        //      end of my entries) and is emitted with ONE LDS atomic into its row's accumulator -------------------------
        T acc = (T)0;
        bool has = false;
#pragma unroll
        for (int i = 0; i < EPL; i++) {
            const T av = need_aval ? (a.a_iso ? iso_v : vreg[i]) : (T)0;
            const T prod = apply_binop<T>(mult, av, xv[i]);
            const bool keep = has && (i > 0) && (h[i] == 0);
            acc = xp[i] ? (keep ? apply_binop<T>(monoid, acc, prod) : prod) : (keep ? acc : (T)0);
            has = xp[i] || keep;
            const bool seg_end = (i == EPL - 1) ? true : (h[i + 1] != 0);
            const int k = (seg_end && has) ? ek[i] - 1 : 64 + lane;
            if (monoid == OP_ANY) acc_slots[k] = (W)acc;
            else atomic_combine_ord<W>(&acc_slots[k], (W)acc, monoid);
            has_slots[k] = 1;
        }
    }
    wave_sync();

    // ---- write rule for my row; the wavefront owns the whole presence word ----------------------------------------------
    if (GRB_DBG(a, 4)) return;
    if (!is_long) {
        t_has = has_slots[lane] != 0;
        t_acc = acc_from_stored<W>(acc_slots[lane], acc_ord);
    }
    bool new_has = false;
    if (in) new_has = write_rule_row<T>(a, row, (actw >> lane) & 1ull, old_has, old_val, t_has, from_acc<T, W>(t_acc));
    const unsigned long long nb = __ballot(in && new_has);
    if (lane == 0) a.w_new_bits[g] = nb;
}


template <typename T, int MONOID_CT, int MULT_CT>
// (8 wavefronts per SIMD: the register allocator otherwise keeps 106 SGPRs = 7 wavefronts; with the bound it moves ~40 scalars to
//  VGPR lanes and the masked bench call goes from 0.932 to 0.924 ms)
#ifndef GRB_ROWS_WPE
#define GRB_ROWS_WPE 8  // (build-time variant: 0 = no occupancy attribute)
#endif
#if GRB_ROWS_WPE > 0
#define GRB_ROWS_WPE_ATTR __attribute__((amdgpu_waves_per_eu(GRB_ROWS_WPE, GRB_ROWS_WPE)))
#else
#define GRB_ROWS_WPE_ATTR
#endif
__global__ __launch_bounds__(ROWS_BLOCK) GRB_ROWS_WPE_ATTR void k_mxv_rows(const PullArgs a)
{
    using W = typename Widen<T>::type;
    constexpr int WIN = 64 * ROWS_EPL, NW = ROWS_BLOCK / 64;
    __shared__ __attribute__((aligned(16))) unsigned char s_mark[NW][WIN];
    __shared__ W s_acc[NW][128];  // 64 rows + one scratch slot per lane ("nothing to emit" of the branch-free fold)
    __shared__ unsigned char s_has[NW][128];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t g = (int64_t)blockIdx.x * NW + wave;
    if ((g << 6) >= a.m) return;  // wave-uniform; wavefronts never wait for each other
    rows_group<T, MONOID_CT, MULT_CT>(a, g, lane, s_mark[wave], s_acc[wave], s_has[wave]);
}

