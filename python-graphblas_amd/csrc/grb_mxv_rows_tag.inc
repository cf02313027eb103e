// Part of grb_mxv.hip (included there, inside namespace grb): k_mxv_rows_tag -- the short rows of a split matrix as TAGGED ROW GROUPS
// ---------------------------------------------------------------------------------------------------
// Round 3.  k_mxv_rows spends most of its ~550 vector-ALU instructions per group of 64 rows (~200 entries) finding out which row an
// entry belongs to (row-start marks in LDS, a wavefront max-scan, a branch-free segmented fold) and shuttling row bounds between
// lanes, behind 8-byte row pointers it reads for every row.  (A wave64 instruction holds a SIMD16 for 4 cycles: that is ~230 us of
// issue time for 262 144 groups.  The long-row strip kernel WAS bound by it -- DESIGN.md section 4.1.0; the short rows turned out
// not to be: this kernel issues a fifth of the instructions and is 10 % faster, its time is a sum of small terms -- entry stream,
// gathers, the per-row write rule -- each near its own limit.)
//
// Here the ROW OF EVERY ENTRY IS STORED with the entry: the short rows are kept a second time as groups of 64 consecutive rows,
// the entries of a group contiguous and padded to a multiple of 4, with one byte per entry naming its row inside the group (64 =
// padding).  A wavefront takes a group: two scalar loads give its entry range (no row pointers, no cross-lane traffic), a lane
// loads 4 consecutive entries (16-byte loads) and their 4 tags (one dword), and every product goes straight to its row's LDS
// accumulator with one native LDS atomic (ds_min_f32 / ds_add / ...); padding accumulates into a 65th slot nobody reads.  Rows
// the mask switches off: their LDS "off" word is -1 and is OR-ed into the column code, which makes the gather out of range --
// free -- with no compare or branch.
// The epilogue (write rule for the 64 rows, presence word by ballot, long rows from the long-row accumulators) is k_mxv_rows'.
// ---------------------------------------------------------------------------------------------------
constexpr int TAG_EPL = 4;

// ---- build (once per matrix, from the short part S) ---------------------------------------------------------------------
// entries of group g, in units of TAG_EPL (rounded up); nonempty[g] bit l = row 64 g + l has an entry
__global__ void k_tag_count(const int64_t *sptr, int64_t m, int64_t ngroups, int64_t *cnt, uint64_t *nonempty)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = r >> 6;
    const bool ne = r < m && sptr[r + 1] > sptr[r];
    const unsigned long long b = __ballot(ne);
    if ((threadIdx.x & 63) == 0 && g <= ngroups) {
        if (g < ngroups) {
            const int64_t r1 = (g + 1) * 64 < m ? (g + 1) * 64 : m;
            cnt[g] = (sptr[r1] - sptr[g * 64] + TAG_EPL - 1) / TAG_EPL;
            nonempty[g] = b;
        } else {
            cnt[g] = 0;
        }
    }
}
__global__ void k_tag_off32(const int64_t *off64, int64_t n1, int32_t *off32)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n1) off32[i] = (int32_t)off64[i];
}
template <typename T>
__global__ void k_tag_fill(const int64_t *sptr, const int32_t *scol, const T *sval, int iso, int64_t m, const int32_t *off,
                           int32_t *tcol, T *tval, unsigned char *ttag, const unsigned long long *vd_table, const unsigned char *vd_codes)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const int64_t g = r >> 6;
    const int64_t b = sptr[r], e = sptr[r + 1];
    const int64_t d = (int64_t)off[g] * TAG_EPL + (b - sptr[g * 64]);
    for (int64_t i = b; i < e; i++) {
        tcol[d + (i - b)] = scol[i];
        bool coded = false;
        if constexpr (sizeof(T) == 4) {
            if (vd_table) {  // dictionary-coded values (grb_mxv_vdict.inc): tval is a byte array
                ((unsigned char *)tval)[d + (i - b)] = (unsigned char)vdict_code(vd_table, vd_codes, ((const uint32_t *)sval)[i]);
                coded = true;
            }
        }
        if (!iso && !coded) tval[d + (i - b)] = sval[i];
        ttag[d + (i - b)] = (unsigned char)(r & 63);
    }
}

// ---- LDS accumulator combine: native LDS atomics for every builtin monoid and accumulator type -----------------------------------
template <typename W>
__device__ __forceinline__ void lds_combine(W *slot, W v, int monoid)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (std::is_floating_point<W>::value) {
        // (atomicMin / atomicMax on a float in LDS compile to compare-and-swap loops; the fetch_min / fetch_max builtins become
        //  ds_min_f32 / ds_max_f32 / ds_min_f64 / ds_max_f64: IEEE minNum / maxNum, a NaN product is dropped as fmin / fmax drop it)
        if (monoid == OP_MIN) { (void)__hip_atomic_fetch_min(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); return; }
        if (monoid == OP_MAX) { (void)__hip_atomic_fetch_max(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); return; }
    }
#endif
    atomic_combine<W>(slot, v, monoid);
}

// K consecutive groups per wavefront, in lockstep: what bounds this kernel is the LIFETIME of a wavefront -- three dependent memory
// round trips (entry range and mask words -> entries -> gathers) of 2-3 us each under load, 8 us per group with 32 wavefronts per
// CU resident -- not instructions or bytes.  With K groups per wavefront the loads of all K are in flight together: the same
// latency buys K times the work (38 VGPRs for one group leave room for four at 8 wavefronts per SIMD).
#ifndef GRB_TAG_GROUPS
#define GRB_TAG_GROUPS 4
#endif
constexpr int TAG_K = GRB_TAG_GROUPS;
#ifndef GRB_TAG_ABL
#define GRB_TAG_ABL 0  // build-time ablation (results WRONG): 1 no window loop, 2 no gathers, 4 no LDS atomics (products summed in a register), 8 no value stores in the write rule
#endif

// The LDS HEAD (end of round 4, k_mxv_rows_tag<..., HEAD = true>; launched for BOOL operands).  What this kernel costs is its gathers:
// one L2 read request and one 128-byte L1 line fill per gathered word (profiles/r04/pmc_units_*.txt: the L1 stalled on misses 60-80 %
// of the time).  In a matrix's popularity order the column codes ARE popularity ranks.  TWO persistent 1024-thread workgroups per CU
// each keep the first HEAD words of the image this call gathers from in LDS; a lane whose column is in the head reads LDS and hands the
// texture path an out-of-range address (no request, no line).  One group per wavefront at a time (64 registers: 32 wavefronts per CU),
// the groups dealt round-robin to the grid's wavefronts.
// Measured (scale 24): a BOOL operand as presence / value pairs -- 16 columns per word, the head holds the 276 Ki hottest columns, ~70 %
// of the references -- 266 -> 238 us.  A full FP32 operand -- 17 Ki values, ~31 % of the references -- 236 -> 268 us masked, 362 -> 400
// unmasked: the persistent form costs more than a third of the gathers is worth, so the host launches the head for BOOL only.  (Earlier
// forms: one workgroup per CU with 31 Ki values and four groups per wavefront 315 / 403 us; groups taken from one atomic counter
// 1.5 ms -- 262 144 atomics on one address.)
constexpr int TAG_HEAD_BLOCK = 1024;
template <typename W> GRB_HD constexpr int tag_head_words()
{
    // half of the 160 KiB of LDS minus the accumulators, masks and flags of 16 wavefronts (one group each), the dictionary and slack
    return (81920 - (TAG_HEAD_BLOCK / 64) * (66 * (int)sizeof(W) + 66 * 4 + 72) - 1024 - 512) / 4 / 256 * 256;
}
template <typename T, int MONOID_CT, int MULT_CT, bool HEAD = false>
__global__ __launch_bounds__(HEAD ? TAG_HEAD_BLOCK : ROWS_BLOCK, HEAD ? 8 : 1) void k_mxv_rows_tag(const PullArgs a)
{
    using W = typename Widen<T>::type;
    constexpr int BLOCK = HEAD ? TAG_HEAD_BLOCK : ROWS_BLOCK;
    constexpr int EPL = TAG_EPL, NW = BLOCK / 64, K = HEAD ? 1 : TAG_K;
    constexpr int HEAD_WORDS = HEAD ? tag_head_words<W>() : 0, HEAD_SLOTS = HEAD_WORDS * 4 / (int)sizeof(T);
    __shared__ W s_acc[NW][K][66];            // 64 rows + the padding slot
    __shared__ uint32_t s_off[NW][K][66];     // per row: 0 = its entries gather, 0xffffffff = they do not (masked-out row); [64] padding
    __shared__ unsigned char s_has[NW][K][72];
    __shared__ uint32_t s_dict[sizeof(T) == 4 ? 256 : 1];  // (dictionary-coded values: the 256 bit patterns)
    __shared__ __attribute__((aligned(16))) uint32_t s_head[HEAD ? HEAD_WORDS : 4];
    if constexpr (sizeof(T) == 4) {
        if (a.vdict) {
            for (int i = threadIdx.x; i < 256; i += BLOCK) s_dict[i] = ((const uint32_t *)a.vdict)[i];
            if constexpr (!HEAD) __syncthreads();  // (the only workgroup barrier of the kernel: before any wavefront leaves)
        }
    }
    const bool head_pv = HEAD && std::is_same<T, bool>::value && a.u_pv != nullptr;
    if constexpr (HEAD) {
        // the first HEAD_WORDS words of the image, a thread's loads in flight before the first is stored (lds_fill)
        const __amdgpu_buffer_rsrc_t head_rs = head_pv ? make_rsrc(a.u_pv, ((a.x_len + 15) >> 4) * 4) : make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
        lds_fill<BLOCK>(s_head, HEAD_WORDS, [&](int k) { return buf_load<uint32_t>(head_rs, (unsigned)k * 4u); });
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // my K groups.  A matrix in its popularity order (grb_mxv_order.inc) has its rows sorted by falling weight and its empty rows at the
    // end: the kernel then covers the first tg_groups groups only (the tail has no product: k_rows_tail applies the write rule to its
    // presence words alone) and a wavefront takes groups j, j + Q, j + 2Q, .. -- one from every K-th of the range, so that the dense
    // groups at the front are spread over all wavefronts instead of filling the first few to the brim.  (HEAD: one group at a time.)
    const int64_t ngroups = a.tg_groups > 0 ? a.tg_groups : (a.m + 63) >> 6;
    const int64_t gstride = (!HEAD && a.tg_stride > 0) ? a.tg_stride : 1;
    const int64_t n_sets = HEAD ? ngroups : (a.tg_stride > 0 ? a.tg_stride : (ngroups + K - 1) / K);
    // (HEAD: wavefront number + a multiple of the grid's wavefronts -- one shared counter for 262 144 groups was 1.5 ms of serialised atomics)
    const int64_t jw_step = HEAD ? (int64_t)gridDim.x * NW : n_sets;
    for (int64_t jw = (int64_t)blockIdx.x * NW + wave; jw < n_sets; jw += jw_step) {  // (wave-uniform: wavefronts never wait for each other)
    const int64_t g0 = (HEAD || a.tg_stride > 0) ? jw : jw * K;
    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const bool need_aval = a.need_aval != 0, need_uval = a.need_uval != 0;
    const bool stage_vals = need_aval && !a.a_iso;
    const bool need_old = (a.accum >= 0) || a.fresh;
    const T iso_v = (a.a_iso && need_aval) ? ((const T *)a.aval)[0] : (T)0;
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t xbits_rs = make_rsrc(a.u_bits, a.u_full ? 0 : ((a.x_len + 63) >> 6) * 8);
    const __amdgpu_buffer_rsrc_t xvbits_rs = make_rsrc(a.u_valbits, a.u_valbits ? ((a.x_len + 63) >> 6) * 8 : 0);
    const __amdgpu_buffer_rsrc_t xpv_rs = make_rsrc(a.u_pv, a.u_pv ? ((a.x_len + 15) >> 4) * 4 : 0);
    // a full operand whose values the multiply does not read (the row reductions) needs no column index at all
    const bool no_cols = a.u_full && !need_uval;
    const int32_t *tcol = a.tg_col;
    const T *tval = (const T *)a.tg_val;
    const uint32_t *ttag = (const uint32_t *)a.tg_tag;

    // ---- everything the K groups need from HBM is requested up front: entry ranges, mask / presence / long-row words, old w ----
    bool live[K];
    int o0[K], o1[K];
    uint64_t actw[K], longw[K], nonempty[K];
    bool old_has[K], is_long[K], act_me[K], in[K], any_active[K];
    T old_val[K];
    bool t_has[K];
    W t_acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int64_t g = g0 + k * gstride;
        live[k] = g < ngroups;  // (wave-uniform)
        const int64_t gs = live[k] ? g : ngroups - 1;
        o0[k] = a.tg_off[gs];
        o1[k] = live[k] ? a.tg_off[gs + 1] : o0[k];
        actw[k] = a.has_mask ? (a.m_comp ? ~a.m_bits[gs] : a.m_bits[gs]) : ~0ull;
        longw[k] = a.long_bits ? a.long_bits[gs] : 0ull;
        nonempty[k] = a.tg_nonempty[gs];
        uint64_t oldw = a.w_old_bits[gs];
        if (GRB_TAG_ABL & 32) longw[k] = 0;
        if (GRB_TAG_ABL & 64) { actw[k] = 0x5555555555555555ull * (uint64_t)(gs | 1); nonempty[k] = ~0ull; oldw = ~0ull; longw[k] = 0; }
        const int64_t row = (gs << 6) + lane;
        in[k] = live[k] && row < a.m;
        old_has[k] = in[k] && ((oldw >> lane) & 1ull);
        old_val[k] = (need_old && in[k] && !(GRB_TAG_ABL & 16)) ? ((const T *)a.w_old_val)[row] : (T)0;
        is_long[k] = live[k] && ((longw[k] >> lane) & 1ull);
        t_has[k] = false;
        t_acc[k] = pull_seed<T, W>(a, monoid);
        act_me[k] = (actw[k] >> lane) & 1ull;
        // (a group without an active short row reads none of its entries; long_tails: long rows hold their cold entries here too)
        any_active[k] = live[k] && (actw[k] & nonempty[k] & (a.long_tails ? ~0ull : ~longw[k])) != 0;
        s_acc[wave][k][lane] = pull_seed<T, W>(a, monoid);
        s_off[wave][k][lane] = act_me[k] ? 0u : 0xffffffffu;
        s_has[wave][k][lane] = 0;
        if (lane == 0) {
            s_acc[wave][k][64] = pull_seed<T, W>(a, monoid);
            s_off[wave][k][64] = 0u;  // (padding entries carry column -1 themselves)
            s_has[wave][k][64] = 0;
        }
    }

    // (dictionary-coded values: the word of four one-byte codes is kept and looked up when the products are formed -- a lookup here would
    //  wait for the load it follows, and with it for every load requested ahead)
    auto load_unit = [&](int unit, bool on, int (&cr)[EPL], T (&vr)[EPL], uint32_t &vcode, uint32_t &tg) {
        if (on) {
            const int64_t e = (int64_t)unit * EPL;
            if (!no_cols) {
                const uint4 c4 = *(const uint4 *)(tcol + e);
                cr[0] = (int)c4.x; cr[1] = (int)c4.y; cr[2] = (int)c4.z; cr[3] = (int)c4.w;
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) cr[i] = 0;
            }
            if (stage_vals) {
                if constexpr (sizeof(T) == 4) {
                    if (a.vdict) vcode = ((const uint32_t *)tval)[unit];  // four one-byte codes
                    else {
                        const uint4 v4 = *(const uint4 *)(tval + e);
                        vr[0] = __builtin_bit_cast(T, v4.x); vr[1] = __builtin_bit_cast(T, v4.y);
                        vr[2] = __builtin_bit_cast(T, v4.z); vr[3] = __builtin_bit_cast(T, v4.w);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < EPL; i++) vr[i] = tval[e + i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) vr[i] = iso_v;
            }
            tg = ttag[unit];
        } else {  // past the group's end: four padding entries
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                cr[i] = -1;
                vr[i] = iso_v;
            }
            vcode = 0u;
            tg = 0x40404040u;
        }
    };
    wave_sync();
    int cnext[K][EPL];
    T vnext[K][EPL];
    uint32_t tnext[K], dnext[K];
    int wins = 0;  // windows of the longest of my groups
#pragma unroll
    for (int k = 0; k < K; k++) {
        tnext[k] = 0x40404040u;
        dnext[k] = 0u;
        if (any_active[k] && o0[k] < o1[k]) {
            load_unit(o0[k] + lane, o0[k] + lane < o1[k], cnext[k], vnext[k], dnext[k], tnext[k]);
            const int wk = (o1[k] - o0[k] + 63) >> 6;
            wins = wk > wins ? wk : wins;
        }
    }
    // the long rows of my groups: their results come from the long-row kernels' accumulators, behind two more dependent loads (slot
    // prefix -> slot) -- requested only now, after the first window's entries, so that the entry loads do not queue behind them
    // (they were part of the prologue: one more round trip before the first entry for every group with a long row)
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (live[k] && longw[k]) {
            const int64_t gs = g0 + k * gstride;
            const int long_slot = a.long_prefix[gs] + __popcll(longw[k] & ((1ull << lane) - 1ull));
            if (is_long[k]) {
                t_has[k] = a.tl_has[long_slot] != 0;
                t_acc[k] = acc_from_stored<W>(((const W *)a.tl_val)[long_slot], a.tl_ord != 0);
            }
        }
    }
    T abl_sum = (T)0;
    if (GRB_TAG_ABL & 1) wins = 0;
    for (int it = 0; it < wins; it++) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int w0 = o0[k] + it * 64;
            if (!(any_active[k] && w0 < o1[k])) continue;  // (wave-uniform)
            W *acc_slots = s_acc[wave][k];
            const uint32_t *off_slots = s_off[wave][k];
            unsigned char *has_slots = s_has[wave][k];
            int creg[EPL];
            T vreg[EPL];
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                creg[i] = cnext[k][i];
                vreg[i] = vnext[k][i];
            }
            const uint32_t tg = tnext[k], dcode = dnext[k];
            // the next window's entries are requested before this window's gathers
            if (w0 + 64 < o1[k]) load_unit(w0 + 64 + lane, w0 + 64 + lane < o1[k], cnext[k], vnext[k], dnext[k], tnext[k]);
            int rk[EPL], cc[EPL];
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                rk[i] = (int)((tg >> (8 * i)) & 0xffu);
                cc[i] = creg[i] | (int)off_slots[rk[i]];  // (-1: padding or a masked-out row -- the gather reads nothing)
                if (GRB_TAG_ABL & 2) cc[i] |= (creg[i] | rk[i]) >= 0 ? -1 : -1;
                if ((GRB_TAG_ABL & 128) && cc[i] >= (1 << 19)) cc[i] &= (1 << 19) - 1;  // (every gather inside the first 2 MiB of the image: all L2 hits)
            }
            // ---- gathers: presence words, then values -- EPL independent random accesses in flight per lane --------------
            bool xp[EPL];
            T xv[EPL];
            bool pv_done = false;
            if constexpr (std::is_same<T, bool>::value) {
                if (a.u_pv) {  // presence and value from one word
                    if constexpr (HEAD) {  // (the word from the LDS head when it is there: the texture path gets an out-of-range address)
                        uint32_t pw[EPL], hw[EPL];
#pragma unroll
                        for (int i = 0; i < EPL; i++) pw[i] = buf_load<uint32_t>(xpv_rs, (unsigned)(cc[i] >> 4) < (unsigned)HEAD_WORDS ? 0xfffffff8u : (unsigned)(cc[i] >> 4) * 4u);
#pragma unroll
                        for (int i = 0; i < EPL; i++) hw[i] = s_head[(unsigned)(cc[i] >> 4) < (unsigned)HEAD_WORDS ? (cc[i] >> 4) : 0];
#pragma unroll
                        for (int i = 0; i < EPL; i++) {
                            const uint32_t w32 = (unsigned)(cc[i] >> 4) < (unsigned)HEAD_WORDS ? hw[i] : pw[i];
                            const int sh = (cc[i] & 15) * 2;
                            xp[i] = (w32 >> sh) & 1u;
                            xv[i] = (w32 >> (sh + 1)) & 1u;
                        }
                    } else {
                        bool_pv_gather<EPL>(xpv_rs, cc, xp, xv);
                    }
                    pv_done = true;
                }
            }
            if (pv_done) {
            } else if (a.u_full) {
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
            } else if (need_uval) {
                if constexpr (std::is_same<T, bool>::value) {
                    uint32_t vw[EPL];
#pragma unroll
                    for (int i = 0; i < EPL; i++) vw[i] = buf_load<uint32_t>(xvbits_rs, xp[i] ? (unsigned)(cc[i] >> 5) * 4u : 0xfffffff8u);
#pragma unroll
                    for (int i = 0; i < EPL; i++) xv[i] = (vw[i] >> (cc[i] & 31)) & 1u;
                } else if (a.u_full) {
                    if constexpr (HEAD) {  // (codes below HEAD_SLOTS: the value from LDS, no line for the texture path; -1 is above as unsigned)
                        T hx[EPL];
#pragma unroll
                        for (int i = 0; i < EPL; i++) xv[i] = buf_gather<T>(xval_rs, (unsigned)cc[i] < (unsigned)HEAD_SLOTS ? 0xfffffff8u : (unsigned)cc[i] * (unsigned)sizeof(T));
#pragma unroll
                        for (int i = 0; i < EPL; i++) hx[i] = ((const T *)s_head)[(unsigned)cc[i] < (unsigned)HEAD_SLOTS ? cc[i] : 0];
#pragma unroll
                        for (int i = 0; i < EPL; i++) xv[i] = (unsigned)cc[i] < (unsigned)HEAD_SLOTS ? hx[i] : xv[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < EPL; i++) xv[i] = buf_gather<T>(xval_rs, (unsigned)cc[i] * (unsigned)sizeof(T));  // (-1: out of range)
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < EPL; i++) xv[i] = buf_gather<T>(xval_rs, xp[i] ? (unsigned)cc[i] * (unsigned)sizeof(T) : 0xfffffff8u);
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) xv[i] = (T)0;
            }
            // ---- every product to its row's accumulator: one native LDS atomic; an absent product goes to the padding slot ----------
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                T av = need_aval ? vreg[i] : (T)0;
                if constexpr (sizeof(T) == 4) {
                    if (a.vdict && stage_vals) av = __builtin_bit_cast(T, s_dict[(dcode >> (8 * i)) & 0xffu]);
                }
                const T prod = apply_binop<T>(mult, av, xv[i]);
                // (full operand: the product of an entry that gathered nothing -- padding, a masked-out row -- lands in a slot that is
                //  never read: the padding slot (tag 64), or the accumulator of a row the write rule ignores)
                // (operand not full: an entry without a present partner does nothing -- NOT redirected to the padding slot: with a
                //  frontier of density 0.3 two thirds of a wavefront's atomics would hit that one LDS address and serialise)
                const int kk = rk[i];
                if (GRB_TAG_ABL & 4) abl_sum = apply_binop<T>(monoid, abl_sum, prod) + (T)(kk & 1);
                else if (a.u_full || xp[i]) {
                    if (monoid == OP_ANY) acc_slots[kk] = (W)prod;
                    else lds_combine<W>(&acc_slots[kk], (W)prod, monoid);
                    if (!a.u_full) has_slots[kk] = 1;
                }
            }
        }
    }
    if ((GRB_TAG_ABL & 4) && abl_sum == (T)12345) s_acc[wave][0][lane] = (W)abl_sum;  // (keeps the products alive)
    wave_sync();

    // ---- write rule for my rows; the wavefront owns the whole presence word of each group -----------------------------------
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (!live[k]) continue;  // (wave-uniform)
        const int64_t g = g0 + k * gstride;
        const int64_t row = (g << 6) + lane;
        if (!is_long[k]) {
            // (full operand: an active row has a product as soon as it has an entry)
            t_has[k] = a.u_full ? (bool)((nonempty[k] >> lane) & 1ull) : s_has[wave][k][lane] != 0;
            t_acc[k] = s_acc[wave][k][lane];
        } else if (a.long_tails) {
            // (round 6: the group also holds the long row's COLD entries; the strips' accumulator -- read above -- is merged into their fold.
            //  A masked-out row gathered nothing: its result is never used)
            const bool s_h = a.u_full ? (bool)((nonempty[k] >> lane) & 1ull) : s_has[wave][k][lane] != 0;
            const W s_a = s_acc[wave][k][lane];
            if (monoid == OP_ANY) t_acc[k] = (s_h && act_me[k] && any_active[k]) ? s_a : t_acc[k];
            else if (any_active[k]) t_acc[k] = apply_binop<W>(monoid, s_a, t_acc[k]);
            t_has[k] = t_has[k] || (s_h && any_active[k]);
        }
        // (an operand image with the absorbing value under its absent entries: the product exists iff the accumulator moved)
        if (a.has_by_value) t_has[k] = t_has[k] && !same_bits<W>(t_acc[k], monoid_identity<T, W>(monoid));
        bool new_has = false;
        if (GRB_TAG_ABL & 8) new_has = in[k] && (act_me[k] ? (t_has[k] || old_has[k]) && from_acc<T, W>(t_acc[k]) != (T)77 : old_has[k]);
        else if (in[k]) new_has = write_rule_row<T>(a, row, act_me[k], old_has[k], old_val[k], t_has[k], from_acc<T, W>(t_acc[k]));
        const unsigned long long nb = __ballot(in[k] && new_has);
        if (lane == 0) a.w_new_bits[g] = nb;
    }
    }  // (the wavefront's groups)
}

// The rows behind the last non-empty one of a matrix in its popularity order have no product: for them the write rule is a function of
// the presence words alone -- C<M, replace> = accum(C, nothing): an entry survives where the mask does not admit its row (unless replace)
// or where an accumulator keeps it.  (accum && !replace: nothing changes and this is not launched.)
__global__ void k_rows_tail(const PullArgs a, int64_t g_first)
{
    const int64_t g = g_first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ngroups = (a.m + 63) >> 6;
    if (g >= ngroups) return;
    const uint64_t actw = a.has_mask ? (a.m_comp ? ~a.m_bits[g] : a.m_bits[g]) : ~0ull;
    const uint64_t oldw = a.w_old_bits[g];
    uint64_t neww;
    if (a.accum >= 0) neww = a.replace ? (oldw & actw) : oldw;
    else neww = a.replace ? 0ull : (oldw & ~actw);
    a.w_new_bits[g] = neww;
}
