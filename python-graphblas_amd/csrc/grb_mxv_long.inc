// Part of grb_mxv.hip (included there, inside namespace grb): the long rows of a split matrix -- k_mxv_long (chunks), k_mxv_long_grp (class-partitioned items), per-call compaction and initialisation
__device__ __forceinline__ void wave_sync()
{
    // LDS operations of one wavefront execute in order; this only stops the compiler from moving them across
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------------
// Long rows (>= split_min_len entries; on power-law graphs 3 % of the rows hold 80 % of the entries): one wavefront
// per chunk of at most PULL_CHUNK entries of ONE row.  No row bookkeeping at all -- 8 consecutive entries per lane
// (16-byte buffer loads), 8 gathers in flight, a lane-local fold, one wavefront reduction by __shfl_down, one
// atomic into the row's accumulator.  A masked-out row returns before touching its entries.
// ---------------------------------------------------------------------------------------------------
constexpr int PULL_CHUNK = 2048;
constexpr int LONG_BLOCK = 1024;        // 16 wavefronts; one persistent workgroup per CU
constexpr int LONG_LDS_WORDS = 39936;   // 156 KiB of the 160 KiB: the head of the x image ([hot | u]: hottest columns first)

template <typename T, int MONOID_CT, int MULT_CT, int LDS_WORDS>
__global__ __launch_bounds__(LONG_BLOCK) void k_mxv_long(const PullArgs a)
{
    using W = typename Widen<T>::type;
    constexpr int EPL = 8;  // entries per lane per step
    // Every gather that misses L1 moves a 128-byte line from L2 for 4 useful bytes; the workgroup therefore keeps
    // the head of the x image in LDS for its whole life (hot-coded columns: the most referenced come first --
    // 32 Ki fp32 entries receive ~45 % of the references of an R-MAT graph; BOOL values are bit-packed: 1 Mi entries).
    __shared__ uint32_t s_x[LDS_WORDS];
    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const int lane = threadIdx.x & 63;
    const bool need_aval = a.need_aval != 0, need_uval = a.need_uval != 0;
    const bool stage_vals = need_aval && !a.a_iso;
    const T *aval = (const T *)a.aval;
    const T iso_v = (a.a_iso && need_aval) ? aval[0] : (T)0;
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t xbits_rs = make_rsrc(a.u_bits, a.u_full ? 0 : ((a.x_len + 63) >> 6) * 8);
    const __amdgpu_buffer_rsrc_t xvbits_rs = make_rsrc(a.u_valbits, a.u_valbits ? ((a.x_len + 63) >> 6) * 8 : 0);
    const __amdgpu_buffer_rsrc_t xpv_rs = make_rsrc(a.u_pv, a.u_pv ? ((a.x_len + 15) >> 4) * 4 : 0);
    constexpr bool IS_BOOL = std::is_same<T, bool>::value;
    // entries of the image resident in LDS
    constexpr int64_t LDS_CAP = IS_BOOL ? (int64_t)LDS_WORDS * 32 : (int64_t)LDS_WORDS * 4 / (int64_t)(sizeof(T) < 4 ? 4 : sizeof(T));
    const int lds_n = (need_uval && !(GRB_DBG(a, 4096))) ? (int)(a.x_len < LDS_CAP ? a.x_len : LDS_CAP) : 0;  // (debug flag 4096: no LDS residency)
    if (need_uval) {
        if constexpr (IS_BOOL) {
            lds_fill<LONG_BLOCK>(s_x, (lds_n + 31) >> 5, [&](int k) { return buf_load<uint32_t>(xvbits_rs, (unsigned)k * 4u); });
        } else if constexpr (sizeof(T) == 8) {
            lds_fill<LONG_BLOCK>((T *)s_x, lds_n, [&](int k) { return buf_load<T>(xval_rs, (unsigned)k * 8u); });
        } else if constexpr (sizeof(T) == 4) {
            lds_fill<LONG_BLOCK>(s_x, lds_n, [&](int k) { return __builtin_bit_cast(uint32_t, buf_load<T>(xval_rs, (unsigned)k * 4u)); });
        } else {  // 1- and 2-byte values: one per 32-bit LDS word
            lds_fill<LONG_BLOCK>(s_x, lds_n, [&](int k) { return (uint32_t)buf_load<T>(xval_rs, (unsigned)k * (unsigned)sizeof(T)); });
        }
    }
    __syncthreads();

    const int64_t wave0 = (int64_t)blockIdx.x * (LONG_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (LONG_BLOCK / 64);
    constexpr int STEP = 64 * EPL;
    const bool nt = (GRB_DBG(a, 64)) != 0;  // diagnostic: non-temporal entry loads
    // The wavefront owns chunks wave0, wave0 + nwaves, ...  Their descriptors (slot -> row -> mask bit -> start, len: a
    // chain of dependent loads) are fetched once, 64 chunks at a time with one chunk per lane, and broadcast from the
    // lanes as needed; masked-out chunks drop out of the ballot and nothing of their rows is read.
    for (int64_t first = wave0; first < a.n_chunks; first += 64 * nwaves) {
        const int64_t my_chunk = first + (int64_t)lane * nwaves;
        int m_len = 0, m_slot = 0, m_start_lo = 0, m_start_hi = 0;
        if (my_chunk < a.n_chunks) {
            m_slot = a.chunk_slot[my_chunk];
            bool act = true;
            if (a.has_mask) {
                const int64_t row = a.long_rows[m_slot];
                act = (((const uint32_t *)a.m_bits)[row >> 5] >> (row & 31)) & 1u;
                if (a.m_comp) act = !act;
            }
            if (act) {
                const int64_t st = a.chunk_start[my_chunk];
                m_start_lo = (int)(uint32_t)st;
                m_start_hi = (int)(st >> 32);
                m_len = a.chunk_len[my_chunk];
            }
        }
        unsigned long long todo = __ballot(m_len > 0);
        if (!todo) continue;
        // software pipeline over the steps (64 * EPL entries) of the active chunks: the entries of step s+1 are in
        // flight while the gathers of step s are
        int cur = __ffsll(todo) - 1;
        todo &= todo - 1;
        int base = 0;
        int c_len = __builtin_amdgcn_readfirstlane(__shfl(m_len, cur));
        int c_slot = __builtin_amdgcn_readfirstlane(__shfl(m_slot, cur));
        int64_t c_start = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(__shfl(m_start_hi, cur)) << 32) |
                                    (uint32_t)__builtin_amdgcn_readfirstlane(__shfl(m_start_lo, cur)));
        int cc_n[EPL];
        T av_n[EPL];
        {
            const __amdgpu_buffer_rsrc_t crs = make_rsrc(a.col + c_start, (int64_t)c_len * 4);
            const __amdgpu_buffer_rsrc_t vrs = make_rsrc(aval + (a.a_iso ? 0 : c_start), stage_vals ? (int64_t)c_len * (int64_t)sizeof(T) : 0);
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const int e = i * 64 + lane;  // coalesced 4-byte loads; entries past the end of the chunk read 0 and are discarded
                const int c = nt ? buf_load_nt<int>(crs, (unsigned)e * 4u) : buf_load<int>(crs, (unsigned)e * 4u);
                cc_n[i] = (e < c_len) ? c : -1;
                av_n[i] = stage_vals ? (nt ? buf_load_nt<T>(vrs, (unsigned)e * (unsigned)sizeof(T)) : buf_load<T>(vrs, (unsigned)e * (unsigned)sizeof(T))) : iso_v;
            }
        }
        T acc = (T)0;
        bool has = false;
        while (true) {
            int cc[EPL];
            T av[EPL];
#pragma unroll
            for (int i = 0; i < EPL; i++) { cc[i] = cc_n[i]; av[i] = av_n[i]; }
            if (GRB_DBG(a, 16384 | 32768)) {  // diagnostic: fold every gather into the first 2^19 / 2^15 entries of the image
                const int gmask = (GRB_DBG(a, 16384)) ? 0x7ffff : 0x7fff;
#pragma unroll
                for (int i = 0; i < EPL; i++) cc[i] = cc[i] >= 0 ? (cc[i] & gmask) : -1;
            }
            // where the next step lies
            int n_cur = cur, n_base = base + STEP, n_len = c_len, n_slot = c_slot;
            int64_t n_start = c_start;
            bool more = true;
            if (n_base >= c_len) {
                n_base = 0;
                if (todo) {
                    n_cur = __ffsll(todo) - 1;
                    todo &= todo - 1;
                    n_len = __builtin_amdgcn_readfirstlane(__shfl(m_len, n_cur));
                    n_slot = __builtin_amdgcn_readfirstlane(__shfl(m_slot, n_cur));
                    n_start = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(__shfl(m_start_hi, n_cur)) << 32) |
                                        (uint32_t)__builtin_amdgcn_readfirstlane(__shfl(m_start_lo, n_cur)));
                } else {
                    more = false;
                    n_len = 0;
                }
            }
            // gathers of this step
            bool xp[EPL];
            T xg[EPL];
            if (a.u_full) {
#pragma unroll
                for (int i = 0; i < EPL; i++) xp[i] = cc[i] >= 0;
            } else {
                uint32_t bw[EPL];
#pragma unroll
                for (int i = 0; i < EPL; i++) bw[i] = buf_load<uint32_t>(xbits_rs, (unsigned)(cc[i] >> 5) * 4u);
#pragma unroll
                for (int i = 0; i < EPL; i++) xp[i] = (bw[i] >> (cc[i] & 31)) & 1u;
            }
            uint32_t vw[EPL];
            if (need_uval && !(GRB_DBG(a, 8192))) {
                // resident entries come from LDS; the others from the image in HBM (an out-of-range offset reads nothing)
                if constexpr (IS_BOOL) {
#pragma unroll
                    for (int i = 0; i < EPL; i++) vw[i] = buf_load<uint32_t>(xvbits_rs, (xp[i] && cc[i] >= lds_n) ? (unsigned)(cc[i] >> 5) * 4u : 0xfffffff8u);
                } else {
#pragma unroll
                    for (int i = 0; i < EPL; i++) xg[i] = buf_load<T>(xval_rs, (xp[i] && cc[i] >= lds_n) ? (unsigned)cc[i] * (unsigned)sizeof(T) : 0xfffffff8u);
                }
            }
            // entries of the next step (issued behind the gathers, consumed one iteration later)
            {
                const __amdgpu_buffer_rsrc_t crs = make_rsrc(a.col + n_start, (int64_t)n_len * 4);
                const __amdgpu_buffer_rsrc_t vrs = make_rsrc(aval + (a.a_iso ? 0 : n_start), stage_vals ? (int64_t)n_len * (int64_t)sizeof(T) : 0);
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    const int e = n_base + i * 64 + lane;
                    const int c = nt ? buf_load_nt<int>(crs, (unsigned)e * 4u) : buf_load<int>(crs, (unsigned)e * 4u);
                    cc_n[i] = (e < n_len) ? c : -1;
                    av_n[i] = stage_vals ? (nt ? buf_load_nt<T>(vrs, (unsigned)e * (unsigned)sizeof(T)) : buf_load<T>(vrs, (unsigned)e * (unsigned)sizeof(T))) : iso_v;
                }
            }
            T xv[EPL];
            if (need_uval && !(GRB_DBG(a, 8192))) {
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    const bool in_lds = xp[i] && cc[i] < lds_n;
                    if constexpr (IS_BOOL) {
                        const uint32_t wv = in_lds ? s_x[cc[i] >> 5] : vw[i];
                        xv[i] = (wv >> (cc[i] & 31)) & 1u;
                    } else {
                        const int li = in_lds ? cc[i] : 0;
                        T xl;
                        if constexpr (sizeof(T) == 8) xl = ((const T *)s_x)[li];
                        else if constexpr (sizeof(T) == 4) xl = __builtin_bit_cast(T, s_x[li]);
                        else xl = (T)s_x[li];
                        xv[i] = in_lds ? xl : xg[i];
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) xv[i] = (T)(need_uval ? 1 : 0);
            }
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const T prod = apply_binop<T>(mult, need_aval ? av[i] : (T)0, xv[i]);
                acc = xp[i] ? (has ? apply_binop<T>(monoid, acc, prod) : prod) : acc;
                has = has || xp[i];
            }
            if (n_cur != cur || !more) {
                // the chunk is complete: wavefront reduction (value + presence), one atomic into the row's accumulator
                int hasi = has ? 1 : 0;
                for (int off = 32; off > 0; off >>= 1) {
                    const T o = __shfl_down(acc, off);
                    const int oh = __shfl_down(hasi, off);
                    if (oh) {
                        acc = hasi ? apply_binop<T>(monoid, acc, o) : o;
                        hasi = 1;
                    }
                }
                if (lane == 0 && hasi) {
                    W *tl = (W *)a.tl_val;
                    if (monoid == OP_ANY) tl[c_slot] = (W)acc;
                    else atomic_combine<W>(&tl[c_slot], (W)acc, monoid);
                    a.tl_has[c_slot] = 1;
                }
                acc = (T)0;
                has = false;
            }
            if (!more) break;
            cur = n_cur; base = n_base; c_len = n_len; c_slot = n_slot; c_start = n_start;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Long rows, class-partitioned.  The gathers of the long rows dominate the SpMV, and a gather costs nothing when it
// hits LDS, one L2 request when it hits L2 and ~3x that when it misses.  So the entries of the long rows are stored a
// second time grouped by COLUMN CLASS = (code >> 5) & 7 (32 consecutive codes = one 128-byte line of 4-byte values),
// and a workgroup only ever works on the class of its own index: blocks are dealt round-robin to the 8 XCDs, so the
// L2 of an XCD sees one eighth of the x image (its hot part fits), and the 156 KiB of LDS a workgroup spends on the
// image head hold the 39 Ki hottest codes OF ITS CLASS -- 312 Ki distinct codes across the chip instead of 39 Ki.
// (Placement only changes speed: any workgroup computes any class correctly.)
//
// The unit of work is an ITEM: at most LONG_ITEM entries of one (class, long row), stored contiguously, starts aligned
// to 4 entries, items of a class sorted by falling length.  16 lanes take one item (four items per wavefront, of about
// the same length): 8 consecutive entries per lane and step straight into registers, gathers, a fold in registers,
// one butterfly reduction over the 16 lanes and ONE atomic into the row's accumulator.  With a mask the admitted items
// are compacted per call (k_long_compact), so masked-out rows are neither streamed nor scheduled.
// ---------------------------------------------------------------------------------------------------
constexpr int LONG_ITEM = 1024;
// codes the image head in LDS can hold per class x 8 classes: BOOL operands are bit-packed (32 values per word, or 16
// (presence, value) pairs per word when u is not full -- the limit is set by the latter), the others take one LDS slot of
// max(4, sizeof) bytes per code
constexpr int64_t long_lds_codes(int type_size_bytes, bool is_bool, int lds_words)
{
    return is_bool ? (int64_t)lds_words * 128 : ((int64_t)lds_words * 4 / (type_size_bytes < 4 ? 4 : type_size_bytes)) * 8;
}
// A column code of the class-partitioned copy as the kernel reads it: c itself when it is gathered from the image, or
// -2 - slot when it is resident in LDS (slot = ((c >> 8) << 5) | (c & 31) within its class; for BOOL the bit slot & 31
// of LDS word slot >> 5); -1 = padding.  A negative code times the value size is out of range for the buffer gather.
__device__ __forceinline__ int long_tcode(int c, int lds_lim) { return c < lds_lim ? -2 - (((c >> 8) << 5) | (c & 31)) : c; }
// ... with ncls classes, for the class strips.  The lines (32 codes) of the hot table are dealt to the classes BOUSTROPHEDON -- group g
// of ncls consecutive lines goes 0, 1, .., ncls - 1 when g is even and ncls - 1, .., 0 when it is odd: codes are ranked by falling
// popularity, so with class = line mod ncls class 0 got the hottest line of EVERY group (R-MAT scale 24: 9 % more chunks than the
// mean, 12 % more than the last class -- and the slowest class of a persistent kernel sets its time).
__device__ __forceinline__ unsigned strip_cls_of_line(unsigned line, unsigned ncls)
{
    const unsigned g = line / ncls, p = line % ncls;
    return (g & 1u) ? ncls - 1u - p : p;
}
// the line that is slot-line g of class cls
__device__ __forceinline__ unsigned strip_line_of(unsigned g, unsigned cls, unsigned ncls) { return g * ncls + ((g & 1u) ? ncls - 1u - cls : cls); }
__device__ __forceinline__ int long_tcode_n(int c, int lds_lim, int ncls) { return c < lds_lim ? -2 - ((((c >> 5) / ncls) << 5) | (c & 31)) : c; }

// LOR (mode 1) / LAND (mode 2) accumulators of BOOL semirings (kept as 0 / 1 words): has the row reached its terminal value?
template <typename W>
__device__ __forceinline__ bool long_terminal(const W *p, int mode)
{
    if constexpr (std::is_integral<W>::value) {
        const W t = __atomic_load_n(p, __ATOMIC_RELAXED);
        return mode == 1 ? (t != (W)0) : (t == (W)0);
    } else {
        return false;
    }
}

template <typename T, int MONOID_CT, int MULT_CT, int LDS_WORDS>
__global__ __launch_bounds__(LONG_BLOCK) void k_mxv_long_grp(const PullArgs a)
{
    using W = typename Widen<T>::type;
    constexpr int EPL = 8, GL = 16, STEP = GL * EPL, NWV = LONG_BLOCK / 64;
    __shared__ uint32_t s_x[LDS_WORDS];
    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane >> 4, gl = lane & 15;
    const int cls = blockIdx.x & 7;
    const bool need_aval = a.need_aval != 0, need_uval = a.need_uval != 0;
    const bool stage_vals = need_aval && !a.a_iso;
    const T *lval = (const T *)a.lval;
    const T iso_v = (a.a_iso && need_aval) ? ((const T *)a.aval)[0] : (T)0;
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t xbits_rs = make_rsrc(a.u_bits, a.u_full ? 0 : ((a.x_len + 63) >> 6) * 8);
    const __amdgpu_buffer_rsrc_t xvbits_rs = make_rsrc(a.u_valbits, a.u_valbits ? ((a.x_len + 63) >> 6) * 8 : 0);
    const __amdgpu_buffer_rsrc_t xpv_rs = make_rsrc(a.u_pv, a.u_pv ? ((a.x_len + 15) >> 4) * 4 : 0);
    constexpr bool IS_BOOL = std::is_same<T, bool>::value;
    // LDS residency of my class (the entries carry pre-translated codes, see long_tcode)
    constexpr int LDS_SLOTS = IS_BOOL ? LDS_WORDS : (int)((int64_t)LDS_WORDS * 4 / (int64_t)(sizeof(T) < 4 ? 4 : sizeof(T)));
    const bool use_lds = need_uval && a.cls_lds_lim > 0;
    if (use_lds) {
        if constexpr (IS_BOOL) {
            if (a.u_pv) {  // LDS word w = (presence, value) pairs of my class's slots 16 w .. 16 w + 15 = 16 consecutive codes
                lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int w) {
                    const unsigned s0 = (unsigned)w << 4;
                    const unsigned c0 = ((s0 >> 5) << 8) | ((unsigned)cls << 5) | (s0 & 31u);
                    return buf_load<uint32_t>(xpv_rs, (c0 >> 4) * 4u);
                });
            } else {
                lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int w) { return buf_load<uint32_t>(xvbits_rs, (unsigned)((w << 3) | cls) * 4u); });
            }
        } else {
            auto load_x = [&](int k) {  // (past the image: 0, never looked up)
                const unsigned c = ((unsigned)(k >> 5) << 8) | ((unsigned)cls << 5) | (unsigned)(k & 31);
                return buf_load<T>(xval_rs, c * (unsigned)sizeof(T));
            };
            if constexpr (sizeof(T) == 8) lds_fill<LONG_BLOCK>((T *)s_x, LDS_SLOTS, load_x);
            else if constexpr (sizeof(T) == 4) lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int k) { return __builtin_bit_cast(uint32_t, load_x(k)); });
            else lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int k) { return (uint32_t)load_x(k); });
        }
    }
    __syncthreads();

    // my class's items: [ib, ib + n_it) of the field arrays (with a mask: of their compacted copy)
    const int64_t ib = a.class_off ? a.class_off[cls] : a.item_begin[cls];
    const int64_t n_it = (a.class_off ? a.class_off[cls + 1] : a.item_begin[cls + 1]) - ib;
    const int64_t nblk = ((int64_t)gridDim.x - cls + 7) >> 3;  // workgroups of my class
    const int64_t wv = (int64_t)(blockIdx.x >> 3) * NWV + wave, nwv = nblk * NWV;
    W *tl = (W *)a.tl_val;

    // Software pipeline over the steps (4 items x 128 entries) of my quads: the item fields of quad q+1 and the entries of
    // the NEXT step (of this quad or the first of the next one) are requested before the gathers of the current step, so a
    // step waits for one memory round trip (its gathers), not three.
    int64_t f_st = 0, n_st = 0;
    int f_len = 0, f_slot = 0, n_len = 0, n_slot = 0;
    // LOR / LAND stop at true / false, ANY at the first product (the bottom-up BFS step: a vertex stops looking once it has a
    // parent); 0 = the monoid has no terminal value worth testing
    int term_mode = 0;
    if constexpr (IS_BOOL) {
        if (monoid == OP_LOR) term_mode = 1;
        else if (monoid == OP_LAND) term_mode = 2;
    }
    if (monoid == OP_ANY && !a.long_has_known) term_mode = 3;
    if (GRB_DBG(a, 262144)) term_mode = 0;  // (diagnostic: no early exit)
#define GRP_ITEM_LOADS(Q)                                                  \
    do {                                                                   \
        const int64_t k_ = (Q) * 4 + grp;                                  \
        n_st = 0; n_len = 0; n_slot = 0;                                   \
        if (k_ < n_it) {                                                   \
            const int64_t it_ = ib + k_;                                   \
            n_st = a.it_start[it_];                                        \
            n_len = a.it_len[it_];                                         \
            n_slot = a.it_slot[it_];                                       \
            /* terminal monoids: an item of a row whose accumulator can no longer change is dropped before its entries    \
               are requested (a stale "not yet" only costs the work) */                                                   \
            if (term_mode == 1 || term_mode == 2) {                        \
                if (long_terminal<W>(&tl[n_slot], term_mode)) n_len = 0;   \
            } else if (term_mode == 3) {                                   \
                if (__atomic_load_n(&a.tl_has[n_slot], __ATOMIC_RELAXED)) n_len = 0; \
            }                                                              \
        }                                                                  \
    } while (0)
    int n_c[EPL];
    T n_v[EPL];
    // (a full operand whose values the multiply does not read -- the row reductions -- needs no column code at all)
    const bool no_cols = a.u_full && !need_uval && !(GRB_DBG(a, 524288));
#define GRP_ENTRY_LOADS(ST, BASE)                                                                   \
    do {                                                                                            \
        const int32_t *cp_ = a.lcol + ((GRB_DBG(a, 2)) ? (int64_t)(lane * 8) : (ST) + gl * EPL + (BASE)); /* (2: diagnostic, no streaming) */ \
        if (no_cols) {                                                                              \
            _Pragma("unroll") for (int i_ = 0; i_ < EPL; i_++) n_c[i_] = 0;                         \
        } else {                                                                                    \
            _Pragma("unroll") for (int q_ = 0; q_ < EPL / 4; q_++) {                                \
                const uint4 c4_ = *(const uint4 *)(cp_ + q_ * 4);                                   \
                n_c[q_ * 4 + 0] = (int)c4_.x; n_c[q_ * 4 + 1] = (int)c4_.y;                         \
                n_c[q_ * 4 + 2] = (int)c4_.z; n_c[q_ * 4 + 3] = (int)c4_.w;                         \
            }                                                                                       \
        }                                                                                           \
        if (stage_vals) {                                                                           \
            const T *vp_ = lval + ((GRB_DBG(a, 2)) ? (int64_t)(lane * 8) : (ST) + gl * EPL + (BASE));   \
            if constexpr (sizeof(T) == 4) {                                                         \
                _Pragma("unroll") for (int q_ = 0; q_ < EPL / 4; q_++) {                            \
                    const uint4 v4_ = *(const uint4 *)(vp_ + q_ * 4);                               \
                    n_v[q_ * 4 + 0] = __builtin_bit_cast(T, v4_.x); n_v[q_ * 4 + 1] = __builtin_bit_cast(T, v4_.y); \
                    n_v[q_ * 4 + 2] = __builtin_bit_cast(T, v4_.z); n_v[q_ * 4 + 3] = __builtin_bit_cast(T, v4_.w); \
                }                                                                                   \
            } else {                                                                                \
                _Pragma("unroll") for (int i_ = 0; i_ < EPL; i_++) n_v[i_] = vp_[i_];               \
            }                                                                                       \
        } else {                                                                                    \
            _Pragma("unroll") for (int i_ = 0; i_ < EPL; i_++) n_v[i_] = iso_v;                     \
        }                                                                                           \
    } while (0)
    const bool ident_fold = monoid == OP_MIN || monoid == OP_MAX || monoid == OP_LOR || monoid == OP_LAND;
    const T ident = from_acc<T, W>(pull_seed<T, W>(a, monoid));
    int64_t q = wv;
    if (q * 4 >= n_it) return;
    GRP_ITEM_LOADS(q);
    f_st = n_st; f_len = n_len; f_slot = n_slot;
    if ((q + nwv) * 4 < n_it) GRP_ITEM_LOADS(q + nwv);
    GRP_ENTRY_LOADS(f_st, 0);
    for (;;) {
        const int64_t st = f_st;
        const int len = f_len, slot = f_slot;
        const bool more = (q + nwv) * 4 < n_it;
        int maxlen = len;
        {
            const int o1 = __shfl_xor(maxlen, 16);
            maxlen = maxlen > o1 ? maxlen : o1;
            const int o2 = __shfl_xor(maxlen, 32);
            maxlen = maxlen > o2 ? maxlen : o2;
            maxlen = __builtin_amdgcn_readfirstlane(maxlen);
        }
        T acc = ident_fold ? ident : (T)0;
        bool has = false;
        for (int base = 0; base < maxlen; base += STEP) {
            int cc[EPL];
            T av[EPL];
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                cc[i] = (base + gl * EPL + i < len) ? n_c[i] : -1;  // (entries past my item belong to others: discarded)
                av[i] = n_v[i];
            }
            // the next step's entries travel behind this step's gathers
            const bool last_step = base + STEP >= maxlen;
            if (!last_step) {
                GRP_ENTRY_LOADS(st, base + STEP);
            } else if (more) {
                f_st = n_st; f_len = n_len; f_slot = n_slot;  // (requested one quad ago)
                GRP_ENTRY_LOADS(f_st, 0);
                if ((q + 2 * nwv) * 4 < n_it) GRP_ITEM_LOADS(q + 2 * nwv);
            }
            if (GRB_DBG(a, 16384 | 32768)) {  // diagnostic: fold the image gathers into 2^19 / 2^14 entries
                const int gmask = (GRB_DBG(a, 16384)) ? 0x7ffff : 0x3fff;
#pragma unroll
                for (int i = 0; i < EPL; i++) cc[i] = cc[i] >= 0 ? (cc[i] & gmask) : cc[i];
            }
            // cc: >= 0 a code to gather from the image, <= -2 an LDS slot, -1 nothing
            bool xp[EPL];
            T xv[EPL];
            bool pv_done = false;
            if constexpr (IS_BOOL) {
                if (a.u_pv && !(GRB_DBG(a, 8192))) {  // presence and value from one word (LDS for the resident codes)
                    uint32_t pw[EPL];
#pragma unroll
                    for (int i = 0; i < EPL; i++) pw[i] = buf_load<uint32_t>(xpv_rs, cc[i] >= 0 ? (unsigned)(cc[i] >> 4) * 4u : 0xfffffff8u);
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const bool in_lds = cc[i] < -1;
                        const int sl = in_lds ? -2 - cc[i] : cc[i];
                        const uint32_t wv32 = in_lds ? s_x[sl >> 4] : pw[i];
                        const int sh = (sl & 15) * 2;
                        xp[i] = (wv32 >> sh) & 1u;
                        xv[i] = (wv32 >> (sh + 1)) & 1u;
                    }
                    pv_done = true;
                }
            }
            if (pv_done) {
            } else if (a.u_full) {
#pragma unroll
                for (int i = 0; i < EPL; i++) xp[i] = cc[i] != -1;
            } else {
                // presence words come from the image for every entry; a resident code is translated back first (its class is
                // the workgroup's): c = ((slot >> 5) << 8) | (cls << 5) | (slot & 31)
                int co[EPL];
                uint32_t bw[EPL];
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    const int sl = -2 - cc[i];
                    co[i] = cc[i] < -1 ? (((sl >> 5) << 8) | (cls << 5) | (sl & 31)) : cc[i];
                    bw[i] = buf_load<uint32_t>(xbits_rs, (unsigned)(co[i] >> 5) * 4u);  // (-1: out of range, reads 0)
                }
#pragma unroll
                for (int i = 0; i < EPL; i++) xp[i] = (bw[i] >> (co[i] & 31)) & 1u;
            }
            if (pv_done) {
            } else if (need_uval && !(GRB_DBG(a, 8192))) {
                if constexpr (IS_BOOL) {
                    uint32_t vw[EPL];
#pragma unroll
                    for (int i = 0; i < EPL; i++) vw[i] = buf_load<uint32_t>(xvbits_rs, xp[i] ? (unsigned)(cc[i] >> 5) * 4u : 0xfffffff8u);
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const bool in_lds = cc[i] < -1;
                        const int sl = in_lds ? -2 - cc[i] : 0;
                        const uint32_t wv32 = in_lds ? s_x[sl >> 5] : vw[i];
                        const int bit = in_lds ? (sl & 31) : (cc[i] & 31);
                        xv[i] = (wv32 >> bit) & 1u;
                    }
                } else {
                    T xg[EPL];
#pragma unroll
                    for (int i = 0; i < EPL; i++) xg[i] = buf_gather<T>(xval_rs, (unsigned)cc[i] * (unsigned)sizeof(T));  // (negative: out of range)
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const bool in_lds = cc[i] < -1;
                        const int li = in_lds ? -2 - cc[i] : 0;
                        T xl;
                        if constexpr (sizeof(T) == 8) xl = ((const T *)s_x)[li];
                        else if constexpr (sizeof(T) == 4) xl = __builtin_bit_cast(T, s_x[li]);
                        else xl = (T)s_x[li];
                        xv[i] = in_lds ? xl : xg[i];
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) xv[i] = (T)(need_uval ? 1 : 0);
            }
            if (ident_fold) {
                // monoids whose identity absorbs "nothing here" exactly: no presence-dependent select in the chain
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    const T prod = apply_binop<T>(mult, need_aval ? av[i] : (T)0, xv[i]);
                    acc = apply_binop<T>(monoid, acc, xp[i] ? prod : ident);
                    has = has || xp[i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    const T prod = apply_binop<T>(mult, need_aval ? av[i] : (T)0, xv[i]);
                    acc = xp[i] ? (has ? apply_binop<T>(monoid, acc, prod) : prod) : acc;
                    has = has || xp[i];
                }
            }
            // terminal monoids: when each of the quad's four items is exhausted or holds the terminal value in one of its
            // lanes, the remaining steps cannot change anything -- hand over to the next quad now
            if (term_mode != 0 && !last_step) {
                bool lane_done = has;  // ANY: any product
                if (term_mode == 1) lane_done = has && (acc != (T)0);
                else if (term_mode == 2) lane_done = has && (acc == (T)0);
                const unsigned long long done = __ballot(lane_done);
                const unsigned long long spent = __ballot(base + STEP >= len);  // (uniform within a 16-lane group)
                bool all_done = true;
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++) all_done = all_done && ((((done >> (16 * g4)) & 0xffffull) != 0) || ((spent >> (16 * g4)) & 1ull));
                if (all_done) {
                    if (more) {
                        f_st = n_st; f_len = n_len; f_slot = n_slot;
                        GRP_ENTRY_LOADS(f_st, 0);
                        if ((q + 2 * nwv) * 4 < n_it) GRP_ITEM_LOADS(q + 2 * nwv);
                    }
                    break;
                }
            }
        }
        // butterfly over my 16 lanes (value + presence), one atomic per item
        int hasi = (has && !(GRB_DBG(a, 4))) ? 1 : 0;
#pragma unroll
        for (int off = GL / 2; off > 0; off >>= 1) {
            const T o = __shfl_xor(acc, off);
            const int oh = __shfl_xor(hasi, off);
            if (oh) {
                acc = hasi ? apply_binop<T>(monoid, acc, o) : o;
                hasi = 1;
            }
        }
        if (gl == 0 && hasi) {
            if (monoid == OP_ANY) tl[slot] = (W)acc;
            else atomic_combine<W>(&tl[slot], (W)acc, monoid);
            if (!a.long_has_known) a.tl_has[slot] = 1;
        }
        if (!more) break;
        if (maxlen == 0) {  // every item of the quad was dropped: the hand-over to the next quad did not happen inside the loop
            f_st = n_st; f_len = n_len; f_slot = n_slot;
            GRP_ENTRY_LOADS(f_st, 0);
            if ((q + 2 * nwv) * 4 < n_it) GRP_ITEM_LOADS(q + 2 * nwv);
        }
        q += nwv;
    }
#undef GRP_ENTRY_LOADS
#undef GRP_ITEM_LOADS
}

// per call with a mask: the (start, length, slot) of the admitted items, compacted in order (classes stay contiguous,
// lengths stay sorted): admitted items per 1024-item block -> scan -> write; class_off[c] = admitted items before class c
constexpr int COMPACT_BLOCK = 1024;
__global__ __launch_bounds__(256) void k_long_compact_count(const int32_t *it_slot, int64_t n_items, const uint32_t *long_act, int64_t *block_cnt)
{
    __shared__ int s_cnt[4];
    const int64_t b0 = (int64_t)blockIdx.x * COMPACT_BLOCK;
    int c = 0;
    for (int k = 0; k < COMPACT_BLOCK / 256; k++) {
        const int64_t i = b0 + k * 256 + threadIdx.x;
        bool act = false;
        if (i < n_items) {
            const int s = it_slot[i];
            act = (long_act[s >> 5] >> (s & 31)) & 1u;
        }
        c += __popcll(__ballot(act));
    }
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        block_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (blockIdx.x == gridDim.x - 1) block_cnt[gridDim.x] = 0;
    }
}
__global__ __launch_bounds__(256) void k_long_compact_write(const int32_t *it_slot, int64_t n_items, const uint32_t *long_act,
                                                            const int64_t *block_off, const int64_t *item_begin_dev,
                                                            const int64_t *it_start, const int32_t *it_len, int64_t *act_start,
                                                            int32_t *act_len, int32_t *act_slot, int64_t *class_off)
{
    __shared__ int s_cnt[4];
    const int64_t b0 = (int64_t)blockIdx.x * COMPACT_BLOCK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t off = block_off[blockIdx.x];
    for (int k = 0; k < COMPACT_BLOCK / 256; k++) {
        const int64_t i = b0 + k * 256 + threadIdx.x;
        bool act = false;
        int s = 0;
        if (i < n_items) {
            s = it_slot[i];
            act = (long_act[s >> 5] >> (s & 31)) & 1u;
        }
        const unsigned long long m = __ballot(act);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; w++) before += s_cnt[w];
        const int64_t rank = off + before + __popcll(m & ((1ull << lane) - 1ull));  // admitted items before item i
        if (act) {  // the kernel reads the fields of admitted item number `rank` without an indirection
            act_start[rank] = it_start[i];
            act_len[rank] = it_len[i];
            act_slot[rank] = s;
        }
        if (i < n_items) {
            for (int c = 0; c < 9; c++)
                if (item_begin_dev[c] == i) class_off[c] = rank;
        }
        off += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        for (int c = 0; c < 9; c++)
            if (item_begin_dev[c] >= n_items) class_off[c] = off;  // (classes that begin at the end of the list)
    }
}

// the write rule for one long row (run by the extra workgroups of the seams launch, after both kernels)
template <typename T>
__device__ __forceinline__ void long_row_write(const PullArgs &a, int64_t slot)
{
    using W = typename Widen<T>::type;
    const int64_t row = a.long_rows[slot];
    bool mact = true;
    if (a.has_mask) {
        mact = (((const uint32_t *)a.m_bits)[row >> 5] >> (row & 31)) & 1u;
        if (a.m_comp) mact = !mact;
    }
    const bool old_has = (a.w_old_bits[row >> 6] >> (row & 63)) & 1ull;
    const T old_val = old_has ? ((const T *)a.w_old_val)[row] : (T)0;
    const bool new_has = write_rule_row<T>(a, row, mact, old_has, old_val, a.tl_has[slot] != 0, from_acc<T, W>(acc_from_stored<W>(((const W *)a.tl_val)[slot], a.tl_ord != 0)));
    const unsigned long long bit = 1ull << (row & 63);
    if (new_has) atomicOr((unsigned long long *)&a.w_new_bits[row >> 6], bit);
    else atomicAnd((unsigned long long *)&a.w_new_bits[row >> 6], ~bit);
}

// build: the first K column codes of every long row, k-major (-1 where the row ends)
__global__ void k_probe_fill(const int64_t *rowptr, const int32_t *col, const int32_t *long_rows, int64_t n_long, int K, int32_t *probe)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_long * K) return;
    const int64_t i = t % n_long;
    const int k = (int)(t / n_long);
    const int64_t row = long_rows[i], p = rowptr[row] + k;
    probe[t] = p < rowptr[row + 1] ? col[p] : -1;
}

// per call: long-row accumulators at the monoid identity; bit s of long_act = the mask admits long row s
// The bottom-up probe (round 5): a BOOL product under a terminal monoid -- q<!visited.S, replace> = A lor.land q, the pulled level of a BFS --
// is decided for a row by the FIRST partner that is present and true, and with a frontier that holds a few per cent of the vertices almost
// every long row has one among its first entries.  `probe` holds the first `k` column codes of every long row (k-major: coalesced over the
// rows); a row that finds its partner here gets its result (true) and leaves the list of active rows -- the item kernels never see it.
// `pv` = the operand as (present, present && true) pairs, 16 codes per word (PullArgs::u_pv; `want` = 2: a TRUE partner decides, LOR.LAND),
// or nullptr and `pbits` = presence bits (ANY.PAIR: any present partner decides).
struct LongProbe {
    const int32_t *probe;
    int k;
    const uint32_t *pv;
    const uint32_t *pbits;
    const bool *iso_val;  // LAND with an iso matrix value: a false one makes every product false (no row is ever decided)
    uint32_t want;
};
template <typename W>
__global__ void k_long_init(W *tl_val, unsigned char *tl_has, int64_t n, W identity, const int32_t *long_rows, const uint64_t *m_bits,
                            int has_mask, int m_comp, uint32_t *long_act, int has_known, int ord, unsigned char *act8 = nullptr,
                            unsigned int *rt_counter = nullptr, LongProbe pb = LongProbe{nullptr, 0, nullptr, nullptr, nullptr, 0u})
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && rt_counter) rt_counter[0] = 0u;  // (the hand-out counter of the sorted row tiles, k_mxv_rtile: this call's)
    bool act = false;
    if (i < n) {
        tl_val[i] = acc_to_stored<W>(identity, ord != 0);
        act = true;
        if (has_mask) {
            const int64_t row = long_rows[i];
            act = (m_bits[row >> 6] >> (row & 63)) & 1ull;
            if (m_comp) act = !act;
        }
        // has_known: every entry of an admitted long row meets a present u entry, so the row has a product
        tl_has[i] = (has_known && act) ? 1 : 0;
        if (pb.probe && act && (!pb.iso_val || pb.iso_val[0])) {
            bool decided = false;
            for (int k = 0; k < pb.k && !decided; k++) {
                const int32_t c = pb.probe[(int64_t)k * n + i];
                if (c < 0) break;
                decided = pb.pv ? ((pb.pv[c >> 4] >> ((c & 15) * 2)) & pb.want) != 0u : ((pb.pbits[c >> 5] >> (c & 31)) & 1u) != 0u;
            }
            if (decided) {
                tl_val[i] = acc_to_stored<W>((W)1, ord != 0);
                tl_has[i] = 1;
                act = false;
            }
        }
        if (act8) act8[i] = act ? 1 : 0;
    }
    const unsigned long long b = __ballot(act);
    const int lane = threadIdx.x & 63;
    if (long_act && lane == 0 && (i >> 6) < ((n + 63) >> 6)) {
        long_act[(i >> 6) * 2] = (uint32_t)b;
        long_act[(i >> 6) * 2 + 1] = (uint32_t)(b >> 32);
    }
}
