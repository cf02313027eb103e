// Part of grb_mxv.hip (included there, inside namespace grb): kernel arguments, the write rule of one row, buffer-descriptor loads
constexpr int PULL_BLOCK = 256;

struct CTile;
struct RTile;
struct PullArgs {
    int64_t m, nnz;
    const int64_t *rowptr;
    const int32_t *col;
    const void *aval;
    int a_iso;
    const void *u_val;
    const uint32_t *u_bits;
    int u_full;
    int monoid, mult;
    int need_aval, need_uval;
    const int64_t *tile_row;
    int64_t n_tiles;
    // write rule
    const uint64_t *m_bits;
    int has_mask, m_comp;
    int accum, replace;
    const void *w_old_val;
    const uint64_t *w_old_bits;
    void *w_new_val;
    uint64_t *w_new_bits;
    int fresh;  // w_new_* are different buffers from w_old_*: every kept entry must be copied
    // seams between tiles
    void *carry_val;
    uint8_t *carry_has;
    void *first_val;
    uint8_t *first_has;  // bit0: has a partial, bit1: the tile's first row started in an earlier tile
    int stream_nt;              // 1: the matrix streams of k_mxv_rtile / k_mxv_rtile_bool / k_mxv_ctile are read non-temporal (a matrix much larger than the caches)
    const uint32_t *u_valbits;  // BOOL semirings: values of the u image, bit-packed (bit = present and true)
    const uint32_t *u_pv;       // BOOL semirings, u not full: presence AND value of the image in one word per 16 codes (bits 2k, 2k+1
                                // of word c >> 4 for code c, k = c & 15): one gather per entry instead of two; replaces u_valbits
    int64_t x_len;       // entries of the u image the column codes index ([hot table | u] when a hot table is in use)
    const uint64_t *long_bits;  // rows the merge-path kernel does NOT own (handled by k_mxv_long), or nullptr
    // long-row kernel (k_mxv_long / k_mxv_long_epilogue)
    const int32_t *long_rows;
    const int32_t *chunk_slot;
    const int64_t *chunk_start;
    const int32_t *chunk_len;
    int64_t n_chunks, n_long;
    int64_t n_long_epi;  // long rows whose write rule the seams launch applies (extra workgroups behind the seam ones)
    const int32_t *long_prefix;  // per 64-row group: long rows before it (slot of a long row = prefix + rank in its word)
    // class-partitioned long rows (k_mxv_long_grp)
    const int32_t *lcol;
    const void *lval;
    const int64_t *it_start;
    const int32_t *it_len;
    const int32_t *it_slot;
    int64_t item_begin[9];
    int cls_lds_lim;           // codes below it are LDS-resident in their class's workgroups (and pre-translated in lcol)
    const int64_t *class_off;  // per call with a mask: the admitted items of class c are [class_off[c], class_off[c+1]) of a
                               // compacted copy of the item fields (it_start / it_len / it_slot then point to it); else nullptr
    int has_by_value;          // the operand image is u with the multiply's ABSORBING value under its absent entries (min_plus: +inf; all present
                               // values finite, all matrix values finite: mxv_core checked) and the kernels run as for a full operand: a row
                               // has a product iff its accumulator left the monoid's identity
    int long_has_known;        // u is full: an admitted long row certainly has a product (tl_has is preset, not stored per item)
    uint32_t *long_act;        // per call: bit s = the mask admits long row s
    unsigned char *long_act8;  // ... the same as one byte per long row (k_mxv_hstrip: one byte load indexed by the slot, no bit arithmetic)
    // long rows as flat class strips (k_mxv_strip): lcol / lval hold the strips
    const unsigned long long *strip_start;  // per chunk of 512 entries: bit l = a segment starts at lane l's 8 entries
    const int32_t *strip_slot;        // per lane (8 entries): accumulator slot of its row; -1 = padding behind a class's last segment
    const uint16_t *strip_slot16;     // ... or (round 6) as 16-bit offsets from strip_slot_base[chunk] (0xffff = padding); strip_slot is then nullptr
    const int32_t *strip_slot_base;
    int tl_ord;                       // tl_val holds floating-point MIN / MAX accumulators in ordered-integer form (grb_ops.hpp)
    int64_t strip_nseg;
    int strip_ncls;                   // column classes of the strips (8, 16, 32 or 64)
    int64_t strip_cb[65];             // chunks of class c: [strip_cb[c], strip_cb[c+1])
    // cold entries of a hot / cold layout as tagged tiles (k_mxv_ctile)
    const int32_t *ct_col;
    const void *ct_val;
    const uint16_t *ct_loc;
    const struct CTile *ct_tiles;
    int ct_mode;                      // 0 three streams; 1 packed words (slot << 19 | column - ct_cbase[tile]), tiles of 8192 slots; 2 ... + one-byte value codes;
                                      // 3 (k_mxv_ctile<.., CODEW>) ct_col holds code << 24 | column code, ct_loc the slots as in mode 0, no ct_val
    const int32_t *ct_cbase;          // (ct_mode 1 and 2) per tile: the first column code of its range
    const int32_t *ct_order;          // tile numbers in walking order: XCD x takes ct_order[ct_xoff[x] .. ct_xoff[x + 1]), column range after column range
    int64_t ct_xoff[9];
    const char *hrec;                 // hot strips (k_mxv_strip<..., HOT = 1>): lane records [8 LDS slots | 8 values], see GB_Matrix_opaque::d_hrec
    int hrec_bytes;
    const int32_t *wg_tab;            // (k_mxv_hstrip over both class levels of an ordered matrix in ONE launch) per workgroup: its class in
                                      // strip_cb_dev, its class inside the level, the level's class count, its number among the class's
                                      // workgroups, their count -- dealt by chunk counts; nullptr: class = blockIdx % strip_ncls
    const int64_t *strip_cb_dev;      // ... chunk bounds of all classes of both levels (device copy)
    int64_t strip_chunks;             // ... total chunks
    const void *vdict;                // the value dictionary of dictionary-coded lane records (hrec_bytes == 24), else nullptr
    // short rows as tagged row groups (k_mxv_rows_tag)
    const int32_t *tg_off;
    const int32_t *tg_col;
    const void *tg_val;
    const unsigned char *tg_tag;
    const uint64_t *tg_nonempty;
    int64_t tg_groups;      // groups the kernel covers (0 = all): the rows behind them are empty (a matrix in its popularity order)
    int64_t tg_stride;      // > 0: wavefront j takes groups j, j + stride, j + 2 stride, .. (0: TAG_K consecutive groups)
    // short rows of an ordered matrix as sorted row tiles (k_mxv_rtile)
    const int32_t *rt_col;
    const uint16_t *rt_tag;
    const void *rt_val;
    const struct RTile *rt_tiles;
    const int32_t *rt_order;
    unsigned int *rt_counter;
    int64_t rt_units;
    int rt_ntiles;
    int long_tails;         // 1: long rows may hold entries in the short part too (their cold entries, GB_Matrix_opaque::tails_max_len): the short-row
                            // kernels fold them and merge the long-row accumulator into the result instead of taking it alone
    void *tl_val;           // per long row: product accumulator (identity-initialised)
    unsigned char *tl_has;  // per long row: any product present
    long long *dbg_times;  // GRB_DEBUG_FLAGS & 8: 10 phase timestamps per tile (thread 0)
    int dbg;             // ablation switches (GRB_DEBUG): 1 = no x gathers, 2 = no A staging loads, 4 = no epilogue
};

// rows consumed by the merge path at diagonal `diag` (row-end list vs nnz list)
__global__ void k_tile_table(const int64_t *rowptr, int64_t m, int64_t nnz, int tile, int64_t n_tiles, int64_t *tile_row)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    const int64_t total = m + nnz;
    int64_t diag = t * (int64_t)tile;
    if (diag > total) diag = total;
    int64_t lo = diag - nnz > 0 ? diag - nnz : 0, hi = diag < m ? diag : m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid + 1] <= diag - mid - 1) lo = mid + 1;
        else hi = mid;
    }
    tile_row[t] = lo;
}

// the starting value of a pull kernel's accumulator: acc_seed -- except under the absorbing fill (has_by_value), which only runs on
// finite matrices with bounded operands (no NaN product can reach it) and detects a product as "the accumulator left the identity"
template <typename T, typename W> GRB_HD W pull_seed(const PullArgs &a, int monoid)
{
    return a.has_by_value ? monoid_identity<T, W>(monoid) : acc_seed<T, W>(monoid);
}

template <typename T> __device__ __forceinline__ bool same_bits(T x, T y)
{
    if constexpr (sizeof(T) == 1) return __builtin_bit_cast(uint8_t, x) == __builtin_bit_cast(uint8_t, y);
    else if constexpr (sizeof(T) == 2) return __builtin_bit_cast(uint16_t, x) == __builtin_bit_cast(uint16_t, y);
    else if constexpr (sizeof(T) == 4) return __builtin_bit_cast(uint32_t, x) == __builtin_bit_cast(uint32_t, y);
    else return __builtin_bit_cast(uint64_t, x) == __builtin_bit_cast(uint64_t, y);
}
// The write rule for one output row.  Returns the new presence; stores the value when present.
// `old_val` is w_old[row] (only read by the caller when old_has and (accum or fresh)).
template <typename T>
__device__ __forceinline__ bool write_rule_row(const PullArgs &a, int64_t row, bool mact, bool old_has, T old_val, bool t_has,
                                               T t_val)
{
    T *w_new = (T *)a.w_new_val;
    if (!mact) {
        const bool keep = a.replace ? false : old_has;
        if (keep && a.fresh) w_new[row] = old_val;
        return keep;
    }
    if (a.accum >= 0) {
        if (old_has && t_has) {
            // (in place, an accumulation that leaves the value as it was -- most relaxations of a min / max accumulator do -- stores
            //  nothing: the stores of the unchanged rows were 20 us of the headline call)
            const T nv = apply_binop<T>(a.accum, old_val, t_val);
            if (a.fresh || !same_bits(nv, old_val)) w_new[row] = nv;
            return true;
        }
        if (old_has) { if (a.fresh) w_new[row] = old_val; return true; }
        if (t_has) { w_new[row] = t_val; return true; }
        return false;
    }
    if (t_has) w_new[row] = t_val;
    return t_has;
}

// keeps a loaded value where it was loaded: without it the compiler sinks an LDS read whose result is only used under a
// per-lane condition into a divergent branch (8 exec-mask regions per step of the long-row kernels)
#if defined(__HIP_DEVICE_COMPILE__)
#define GRB_PIN(x) asm volatile("" : "+v"(x))
#else
#define GRB_PIN(x) ((void)0)
#endif

// Ablation / diagnostic switches (PullArgs::dbg, option "debug_flags") exist in the kernels of an ABLATION build only
// (-DGRB_ABLATE: scripts/variants_ab.sh, the emulator build of the CPU test tier); the shipped library compiles them out.
#ifdef GRB_ABLATE
#define GRB_DBG(a, bits) ((a).dbg & (bits))
#define EARLY_EXIT(level) do { if (((a.dbg >> 8) & 15) == (level)) return; } while (0)
#define PHASE_STAMP(i) do { if (a.dbg_times && threadIdx.x == 0) a.dbg_times[blockIdx.x * 10 + (i)] = clock64(); } while (0)
#else
#define GRB_DBG(a, bits) 0
#define EARLY_EXIT(level) do { } while (0)
#define PHASE_STAMP(i) do { } while (0)
#endif

// ---- buffer-descriptor loads: the hardware range check returns 0 for out-of-range offsets, so gathers of
//      "no column" (index -1) and tile tails need neither a branch nor an exec-mask dance -------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, int64_t bytes)
{
    const int64_t lim = bytes < 0 ? 0 : (bytes > 0xfffffff0ll ? 0xfffffff0ll : bytes);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)(unsigned)lim, 0x00020000);
}
// streaming variant (aux 2 = non-temporal): for data read once, so that it does not displace the x image from the caches
template <typename T>
__device__ __forceinline__ T buf_load_nt(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    if constexpr (sizeof(T) == 1) return __builtin_bit_cast(T, (unsigned char)__builtin_amdgcn_raw_buffer_load_b8(r, byte_off, 0, 2));
    else if constexpr (sizeof(T) == 2) return __builtin_bit_cast(T, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, byte_off, 0, 2));
    else if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, (unsigned int)__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 2));
    else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 2);
        const unsigned long long u = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
        return __builtin_bit_cast(T, u);
    }
}
// the value gathers of the operand image go through buf_gather: its cache-policy bits are a build-time knob (GRB_GATHER_AUX:
// 0 = default, 2 = non-temporal, ...) so that "does a gather miss have to move a whole line" can be tested with one rebuild
#ifndef GRB_GATHER_AUX
#define GRB_GATHER_AUX 0
#endif
template <typename T>
__device__ __forceinline__ T buf_gather(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    if constexpr (sizeof(T) == 1) return __builtin_bit_cast(T, (unsigned char)__builtin_amdgcn_raw_buffer_load_b8(r, byte_off, 0, GRB_GATHER_AUX));
    else if constexpr (sizeof(T) == 2) return __builtin_bit_cast(T, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, byte_off, 0, GRB_GATHER_AUX));
    else if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, (unsigned int)__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, GRB_GATHER_AUX));
    else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, GRB_GATHER_AUX);
        const unsigned long long u = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
        return __builtin_bit_cast(T, u);
    }
}
template <typename T>
__device__ __forceinline__ T buf_load(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    if constexpr (sizeof(T) == 1) return __builtin_bit_cast(T, (unsigned char)__builtin_amdgcn_raw_buffer_load_b8(r, byte_off, 0, 0));
    else if constexpr (sizeof(T) == 2) return __builtin_bit_cast(T, (unsigned short)__builtin_amdgcn_raw_buffer_load_b16(r, byte_off, 0, 0));
    else if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, (unsigned int)__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
    else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0);
        const unsigned long long u = (unsigned long long)v[0] | ((unsigned long long)v[1] << 32);
        return __builtin_bit_cast(T, u);
    }
}

__device__ __forceinline__ uint4 buf_load_x4(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
}
// The matrix STREAMS of the kernels that gather from the operand in HBM (k_mxv_rtile, k_mxv_rtile_bool, k_mxv_ctile): every byte of them is read
// once per call, while the operand lines the gathers fetch are wanted again -- for a LARGE matrix the streams are read NON-TEMPORAL (`nt`, wave-uniform:
// PullArgs::stream_nt) so that they do not displace those lines from L2 (profiles/r05/stream_cache_policy.txt: headline k_mxv_rtile 198 -> 186 us,
// k_mxv_ctile 130 -> 115-125, the BFS step's k_mxv_rtile_bool 146 -> 140).  A matrix whose cached layouts fit the 256 MB infinity cache is better off
// with plain loads -- its streams are still there at the next call (a rank's block of an 8-way run: 0.109 ms plain, 0.120 non-temporal) --: the host
// decides by the entry count (option "stream_nt_min_nnz").  k_mxv_hstrip gathers from LDS only and keeps plain loads (154 -> 158 us with nt).
typedef uint32_t grb_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t grb_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 buf_stream_x4(__amdgpu_buffer_rsrc_t r, unsigned byte_off, bool nt)
{
    if (nt) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 2);
        return make_uint4(v[0], v[1], v[2], v[3]);
    }
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ uint2 buf_stream_x2(__amdgpu_buffer_rsrc_t r, unsigned byte_off, bool nt)
{
    if (nt) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 2);
        return make_uint2(v[0], v[1]);
    }
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0);
    return make_uint2(v[0], v[1]);
}
__device__ __forceinline__ uint32_t buf_stream_x1(__amdgpu_buffer_rsrc_t r, unsigned byte_off, bool nt)
{
    if (nt) return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 2);
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0);
}
// (the same for streams read through plain pointers: k_mxv_ctile)
__device__ __forceinline__ uint4 ptr_stream_x4(const void *p, bool nt)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (nt) {
        const grb_u32x4 v = __builtin_nontemporal_load((const grb_u32x4 *)p);
        return make_uint4(v[0], v[1], v[2], v[3]);
    }
#endif
    (void)nt;
    return *(const uint4 *)p;
}
__device__ __forceinline__ uint2 ptr_stream_x2(const void *p, bool nt)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (nt) {
        const grb_u32x2 v = __builtin_nontemporal_load((const grb_u32x2 *)p);
        return make_uint2(v[0], v[1]);
    }
#endif
    (void)nt;
    return *(const uint2 *)p;
}

// LDS heads of the persistent 1024-thread kernels: dst[k] = load(k) for k < n, a thread's loads issued FILL_U at a time before the
// first of them is stored.  (Written as "for k: dst[k] = load(k)" the compiler emits load, wait, store per element -- 39 memory round
// trips in a row in front of the first chunk of every workgroup, ~20 % of k_mxv_hstrip at scale 24; ISA of 28 Sep, round 4.)
constexpr int FILL_U = 13;
template <int BLOCK, typename E, typename F>
__device__ __forceinline__ void lds_fill(E *dst, int n, F load)
{
    for (int k0 = threadIdx.x; k0 < n; k0 += BLOCK * FILL_U) {
        E t[FILL_U];
#pragma unroll
        for (int u = 0; u < FILL_U; u++) {
            const int k = k0 + u * BLOCK;
            t[u] = E();
            if (k < n) t[u] = load(k);
        }
#pragma unroll
        for (int u = 0; u < FILL_U; u++) {
            const int k = k0 + u * BLOCK;
            if (k < n) dst[k] = t[u];
        }
    }
}

// ---- wavefront scans in the vector ALU ------------------------------------------------------------------------------------------
// __shfl_up is ds_bpermute: every step of a shuffle scan is a round trip through the LDS pipeline, six of them in a dependent chain.
// DPP moves the data inside the vector ALU: row_shr 1 / 2 / 4 / 8 inside the rows of 16 lanes, then row_bcast:15 (lane 15 of the
// previous row into rows 1 and 3) and row_bcast:31 (lane 31 into rows 2 and 3); a lane without a source keeps `old` = the identity.
__device__ __forceinline__ int wave_inclusive_max_nonneg(int v)  // (values >= 0: the identity is 0)
{
    int t;
    t = __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); v = v > t ? v : t;
    t = __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false); v = v > t ? v : t;
    return v;
}
// the value of the lane below (lane 0: `first`): wave_shr:1, the one DPP shift that crosses the rows
__device__ __forceinline__ int wave_lane_below(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }
