// Part of grb_mxv.hip (included there, inside namespace grb): the long rows of a split matrix as flat CLASS STRIPS -- k_mxv_strip
// ---------------------------------------------------------------------------------------------------
// The long rows once more, as one flat stream of entries per column class (class = XCD, as in k_mxv_long_grp: table codes
// interleave by 128-byte line, the columns behind the table split into 8 contiguous ranges and those into sub-ranges), sorted
// by (sub-range, row).  A SEGMENT is the run of entries of one (class, sub-range, row); every segment starts at a multiple of
// 8 entries (padding: code -1, on average 3.5 entries per segment), so the 8 consecutive entries a lane takes (two 16-byte
// loads per array) belong to ONE segment, and where segments start is one bit per lane: a 64-bit mask per CHUNK of 512
// entries = one step of one wavefront.  Chunks of a class are dealt round-robin to the wavefronts of the
// class's workgroups: perfectly balanced, no per-row or per-item descriptors, nothing to chase -- everything a chunk needs
// (entries, its two masks, its segment base) has an address known in advance and is requested one chunk ahead.
//
// Per chunk: a lane knows the accumulator slot of its 8 entries (`lane_slot`, 4 bytes per lane); with a mask it looks up its
// row's bit (and, for the terminal monoids of the BFS step, whether its row is already decided) three chunks ahead, and lanes
// of masked-out or decided rows neither load their entries nor gather; gathers come from the LDS head
// of the class or from the image (as in k_mxv_long_grp); a lane folds its 8 products, lanes of one segment are joined by a
// segmented scan whose boundaries come from the start mask (6 shuffles of the value, no flags travel), and the last lane of
// every segment sends ONE atomic to its row's accumulator -- segments of a strip are sorted by row, so the atomics of a
// wavefront fall into a few consecutive 128-byte lines.  MIN / MAX accumulators of floating-point types are kept in the
// ordered-integer form (grb_ops.hpp) so that the atomic is one instruction instead of a compare-and-swap loop.
// Rows from `split_min_len` entries go this way: 8 bytes per entry for 4-byte types, 4 for iso matrices, + 0.5 for the slots.
// ---------------------------------------------------------------------------------------------------
constexpr int STRIP_CH = 512;  // entries per chunk
#ifndef GRB_STRIP_ABL
#define GRB_STRIP_ABL 0  // build-time ablation of k_mxv_strip (scripts/variants_ab.sh; results are WRONG): 1 no scan, 2 no emission (the compiler then drops the fold AND the loads that feed it: proves nothing), 4 no LDS reads, 8 no image gathers, 16 emission by a plain store to the row's accumulator instead of the atomic, 32 emission by a plain store to a slot of the lane's own (chunk, lane) -- coalesced, nothing dead
#endif
template <size_t N> struct UintOfSize;
template <> struct UintOfSize<1> { using type = uint8_t; };
template <> struct UintOfSize<2> { using type = uint16_t; };
template <> struct UintOfSize<4> { using type = uint32_t; };
template <> struct UintOfSize<8> { using type = uint64_t; };

// ---- build (once per matrix) -------------------------------------------------------------------------------------------
// Over the sorted (key, source) pairs of the long rows' entries, key = (virtual class << 32) | slot: a segment starts where the
// key changes.  Pass 1 counts the starts per block of 512 positions; after a scan pass 2 numbers them and records every
// segment's first position, slot and key.
__device__ __forceinline__ bool strip_starts(const uint64_t *skeys, int64_t p, int64_t n)
{
    return p < n && (p == 0 || skeys[p] != skeys[p - 1]);
}
__global__ __launch_bounds__(STRIP_CH) void k_strip_count(const uint64_t *skeys, int64_t n, int64_t *blk_cnt)
{
    __shared__ int s_cnt[STRIP_CH / 64];
    const int64_t p = (int64_t)blockIdx.x * STRIP_CH + threadIdx.x;
    const unsigned long long b = __ballot(strip_starts(skeys, p, n));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < STRIP_CH / 64; w++) c += s_cnt[w];
        blk_cnt[blockIdx.x] = c;
        if (blockIdx.x == gridDim.x - 1) blk_cnt[gridDim.x] = 0;
    }
}
// segment number of sorted position p inside its block (the block's base added by the caller); *is_start = p starts one
__device__ __forceinline__ int strip_rank_in_block(const uint64_t *skeys, int64_t p, int64_t n, int *s_cnt, bool *is_start)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool st = strip_starts(skeys, p, n);
    const unsigned long long b = __ballot(st);
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int r = __popcll(b & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull)));  // starts at or before me in my wavefront
    for (int w = 0; w < wave; w++) r += s_cnt[w];
    *is_start = st;
    return r - 1;  // (-1: my segment started in an earlier block)
}
__global__ __launch_bounds__(STRIP_CH) void k_strip_seg_fill(const uint64_t *skeys, int64_t n, const int64_t *blk_off, int64_t *seg_first)
{
    __shared__ int s_cnt[STRIP_CH / 64];
    const int64_t p = (int64_t)blockIdx.x * STRIP_CH + threadIdx.x;
    bool st;
    const int r = strip_rank_in_block(skeys, p, n, s_cnt, &st);
    if (st) {
        const int64_t s = blk_off[blockIdx.x] + r;
        seg_first[s] = p;
    }
    if (p == 0) seg_first[blk_off[gridDim.x]] = n;  // sentinel behind the last segment
}
// padded length of every segment (multiple of 8 entries)
__global__ void k_strip_plen(const int64_t *seg_first, int64_t n_seg, int64_t *plen)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_seg) plen[s] = (seg_first[s + 1] - seg_first[s] + 7) & ~7ll;
    else if (s == n_seg) plen[s] = 0;
}
// sc[c] = first segment of class c (c = 0..ncls; keys of segments ascend), raw[c] = unpadded-by-class offset of that segment
// (hot > 0: the first `hot` classes are one virtual class each, the others `sub` virtual classes each -- the hot / cold strips)
__device__ __forceinline__ uint64_t strip_class_vstart(int c, unsigned sub, int hot) { return c < hot ? (uint64_t)c : (uint64_t)hot + (uint64_t)(c - hot) * sub; }
__device__ __forceinline__ int strip_class_of(uint64_t v, unsigned sub, int hot) { return v < (uint64_t)hot ? (int)v : hot + (int)((v - (uint64_t)hot) / sub); }
__global__ void k_strip_class_bounds(const uint64_t *skeys, const int64_t *seg_first, int64_t n_seg, int64_t n_long, unsigned sub,
                                     const int64_t *off, int64_t *sc, int64_t *raw, int ncls, int hot = 0)
{
    const int c = threadIdx.x;
    if (c > ncls) return;
    const uint64_t want = strip_class_vstart(c, sub, hot) << 32;
    int64_t lo = 0, hi = n_seg;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skeys[seg_first[mid]] < want) lo = mid + 1;
        else hi = mid;
    }
    sc[c] = lo;
    raw[c] = off[lo];
}
// entries to their places: class c's segments sit at off[s] + cshift[c]; one bit of the chunk's start mask per segment
template <typename T>
__global__ __launch_bounds__(STRIP_CH) void k_strip_place(const uint64_t *skeys, const uint32_t *sidx, int64_t n, const int64_t *blk_off,
                                                          const int64_t *seg_first, const int64_t *off, const int64_t *cshift,
                                                          int64_t n_long, unsigned sub, const int32_t *col, const T *val, int iso,
                                                          int lds_lim, int ncls, int32_t *lcol, T *lval, unsigned long long *start_mask,
                                                          int32_t *lane_slot, char *hrec, int hrec_bytes, int64_t cold_base,
                                                          int hot, const unsigned long long *vd_table, const unsigned char *vd_codes, int hub_ncls, int hub_lim)
{
    __shared__ int s_cnt[STRIP_CH / 64];
    const int64_t p = (int64_t)blockIdx.x * STRIP_CH + threadIdx.x;
    bool st;
    const int r = strip_rank_in_block(skeys, p, n, s_cnt, &st);
    if (p >= n) return;
    const int64_t s = blk_off[blockIdx.x] + r;
    const int c = strip_class_of(skeys[p] >> 32, sub, hot);
    const int64_t d0 = off[s] + cshift[c];
    const int64_t d = d0 + (p - seg_first[s]);
    const uint32_t j = sidx[p];
    if (hrec) {  // hot / cold strips: classes below ncls are hot (lane records in hrec), the others cold (lcol / lval from cold_base)
        if (c < ncls + hub_ncls) {
            char *rp = hrec + (d >> 3) * (int64_t)hrec_bytes;
            // (-2 - LDS slot; classes from ncls on are the hub level's: hub_ncls classes with their own resident range)
            const int tc = c < ncls ? long_tcode_n(col[j], lds_lim, ncls) : long_tcode_n(col[j], hub_lim, hub_ncls);
            if constexpr (std::is_same<T, bool>::value) {
                ((int32_t *)rp)[d & 7] = tc;
                if (!iso) ((T *)(rp + 32))[d & 7] = val[j];
            } else {
                ((uint16_t *)rp)[d & 7] = (uint16_t)(-2 - tc);
                bool coded = false;
                if constexpr (sizeof(T) == 4) {
                    if (vd_table) {  // dictionary-coded values (grb_mxv_vdict.inc): one byte per entry behind the slots
                        ((unsigned char *)(rp + 16))[d & 7] = (unsigned char)vdict_code(vd_table, vd_codes, ((const uint32_t *)val)[j]);
                        coded = true;
                    }
                }
                if (!iso && !coded) ((T *)(rp + 16))[d & 7] = val[j];
            }
        } else {
            lcol[d - cold_base] = col[j];
            if (!iso) lval[d - cold_base] = val[j];
        }
    } else {
        lcol[d] = long_tcode_n(col[j], lds_lim, ncls);
        if (!iso) lval[d] = val[j];
    }
    if (st) atomicOr(&start_mask[d0 / STRIP_CH], 1ull << ((d0 >> 3) & 63));
    if (((p - seg_first[s]) & 7) == 0) lane_slot[d >> 3] = (int32_t)(uint32_t)skeys[p];  // the row of every lane's 8 entries
}
// the padding behind the last segment of a class (up to the end of its last chunk) starts a segment of its own: the last
// real lane then knows it is the last of its segment, and the padding (slot -1, never admitted) emits nothing
__global__ void k_strip_pad_starts(const int64_t *sc, const int64_t *off, const int64_t *cshift, const int64_t *cend, int ncls,
                                   unsigned long long *start_mask)
{
    const int c = threadIdx.x;
    if (c >= ncls) return;
    const int64_t pos = off[sc[c + 1]] + cshift[c];
    if (pos < cend[c]) atomicOr(&start_mask[pos / STRIP_CH], 1ull << ((pos >> 3) & 63));
}
// Round 6: the lanes' slots as 16-bit offsets from the smallest slot of their chunk (one wavefront per chunk of 64 lanes).  The
// segments of a class follow each other by row, so a chunk's slots span a few hundred rows; a chunk that spans 65535 or more raises
// `too_wide` and the matrix keeps its 32-bit slots.
__global__ void k_strip_slot16(const int32_t *lane_slot, int64_t n_chunks, uint16_t *slot16, int32_t *base, unsigned int *too_wide)
{
    const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= n_chunks) return;  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int32_t sl = lane_slot[c * 64 + lane];
    int32_t lo = sl >= 0 ? sl : 0x7fffffff, hi = sl;
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (lo == 0x7fffffff) lo = 0;  // (a chunk of padding only)
    if (lane == 0) {
        base[c] = lo;
        if (hi >= 0 && (int64_t)hi - (int64_t)lo >= 0xffff) atomicOr(too_wide, 1u);
    }
    slot16[c * 64 + lane] = sl >= 0 ? (uint16_t)((sl - lo) & 0xffff) : (uint16_t)0xffffu;
}
// hot strips: the LDS slot padding entries point at = the slot behind the head (non-BOOL types: one slot of max(4, sizeof) bytes per code)
template <typename T> GRB_HD constexpr int hot_pad_code(int lds_words) { return (int)((int64_t)lds_words * 4 / (int64_t)(sizeof(T) < 4 ? 4 : sizeof(T))); }
// every lane record of the hot strips starts as eight padding entries: slot = the padding slot, value 0
template <typename T>
__global__ void k_hrec_init(char *hrec, int64_t n_rec, int rec_bytes, int pad_code)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    uint32_t *p = (uint32_t *)(hrec + r * (int64_t)rec_bytes);
    const uint32_t pc = (uint32_t)pad_code * 0x10001u;
    for (int q = 0; q < 4; q++) p[q] = pc;
    for (int q = 4; q < rec_bytes / 4; q++) p[q] = 0u;
}
__device__ __forceinline__ unsigned long long lanes_le(int lane) { return lane == 63 ? ~0ull : ((2ull << lane) - 1ull); }

// HOT = 1 (split kind 3, the hot strips of a hot / cold layout): every entry of the stream is LDS-resident in its class and a lane's
// 8 entries are ONE record [8 LDS slots, u16 (u32 for BOOL: its bit-packed image has more slots) | 8 values]: 6 instead of 8 bytes
// per entry of a 4-byte type, one run of 48 bytes per lane -- a lane of a masked-out row skips its whole record, and the kernel
// issues no image gather at all.  The entries that are not resident go to tagged tiles (k_mxv_ctile, grb_mxv_ctile.inc).
template <typename T, int MONOID_CT, int MULT_CT, int LDS_WORDS, int HOT = 0>
__global__ __launch_bounds__(LONG_BLOCK) void k_mxv_strip(const PullArgs a)
{
    using W = typename Widen<T>::type;
    constexpr int EPL = 8, NWV = LONG_BLOCK / 64;
    __shared__ uint32_t s_x[LDS_WORDS];
    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ncls = a.strip_ncls;  // column classes (a multiple of 8: class c runs on XCD c % 8)
    const int cls = (int)(blockIdx.x % (unsigned)ncls);
    const bool need_aval = a.need_aval != 0, need_uval = a.need_uval != 0;
    const bool stage_vals = need_aval && !a.a_iso;
    const T *lval = (const T *)a.lval;
    const T iso_v = (a.a_iso && need_aval) ? ((const T *)a.aval)[0] : (T)0;
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t xbits_rs = make_rsrc(a.u_bits, a.u_full ? 0 : ((a.x_len + 63) >> 6) * 8);
    const __amdgpu_buffer_rsrc_t xvbits_rs = make_rsrc(a.u_valbits, a.u_valbits ? ((a.x_len + 63) >> 6) * 8 : 0);
    const __amdgpu_buffer_rsrc_t xpv_rs = make_rsrc(a.u_pv, a.u_pv ? ((a.x_len + 15) >> 4) * 4 : 0);
    const __amdgpu_buffer_rsrc_t act_rs = make_rsrc(a.long_act, a.has_mask ? ((a.n_long + 63) >> 6) * 8 : 0);
    constexpr bool IS_BOOL = std::is_same<T, bool>::value;
    constexpr int LDS_SLOTS = IS_BOOL ? LDS_WORDS : (int)((int64_t)LDS_WORDS * 4 / (int64_t)(sizeof(T) < 4 ? 4 : sizeof(T)));
    // LDS residency of my class (the entries carry pre-translated codes, see long_tcode) -- as in k_mxv_long_grp
    const bool use_lds = need_uval && a.cls_lds_lim > 0;
    if (use_lds) {
        if constexpr (IS_BOOL) {
            if (a.u_pv) {
                lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int w) {
                    const unsigned s0 = (unsigned)w << 4;
                    const unsigned c0 = (strip_line_of(s0 >> 5, (unsigned)cls, (unsigned)ncls) << 5) | (s0 & 31u);
                    return buf_load<uint32_t>(xpv_rs, (c0 >> 4) * 4u);
                });
            } else {
                lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int w) { return buf_load<uint32_t>(xvbits_rs, strip_line_of((unsigned)w, (unsigned)cls, (unsigned)ncls) * 4u); });
            }
        } else {
            auto load_x = [&](int k) {  // (past the image: 0, never looked up)
                const unsigned c = (strip_line_of((unsigned)(k >> 5), (unsigned)cls, (unsigned)ncls) << 5) | (unsigned)(k & 31);
                return buf_load<T>(xval_rs, c * (unsigned)sizeof(T));
            };
            if constexpr (sizeof(T) == 8) lds_fill<LONG_BLOCK>((T *)s_x, LDS_SLOTS, load_x);
            else if constexpr (sizeof(T) == 4) lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int k) { return __builtin_bit_cast(uint32_t, load_x(k)); });
            else lds_fill<LONG_BLOCK>(s_x, LDS_SLOTS, [&](int k) { return (uint32_t)load_x(k); });
        }
    }
    __syncthreads();

    const int64_t cb1 = a.strip_cb[cls + 1];
    const int64_t nblk = ((int64_t)gridDim.x - cls + ncls - 1) / ncls;  // workgroups of my class
    const int64_t nwv = nblk * NWV;
    int64_t ch = a.strip_cb[cls] + (int64_t)(blockIdx.x / (unsigned)ncls) * NWV + wave;
    if (ch >= cb1) return;
    W *tl = (W *)a.tl_val;
    const bool masked = a.has_mask != 0;
    const bool by_has = monoid == OP_ANY;  // ANY has no identity: presence travels with the value
    const T ident = from_acc<T, W>(pull_seed<T, W>(a, monoid));
    const unsigned long long le = lanes_le(lane);

    int n_c[EPL];
    T n_v[EPL];
    constexpr int HOT_CODE_BYTES = std::is_same<T, bool>::value ? 32 : 16;
    auto hot_record_loads = [&](int64_t chunk, int (&n_c)[8], T (&n_v)[8], bool stage_vals, T iso_v) {
        const char *rp = a.hrec + (chunk * 64 + lane) * (int64_t)a.hrec_bytes;
        if constexpr (std::is_same<T, bool>::value) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const uint4 c4 = *(const uint4 *)(rp + q * 16);
                n_c[q * 4 + 0] = (int)c4.x; n_c[q * 4 + 1] = (int)c4.y; n_c[q * 4 + 2] = (int)c4.z; n_c[q * 4 + 3] = (int)c4.w;
            }
        } else {
            const uint2 c2a = *(const uint2 *)rp, c2b = *(const uint2 *)(rp + 8);  // (24-byte dictionary records are 8-byte aligned)
            const uint32_t w4[4] = {c2a.x, c2a.y, c2b.x, c2b.y};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                constexpr int PADC = hot_pad_code<T>(LDS_WORDS);  // the slot padding entries carry (k_mxv_hstrip reads the identity there)
                const int lo16 = (int)(w4[q] & 0xffffu), hi16 = (int)(w4[q] >> 16);
                n_c[q * 2 + 0] = lo16 == PADC ? -1 : -2 - lo16;
                n_c[q * 2 + 1] = hi16 == PADC ? -1 : -2 - hi16;
            }
        }
        if (stage_vals && a.vdict) {
            // dictionary-coded record: 8 one-byte codes behind the slots, the values from the 1 KiB dictionary (L1-resident)
            const uint2 cd = *(const uint2 *)(rp + HOT_CODE_BYTES);
#pragma unroll
            for (int i = 0; i < 8; i++) n_v[i] = ((const T *)a.vdict)[((i < 4 ? cd.x : cd.y) >> (8 * (i & 3))) & 0xffu];
        } else if (stage_vals) {
            const T *vp = (const T *)(rp + HOT_CODE_BYTES);
            if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const uint4 v4 = *(const uint4 *)(vp + q * 4);
                    n_v[q * 4 + 0] = __builtin_bit_cast(T, v4.x); n_v[q * 4 + 1] = __builtin_bit_cast(T, v4.y);
                    n_v[q * 4 + 2] = __builtin_bit_cast(T, v4.z); n_v[q * 4 + 3] = __builtin_bit_cast(T, v4.w);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) n_v[i] = vp[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) n_v[i] = iso_v;
        }
    };
#define STRIP_ENTRY_LOADS(CH)                                                                        \
    do {                                                                                             \
        if constexpr (HOT) { hot_record_loads((CH), n_c, n_v, stage_vals, iso_v); break; }           \
        const int64_t e_ = (CH) * STRIP_CH + lane * EPL;                                             \
        const int32_t *cp_ = a.lcol + e_;                                                            \
        _Pragma("unroll") for (int q_ = 0; q_ < EPL / 4; q_++) {                                     \
            const uint4 c4_ = *(const uint4 *)(cp_ + q_ * 4);                                        \
            n_c[q_ * 4 + 0] = (int)c4_.x; n_c[q_ * 4 + 1] = (int)c4_.y;                              \
            n_c[q_ * 4 + 2] = (int)c4_.z; n_c[q_ * 4 + 3] = (int)c4_.w;                              \
        }                                                                                            \
        if (stage_vals) {                                                                            \
            const T *vp_ = lval + e_;                                                                \
            if constexpr (sizeof(T) == 4) {                                                          \
                _Pragma("unroll") for (int q_ = 0; q_ < EPL / 4; q_++) {                             \
                    const uint4 v4_ = *(const uint4 *)(vp_ + q_ * 4);                                \
                    n_v[q_ * 4 + 0] = __builtin_bit_cast(T, v4_.x); n_v[q_ * 4 + 1] = __builtin_bit_cast(T, v4_.y); \
                    n_v[q_ * 4 + 2] = __builtin_bit_cast(T, v4_.z); n_v[q_ * 4 + 3] = __builtin_bit_cast(T, v4_.w); \
                }                                                                                    \
            } else {                                                                                 \
                _Pragma("unroll") for (int i_ = 0; i_ < EPL; i_++) n_v[i_] = vp_[i_];                \
            }                                                                                        \
        } else {                                                                                     \
            _Pragma("unroll") for (int i_ = 0; i_ < EPL; i_++) n_v[i_] = iso_v;                      \
        }                                                                                            \
    } while (0)
    // Two chunks are under way at any time: while chunk k is folded, the image gathers of chunk k+1 and the entries of chunk
    // k+2 are in flight (loads return in order: a chunk's gathers are issued behind the entries they depend on and ahead of
    // the entries of the chunk after it).
    using G = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;  // a gathered value, or a word of presence / value bits
    struct Stage {
        int cc[EPL];   // >= 0 a code gathered from the image, <= -2 an LDS slot, -1 nothing (padding, masked-out row)
        T av[EPL];
        G g[EPL];
        int slot;      // accumulator slot of my segment's row
        unsigned long long start;
    };
    const bool pv_path = IS_BOOL && a.u_pv != nullptr;
    // what the first-level gather of an entry fetches: (presence, value) words, value bits, values -- or presence words when u
    // is not full (the values then follow inside the fold, un-pipelined: two dependent gathers)
    auto issue = [&](Stage &st, unsigned long long start, bool on, int slot) {
#pragma unroll
        for (int i = 0; i < EPL; i++) {
            st.cc[i] = on ? n_c[i] : -1;
            st.av[i] = n_v[i];
        }
        st.start = start;
        st.slot = slot;
        if (HOT && (pv_path || a.u_full)) {  // (every code is resident: nothing comes from the image)
#pragma unroll
            for (int i = 0; i < EPL; i++) st.g[i] = (G)0;
        } else if (pv_path && !(GRB_STRIP_ABL & 8)) {
#pragma unroll
            for (int i = 0; i < EPL; i++) st.g[i] = (G)buf_load<uint32_t>(xpv_rs, st.cc[i] >= 0 ? (unsigned)(st.cc[i] >> 4) * 4u : 0xfffffff8u);
        } else if (!a.u_full) {
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const int sl = -2 - st.cc[i];
                const int co = st.cc[i] < -1 ? (int)((strip_line_of((unsigned)(sl >> 5), (unsigned)cls, (unsigned)ncls) << 5) | (unsigned)(sl & 31)) : st.cc[i];  // (a resident code, translated back)
                st.g[i] = (G)buf_load<uint32_t>(xbits_rs, (unsigned)(co >> 5) * 4u);  // (-1: out of range, reads 0)
            }
        } else if (need_uval && !(GRB_STRIP_ABL & 8)) {
            if constexpr (IS_BOOL) {
#pragma unroll
                for (int i = 0; i < EPL; i++) st.g[i] = (G)buf_load<uint32_t>(xvbits_rs, st.cc[i] >= 0 ? (unsigned)(st.cc[i] >> 5) * 4u : 0xfffffff8u);
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    const T v = buf_gather<T>(xval_rs, (unsigned)st.cc[i] * (unsigned)sizeof(T));  // (negative: out of range)
                    if constexpr (sizeof(T) == 8) st.g[i] = __builtin_bit_cast(uint64_t, v);
                    else if constexpr (sizeof(T) == 4) st.g[i] = __builtin_bit_cast(uint32_t, v);
                    else st.g[i] = (uint32_t)__builtin_bit_cast(typename UintOfSize<sizeof(T)>::type, v);
                }
            }
        }
    };
    auto lds_value = [&](int cc) -> T {  // the value of a resident code (any slot for the others: the caller selects)
        if (GRB_STRIP_ABL & 4) return (T)(cc & 3);
        const int li = cc < -1 ? -2 - cc : 0;
        if constexpr (sizeof(T) == 8) {
            uint64_t w64 = ((const uint64_t *)s_x)[li];
            GRB_PIN(w64);
            return __builtin_bit_cast(T, w64);
        } else {
            uint32_t w32 = s_x[li];
            GRB_PIN(w32);
            if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, w32);
            else return (T)w32;
        }
    };
    auto g_value = [&](G g) -> T {
        if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, g);
        else if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, g);
        else return __builtin_bit_cast(T, (typename UintOfSize<sizeof(T)>::type)g);
    };
    auto fold = [&](const Stage &st) {
        bool xp[EPL];
        T xv[EPL];
        if (pv_path) {
            if constexpr (IS_BOOL) {
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    const bool in_lds = st.cc[i] < -1;
                    const int sl = in_lds ? -2 - st.cc[i] : st.cc[i];
                    uint32_t lw = (GRB_STRIP_ABL & 4) ? 0x55555555u : s_x[in_lds ? (sl >> 4) : 0];
                    GRB_PIN(lw);
                    const uint32_t wv32 = in_lds ? lw : (uint32_t)st.g[i];
                    const int sh = (sl & 15) * 2;
                    xp[i] = (wv32 >> sh) & 1u;
                    xv[i] = (wv32 >> (sh + 1)) & 1u;
                }
            }
        } else if (!a.u_full) {
            int co[EPL];
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const int sl = -2 - st.cc[i];
                co[i] = st.cc[i] < -1 ? (int)((strip_line_of((unsigned)(sl >> 5), (unsigned)cls, (unsigned)ncls) << 5) | (unsigned)(sl & 31)) : st.cc[i];
                xp[i] = ((uint32_t)st.g[i] >> (co[i] & 31)) & 1u;
            }
            if (need_uval) {  // second level: the values of the present entries
                if constexpr (IS_BOOL) {
                    uint32_t vw[EPL];
#pragma unroll
                    for (int i = 0; i < EPL; i++) vw[i] = buf_load<uint32_t>(xvbits_rs, (xp[i] && st.cc[i] >= 0) ? (unsigned)(st.cc[i] >> 5) * 4u : 0xfffffff8u);
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const bool in_lds = st.cc[i] < -1;
                        const int sl = in_lds ? -2 - st.cc[i] : 0;
                        uint32_t lw = s_x[sl >> 5];
                        GRB_PIN(lw);
                        const uint32_t wv32 = in_lds ? lw : vw[i];
                        xv[i] = (wv32 >> (in_lds ? (sl & 31) : (st.cc[i] & 31))) & 1u;
                    }
                } else {
                    T xg[EPL];
#pragma unroll
                    for (int i = 0; i < EPL; i++) xg[i] = buf_gather<T>(xval_rs, (xp[i] && st.cc[i] >= 0) ? (unsigned)st.cc[i] * (unsigned)sizeof(T) : 0xfffffff8u);
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const T xl = lds_value(st.cc[i]);
                        xv[i] = st.cc[i] < -1 ? xl : xg[i];
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) xv[i] = (T)0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < EPL; i++) xp[i] = st.cc[i] != -1;
            if (need_uval) {
                if constexpr (IS_BOOL) {
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const bool in_lds = st.cc[i] < -1;
                        const int sl = in_lds ? -2 - st.cc[i] : 0;
                        uint32_t lw = s_x[sl >> 5];
                        GRB_PIN(lw);
                        const uint32_t wv32 = in_lds ? lw : (uint32_t)st.g[i];
                        xv[i] = (wv32 >> (in_lds ? (sl & 31) : (st.cc[i] & 31))) & 1u;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const T xl = lds_value(st.cc[i]);
                        xv[i] = st.cc[i] < -1 ? xl : g_value(st.g[i]);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; i++) xv[i] = (T)0;
            }
        }
        // ---- my 8 products (one segment); an absent product is the monoid's identity ----
        T acc = by_has ? (T)0 : ident;
        bool has = false;
#pragma unroll
        for (int i = 0; i < EPL; i++) {
            const T prod = apply_binop<T>(mult, need_aval ? st.av[i] : (T)0, xv[i]);
            if (by_has) acc = xp[i] ? prod : acc;
            else acc = apply_binop<T>(monoid, acc, xp[i] ? prod : ident);
            has = has || xp[i];
        }
        // ---- lanes of one segment are joined: a segmented inclusive scan whose boundaries come from the start mask (lane
        //      l - off joins while it is not in front of `first`); no flags travel ----
        const bool is_last = lane == 63 || ((st.start >> (lane + 1)) & 1ull);
        const unsigned long long sm = st.start & le;
        const int first = sm ? 63 - __clzll(sm) : 0;  // first lane of my segment inside this chunk
        const unsigned long long hasm = __ballot(has);
        const unsigned long long mine = le & ~((1ull << first) - 1ull);  // lanes first .. me
        const bool seg_has = (hasm & mine) != 0;
        if (by_has) {  // ANY: the value of the nearest lane of my segment that has one
            const unsigned long long cand = hasm & mine;
            acc = __shfl(acc, cand ? 63 - __clzll(cand) : lane);
        } else if (!(GRB_STRIP_ABL & 1)) {
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const T pv = __shfl_up(acc, off);
                if (lane - off >= first) acc = apply_binop<T>(monoid, pv, acc);
            }
        }
        if (is_last && seg_has && !(GRB_STRIP_ABL & 2)) {
            if (GRB_STRIP_ABL & 16) tl[st.slot] = (W)acc;
            else if (GRB_STRIP_ABL & 32) tl[ch * 64 + lane] = (W)acc;
            else if (monoid == OP_ANY) tl[st.slot] = (W)acc;
            else if (a.tl_ord) atomic_combine_ord<W>(&tl[st.slot], (W)acc, monoid);
            else atomic_combine<W>(&tl[st.slot], (W)acc, monoid);
            if (!a.long_has_known) a.tl_has[st.slot] = 1;
        }
    };
    // LOR / LAND stop at true / false, ANY at the first product (the bottom-up BFS step: a vertex stops looking once it has a
    // parent): lanes of a row whose accumulator can no longer change read nothing (a stale "not yet" only costs the work)
    int term_mode = 0;
    if constexpr (IS_BOOL) {
        if (monoid == OP_LOR) term_mode = 1;
        else if (monoid == OP_LAND) term_mode = 2;
    }
    if (monoid == OP_ANY && !a.long_has_known) term_mode = 3;
    // Five chunks are under way: the lanes' slots of chunk k+4, the mask words (and terminal tests) of chunk k+3, the entries of
    // chunk k+2 -- only the lanes the mask admits ask for theirs --, the image gathers of chunk k+1, the fold of chunk k.  Every
    // address but the mask word's is known in advance, and no wait is for the newest loads.
    auto chunk_at = [&](int d) { return ch + (int64_t)d * nwv; };
    auto load_slot = [&](int64_t c) -> int {
        if (c >= cb1) return -1;
        if (a.strip_slot16) {  // (round 6: 16-bit offsets from the chunk's smallest slot, 0xffff = padding)
            const unsigned d = a.strip_slot16[c * (STRIP_CH / EPL) + lane];
            return d == 0xffffu ? -1 : a.strip_slot_base[c] + (int)d;
        }
        return a.strip_slot[c * (STRIP_CH / EPL) + lane];
    };
    auto load_start = [&](int64_t c) -> unsigned long long { return c < cb1 ? a.strip_start[c] : 0ull; };
    struct Probe { uint32_t actw; int term; };
    auto probe = [&](int slot) -> Probe {  // (slot -1: padding behind the last segment of the class)
        Probe pr;
        pr.actw = masked ? buf_load<uint32_t>(act_rs, slot >= 0 ? (unsigned)(slot >> 5) * 4u : 0xfffffff8u) : 0xffffffffu;
        pr.term = 0;
        if (slot >= 0) {
            if (term_mode == 1 || term_mode == 2) pr.term = long_terminal<W>(&tl[slot], term_mode) ? 1 : 0;
            else if (term_mode == 3) pr.term = __atomic_load_n(&a.tl_has[slot], __ATOMIC_RELAXED) ? 1 : 0;
        }
        return pr;
    };
    auto admitted = [&](int slot, const Probe &pr) -> bool { return slot >= 0 && ((pr.actw >> (slot & 31)) & 1u) && !pr.term; };
    auto load_entries = [&](int64_t c, bool on) {
        if (on) {
            STRIP_ENTRY_LOADS(c);
        } else {
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                n_c[i] = -1;
                n_v[i] = iso_v;
            }
        }
    };
    // prologue: fill the pipeline
    int slot0 = load_slot(chunk_at(0)), slot1 = load_slot(chunk_at(1)), slot2 = load_slot(chunk_at(2)), slot3 = load_slot(chunk_at(3));
    unsigned long long start0 = load_start(chunk_at(0)), start1 = load_start(chunk_at(1)), start2 = load_start(chunk_at(2)),
                       start3 = load_start(chunk_at(3));
    Probe pr0 = probe(slot0), pr1 = probe(slot1), pr2 = probe(slot2);
    bool on0 = admitted(slot0, pr0);
    load_entries(chunk_at(0), on0);
    Stage cur, nxt;
    issue(cur, start0, on0, slot0);
    bool on1 = chunk_at(1) < cb1 && admitted(slot1, pr1);
    if (chunk_at(1) < cb1) load_entries(chunk_at(1), on1);
    for (;;) {
        // state: cur = chunk k (gathers issued), entries of k+1 in flight (on1), probe of k+2 (pr2) in flight, slots up to k+3
        const bool more = chunk_at(1) < cb1;
        if (more) {
            issue(nxt, start1, on1, slot1);  // (waits for the entries of chunk k+1, hence also for the gathers of chunk k)
            const bool on2 = chunk_at(2) < cb1 && admitted(slot2, pr2);
            if (chunk_at(2) < cb1) load_entries(chunk_at(2), on2);
            on1 = on2;
            pr2 = probe(slot3);                      // chunk k+3
            slot1 = slot2; start1 = start2;
            slot2 = slot3; start2 = start3;
            slot3 = load_slot(chunk_at(4));          // chunk k+4
            start3 = load_start(chunk_at(4));
        }
        fold(cur);
        if (!more) break;
        cur = nxt;
        ch += nwv;
    }
#undef STRIP_ENTRY_LOADS
}

// ---------------------------------------------------------------------------------------------------
// k_mxv_hstrip: the HOT strips of a hot / cold layout on the fast path -- a specialised semiring over a 4- or 8-byte type, a full
// operand whose values are read.  k_mxv_strip spends ~370 vector-ALU instructions per chunk of 512 entries; a wave64 instruction
// holds a SIMD16 for 4 cycles, so 406 k chunks x 370 x 4 cycles over 1024 SIMDs at 2.4 GHz = 244 us of its 322 us are instruction
// issue: the kernel is bound by the VALU, not by bytes, atomics or LDS.  This kernel does the same work in ~60:
//   * padding entries carry the LDS slot PAD whose word makes the product the monoid's identity (x_pad = identity for
//     (min | max).plus, 0 for plus.times; a_pad = 0): no validity flags, no selects -- an entry is ds_read, multiply, fold;
//   * the LDS byte address of an entry is two instructions from its packed 16-bit slot; nothing is translated or compared;
//   * the segmented scan takes its lane masks from SCALAR arithmetic on the chunk's start mask (runs of continuing lanes of
//     length >= 1, 2, 4, ...: c1 = ~start, c2 = c1 & c1 << 1, c4 = c2 & c2 << 2, ...) and stops at the first empty mask -- most
//     chunks need two or three of the six steps; a step is ds_bpermute + fold + v_cndmask with the scalar mask;
//   * a lane learns whether the mask admits its row from ONE byte load indexed by its slot (act8, written by k_long_init);
//   * every address but the LDS one is a scalar offset plus a per-lane constant.
// Everything else (layout, chunk dealing, five chunks under way, one atomic per segment) is k_mxv_strip's.
// ---------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T strip_select_mask(unsigned long long m, T keep, T take, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (sizeof(T) == 4) {
        uint32_t r;
        asm volatile("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, keep)), "v"(__builtin_bit_cast(uint32_t, take)), "s"(m));
        return __builtin_bit_cast(T, r);
    } else {
        const uint64_t k = __builtin_bit_cast(uint64_t, keep), t = __builtin_bit_cast(uint64_t, take);
        uint32_t lo, hi;
        asm volatile("v_cndmask_b32 %0, %1, %2, %3" : "=v"(lo) : "v"((uint32_t)k), "v"((uint32_t)t), "s"(m));
        asm volatile("v_cndmask_b32 %0, %1, %2, %3" : "=v"(hi) : "v"((uint32_t)(k >> 32)), "v"((uint32_t)(t >> 32)), "s"(m));
        return __builtin_bit_cast(T, (uint64_t)lo | ((uint64_t)hi << 32));
    }
#else
    return ((m >> lane) & 1ull) ? take : keep;
#endif
}
__device__ __forceinline__ unsigned long long strip_uniform64(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
// can the fast kernel run this semiring?  (the padding trick needs an operand value that turns every product into the identity)
template <typename T> GRB_HD constexpr bool hstrip_fast_semiring(int monoid, int mult)
{
    return !std::is_same<T, bool>::value && (sizeof(T) == 4 || sizeof(T) == 8) &&
           ((mult == OP_PLUS && (monoid == OP_MIN || monoid == OP_MAX)) || (mult == OP_TIMES && monoid == OP_PLUS));
}

#ifndef GRB_HSTRIP_DEPTH
#define GRB_HSTRIP_DEPTH 3  // iterations between a stage of k_mxv_hstrip and the stage that consumes it
#endif
#ifndef GRB_HSTRIP_ABL
#define GRB_HSTRIP_ABL 0  // build-time ablation of k_mxv_hstrip (results WRONG): 1 no LDS fill, 2 no LDS reads, 4 no scan, 8 plain store instead of the atomic
#endif
template <typename T, int MONOID_CT, int MULT_CT, int LDS_WORDS, bool DICT = false, bool SLOT16 = false>
__global__ __launch_bounds__(LONG_BLOCK) void k_mxv_hstrip(const PullArgs a)
{
    static_assert(!DICT || sizeof(T) == 4, "value dictionaries exist for 4-byte types");
    static_assert(MONOID_CT >= 0 && MULT_CT >= 0, "the fast hot-strip kernel is compiled per semiring");
    using W = typename Widen<T>::type;
    static_assert(std::is_same<W, T>::value, "4- and 8-byte types accumulate in their own type");
    using U = typename UintOfSize<sizeof(T)>::type;
    constexpr int EPL = 8, NWV = LONG_BLOCK / 64;
    constexpr int LDS_SLOTS = (int)((int64_t)LDS_WORDS * 4 / (int64_t)sizeof(T));
    constexpr int PAD = LDS_SLOTS;  // the slot padding entries point at
    constexpr int SH = sizeof(T) == 8 ? 3 : 2;
    __shared__ __attribute__((aligned(16))) uint32_t s_x[LDS_WORDS + 32];
    __shared__ T s_dict[DICT ? 256 : 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // my class: blockIdx % ncls -- or, one launch over the two class levels of an ordered matrix, what the workgroup table says
    int ncls = a.strip_ncls, cls = (int)(blockIdx.x % (unsigned)ncls);
    int64_t cb0, cb1, nblk, myblk, chunks_total;
    if (a.wg_tab) {
        const int32_t *t = a.wg_tab + 5 * (int64_t)blockIdx.x;
        const int gcls = __builtin_amdgcn_readfirstlane(t[0]);
        cls = __builtin_amdgcn_readfirstlane(t[1]);
        ncls = __builtin_amdgcn_readfirstlane(t[2]);
        myblk = __builtin_amdgcn_readfirstlane(t[3]);
        nblk = __builtin_amdgcn_readfirstlane(t[4]);
        cb0 = a.strip_cb_dev[gcls];
        cb1 = a.strip_cb_dev[gcls + 1];
        chunks_total = a.strip_chunks;
    } else {
        cb0 = a.strip_cb[cls];
        cb1 = a.strip_cb[cls + 1];
        nblk = ((int64_t)gridDim.x - cls + ncls - 1) / ncls;  // workgroups of my class
        myblk = (int64_t)(blockIdx.x / (unsigned)ncls);
        chunks_total = a.strip_cb[ncls];
    }
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    if constexpr (DICT) {
        if (threadIdx.x < 256) s_dict[threadIdx.x] = ((const T *)a.vdict)[threadIdx.x];
    }
    // the head of my class, and the padding slot: 16-byte pieces of the operand's lines, ALL of a thread's loads issued before the first
    // is stored (a load, a wait, a store per word was 39 memory latencies in a row in front of every workgroup's first chunk)
    {
        constexpr int VEC = 16 / (int)sizeof(T), NG = LDS_SLOTS / VEC, NIT = (NG + LONG_BLOCK - 1) / LONG_BLOCK;
        static_assert(LDS_SLOTS % VEC == 0 && 32 % VEC == 0, "the head is filled in 16-byte pieces inside 32-slot lines");
        const int n_fill = (GRB_HSTRIP_ABL & 1) ? 256 : NG;
        const unsigned x_bytes = (unsigned)(a.x_len * (int64_t)sizeof(T) > 0xfffffff0ll ? 0xfffffff0ll : a.x_len * (int64_t)sizeof(T));
        uint4 piece[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int g = it * LONG_BLOCK + (int)threadIdx.x, k = g * VEC;
            const unsigned c = (strip_line_of((unsigned)(k >> 5), (unsigned)cls, (unsigned)ncls) << 5) | (unsigned)(k & 31);
            const unsigned off = c * (unsigned)sizeof(T);
            piece[it] = make_uint4(0u, 0u, 0u, 0u);  // (past the image: 0, never looked up)
            if (g < n_fill) {
                if (off + 16u <= x_bytes) piece[it] = buf_load_x4(xval_rs, off);
                else {  // (the piece that straddles the end of the image: word by word -- the range check of a wide load is not relied on)
                    piece[it].x = buf_load<uint32_t>(xval_rs, off);
                    piece[it].y = buf_load<uint32_t>(xval_rs, off + 4u);
                    piece[it].z = buf_load<uint32_t>(xval_rs, off + 8u);
                    piece[it].w = buf_load<uint32_t>(xval_rs, off + 12u);
                }
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int g = it * LONG_BLOCK + (int)threadIdx.x;
            if (g < n_fill) *(uint4 *)((char *)s_x + (size_t)g * 16) = piece[it];
        }
    }
    // (the padding slot: its products must not move an accumulator.  Integers: 0 for times, the identity for plus (value 0 + identity).
    //  Floating point: the accumulators start at acc_seed -- NaN for min / max, which a NaN padding product (value + NaN) leaves alone;
    //  -0.0 for plus, which a -0.0 padding product (0 * -0.0) leaves alone; +inf would turn a row of NaN products into +inf)
    if (threadIdx.x == 0) {
        if constexpr (std::is_floating_point<T>::value) ((T *)s_x)[PAD] = MULT_CT == OP_TIMES ? -(T)0 : (T)__builtin_nan("");
        else ((T *)s_x)[PAD] = MULT_CT == OP_TIMES ? (T)0 : monoid_identity<T, W>(MONOID_CT);
    }
    __syncthreads();

    (void)chunks_total;
    const int64_t nwv = nblk * NWV;
    const int64_t ch = cb0 + myblk * NWV + wave;
    if (ch >= cb1) return;
    W *tl = (W *)a.tl_val;
    const bool masked = a.has_mask != 0;
    const uint32_t unmasked_bit = masked ? 0u : 1u;
    // (acc_seed even under the absorbing fill: a padding or NaN product is dropped by fmin / fmax, and the accumulators this kernel
    //  sends to -- tl, seeded by k_long_init -- keep the fill's identity; a compile-time NaN also folds the first fmin away)
    const T ident = acc_seed<T, W>(MONOID_CT);
    // Every stream of the chunk loop is read through a buffer descriptor over MY CLASS's part of it, with 32-bit offsets from the
    // class's first chunk (the host checks that a class stays below 2 GiB): a load that has nothing to read -- a step behind my last
    // chunk, a lane the mask switches off -- is issued all the same, with an offset beyond the descriptor (it returns 0 and moves no
    // data).  What matters is that the NUMBER of memory instructions per iteration does not depend on the data: the compiler counts
    // the loads between a request and its use to wait for exactly that request (s_waitcnt vmcnt(N)), and with a single load under a
    // condition it counts the path WITHOUT it -- every wait became vmcnt(0), the whole pipeline below drained once per iteration, and
    // an iteration cost a memory round trip (rounds 3-4: 3.6 us per chunk and wavefront; ISA of 28 Sep).
    constexpr unsigned OOR = 0xc0000000u;  // (beyond any descriptor here, and OOR + a record does not wrap)
    constexpr int REC = DICT ? 24 : 16 + EPL * (int)sizeof(T);
    const int64_t cls_chunks = cb1 - cb0;
    // (SLOT16, round 6: the slot stream is 16-bit offsets from the chunk's smallest slot + one base per chunk -- both loads are issued in every
    //  iteration; the slot is put together where it is used, never where it is loaded)
    const __amdgpu_buffer_rsrc_t slot_rs = SLOT16 ? make_rsrc(a.strip_slot16 + cb0 * (STRIP_CH / EPL), cls_chunks * (STRIP_CH / EPL) * 2)
                                                  : make_rsrc(a.strip_slot + cb0 * (STRIP_CH / EPL), cls_chunks * (STRIP_CH / EPL) * 4);
    const __amdgpu_buffer_rsrc_t sbase_rs = make_rsrc(a.strip_slot_base + (SLOT16 ? cb0 : 0), SLOT16 ? cls_chunks * 4 : 0);
    const __amdgpu_buffer_rsrc_t start_rs = make_rsrc(a.strip_start + cb0, cls_chunks * 8);
    const __amdgpu_buffer_rsrc_t rec_rs = make_rsrc(a.hrec + cb0 * 64 * (int64_t)REC, cls_chunks * 64 * (int64_t)REC);
    const __amdgpu_buffer_rsrc_t act_rs = make_rsrc(a.long_act8, masked ? a.n_long : 0);
    const int64_t n_mine = (cb1 - ch + nwv - 1) / nwv;  // my chunks: ordinals 0 .. n_mine - 1
    const unsigned rel0 = (unsigned)(ch - cb0), rstep = (unsigned)nwv;
    // (DICT: the ring carries the 8 one-byte codes -- two registers -- instead of 8 values; the fold looks them up in LDS)
    struct Rec { uint32_t c[4]; T v[DICT ? 2 : EPL]; };
    struct Slot { int v; int b; };  // (32-bit slots: v = the slot, b unused; SLOT16: v = the 16-bit offset, b = the chunk's base)
    auto load_slot = [&](int64_t ord) -> Slot {  // (slot -1 in the stream: padding behind the last segment of the class)
        Slot s;
        if constexpr (SLOT16) {
            const unsigned chunk = rel0 + (unsigned)ord * rstep;
            s.v = (int)buf_load<unsigned short>(slot_rs, ord < n_mine ? chunk * (unsigned)(STRIP_CH / EPL * 2) + (unsigned)lane * 2u : OOR);
            s.b = buf_load<int>(sbase_rs, ord < n_mine ? chunk * 4u : OOR);
        } else {
            const unsigned off = ord < n_mine ? (rel0 + (unsigned)ord * rstep) * (unsigned)(STRIP_CH / EPL * 4) + (unsigned)lane * 4u : OOR;
            s.v = buf_load<int>(slot_rs, off);
            s.b = 0;
        }
        return s;
    };
    // (a load beyond the descriptor returns 0: offset 0 from base 0 -- a step behind my last chunk; lane_on tests the ordinal)
    auto slot_of = [&](const Slot &s) -> int { return SLOT16 ? (s.v == 0xffff ? -1 : s.b + s.v) : s.v; };
    auto load_start = [&](int64_t ord) -> unsigned long long {
        return buf_load<unsigned long long>(start_rs, ord < n_mine ? (rel0 + (unsigned)ord * rstep) * 8u : OOR);
    };
    // the mask byte of the lane's row (0 for slot -1: beyond the descriptor); no mask: the descriptor is empty, `unmasked_bit` stands in
    auto probe = [&](int slot) -> uint32_t { return (uint32_t)buf_load<unsigned char>(act_rs, (unsigned)slot); };
    auto lane_on = [&](int64_t ord, int slot, uint32_t pr) -> bool { return ord < n_mine && slot >= 0 && (pr | unmasked_bit) != 0u; };
    auto load_rec = [&](int64_t ord, bool on, Rec &r) {  // (a lane that is off reads zeros: its products go nowhere -- the fold emits for lanes that are on)
        const unsigned base = on ? ((rel0 + (unsigned)ord * rstep) * 64u + (unsigned)lane) * (unsigned)REC : OOR;
        const uint4 c4 = buf_load_x4(rec_rs, base);
        r.c[0] = c4.x; r.c[1] = c4.y; r.c[2] = c4.z; r.c[3] = c4.w;
        if constexpr (DICT) {
            const unsigned long long cd = buf_load<unsigned long long>(rec_rs, base + 16u);
            r.v[0] = __builtin_bit_cast(T, (uint32_t)cd);
            r.v[1] = __builtin_bit_cast(T, (uint32_t)(cd >> 32));
        } else if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const uint4 v4 = buf_load_x4(rec_rs, base + 16u + 16u * (unsigned)q);
                r.v[q * 4 + 0] = __builtin_bit_cast(T, v4.x); r.v[q * 4 + 1] = __builtin_bit_cast(T, v4.y);
                r.v[q * 4 + 2] = __builtin_bit_cast(T, v4.z); r.v[q * 4 + 3] = __builtin_bit_cast(T, v4.w);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v4 = buf_load_x4(rec_rs, base + 16u + 16u * (unsigned)q);
                r.v[q * 2 + 0] = __builtin_bit_cast(T, (uint64_t)v4.x | ((uint64_t)v4.y << 32));
                r.v[q * 2 + 1] = __builtin_bit_cast(T, (uint64_t)v4.z | ((uint64_t)v4.w << 32));
            }
        }
    };
    auto fold = [&](const Rec &r, unsigned long long start, int slot, bool on) {
        // ---- my 8 products: LDS word of the slot, multiply, fold (padding: the identity by construction) ----
        T x[EPL];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t lo = (r.c[q] & 0xffffu) << SH, hi = (r.c[q] >> 16) << SH;
            if (GRB_HSTRIP_ABL & 2) {
                x[q * 2 + 0] = __builtin_bit_cast(T, (U)lo);
                x[q * 2 + 1] = __builtin_bit_cast(T, (U)hi);
                continue;
            }
            x[q * 2 + 0] = *(const T *)((const char *)s_x + lo);
            x[q * 2 + 1] = *(const T *)((const char *)s_x + hi);
        }
        T acc = ident;
        if constexpr (DICT) {
            const uint32_t c0 = __builtin_bit_cast(uint32_t, r.v[0]), c1 = __builtin_bit_cast(uint32_t, r.v[1]);
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const T av = s_dict[((i < 4 ? c0 : c1) >> (8 * (i & 3))) & 0xffu];  // (code 0 of a padding entry: any finite value -- x is the absorbing word)
                T prod = apply_binop<T>(MULT_CT, av, x[i]);
                if constexpr (MULT_CT == OP_TIMES) {
                    // (a padding entry's value is code 0, of either sign: its product is set to -0.0, the sum's seed, by the slot)
                    const uint32_t sl = (i & 1) ? (r.c[i >> 1] >> 16) : (r.c[i >> 1] & 0xffffu);
                    if (sl == (uint32_t)PAD) prod = -(T)0;
                }
                acc = apply_binop<T>(MONOID_CT, acc, prod);
            }
        } else {
#pragma unroll
            for (int i = 0; i < EPL; i++) acc = apply_binop<T>(MONOID_CT, acc, apply_binop<T>(MULT_CT, r.v[i], x[i]));
        }
        // ---- lanes of one segment are joined: segmented inclusive scan, lane masks from scalar arithmetic on the start mask ----
        const unsigned long long st = strip_uniform64(start);
        unsigned long long cm = ~st;  // lanes that continue the segment of the lane below
        cm &= ~1ull;                  // (lane 0 has nobody below it in this chunk)
        if (GRB_HSTRIP_ABL & 4) cm = 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            if (cm == 0) break;  // (wave-uniform: no segment of this chunk spans more lanes)
            const T below = __shfl_up(acc, off);
            acc = strip_select_mask<T>(cm, acc, apply_binop<T>(MONOID_CT, below, acc), lane);
            cm &= cm << off;     // runs of at least 2 off continuing lanes
        }
        // ---- the last lane of every segment sends the segment's product to its row's accumulator ----
        const unsigned long long last = (st >> 1) | (1ull << 63);
        const uint32_t is_last = strip_select_mask<uint32_t>(last, 0u, 1u, lane);
        if (is_last && on) {
            if (GRB_HSTRIP_ABL & 8) tl[slot] = (W)acc;
            else if (a.tl_ord) atomic_combine_ord<W>(&tl[slot], (W)acc, MONOID_CT);
            else atomic_combine<W>(&tl[slot], (W)acc, MONOID_CT);
        }
    };
    // A DEEP software pipeline.  With one workgroup per CU (the LDS head) a SIMD holds 4 wavefronts, a chunk is ~0.1 us of work,
    // a loaded memory round trip ~2-3 us: the stream only flows when every wavefront has many chunks under way.  Ordinal j = my
    // j-th chunk.  In iteration j: the slots of chunk j + 3 D are requested, the mask bytes of chunk j + 2 D (they need its slots),
    // the records and the start mask of chunk j + D (only the lanes the mask admits ask for their records: the others ask beyond
    // the descriptor), and chunk j is folded -- every consumer is D iterations behind its producer, and since loads return in order
    // and every iteration issues the SAME memory instructions no wait covers a load younger than the one it needs.  The loop is
    // unrolled 16 times so that the stage registers are rings with STATIC indices: no register is ever copied, and only live ranges
    // cost registers.  Steps behind my last chunk issue their (empty) loads too and fold nothing.
    // (8-byte types: 20 registers per record in flight -- two iterations between the stages keep the kernel inside its 128 registers)
    constexpr int DEPTH = sizeof(T) == 8 ? 2 : GRB_HSTRIP_DEPTH;
    constexpr int RING = 16, DR = DEPTH, DP = DEPTH, DS = DEPTH;
    static_assert(DR + DP + DS < RING, "the slot ring must hold every chunk between its request and its fold");
    Slot sl[RING];
    uint32_t pr[RING];
    unsigned long long stt[RING];
    bool onr[RING];
    Rec rc[RING];
    // prologue: the pipeline is filled stage by stage
#pragma unroll
    for (int q = 0; q < DR + DP + DS; q++) sl[q] = load_slot(q);
#pragma unroll
    for (int q = 0; q < DR + DP; q++) pr[q] = probe(slot_of(sl[q]));
#pragma unroll
    for (int q = 0; q < DR; q++) {
        onr[q] = lane_on(q, slot_of(sl[q]), pr[q]);
        load_rec(q, onr[q], rc[q]);
        stt[q] = load_start(q);
    }
    for (int64_t jb = 0; jb < n_mine; jb += RING) {
#pragma unroll
        for (int u = 0; u < RING; u++) {
            const int64_t j = jb + u;  // (no early exit inside the unrolled body: the ring indices must stay static)
            sl[(u + DR + DP + DS) % RING] = load_slot(j + DR + DP + DS);
            pr[(u + DR + DP) % RING] = probe(slot_of(sl[(u + DR + DP) % RING]));
            onr[(u + DR) % RING] = lane_on(j + DR, slot_of(sl[(u + DR) % RING]), pr[(u + DR) % RING]);
            load_rec(j + DR, onr[(u + DR) % RING], rc[(u + DR) % RING]);
            stt[(u + DR) % RING] = load_start(j + DR);
            if (j < n_mine) fold(rc[u], stt[u], slot_of(sl[u]), onr[u]);
        }
    }
}
