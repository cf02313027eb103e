// Part of grb_mxv.hip (included there, inside namespace grb): k_mxv_ctile -- the COLD entries of the long rows as tagged tiles
// ---------------------------------------------------------------------------------------------------
// The entries of the long rows whose column is NOT LDS-resident in the hot strips (a fifth of them on an R-MAT graph) are gathered
// from the operand image through the vector-memory path.  As strips (segments of one (row, column class), padded to 8 entries)
// they cost 254 us of a 720 us call: a long row has only a handful of cold entries per column range, so either the ranges are wide
// (8 x 8 MB of image at scale 24: every gather misses the 4 MB L2 of its XCD and moves a 128-byte line over the fabric, ~11 us per
// million) or the segments are two entries long and the padding doubles the stream.
//
// Here they are stored like the short rows (grb_mxv_rows_tag.inc): WITHOUT segments or padding, every entry with the row it
// belongs to -- sorted by (column range, row), cut into TILES of one column range x 4096 consecutive long rows, an entry = column
// code + value + 16-bit row-inside-the-tile.  A 512-thread workgroup takes a tile: accumulators, mask bytes and "has a product"
// bytes of its 4096 rows in LDS, the entries streamed four per lane, one native LDS atomic per product, and at the end one global
// atomic per row that received something.  Column ranges are ~3 MB of image, and workgroup b (XCD b mod 8) works on the ranges
// r = b mod 8 (mod 8), one after the other: the 32 CUs of an XCD gather from ONE range at a time, which stays in their L2.
// ---------------------------------------------------------------------------------------------------
// Round 4: what a gather costs is the number of DISTINCT 128-byte lines its 64 lanes touch (~3 clocks each in the CU's texture
// addresser: ablation builds, profiles/r04/tile_ablations.txt -- the gathers are 102 of this kernel's 224 us, its LDS atomics nothing, the
// flush 28).  The entries of a tile are therefore sorted BY COLUMN CODE (the row travels with the entry anyway), and a tile holds 16 Ki
// slots instead of 4 Ki: neighbouring lanes then gather from the same lines -- on a matrix in its popularity order (grb_mxv_order.inc),
// whose hot lines are few, 19 distinct lines per instruction instead of 63 (simulated on R-MAT 24: 16 ranges x 16 Ki slots).  The
// per-slot flags are bit masks so that two such workgroups fit a CU.
#ifndef GRB_CT_SLOTS
#define GRB_CT_SLOTS 16384
#endif
#ifndef GRB_CT_BLOCK
#define GRB_CT_BLOCK 1024
#endif
constexpr int CT_SLOTS = GRB_CT_SLOTS;  // long rows per tile
constexpr int CT_PACK_SLOTS = 8192, CT_PACK_COLBITS = 19;  // (round 6, packed words: slot << 19 | column - range base; 13 + 19 bits)
constexpr int CT_BLOCK = GRB_CT_BLOCK;
constexpr int CT_EPL = 4;
#ifndef GRB_CT_WGS_PER_CU
#define GRB_CT_WGS_PER_CU 2  // (round 4: 68 KiB of LDS per 1024-thread workgroup with 16 Ki slots.  Round 3, 4 Ki slots sorted by row: (24 KiB of LDS per 512-thread workgroup for 4-byte accumulators: 32 wavefronts per CU.  Measured on the headline
                             //  call, ms: 8192 rows x 256 threads x 3 per CU 0.716-0.735; 8192 x 1024 x 2 0.677; 4096 x 256 x 6 0.671-0.676;
                             //  4096 x 512 x 4 0.674; 2048 x 256 x 8 0.691; 1024 x 256 x 8 0.718 -- profiles/r03/ctile_variants*.txt)
#endif
constexpr int CT_WGS_PER_CU = GRB_CT_WGS_PER_CU;
#ifndef GRB_CT_ABL
#define GRB_CT_ABL 0  // build-time ablation (results WRONG): 1 no operand gathers (the value of the entry stands in), 2 no flush of the tile's accumulators, 4 no LDS atomics
#endif
struct alignas(16) CTile {
    int64_t u0;       // first entry / CT_EPL
    int32_t n_units;  // entries / CT_EPL (padded)
    int32_t base;     // first long-row slot of the tile
};
template <typename W> struct CtSlots { static constexpr int value = sizeof(W) > 4 ? CT_SLOTS / 2 : CT_SLOTS; };  // (8-byte accumulators: half the slots)

#ifndef GRB_CT_MAX_ENTRIES
#define GRB_CT_MAX_ENTRIES 16384  // a (column range, slot block) pair with more entries is cut into several tiles: the hub rows of a
                                  // power-law graph put a hundred times the mean into the first slot blocks, and the last workgroup sets the time
#endif
constexpr int64_t CT_MAX_ENTRIES = GRB_CT_MAX_ENTRIES;
// entries of the pair t = (column range t / n_sb, slot block t % n_sb) in the sorted keys of the cold part: [first[t], first[t + 1])
__global__ void k_ctile_first(const uint64_t *skeys, int64_t n, int64_t n_tiles, int n_sb, unsigned v0, int64_t *first, int slots)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    const uint64_t want = (((uint64_t)v0 + (uint64_t)(t / n_sb)) << 32) | (uint64_t)((t % n_sb) * (int64_t)slots);
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skeys[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    first[t] = lo;
}
// tile t holds the cold entries [efirst[t], efirst[t + 1]) of the (column range, slot)-sorted list (a pair's entries, or a piece of
// them); inside the tile they are re-sorted by column code: key2 = (tile, code), payload = the entry's place in the first order
__global__ void k_ctile_keys2(const uint32_t *sidx, int64_t p0, int64_t n_cold, const int64_t *efirst, int64_t n_tiles, const int32_t *col,
                              uint64_t *key2, uint32_t *pay)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cold) return;
    const int64_t p = p0 + c;
    int64_t lo = 0, hi = n_tiles;  // last t with efirst[t] <= p
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (efirst[mid] <= p) lo = mid;
        else hi = mid;
    }
    key2[c] = ((uint64_t)lo << 32) | (uint64_t)(uint32_t)col[sidx[p]];
    pay[c] = (uint32_t)c;
}
template <typename T>
__global__ void k_ctile_place(const uint64_t *skeys, const uint32_t *sidx, int64_t p0, int64_t n_cold, const uint64_t *key2s, const uint32_t *pays,
                              const int64_t *efirst, const CTile *tiles, const T *val, int iso, int32_t *tcol, T *tval, uint16_t *tloc,
                              const unsigned long long *vd_table, const unsigned char *vd_codes, const int32_t *cbase, int code_word)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (place in the (tile, code) order)
    if (q >= n_cold) return;
    const uint64_t k2 = key2s[q];
    const int64_t t = (int64_t)(k2 >> 32);
    const int64_t p = p0 + (int64_t)pays[q];  // (place in the (column range, slot) order: its key holds the slot)
    const int64_t slot = (int64_t)(uint32_t)skeys[p];
    const int64_t d = tiles[t].u0 * CT_EPL + (q - (efirst[t] - p0));
    // (cbase: packed words -- the row slot inside the tile above the column's offset in the tile's range; no tloc array.  The padding word
    //  0xffffffff is slot 8191 / offset 2^19 - 1: told from a real entry by its offset -- a range is at most 2^19 codes wide, so a real
    //  0xffffffff is no real entry: the host keeps every range below 2^19 - 1 codes)
    if (cbase) tcol[d] = (int32_t)((((uint32_t)(slot - tiles[t].base)) << CT_PACK_COLBITS) | (((uint32_t)k2 - (uint32_t)cbase[t]) & ((1u << CT_PACK_COLBITS) - 1u)));
    else tcol[d] = (int32_t)(uint32_t)k2;
    bool coded = false;
    if constexpr (sizeof(T) == 4) {
        if (vd_table) {  // dictionary-coded values (grb_mxv_vdict.inc): tval is a byte array -- or (code_word, ct_mode 3) the code rides in the column word
            const uint32_t code = (uint32_t)vdict_code(vd_table, vd_codes, ((const uint32_t *)val)[sidx[p]]) & 0xffu;
            if (code_word) tcol[d] = (int32_t)((code << 24) | ((uint32_t)k2 & 0x00ffffffu));  // (the host takes this mode below 2^24 column codes only)
            else ((unsigned char *)tval)[d] = (unsigned char)code;
            coded = true;
        }
    }
    if (!iso && !coded) tval[d] = val[sidx[p]];
    if (tloc) tloc[d] = (uint16_t)(slot - tiles[t].base);
}

// ct_mode 3: a padding entry cannot be told by its WORD -- 0xffffffff is the real entry (column 2^24 - 1, code 255) -- so it is told by its SLOT:
// the padding behind a tile's last entry carries slot CT_SLOTS, one past the tile's rows, whose bit in the spare word of s_off is always set.
// The kernel then treats it like an entry of a masked-out row: column -1, an out-of-range address, nothing gathered, no product (as mode 0
// does with its padding column -1).
__global__ void k_ctile_pad_slots(const CTile *tiles, const int64_t *efirst, int64_t n_tiles, uint16_t *tloc, uint16_t pad_slot)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const int64_t d0 = tiles[t].u0 * CT_EPL, d1 = d0 + (int64_t)tiles[t].n_units * CT_EPL;
    for (int64_t d = d0 + (efirst[t + 1] - efirst[t]); d < d1; d++) tloc[d] = pad_slot;  // (at most CT_EPL - 1 of them)
}

// CODEW (PullArgs::ct_mode 3, 4-byte types with a value dictionary): an entry is the word code << 24 | column code and a 16-bit slot -- two
// stream loads per unit, the value from the dictionary in LDS (as k_mxv_rtile<.., DICT, PACK>)
template <typename T, int MONOID_CT, int MULT_CT, bool CODEW = false>
__global__ __launch_bounds__(CT_BLOCK) void k_mxv_ctile(const PullArgs a)
{
    using W = typename Widen<T>::type;
    constexpr int EPL = CT_EPL, SLOTS = CtSlots<W>::value;
    static_assert(!CODEW || (sizeof(T) == 4 && !std::is_same<T, bool>::value && SLOTS == CT_SLOTS), "code words: 4-byte values, tiles of CT_SLOTS slots");
    __shared__ W s_acc[SLOTS];
    __shared__ uint32_t s_off[SLOTS / 32 + (CODEW ? 1 : 0)];  // bit = the mask switches the row off: its entries gather nothing (CODEW: + the padding slot's word)
    __shared__ uint32_t s_has[SLOTS / 32];  // bit = the row received a product
    __shared__ uint32_t s_dict[sizeof(T) == 4 ? 256 : 1];  // (ct_mode 2: the 256 bit patterns of the value dictionary)
    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const bool need_aval = a.need_aval != 0, need_uval = a.need_uval != 0;
    const bool stage_vals = need_aval && !a.a_iso;
    const bool snt = a.stream_nt != 0;  // (wave-uniform: a large matrix streams non-temporal, grb_mxv_common.inc)
    const T iso_v = (a.a_iso && need_aval) ? ((const T *)a.aval)[0] : (T)0;
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t xbits_rs = make_rsrc(a.u_bits, a.u_full ? 0 : ((a.x_len + 63) >> 6) * 8);
    const __amdgpu_buffer_rsrc_t xvbits_rs = make_rsrc(a.u_valbits, a.u_valbits ? ((a.x_len + 63) >> 6) * 8 : 0);
    const __amdgpu_buffer_rsrc_t xpv_rs = make_rsrc(a.u_pv, a.u_pv ? ((a.x_len + 15) >> 4) * 4 : 0);
    const int32_t *tcol = a.ct_col;
    const T *tval = (const T *)a.ct_val;
    const uint16_t *tloc = a.ct_loc;
    W *tl = (W *)a.tl_val;
    const W ident = pull_seed<T, W>(a, monoid);
    // (round 6, PullArgs::ct_mode: packed words -- slot << 19 | column - range base -- in tiles of CT_PACK_SLOTS slots; mode 2: one-byte value codes)
    const int packed = CODEW ? 0 : a.ct_mode;
    const int slots_rt = packed ? (CT_PACK_SLOTS < SLOTS ? CT_PACK_SLOTS : SLOTS) : SLOTS;
    if constexpr (CODEW) {  // (256 loads in flight at once; the barrier behind the first tile's set-up covers them)
        for (int i = threadIdx.x; i < 256; i += CT_BLOCK) s_dict[i] = ((const uint32_t *)a.vdict)[i];
        if (threadIdx.x == 0) s_off[SLOTS / 32] = ~0u;
    } else if constexpr (sizeof(T) == 4) {
        if (packed == 2) {
            for (int i = threadIdx.x; i < 256; i += CT_BLOCK) s_dict[i] = ((const uint32_t *)a.vdict)[i];
            __syncthreads();
        }
    }
    // my tiles: the tiles of my XCD's column ranges, range after range (a.ct_order lists them per XCD); the workgroups of an XCD
    // share them round-robin, so that its 32 CUs gather from one range at a time
    const int xcd = (int)(blockIdx.x & 7u), li = (int)(blockIdx.x >> 3), nx = (int)(gridDim.x >> 3);
    const int64_t x0 = a.ct_xoff[xcd], x1 = a.ct_xoff[xcd + 1];
    for (int64_t tl_i = x0 + li; tl_i < x1; tl_i += nx) {
        const CTile tile = a.ct_tiles[a.ct_order[tl_i]];
        if (tile.n_units == 0) continue;  // (uniform over the workgroup)
        const int cbase = packed ? a.ct_cbase[a.ct_order[tl_i]] : 0;
        const int rows_here = (int)((a.n_long - tile.base < slots_rt) ? a.n_long - tile.base : slots_rt);
        for (int i = threadIdx.x; i < slots_rt; i += CT_BLOCK) s_acc[i] = ident;
        for (int i = threadIdx.x; i < slots_rt / 32; i += CT_BLOCK) {
            s_has[i] = 0u;
            // (tile.base is a multiple of SLOTS, hence of 32: word i of the tile is word (base >> 5) + i of the per-call activity bits)
            const int64_t wd = ((int64_t)tile.base >> 5) + i;
            s_off[i] = (a.has_mask && (int64_t)i * 32 < rows_here) ? ~a.long_act[wd] : 0u;
        }
        __syncthreads();
        const int64_t u_end = tile.u0 + tile.n_units;
        // UB units of four entries per thread and pass: the entries of all of them requested first, then all their gathers, then the products
        // (a unit behind the tile's end re-reads the last one and is switched off).  One unit: 2 / 4 / 8 were measured slower (docs/HISTORY.md).
        // The arrays keep the unit dimension: written without it the compiler lays the pass out differently (k_mxv_ctile<bool, ..> takes
        // two more registers), and this loop is the hot path of the cold tiles.
        constexpr int UB = 1;
        for (int64_t ub0 = tile.u0; ub0 < u_end; ub0 += (int64_t)CT_BLOCK * UB) {  // (uniform over the workgroup)
            const int64_t ub = ub0 + threadIdx.x;
            int creg[UB][EPL], rk[UB][EPL], cc[UB][EPL];
            T vreg[UB][EPL];
            unsigned vcode[UB][EPL];  // (CODEW: the entries' dictionary codes)
            bool uv[UB];
#pragma unroll
            for (int k = 0; k < UB; k++) {
                const int64_t u = ub + (int64_t)k * CT_BLOCK;
                uv[k] = u < u_end;
                const int64_t e = (uv[k] ? u : u_end - 1) * EPL;
                const uint4 c4 = ptr_stream_x4(tcol + e, snt);
                creg[k][0] = (int)c4.x; creg[k][1] = (int)c4.y; creg[k][2] = (int)c4.z; creg[k][3] = (int)c4.w;
                if constexpr (CODEW) {  // (the slots as in mode 0; the column in the low 24 bits, the value code above it)
                    const uint2 l2 = ptr_stream_x2(tloc + e, snt);
                    rk[k][0] = (int)(l2.x & 0xffffu); rk[k][1] = (int)(l2.x >> 16); rk[k][2] = (int)(l2.y & 0xffffu); rk[k][3] = (int)(l2.y >> 16);
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const unsigned w = (unsigned)creg[k][i];
                        creg[k][i] = (int)(w & 0x00ffffffu);
                        vcode[k][i] = w >> 24;  // (looked up behind the gathers' issue: the LDS reads travel under them)
                    }
                } else if (packed) {  // (uniform: the row slot above the column's offset in the tile's range; the all-ones word is padding)
#pragma unroll
                    for (int i = 0; i < EPL; i++) {
                        const unsigned w = (unsigned)creg[k][i];
                        rk[k][i] = (int)(w >> CT_PACK_COLBITS);
                        creg[k][i] = w == 0xffffffffu ? -1 : cbase + (int)(w & ((1u << CT_PACK_COLBITS) - 1u));
                        if (w == 0xffffffffu) rk[k][i] = 0;
                    }
                } else {
                    const uint2 l2 = ptr_stream_x2(tloc + e, snt);
                    rk[k][0] = (int)(l2.x & 0xffffu); rk[k][1] = (int)(l2.x >> 16); rk[k][2] = (int)(l2.y & 0xffffu); rk[k][3] = (int)(l2.y >> 16);
                }
                bool vals_done = CODEW;
                if constexpr (sizeof(T) == 4 && !CODEW) {
                    if (stage_vals && packed == 2) {  // (one-byte codes, four per unit: the values from the dictionary in LDS)
                        const uint32_t cd = ((const uint32_t *)tval)[uv[k] ? u : u_end - 1];
#pragma unroll
                        for (int i = 0; i < EPL; i++) vreg[k][i] = __builtin_bit_cast(T, s_dict[(cd >> (8 * i)) & 0xffu]);
                        vals_done = true;
                    }
                }
                if (vals_done) {
                } else if (stage_vals) {
                    if constexpr (sizeof(T) == 4) {
                        // (full values: one-byte dictionary codes + an LDS lookup were measured 7 % slower here, profiles/r04/value_dict.txt)
                        const uint4 v4 = ptr_stream_x4(tval + e, snt);
                        vreg[k][0] = __builtin_bit_cast(T, v4.x); vreg[k][1] = __builtin_bit_cast(T, v4.y);
                        vreg[k][2] = __builtin_bit_cast(T, v4.z); vreg[k][3] = __builtin_bit_cast(T, v4.w);
                    } else {
#pragma unroll
                        for (int i = 0; i < EPL; i++) vreg[k][i] = tval[e + i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < EPL; i++) vreg[k][i] = iso_v;
                }
            }
#pragma unroll
            for (int k = 0; k < UB; k++)
#pragma unroll
                for (int i = 0; i < EPL; i++)  // (-1: padding, a masked-out row, a unit behind the tile -- the gather reads nothing)
                    cc[k][i] = uv[k] ? (creg[k][i] | -(int)((s_off[rk[k][i] >> 5] >> (rk[k][i] & 31)) & 1u)) : -1;
            // ---- gathers: presence words, then values ----------------------------------------------------------------------
            bool xp[UB][EPL];
            T xv[UB][EPL];
            bool pv_done = false;
            if constexpr (std::is_same<T, bool>::value) {
                if (a.u_pv) {
#pragma unroll
                    for (int k = 0; k < UB; k++) bool_pv_gather<EPL>(xpv_rs, cc[k], xp[k], xv[k]);
                    pv_done = true;
                }
            }
            if (pv_done) {
            } else if (a.u_full) {
#pragma unroll
                for (int k = 0; k < UB; k++)
#pragma unroll
                    for (int i = 0; i < EPL; i++) xp[k][i] = cc[k][i] >= 0;
            } else {
                uint32_t bw[UB][EPL];
#pragma unroll
                for (int k = 0; k < UB; k++)
#pragma unroll
                    for (int i = 0; i < EPL; i++) bw[k][i] = buf_load<uint32_t>(xbits_rs, (unsigned)(cc[k][i] >> 5) * 4u);
#pragma unroll
                for (int k = 0; k < UB; k++)
#pragma unroll
                    for (int i = 0; i < EPL; i++) xp[k][i] = (bw[k][i] >> (cc[k][i] & 31)) & 1u;
            }
            if (pv_done) {
            } else if (need_uval) {
                if constexpr (std::is_same<T, bool>::value) {
                    uint32_t vw[UB][EPL];
#pragma unroll
                    for (int k = 0; k < UB; k++)
#pragma unroll
                        for (int i = 0; i < EPL; i++) vw[k][i] = buf_load<uint32_t>(xvbits_rs, xp[k][i] ? (unsigned)(cc[k][i] >> 5) * 4u : 0xfffffff8u);
#pragma unroll
                    for (int k = 0; k < UB; k++)
#pragma unroll
                        for (int i = 0; i < EPL; i++) xv[k][i] = (vw[k][i] >> (cc[k][i] & 31)) & 1u;
                } else if (GRB_CT_ABL & 1) {
#pragma unroll
                    for (int k = 0; k < UB; k++)
#pragma unroll
                        for (int i = 0; i < EPL; i++) xv[k][i] = vreg[k][i];
                } else {
#pragma unroll
                    for (int k = 0; k < UB; k++)
#pragma unroll
                        for (int i = 0; i < EPL; i++) xv[k][i] = buf_gather<T>(xval_rs, xp[k][i] ? (unsigned)cc[k][i] * (unsigned)sizeof(T) : 0xfffffff8u);
                }
            } else {
#pragma unroll
                for (int k = 0; k < UB; k++)
#pragma unroll
                    for (int i = 0; i < EPL; i++) xv[k][i] = (T)0;
            }
            if constexpr (CODEW) {  // (one LDS read per entry: the value of its code)
#pragma unroll
                for (int k = 0; k < UB; k++)
#pragma unroll
                    for (int i = 0; i < EPL; i++) vreg[k][i] = stage_vals ? __builtin_bit_cast(T, s_dict[vcode[k][i]]) : iso_v;
            }
            // ---- every present product to its row's LDS accumulator: one native LDS atomic -------------------------------------
#pragma unroll
            for (int k = 0; k < UB; k++)
#pragma unroll
                for (int i = 0; i < EPL; i++) {
                    if (!xp[k][i]) continue;
                    const int r = rk[k][i];
                    const T prod = apply_binop<T>(mult, need_aval ? vreg[k][i] : (T)0, xv[k][i]);
                    if (GRB_CT_ABL & 4) { if (prod == (T)12345) s_acc[r] = (W)prod; atomicOr(&s_has[r >> 5], 1u << (r & 31)); continue; }
                    if (monoid == OP_ANY) s_acc[r] = (W)prod;
                    else lds_combine<W>(&s_acc[r], (W)prod, monoid);
                    atomicOr(&s_has[r >> 5], 1u << (r & 31));
                }
        }
        __syncthreads();
        if (GRB_CT_ABL & 2) continue;
        // ---- the rows that received a product send it to their accumulator (other tiles -- other column ranges -- do the same) ----
        for (int i = threadIdx.x; i < rows_here; i += CT_BLOCK) {
            if (!((s_has[i >> 5] >> (i & 31)) & 1u)) continue;
            const int64_t s = tile.base + i;
            if (monoid == OP_ANY) tl[s] = s_acc[i];
            else if (a.tl_ord) atomic_combine_ord<W>(&tl[s], s_acc[i], monoid);
            else atomic_combine<W>(&tl[s], s_acc[i], monoid);
            if (!a.long_has_known) a.tl_has[s] = 1;
        }
        __syncthreads();
    }
}
