// Part of grb_mxv.hip (included there, inside namespace grb): k_mxv_rtile -- the short rows of an ordered matrix as SORTED ROW TILES
// ---------------------------------------------------------------------------------------------------
// Round 5.  What k_mxv_rows_tag costs is its gathers: one L2 read request and one 128-byte L1 line fill per gathered operand value
// (profiles/r04/pmc_units_*.txt: 62.9 distinct lines per gather instruction, the L1 stalled on misses 80 % of the time), because a
// group of 64 rows holds ~460 entries whose columns are all over the operand.  The row of every entry already travels with it -- so
// nothing ties the ORDER of the entries to their rows.  Here the short rows are cut into TILES of up to RT_ROWS consecutive rows and
// ~32 Ki entries (dense rows at the front of a popularity-ordered matrix: few rows per tile; the thin tail: many), and the entries of
// a tile are SORTED BY COLUMN CODE.  Codes are popularity ranks: the first entries of every tile all hit the few hottest lines of
// the operand, and 64 consecutive entries -- one gather instruction -- touch a fraction of the lines 64 entries of a row group touch.
// A 512-thread workgroup takes a tile: the accumulators of its rows in LDS (one native LDS atomic per product, as in the row
// groups and the cold tiles), the entries streamed in blocks of 256 -- stored lane-transposed, so that a lane's 16-byte load brings
// entries l, 64 + l, 128 + l, 192 + l of the block and gather instruction i covers the 64 CONSECUTIVE sorted entries 64 i .. 64 i + 63 --,
// the next block's loads issued before this block's gathers (static load counts, predication through the address: DESIGN 4.1.0),
// then the write rule of its rows with coalesced loads and stores, the long rows of the tile taking their products from the long-row
// kernels' accumulators as in k_mxv_rows_tag.  Tiles are handed out heaviest first from one counter (a few thousand atomics per call).
// Runs: a specialised semiring over a FULL operand (or an image with the absorbing value under its absent entries) whose values are
// read, a matrix that is not iso, an output written in place; everything else keeps the tagged row groups.
// ---------------------------------------------------------------------------------------------------
#ifndef GRB_RT_BLOCK
#define GRB_RT_BLOCK 1024
#endif
constexpr int RT_BLOCK = GRB_RT_BLOCK, RT_NW = RT_BLOCK / 64, RT_EPL = 4;
constexpr int RT_ROWS_MAX = 16384;  // rows of a tile with 4-byte accumulators (8-byte: half), the larger of the two compiled sizes
#ifndef GRB_RT_HEAD_SIM
#define GRB_RT_HEAD_SIM 0  // build-time ablation (results WRONG): gathers of column codes below this are not issued
#endif
#ifndef GRB_RT_ABL
#define GRB_RT_ABL 0  // build-time ablation (results WRONG): 1 no operand gathers, 2 no LDS atomics, 4 no write rule, 8 gathers folded into 2 MiB
#endif
struct alignas(16) RTile {
    int64_t u0;       // first unit (4 entries) of the tile in rt_col / rt_tag / rt_val
    int32_t n_units;  // units: a multiple of 64 (whole blocks of 256 entries, padded with column -1 / the spare accumulator)
    int32_t g0, g1;   // its row groups of 64: [g0, g1)
    int32_t rsv;
};
static_assert(sizeof(RTile) == 32, "RTile is two 16-byte loads");
template <typename W> GRB_HD constexpr int rt_rows(int rows4) { return sizeof(W) > 4 ? rows4 / 2 : rows4; }

// ---- build (once per matrix, from the short part S of an ordered matrix) ----------------------------------------------------
// tile key of group g: entries before it / entries per tile + rows before it / rows per tile -- both terms grow with g, a run of equal
// keys holds at most one tile's worth of either
__global__ void k_rtile_heads(const int64_t *sptr, int64_t ngroups, int64_t ents_per_tile, int groups_per_tile, int64_t *flag)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    auto key = [&](int64_t x) { return sptr[x * 64] / ents_per_tile + x / groups_per_tile; };
    flag[g] = (g == 0 || key(g) != key(g - 1)) ? 1 : 0;
}
// tiles[t].g0 / e0[t] from the groups that start a tile (tidx = exclusive scan of the flags)
__global__ void k_rtile_starts(const int64_t *sptr, const int64_t *flag, const int64_t *tidx, int64_t ngroups, int32_t *g0, int64_t *e0)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups || !flag[g]) return;
    g0[tidx[g]] = (int32_t)g;
    e0[tidx[g]] = sptr[g * 64];
}
// units of tile t (whole blocks of 256 entries)
__global__ void k_rtile_units(const int64_t *e0, int64_t n_tiles, int64_t e_end, int64_t *units)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    if (t == n_tiles) { units[t] = 0; return; }
    const int64_t e1 = t + 1 < n_tiles ? e0[t + 1] : e_end;
    units[t] = ((e1 - e0[t] + 255) / 256) * 64;
}
__global__ void k_rtile_table(const int32_t *g0, const int64_t *ustart, int64_t n_tiles, int64_t ngroups, RTile *tiles)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    RTile r;
    r.u0 = ustart[t];
    r.n_units = (int32_t)(ustart[t + 1] - ustart[t]);
    r.g0 = g0[t];
    r.g1 = t + 1 < n_tiles ? g0[t + 1] : (int32_t)ngroups;
    r.rsv = 0;
    tiles[t] = r;
}
// sort keys of the entries: (tile, column code), payload = the entry's place in S; the entry's row inside its tile on the side
__global__ void k_rtile_keys(const int64_t *sptr, const int32_t *scol, int64_t rows, const int64_t *flag, const int64_t *tidx, const int32_t *g0,
                             uint64_t *key, uint32_t *pay, uint16_t *rtag)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int64_t g = r >> 6;
    const int64_t t = tidx[g] + flag[g] - 1;
    const uint16_t tag = (uint16_t)(r - (int64_t)g0[t] * 64);
    for (int64_t p = sptr[r]; p < sptr[r + 1]; p++) {
        key[p] = ((uint64_t)t << 32) | (uint64_t)(uint32_t)scol[p];
        pay[p] = (uint32_t)p;
        rtag[p] = tag;
    }
}
template <typename T>
__global__ void k_rtile_place(const uint64_t *skey, const uint32_t *spay, int64_t n, const int64_t *e0, const RTile *tiles, const uint16_t *rtag,
                              const T *sval, int32_t *tcol, uint16_t *ttag, T *tval, const unsigned long long *vd_table, const unsigned char *vd_codes, int iso,
                              int pack)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint64_t k = skey[q];
    const int64_t t = (int64_t)(k >> 32);
    const int64_t rank = q - e0[t];  // (the tiles follow each other in S as in the sorted order)
    // lane-transposed blocks of 256: sorted entry 64 i + l of a block sits at 4 l + i
    const int64_t d = tiles[t].u0 * RT_EPL + (rank >> 8) * 256 + (rank & 63) * 4 + ((rank >> 6) & 3);
    const uint32_t p = spay[q];
    tcol[d] = (int32_t)(uint32_t)k;
    ttag[d] = rtag[p];
    bool coded = false;
    if constexpr (sizeof(T) == 4) {
        if (vd_table) {  // dictionary-coded values (grb_mxv_vdict.inc): tval is a byte array
            const unsigned code = (unsigned)vdict_code(vd_table, vd_codes, ((const uint32_t *)sval)[p]) & 0xffu;
            // (pack: at most 2^24 columns -- the code rides in the top byte of the column word, there is no value array; the padding
            //  words stay 0xffffffff: an entry with column 2^24 - 1 AND code 255 is told from them by its tag)
            if (pack) tcol[d] = (int32_t)((code << 24) | ((uint32_t)k & 0x00ffffffu));
            else ((unsigned char *)tval)[d] = (unsigned char)code;
            coded = true;
        }
    }
    if (!coded && !iso) tval[d] = sval[p];  // (an iso matrix -- the BOOL adjacency matrices -- keeps no values in the tiles)
}
// Round 6 (Context::lazy_tagged): the entries of the tagged row groups (grb_mxv_rows_tag.inc) from the tiles, when a call arrives that the tiles do not
// take and the short part's CSR arrays are gone.  One workgroup per tile; an entry goes to its group's next free place (a counter per group: the order
// inside a group does not matter to k_mxv_rows_tag).  VB: bytes of a value in the tiles' value stream -- 0 none (iso), 1 dictionary codes, -1 codes in the
// top byte of the column word (packed), else sizeof(T) -- the tagged groups keep codes as codes and values as values.
template <typename T>
__global__ void k_tag_from_tiles(const RTile *tiles, const int32_t *rcol, const uint16_t *rtag, const void *rval, int vmode, int rows_cap, const int32_t *tg_off,
                                 int32_t *gcnt, int32_t *tcol, void *tval, unsigned char *ttag)
{
    const RTile t = tiles[blockIdx.x];
    const int64_t e0 = t.u0 * RT_EPL, e1 = e0 + (int64_t)t.n_units * RT_EPL;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int tag = rtag[e];
        if (tag >= rows_cap) continue;  // (padding of the tile's last block)
        const int64_t g = (int64_t)t.g0 + (tag >> 6);
        const int64_t d = (int64_t)tg_off[g] * TAG_EPL + atomicAdd(&gcnt[g], 1);
        const uint32_t w = (uint32_t)rcol[e];
        tcol[d] = vmode == -1 ? (int32_t)(w & 0x00ffffffu) : (int32_t)w;
        ttag[d] = (unsigned char)(tag & 63);
        if (vmode == -1) ((unsigned char *)tval)[d] = (unsigned char)(w >> 24);
        else if (vmode == 1) ((unsigned char *)tval)[d] = ((const unsigned char *)rval)[e];
        else if (vmode > 1) ((T *)tval)[d] = ((const T *)rval)[e];
    }
}
__global__ void k_rtile_pad_tags(uint16_t *ttag, int64_t n, uint16_t pad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ttag[i] = pad;
}

__device__ __forceinline__ uint2 buf_load_x2(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0);
    return uint2{(unsigned)v[0], (unsigned)v[1]};
}

// (wavefronts per SIMD the compiler must leave room for: 8 = two 1024-thread workgroups per CU within 64 registers a thread.  Measured, headline
//  call: 512 threads 8 / 6 wavefronts 223 / 208 us; 1024 threads 4 / 6 / 8 wavefronts 0.499 / 0.496 / 0.490 ms per call -- profiles/r05/rtile_runs.txt)
#ifndef GRB_RT_WAVES
#define GRB_RT_WAVES 8
#endif
#ifndef GRB_RT_DEPTH
#define GRB_RT_DEPTH 1
#endif
template <typename T, int MONOID_CT, int MULT_CT, int ROWS4, bool DICT, bool PACK = false>
__global__ __launch_bounds__(RT_BLOCK, (ROWS4 <= 8192 && sizeof(T) == 4) ? GRB_RT_WAVES : 4) void k_mxv_rtile(const PullArgs a)
{
    static_assert(!DICT || sizeof(T) == 4, "value dictionaries exist for 4-byte types");
    static_assert(!PACK || DICT, "packed words carry dictionary codes");
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4- and 8-byte types");
    using W = typename Widen<T>::type;
    constexpr int EPL = RT_EPL, ROWS = rt_rows<W>(ROWS4), NGRP = ROWS / 64, GPW = NGRP / RT_NW;  // (GPW groups of 64 rows per wavefront)
    static_assert(NGRP % RT_NW == 0, "the groups of a tile are dealt evenly to the wavefronts");
    __shared__ W s_acc[ROWS + 64];            // + the spare accumulator of the padding entries (tag ROWS)
    __shared__ uint32_t s_off[ROWS / 32 + 2]; // bit = the mask switches the row off: its entries gather nothing
    __shared__ uint64_t s_words[3][NGRP];     // per group of the tile: presence word of the old w, long-row word, "row has an entry" word
    __shared__ uint32_t s_dict[DICT ? 256 : 1];
    __shared__ int s_next[2];
    __shared__ RTile s_desc[2];
    const int monoid = MONOID_CT >= 0 ? MONOID_CT : a.monoid;
    const int mult = MULT_CT >= 0 ? MULT_CT : a.mult;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool snt = a.stream_nt != 0;  // (wave-uniform: a large matrix streams non-temporal, grb_mxv_common.inc)
    const bool need_old = (a.accum >= 0) || a.fresh;
    const W ident = pull_seed<T, W>(a, monoid);
    const __amdgpu_buffer_rsrc_t xval_rs = make_rsrc(a.u_val, a.x_len * (int64_t)sizeof(T));
    const __amdgpu_buffer_rsrc_t col_rs = make_rsrc(a.rt_col, a.rt_units * 16);
    const __amdgpu_buffer_rsrc_t tag_rs = make_rsrc(a.rt_tag, a.rt_units * 8);
    const __amdgpu_buffer_rsrc_t val_rs = make_rsrc(a.rt_val, a.rt_units * (DICT ? 4 : 4 * (int64_t)sizeof(T)));
    const __amdgpu_buffer_rsrc_t wold_rs = make_rsrc(a.w_old_val, need_old ? a.m * (int64_t)sizeof(T) : 0);  // (the host keeps m sizeof(T) below 4 GiB)
    if constexpr (DICT) {
        for (int i = threadIdx.x; i < 256; i += RT_BLOCK) s_dict[i] = ((const uint32_t *)a.vdict)[i];
    }
    if (threadIdx.x == 0) {
        const int first = (int)atomicAdd(a.rt_counter, 1u);
        s_next[0] = first;
        if (first < a.rt_ntiles) s_desc[0] = a.rt_tiles[a.rt_order ? a.rt_order[first] : first];  // (handed out heaviest first)
    }
    __syncthreads();
    for (int it = 0;; it++) {
        const int ti = s_next[it & 1];
        if (ti >= a.rt_ntiles) break;  // (uniform over the workgroup)
        const RTile tile = s_desc[it & 1];
        // (the next tile's number is asked for now and read when this tile's entries are through; its descriptor travels while the write rule runs)
        unsigned nxt_tile = 0u;
        if (threadIdx.x == 0) nxt_tile = atomicAdd(a.rt_counter, 1u);
        const int ng = tile.g1 - tile.g0;
        const int nblk = tile.n_units >> 6;
        const unsigned ubase = (unsigned)tile.u0;
        auto unit_at = [&](int b) { return b < nblk ? ubase + (unsigned)b * 64u + (unsigned)lane : 0x0fffffffu; };  // (behind the tile: out of range)
        struct Blk {
            uint4 c;
            uint2 t;
            uint4 v0, v1;
        };
        auto load_blk = [&](int b) {
            Blk r;
            const unsigned u = unit_at(b);
            r.c = buf_stream_x4(col_rs, u * 16u, snt);
            r.t = buf_stream_x2(tag_rs, u * 8u, snt);
            if constexpr (PACK) {
                r.v0.x = r.v0.y = r.v0.z = r.v0.w = 0u;  // (the codes ride in the column words)
                r.v1 = r.v0;
            } else if constexpr (DICT) {
                r.v0.x = buf_stream_x1(val_rs, u * 4u, snt);
                r.v0.y = r.v0.z = r.v0.w = 0u;
                r.v1 = r.v0;
            } else if constexpr (sizeof(T) == 4) {
                r.v0 = buf_stream_x4(val_rs, u * 16u, snt);
                r.v1 = r.v0;
            } else {
                r.v0 = buf_stream_x4(val_rs, u * 32u, snt);
                r.v1 = buf_stream_x4(val_rs, u * 32u + 16u, snt);
            }
            return r;
        };
        // ---- what the tile needs from HBM besides its entries is requested in front of the first barrier: the first two blocks of every
        //      wavefront and the presence / mask / long-row words of its groups (into LDS).  The write rule then asks for the old values of ALL
        //      its rows at once.  (First form of this kernel: the write rule took four groups per wavefront at a time, every step behind its own
        //      round trips with nothing else in flight -- 229 us, 166 of them not gathers; profiles/r05/rtile_first_run.txt.  Old values kept
        //      in registers from the tile's start: 90 registers, two workgroups per CU instead of three.) -------------------------------------
        constexpr int DEPTH = GRB_RT_DEPTH, RING = 3 * DEPTH;  // (see the block loop below)
        static_assert(DEPTH == 1 || DEPTH == 2, "one or two steps between the stages");
        Blk eb[RING];
        T xb[RING][EPL];
#pragma unroll
        for (int q = 0; q < 2 * DEPTH; q++) eb[q] = load_blk(wave + q * RT_NW);
        for (int i = threadIdx.x; i < ng * 64 + 64; i += RT_BLOCK) s_acc[i < ng * 64 ? i : ROWS + (i - ng * 64)] = ident;
        for (int i = threadIdx.x; i < ng + 1; i += RT_BLOCK) {
            uint64_t actw = 0ull;
            if (i < ng) {
                const int64_t g = tile.g0 + i;
                actw = a.has_mask ? (a.m_comp ? ~a.m_bits[g] : a.m_bits[g]) : ~0ull;
                s_words[0][i] = a.w_old_bits[g];
                s_words[1][i] = a.long_bits ? a.long_bits[g] : 0ull;
                s_words[2][i] = a.tg_nonempty[g];
            }
            const int at = i < ng ? i * 2 : ROWS / 32;  // (the spare word pair: padding entries carry column -1 themselves)
            s_off[at] = i < ng ? ~(uint32_t)actw : 0u;
            s_off[at + 1] = i < ng ? ~(uint32_t)(actw >> 32) : 0u;
        }
        __syncthreads();
        // ---- the entries, block after block: wavefront w takes blocks w, w + RT_NW, ... -----------------------------------------
        // Three blocks under way per wavefront (the gathers of a block are a memory round trip that nothing else of the block can hide):
        // in the step that folds block j the entries of block j + 2 are requested, then the operand values of block j + 1 (its entries
        // arrived a step ago), then block j's products go to the accumulators (its values were requested a step ago).  Every step
        // issues the same seven memory instructions, so the waits are s_waitcnt vmcnt(N) with N > 0 (DESIGN 4.1.0).
        auto gather_blk = [&](const Blk &e, T (&xv)[EPL]) {
            int creg[EPL] = {(int)e.c.x, (int)e.c.y, (int)e.c.z, (int)e.c.w};
            const int rk[EPL] = {(int)(e.t.x & 0xffffu), (int)(e.t.x >> 16), (int)(e.t.y & 0xffffu), (int)(e.t.y >> 16)};
            if constexpr (PACK) {  // (column in the low 24 bits; a padding entry -- tag ROWS, the spare accumulator -- gathers nothing)
#pragma unroll
                for (int i = 0; i < EPL; i++) creg[i] = rk[i] >= ROWS ? -1 : (creg[i] & 0x00ffffff);
            }
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const int cc = creg[i] | -(int)((s_off[rk[i] >> 5] >> (rk[i] & 31)) & 1u);  // (-1: padding or a masked-out row -- the gather reads nothing)
                int cg = cc;
                if (GRB_RT_ABL & 8) cg = cc < 0 ? cc : (cc & 0x7ffff);      // (ablation: every gather folded into the first 2 MiB -- all L2 hits)
                if (GRB_RT_HEAD_SIM > 0) cg = cg < GRB_RT_HEAD_SIM ? -1 : cg;  // (ablation: the gathers an LDS head of that many codes would take away)
                xv[i] = (GRB_RT_ABL & 1) ? (T)(cc & 7) : buf_gather<T>(xval_rs, (unsigned)cg * (unsigned)sizeof(T));
            }
        };
        auto fold_blk = [&](const Blk &e, const T (&xv)[EPL]) {
            const int rk[EPL] = {(int)(e.t.x & 0xffffu), (int)(e.t.x >> 16), (int)(e.t.y & 0xffffu), (int)(e.t.y >> 16)};
            T av[EPL];
            if constexpr (PACK) {
                const unsigned cw[EPL] = {e.c.x, e.c.y, e.c.z, e.c.w};
#pragma unroll
                for (int i = 0; i < EPL; i++) av[i] = __builtin_bit_cast(T, s_dict[cw[i] >> 24]);
            } else if constexpr (DICT) {
#pragma unroll
                for (int i = 0; i < EPL; i++) av[i] = __builtin_bit_cast(T, s_dict[(e.v0.x >> (8 * i)) & 0xffu]);
            } else if constexpr (sizeof(T) == 4) {
                av[0] = __builtin_bit_cast(T, e.v0.x); av[1] = __builtin_bit_cast(T, e.v0.y);
                av[2] = __builtin_bit_cast(T, e.v0.z); av[3] = __builtin_bit_cast(T, e.v0.w);
            } else {
                av[0] = __builtin_bit_cast(T, (unsigned long long)e.v0.x | ((unsigned long long)e.v0.y << 32));
                av[1] = __builtin_bit_cast(T, (unsigned long long)e.v0.z | ((unsigned long long)e.v0.w << 32));
                av[2] = __builtin_bit_cast(T, (unsigned long long)e.v1.x | ((unsigned long long)e.v1.y << 32));
                av[3] = __builtin_bit_cast(T, (unsigned long long)e.v1.z | ((unsigned long long)e.v1.w << 32));
            }
            // (a product that gathered nothing -- padding, a masked-out row -- lands in the spare accumulator or in one the write rule ignores)
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const T prod = apply_binop<T>(mult, av[i], xv[i]);
                if (GRB_RT_ABL & 2) { if (prod == (T)12345) s_acc[rk[i]] = (W)prod; continue; }
                if (monoid == OP_ANY) s_acc[rk[i]] = (W)prod;
                else lds_combine<W>(&s_acc[rk[i]], (W)prod, monoid);
            }
        };
        // (the stage registers are rings with STATIC indices -- the loop is unrolled over the ring: a register that is copied must first
        //  have arrived, and the copies of a rotating "e0 = e1; e1 = e2" waited for every load of the step: vmcnt(0), ISA of round 5)
        // DEPTH = steps between a stage and the stage that consumes it: the entries of block j + 2 DEPTH, the gathers of block j + DEPTH,
        // the fold of block j.  A step is bound to one memory round trip (its gathers wait for entries requested DEPTH steps ago, its
        // fold for gathers issued DEPTH steps ago), so DEPTH blocks per stage are what a wavefront keeps in flight.
        // (RING = 3 DEPTH: at least the 2 DEPTH + 1 entry blocks that are live at a time)
        const int n_mine = wave < nblk ? (nblk - wave + RT_NW - 1) / RT_NW : 0;  // my blocks: ordinals 0 .. n_mine - 1 = blocks wave + ordinal RT_NW
#pragma unroll
        for (int q = 0; q < DEPTH; q++) gather_blk(eb[q], xb[q]);  // (behind the tile: an out-of-range load brought column 0 / row 0 -- gathered, never folded)
        for (int jb = 0; jb < n_mine; jb += RING) {
#pragma unroll
            for (int u = 0; u < RING; u++) {
                const int j = jb + u;  // (no early exit inside the unrolled body: the ring indices must stay static)
                eb[(u + 2 * DEPTH) % RING] = load_blk(wave + (j + 2 * DEPTH) * RT_NW);  // (behind the tile it moves nothing)
                gather_blk(eb[(u + DEPTH) % RING], xb[(u + DEPTH) % RING]);
                if (j < n_mine) fold_blk(eb[u], xb[u]);
            }
        }
        // (a wavefront that is through with its blocks asks for the old values of its rows before it waits for the others: the round trip
        //  runs while the last products of the tile drain)
        T oldv[GPW];  // (wavefront w owns the groups w, w + RT_NW, ...: all their old values requested at once)
#pragma unroll
        for (int k = 0; k < GPW; k++) {
            const int gi = wave + k * RT_NW;
            const int64_t row = ((int64_t)(tile.g0 + gi) << 6) + lane;
            const unsigned off = (gi < ng && row * (int64_t)sizeof(T) < 0xfffffff0ll) ? (unsigned)(row * (int64_t)sizeof(T)) : 0xfffffff8u;
            oldv[k] = buf_load<T>(wold_rs, off);  // (no accumulator and nothing to copy: an empty descriptor -- nothing moves)
        }
        __syncthreads();
        // ---- the next tile's descriptor sets out; the write rule of this tile's rows needs nothing more from HBM but its long rows' products ----
        int64_t nxt_u0 = 0;
        int nxt_units = 0, nxt_g0 = 0, nxt_g1 = 0;
        if (threadIdx.x == 0 && (int)nxt_tile < a.rt_ntiles) {
            const RTile *d = a.rt_tiles + (a.rt_order ? a.rt_order[nxt_tile] : (int)nxt_tile);
            nxt_u0 = d->u0; nxt_units = d->n_units; nxt_g0 = d->g0; nxt_g1 = d->g1;
        }
#pragma unroll
        for (int k = 0; k < GPW && !(GRB_RT_ABL & 4); k++) {
            const int gi = wave + k * RT_NW;
            if (gi >= ng) break;  // (wave-uniform)
            const int64_t g = tile.g0 + gi;
            const int64_t row = (g << 6) + lane;
            const uint64_t actw = ~((uint64_t)s_off[gi * 2] | ((uint64_t)s_off[gi * 2 + 1] << 32));
            const uint64_t oldw = s_words[0][gi], longw = s_words[1][gi], nonempty = s_words[2][gi];
            const bool in = row < a.m;
            const bool old_has = in && ((oldw >> lane) & 1ull), is_long = (longw >> lane) & 1ull, act_me = (actw >> lane) & 1ull;
            bool t_has = (nonempty >> lane) & 1ull;  // (full operand: an active row has a product as soon as it has an entry)
            W t_acc = s_acc[gi * 64 + lane];
            if (longw) {  // (wave-uniform: the long rows of the group take their products from the long-row kernels)
                const int long_slot = a.long_prefix[g] + __popcll(longw & ((1ull << lane) - 1ull));
                if (is_long) {
                    // (long_tails, round 6: the tile also holds the row's COLD entries -- folded into s_acc like a short row's -- and the strips'
                    //  accumulator is merged into them; a row without cold entries finds the identity in s_acc.  ANY takes whichever exists.)
                    const bool l_has = a.tl_has[long_slot] != 0;
                    const W l_acc = acc_from_stored<W>(((const W *)a.tl_val)[long_slot], a.tl_ord != 0);
                    if (!a.long_tails) { t_has = l_has; t_acc = l_acc; }
                    else {
                        if (monoid == OP_ANY) t_acc = (t_has && act_me) ? t_acc : l_acc;
                        else t_acc = apply_binop<W>(monoid, t_acc, l_acc);
                        t_has = t_has || l_has;
                    }
                }
            }
            // (an operand image with the absorbing value under its absent entries: the product exists iff the accumulator moved)
            if (a.has_by_value) t_has = t_has && !same_bits<W>(t_acc, ident);
            bool new_has = false;
            if (in) new_has = write_rule_row<T>(a, row, act_me, old_has, oldv[k], t_has, from_acc<T, W>(t_acc));
            const unsigned long long nb = __ballot(in && new_has);
            if (lane == 0) a.w_new_bits[g] = nb;
        }
        if (threadIdx.x == 0) {
            s_next[(it + 1) & 1] = (int)nxt_tile;
            RTile *d = &s_desc[(it + 1) & 1];
            d->u0 = nxt_u0; d->n_units = nxt_units; d->g0 = nxt_g0; d->g1 = nxt_g1;
        }
        __syncthreads();  // (the next tile re-initialises the accumulators)
    }
}

// ---------------------------------------------------------------------------------------------------
// The same for BOOL products over an operand that is not full (the BFS level step q<!visited.S, replace> = A lor.land q): the operand is
// the image of presence / value PAIRS (PullArgs::u_pv: 16 columns per 32-bit word, 512 per 128-byte line), so the sorted entries of a tile
// share their lines sixteen times better than 4-byte values do; the accumulators are two bits per row -- "met a present entry" and "met a
// true one" -- in one LDS word per 16 rows, set with one LDS atomic OR per present partner.  LOR.LAND over an iso (or unread) matrix and
// ANY.PAIR; everything else keeps the tagged row groups.
// ---------------------------------------------------------------------------------------------------
template <int MONOID_CT, int MULT_CT, int ROWS>
__global__ __launch_bounds__(RT_BLOCK, ROWS <= 8192 ? GRB_RT_WAVES : 4) void k_mxv_rtile_bool(const PullArgs a)
{
    static_assert((MONOID_CT == OP_LOR && MULT_CT == OP_LAND) || (MONOID_CT == OP_ANY && MULT_CT == OP_PAIR), "lor.land and any.pair");
    using T = bool;
    using W = typename Widen<T>::type;
    constexpr int EPL = RT_EPL, NGRP = ROWS / 64, GPW = NGRP / RT_NW;
    static_assert(NGRP % RT_NW == 0, "the groups of a tile are dealt evenly to the wavefronts");
    __shared__ uint32_t s_pair[ROWS / 16 + 4];  // per row two bits: 2 r = a product exists, 2 r + 1 = a true product exists; + the spare word of the padding entries
    __shared__ uint32_t s_off[ROWS / 32 + 2];
    __shared__ uint64_t s_words[4][NGRP];  // (old presence, long rows, non-empty rows, rows the mask admits)
    __shared__ int s_next[2];
    __shared__ RTile s_desc[2];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool snt = a.stream_nt != 0;  // (wave-uniform: a large matrix streams non-temporal, grb_mxv_common.inc)
    const bool need_old = (a.accum >= 0) || a.fresh;
    const bool iso_true = !a.need_aval || ((const T *)a.aval)[0];  // (LAND with an iso matrix value: false makes every product false)
    // (a multiply that does not read the operand's values -- PAIR -- comes without the pair image: the presence bits stand in)
    const bool use_pv = a.u_pv != nullptr;
    const __amdgpu_buffer_rsrc_t xpv_rs = use_pv ? make_rsrc(a.u_pv, ((a.x_len + 15) >> 4) * 4) : make_rsrc(a.u_bits, ((a.x_len + 63) >> 6) * 8);
    const int wsh = use_pv ? 4 : 5;  // columns per word: 16 pairs / 32 presence bits
    const __amdgpu_buffer_rsrc_t col_rs = make_rsrc(a.rt_col, a.rt_units * 16);
    const __amdgpu_buffer_rsrc_t tag_rs = make_rsrc(a.rt_tag, a.rt_units * 8);
    const __amdgpu_buffer_rsrc_t wold_rs = make_rsrc(a.w_old_val, need_old ? a.m : 0);
    if (threadIdx.x == 0) {
        const int first = (int)atomicAdd(a.rt_counter, 1u);
        s_next[0] = first;
        if (first < a.rt_ntiles) s_desc[0] = a.rt_tiles[a.rt_order ? a.rt_order[first] : first];  // (handed out heaviest first)
    }
    __syncthreads();
    for (int it = 0;; it++) {
        const int ti = s_next[it & 1];
        if (ti >= a.rt_ntiles) break;
        const RTile tile = s_desc[it & 1];
        unsigned nxt_tile = 0u;
        if (threadIdx.x == 0) nxt_tile = atomicAdd(a.rt_counter, 1u);
        const int ng = tile.g1 - tile.g0;
        const int nblk = tile.n_units >> 6;
        const unsigned ubase = (unsigned)tile.u0;
        auto unit_at = [&](int b) { return b < nblk ? ubase + (unsigned)b * 64u + (unsigned)lane : 0x0fffffffu; };
        struct Blk {
            uint4 c;
            uint2 t;
        };
        auto load_blk = [&](int b) {
            Blk r;
            const unsigned u = unit_at(b);
            r.c = buf_stream_x4(col_rs, u * 16u, snt);
            r.t = buf_stream_x2(tag_rs, u * 8u, snt);
            return r;
        };
        constexpr int DEPTH = GRB_RT_DEPTH, RING = 3 * DEPTH;
        Blk eb[RING];
        uint32_t xb[RING][EPL];
#pragma unroll
        for (int q = 0; q < 2 * DEPTH; q++) eb[q] = load_blk(wave + q * RT_NW);
        for (int i = threadIdx.x; i < ng * 4 + 4; i += RT_BLOCK) s_pair[i < ng * 4 ? i : ROWS / 16 + (i - ng * 4)] = 0u;
        for (int i = threadIdx.x; i < ng + 1; i += RT_BLOCK) {
            uint64_t actw = 0ull;
            if (i < ng) {
                const int64_t g = tile.g0 + i;
                actw = a.has_mask ? (a.m_comp ? ~a.m_bits[g] : a.m_bits[g]) : ~0ull;
                s_words[0][i] = a.w_old_bits[g];
                s_words[1][i] = a.long_bits ? a.long_bits[g] : 0ull;
                s_words[2][i] = a.tg_nonempty[g];
                s_words[3][i] = actw;
            }
            const int at = i < ng ? i * 2 : ROWS / 32;
            s_off[at] = i < ng ? ~(uint32_t)actw : 0u;
            s_off[at + 1] = i < ng ? ~(uint32_t)(actw >> 32) : 0u;
        }
        __syncthreads();
        auto gather_blk = [&](const Blk &e, uint32_t (&pw)[EPL]) {
            const int creg[EPL] = {(int)e.c.x, (int)e.c.y, (int)e.c.z, (int)e.c.w};
            const int rk[EPL] = {(int)(e.t.x & 0xffffu), (int)(e.t.x >> 16), (int)(e.t.y & 0xffffu), (int)(e.t.y >> 16)};
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const int cc = creg[i] | -(int)((s_off[rk[i] >> 5] >> (rk[i] & 31)) & 1u);  // (-1: padding or a masked-out row)
                pw[i] = buf_load<uint32_t>(xpv_rs, (unsigned)(cc >> wsh) * 4u);  // (-1 >> 4 = -1: out of range, 0 -- "absent")
            }
        };
        auto fold_blk = [&](const Blk &e, const uint32_t (&pw)[EPL]) {
            const int creg[EPL] = {(int)e.c.x, (int)e.c.y, (int)e.c.z, (int)e.c.w};
            const int rk[EPL] = {(int)(e.t.x & 0xffffu), (int)(e.t.x >> 16), (int)(e.t.y & 0xffffu), (int)(e.t.y >> 16)};
#pragma unroll
            for (int i = 0; i < EPL; i++) {
                const uint32_t pv = use_pv ? (pw[i] >> ((creg[i] & 15) * 2)) & 3u : (pw[i] >> (creg[i] & 31)) & 1u;  // bit 0 presence, bit 1 value (a gather that read nothing: 0)
                if (!(pv & 1u)) continue;
                const bool prod = MULT_CT == OP_PAIR ? true : (iso_true && (pv & 2u));
                atomicOr(&s_pair[rk[i] >> 4], (1u | (prod ? 2u : 0u)) << ((rk[i] & 15) * 2));
                // (LOR and ANY are terminal: a row with a true product is decided -- its entries still to come gather nothing, like those of a
                //  row the mask switches off; the write rule takes the mask from s_words[3])
                if (prod) atomicOr(&s_off[rk[i] >> 5], 1u << (rk[i] & 31));
            }
        };
        const int n_mine = wave < nblk ? (nblk - wave + RT_NW - 1) / RT_NW : 0;
#pragma unroll
        for (int q = 0; q < DEPTH; q++) gather_blk(eb[q], xb[q]);
        for (int jb = 0; jb < n_mine; jb += RING) {
#pragma unroll
            for (int u = 0; u < RING; u++) {
                const int j = jb + u;
                eb[(u + 2 * DEPTH) % RING] = load_blk(wave + (j + 2 * DEPTH) * RT_NW);
                gather_blk(eb[(u + DEPTH) % RING], xb[(u + DEPTH) % RING]);
                if (j < n_mine) fold_blk(eb[u], xb[u]);
            }
        }
        T oldv[GPW];
#pragma unroll
        for (int k = 0; k < GPW; k++) {
            const int gi = wave + k * RT_NW;
            const int64_t row = ((int64_t)(tile.g0 + gi) << 6) + lane;
            const unsigned off = (gi < ng && row < 0xfffffff0ll) ? (unsigned)row : 0xfffffff8u;
            oldv[k] = buf_load<unsigned char>(wold_rs, off) != 0;
        }
        __syncthreads();
        int64_t nxt_u0 = 0;
        int nxt_units = 0, nxt_g0 = 0, nxt_g1 = 0;
        if (threadIdx.x == 0 && (int)nxt_tile < a.rt_ntiles) {
            const RTile *d = a.rt_tiles + (a.rt_order ? a.rt_order[nxt_tile] : (int)nxt_tile);
            nxt_u0 = d->u0; nxt_units = d->n_units; nxt_g0 = d->g0; nxt_g1 = d->g1;
        }
#pragma unroll
        for (int k = 0; k < GPW; k++) {
            const int gi = wave + k * RT_NW;
            if (gi >= ng) break;  // (wave-uniform)
            const int64_t g = tile.g0 + gi;
            const int64_t row = (g << 6) + lane;
            const uint64_t actw = s_words[3][gi];
            const uint64_t oldw = s_words[0][gi], longw = s_words[1][gi];
            const bool in = row < a.m;
            const bool old_has = in && ((oldw >> lane) & 1ull), is_long = (longw >> lane) & 1ull, act_me = (actw >> lane) & 1ull;
            const uint32_t pr = (s_pair[gi * 4 + (lane >> 4)] >> ((lane & 15) * 2)) & 3u;
            bool t_has = pr & 1u;
            T t_val = (pr & 2u) != 0;
            if (longw) {  // (wave-uniform: the long rows of the group take their products from the long-row kernel)
                const int long_slot = a.long_prefix[g] + __popcll(longw & ((1ull << lane) - 1ull));
                if (is_long) {
                    t_has = a.tl_has[long_slot] != 0;
                    t_val = from_acc<T, W>(acc_from_stored<W>(((const W *)a.tl_val)[long_slot], a.tl_ord != 0));
                }
            }
            bool new_has = false;
            if (in) new_has = write_rule_row<T>(a, row, act_me, old_has, oldv[k], t_has, t_val);
            const unsigned long long nb = __ballot(in && new_has);
            if (lane == 0) a.w_new_bits[g] = nb;
        }
        if (threadIdx.x == 0) {
            s_next[(it + 1) & 1] = (int)nxt_tile;
            RTile *d = &s_desc[(it + 1) & 1];
            d->u0 = nxt_u0; d->n_units = nxt_units; d->g0 = nxt_g0; d->g1 = nxt_g1;
        }
        __syncthreads();
    }
}
