// grb_context.hip -- library context: device selection, stream, stream-ordered memory, timing hooks.
// Counterpart of the reference's `initialize(blocking=..., memory_manager="numpy")` call at
// graphblas/__init__.py:170-173 (there: SuiteSparse GrB_init on the host; here: a gfx950 device is
// mandatory -- there is no CPU fallback).
#include <chrono>
#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "grb_internal.hpp"

namespace grb {

// The debug flags: the shipped library only knows the switches that choose between two correct paths on the host side
// (128 no long/short row split, 256 no LDS bitmap in the symbolic SpGEMM pass, 2048 no (presence, value) packing, 65536 no
// row-length path); the kernel ablation switches -- some of which make results wrong on purpose -- are compiled in by
// -DGRB_ABLATE only (make ablate; the emulator build of the CPU test tier).
#ifdef GRB_ABLATE
static constexpr int DEBUG_FLAGS_MASK = ~0;
#else
static constexpr int DEBUG_FLAGS_MASK = 128 | 256 | 2048 | 65536;
#endif


Context &ctx()
{
    static Context c;
    return c;
}

void require_init()
{
    if (!ctx().initialized) fail(GrB_PANIC, "GrB_init has not been called (or no HIP device is available)");
}

// Device memory: hipMallocAsync / hipFreeAsync on the library's stream, behind a size-class cache.  Every kernel of the
// library runs in order on that one stream, so a block freed by one call can be handed to the next allocation of its
// size class without touching the HIP allocator (whose stream-ordered calls were measured to leave the GPU idle for
// tens of microseconds between two GrB calls).  The cache is emptied when an allocation fails, when the stream changes
// and at GrB_finalize.
namespace {
struct BlockCache {
    std::mutex mu;
    std::unordered_map<size_t, std::vector<void *>> free_blocks;  // size class -> blocks
    std::unordered_map<void *, size_t> size_of;                   // live + cached blocks -> size class
    size_t cached_bytes = 0;
};
BlockCache &cache()
{
    static BlockCache c;
    return c;
}
// classes: multiples of 512 B up to 64 KiB, then eight steps per power of two (at most 12.5 % over-allocation)
size_t size_class(size_t bytes)
{
    if (bytes <= 65536) return (bytes + 511) & ~(size_t)511;
    int top = 63 - __builtin_clzll((unsigned long long)bytes);
    const size_t step = (size_t)1 << (top - 3);
    return (bytes + step - 1) & ~(step - 1);
}
}  // namespace

void dev_cache_release()
{
    BlockCache &c = cache();
    std::lock_guard<std::mutex> lock(c.mu);
    for (auto &kv : c.free_blocks)
        for (void *p : kv.second) {
            c.size_of.erase(p);
            (void)hipFreeAsync(p, ctx().stream);
        }
    c.free_blocks.clear();
    c.cached_bytes = 0;
}

void *dev_alloc(size_t bytes)
{
    if (bytes == 0) bytes = 16;
    BlockCache &c = cache();
    const size_t cls = size_class(bytes);
    if (ctx().alloc_cache) {
        std::lock_guard<std::mutex> lock(c.mu);
        auto it = c.free_blocks.find(cls);
        if (it != c.free_blocks.end() && !it->second.empty()) {
            void *p = it->second.back();
            it->second.pop_back();
            c.cached_bytes -= cls;
            return p;
        }
    }
    void *p = nullptr;
    hipError_t e = hipMallocAsync(&p, cls, ctx().stream);
    if ((e != hipSuccess || !p) && c.cached_bytes) {
        (void)hipGetLastError();
        dev_cache_release();
        (void)hipStreamSynchronize(ctx().stream);
        p = nullptr;
        e = hipMallocAsync(&p, cls, ctx().stream);
    }
    if (e != hipSuccess || !p) {
        (void)hipGetLastError();
        fail(GrB_OUT_OF_MEMORY, "device allocation of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
    }
    if (ctx().alloc_cache) {
        std::lock_guard<std::mutex> lock(c.mu);
        c.size_of[p] = cls;
    }
    return p;
}

void *dev_alloc_zero(size_t bytes)
{
    void *p = dev_alloc(bytes);
    GRB_HIP(hipMemsetAsync(p, 0, bytes ? bytes : 16, ctx().stream));
    return p;
}

void dev_free(void *p)
{
    if (!p) return;
    BlockCache &c = cache();
    {
        std::lock_guard<std::mutex> lock(c.mu);
        auto it = c.size_of.find(p);
        if (it != c.size_of.end()) {
            if (ctx().alloc_cache && ctx().initialized) {
                c.free_blocks[it->second].push_back(p);
                c.cached_bytes += it->second;
                return;
            }
            c.size_of.erase(it);
        }
    }
    (void)hipFreeAsync(p, ctx().stream);
}

// Host <-> device copies of the library's own small tables (tile descriptors, class bounds, counts): through page-locked memory of the
// context -- 4 KiB for the scalars, STAGE_BYTES for the tables -- instead of the runtime's staging of pageable memory.  Measured on the
// layout-building call of the headline matrix (profiles/r05/layout_build_timeline.txt): host time inside its 26 hipMemcpyAsync calls
// 13.0 -> 6.6 ms; the call's wall time does not move (44 ms: 39 ms of kernels, the waits reappear in the synchronisations).
// Larger copies (the caller's tuples at ingress / egress) keep the runtime's path.
static constexpr size_t STAGE_BYTES = 8u << 20;
static void *stage_block(size_t bytes)
{
    Context &c = ctx();
    if (bytes <= 4096) {
        if (!c.host_pinned && hipHostMalloc(&c.host_pinned, 4096, 0) != hipSuccess) {
            (void)hipGetLastError();
            c.host_pinned = nullptr;
        }
        if (c.host_pinned) return c.host_pinned;
    }
    if (bytes <= STAGE_BYTES) {
        if (!c.host_stage && !c.host_stage_failed && hipHostMalloc(&c.host_stage, STAGE_BYTES, 0) != hipSuccess) {
            (void)hipGetLastError();
            c.host_stage = nullptr;
            c.host_stage_failed = true;
        }
        return c.host_stage;
    }
    return nullptr;
}
void preload_stage() { (void)stage_block(4096); (void)stage_block(STAGE_BYTES); }
// (GRB_TRACE_COPIES=1: every host <-> device copy of the library that holds the host for more than 0.5 ms, on stderr)
static bool trace_copies()
{
    static const bool on = [] { const char *e = getenv("GRB_TRACE_COPIES"); return e && atoi(e) != 0; }();
    return on;
}
struct CopyTrace {
    const char *what;
    size_t bytes;
    bool staged;
    std::chrono::steady_clock::time_point t0;
    CopyTrace(const char *w, size_t b, bool s) : what(w), bytes(b), staged(s), t0(std::chrono::steady_clock::now()) {}
    ~CopyTrace()
    {
        if (!trace_copies()) return;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms > 0.5) fprintf(stderr, "[grb copy] %s %zu bytes %s: %.2f ms\n", what, bytes, staged ? "staged" : "direct", ms);
    }
};
void h2d(void *dst, const void *src, size_t bytes)
{
    if (!bytes) return;
    Context &c = ctx();
    if (void *st = stage_block(bytes)) {
        CopyTrace tr("h2d", bytes, true);
        memcpy(st, src, bytes);
        GRB_HIP(hipMemcpyAsync(dst, st, bytes, hipMemcpyHostToDevice, c.stream));
        GRB_HIP(hipStreamSynchronize(c.stream));  // (the block is free for the next copy)
        return;
    }
    CopyTrace tr("h2d", bytes, false);
    GRB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c.stream));
    GRB_HIP(hipStreamSynchronize(c.stream));  // the caller's host buffer is only borrowed for the call
}
void d2h(void *dst, const void *src, size_t bytes)
{
    // (entry counts, reduced scalars, the push path's counters, tile tables: a copy into pageable memory is staged by the runtime -- the
    //  page-locked blocks take them directly)
    Context &c = ctx();
    if (bytes) {
        if (void *st = stage_block(bytes)) {
            CopyTrace tr("d2h", bytes, true);
            GRB_HIP(hipMemcpyAsync(st, src, bytes, hipMemcpyDeviceToHost, c.stream));
            GRB_HIP(hipStreamSynchronize(c.stream));
            memcpy(dst, st, bytes);
            return;
        }
        CopyTrace tr("d2h", bytes, false);
        GRB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c.stream));
        GRB_HIP(hipStreamSynchronize(c.stream));
        return;
    }
    GRB_HIP(hipStreamSynchronize(c.stream));
}
void d2d(void *dst, const void *src, size_t bytes)
{
    if (bytes) GRB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx().stream));
}
void sync_stream() { GRB_HIP(hipStreamSynchronize(ctx().stream)); }

// ---- the options (GrX_option_set / _get / GrX_options_reset, GRB_<NAME> in the environment): ONE row each ---------------------
// A row names the option, the field of the context that holds it (an int or an int64_t: a value is cast to the field's type, as
// ever) and what happens to a value before it is stored: ANY keeps it, WITHIN rejects it outside [lo, hi], ONE_OF rejects it unless it
// is lo or hi, CLAMP moves it into [lo, hi].  A hook, for the few options that need more, runs after the rule: it may change the value
// and rejects it by returning false.  include/grb_mi355x.h says what every option means, grb_internal.hpp holds the defaults.
namespace {
struct Option {
    const char *name;
    int Context::*i;
    int64_t Context::*l;
    enum Rule { ANY, WITHIN, ONE_OF, CLAMP } rule;
    int64_t lo, hi;
    bool (*hook)(int64_t &value);
};
using Hook = bool (*)(int64_t &);
constexpr int64_t MAX64 = INT64_MAX, P30 = 1 << 30;
constexpr Option opt(const char *n, int Context::*f, Option::Rule r = Option::ANY, int64_t lo = 0, int64_t hi = 0, Hook h = nullptr) { return {n, f, nullptr, r, lo, hi, h}; }
constexpr Option opt(const char *n, int64_t Context::*f, Option::Rule r = Option::ANY, int64_t lo = 0, int64_t hi = 0, Hook h = nullptr) { return {n, nullptr, f, r, lo, hi, h}; }

// kernel ablation switches exist in -DGRB_ABLATE builds only
bool known_debug_flags(int64_t &v) { return !((int)v & ~DEBUG_FLAGS_MASK); }
// (2 = sliced ELLPACK, 3 = persistent row groups with an LDS head, 4 = a lane per row: measured slower in rounds 1-2, removed)
bool short_kernel_exists(int64_t &v) { return v != 2 && v != 3 && v != 4; }
bool snap_long_classes(int64_t &v) { if (v != 16 && v != 32 && v != 64) v = 8; return true; }
bool window_group(int64_t &v) { return (v & (v - 1)) == 0; }  // (0, 1, 2, 4, 8)
// (whoever sets "ctile_pack" names the layout of the cold tiles -- 0, the three streams, included: the code words, which are on by default, give way
//  until "ctile_code" is set again.  GrX_options_reset stores both, in the table's order, and so returns to what GrB_init left.)
bool explicit_cold_layout(int64_t &) { ctx().ctile_code = 0; return true; }
bool release_cache_when_off(int64_t &v) { if (!v) dev_cache_release(); return true; }

const Option OPTIONS[] = {
    opt("debug_flags", &Context::debug_flags, Option::ANY, 0, 0, known_debug_flags),
    opt("pull_ipt", &Context::tune_pull_ipt),
    opt("hot_min_cols", &Context::hot_min_cols),
    opt("hot_k", &Context::hot_k),
    opt("push_mode", &Context::push_mode),
    opt("split_min_nnz", &Context::split_min_nnz),
    opt("split_min_len", &Context::split_min_len, Option::CLAMP, 0, P30),
    opt("short_kernel", &Context::short_kernel, Option::WITHIN, 0, 6, short_kernel_exists),
    opt("lazy_layout", &Context::lazy_layout),
    opt("lazy_min_nnz", &Context::lazy_min_nnz),
    opt("lean_min_nnz", &Context::lean_min_nnz, Option::CLAMP, 0, MAX64),
    opt("long_kernel", &Context::long_kernel),
    opt("long_classes", &Context::long_classes, Option::ANY, 0, 0, snap_long_classes),
    opt("long_sub", &Context::long_sub, Option::CLAMP, 0, 16),
    opt("long_sub_min_len", &Context::long_sub_min_len),
    opt("mxm_mask_mode", &Context::mxm_mask_mode),
    opt("mat_write_kernel", &Context::mat_write_kernel, Option::WITHIN, 0, 1),
    opt("mxm_heavy_kernel", &Context::mxm_heavy_kernel),
    opt("drop_hot_cols", &Context::drop_hot_cols),
    opt("mxm_unit_min_flops", &Context::mxm_unit_min_flops),
    opt("mxm_unit_min_per_window", &Context::mxm_unit_min_per_window),
    opt("mxm_masked_units_min_flops", &Context::mxm_masked_units_min_flops),
    opt("mxm_unit_small", &Context::mxm_unit_small, Option::WITHIN, 1, P30),  // (class limits of the SpGEMM units: entry counts)
    opt("mxm_unit_mid", &Context::mxm_unit_mid, Option::WITHIN, 1, P30),
    opt("mxm_unit_dense", &Context::mxm_unit_dense, Option::WITHIN, 1, P30),
    opt("mxm_sym_windows", &Context::mxm_sym_windows, Option::WITHIN, 1, 64),
    opt("mxm_window_groups", &Context::mxm_window_groups, Option::WITHIN, 0, 8, window_group),
    opt("mxm_xcd_map", &Context::mxm_xcd_map, Option::WITHIN, 0, 1),
    opt("mxm_checksum_pass", &Context::mxm_checksum_pass, Option::WITHIN, 0, 1),
    opt("mxm_bitmap_pool_mb", &Context::mxm_bitmap_pool_mb),
    opt("mxm_bitmap_min_cnt", &Context::mxm_bitmap_min_cnt),
    opt("mxm_bitmap_pool_cap", &Context::mxm_bitmap_pool_cap),
    opt("vec_pad_min_bytes", &Context::vec_pad_min_bytes),
    opt("hub_min_len", &Context::hub_min_len, Option::CLAMP, 0, P30),
    opt("fill_absent", &Context::fill_absent, Option::WITHIN, 0, 1),
    opt("rows_tile", &Context::rows_tile, Option::WITHIN, 0, 2),
    opt("lazy_tagged", &Context::lazy_tagged, Option::WITHIN, 0, 1),
    opt("ctile_pack", &Context::ctile_pack, Option::WITHIN, 0, 2, explicit_cold_layout),
    opt("ctile_code", &Context::ctile_code, Option::WITHIN, 0, 1),  // (behind ctile_pack: GrB_init and GrX_options_reset store the rows in this order)
    opt("strip_slot16", &Context::strip_slot16, Option::WITHIN, 0, 1),
    opt("rtile_pack", &Context::rtile_pack, Option::WITHIN, 0, 1),
    opt("cold_in_rows", &Context::cold_in_rows, Option::CLAMP, 0, P30),
    opt("stream_nt_min_nnz", &Context::stream_nt_min_nnz, Option::CLAMP, 0, MAX64),
    opt("bool_probe", &Context::bool_probe, Option::WITHIN, 0, 16),
    opt("rtile_rows", &Context::rtile_rows, Option::ONE_OF, 8192, 16384),
    opt("rtile_entries", &Context::rtile_entries, Option::WITHIN, 256, 1 << 24),
    opt("rows_head", &Context::rows_head, Option::WITHIN, 0, 1),
    opt("rows_head_min_groups", &Context::rows_head_min_groups, Option::CLAMP, 0, MAX64),
    opt("push_small", &Context::push_small, Option::WITHIN, 0, 1),
    opt("value_dict", &Context::value_dict, Option::WITHIN, 0, 1),
    opt("order_mode", &Context::order_mode, Option::WITHIN, 0, 1),
    opt("order_min_nnz", &Context::order_min_nnz, Option::CLAMP, 0, MAX64),
    opt("alloc_cache", &Context::alloc_cache, Option::ANY, 0, 0, release_cache_when_off),
};
constexpr size_t N_OPTIONS = sizeof(OPTIONS) / sizeof(OPTIONS[0]);
int64_t option_initial[N_OPTIONS];  // every option as GrB_init left it: the compiled default, or the environment's override

const Option *option_find(const char *name)
{
    for (const Option &o : OPTIONS)
        if (!strcmp(o.name, name)) return &o;
    return nullptr;
}
int64_t option_load(const Option &o) { return o.i ? (int64_t)(ctx().*o.i) : ctx().*o.l; }
GrB_Info option_store(const Option &o, int64_t v)
{
    if (o.rule == Option::WITHIN && (v < o.lo || v > o.hi)) return GrB_INVALID_VALUE;
    if (o.rule == Option::ONE_OF && v != o.lo && v != o.hi) return GrB_INVALID_VALUE;
    if (o.rule == Option::CLAMP) v = std::max(o.lo, std::min(v, o.hi));
    if (o.hook && !o.hook(v)) return GrB_INVALID_VALUE;
    if (o.i) ctx().*o.i = (int)v;
    else ctx().*o.l = v;
    return GrB_SUCCESS;
}
}  // namespace

}  // namespace grb

using namespace grb;

extern "C" GrB_Info GrB_init(GrB_Mode mode)
{
    Context &c = ctx();
    if (c.initialized) return GrB_INVALID_VALUE;
    if (mode != GrB_BLOCKING && mode != GrB_NONBLOCKING) return GrB_INVALID_VALUE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return GrB_PANIC;  // fail loudly: the product has no CPU path
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return GrB_PANIC;
    c.device = dev;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) c.num_cus = cus;
    }
    c.blocking = (mode == GrB_BLOCKING);
    c.stream = nullptr;
    // keep freed blocks in the pool: BFS/SSSP loops allocate and free the same temporaries every call
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
        uint64_t thresh = UINT64_MAX;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thresh);
    }
    (void)hipGetLastError();
    if (hipEventCreate(&c.ev0) != hipSuccess || hipEventCreate(&c.ev1) != hipSuccess) return GrB_PANIC;
    // The HIP runtime loads a translation unit's code object at the first launch of one of its kernels: several ms for the
    // SpMV unit with its template instantiations -- paid by whichever product came first (it showed up as 8 of the 12.7 ms of
    // the first GrB_mxv of the scale-24 bench).  Load them here, once per process (GRB_PRELOAD=0: on demand, as before).
    if (const char *e = getenv("GRB_PRELOAD"); !e || atoi(e) != 0) {
        preload_mxv();
        preload_mxm();
        preload_vecops();
        preload_object();
        preload_prim();
        preload_select();
        preload_extract();
        preload_apply();
        preload_assign();
        preload_kron();
        preload_diag();
        preload_mxv_posn();
        preload_sort();
        preload_stage();  // (the page-locked blocks of h2d / d2h: not inside the first matrix's layout build)
    }
    if (const char *e = getenv("GRB_DEBUG_FLAGS")) c.debug_flags = atoi(e) & DEBUG_FLAGS_MASK;
    c.initialized = true;  // (an option may release the block cache: only once the context is complete)
    // every option from the environment, as GRB_<NAME in upper case>, through the validation of GrX_option_set (an invalid value is ignored);
    // GRB_DEBUG_FLAGS was read above, where bits the build does not know are dropped instead of rejected
    for (size_t k = 0; k < N_OPTIONS; k++) {
        const Option &o = OPTIONS[k];
        std::string env = "GRB_";
        for (const char *p = o.name; *p; p++) env += (char)toupper((unsigned char)*p);
        const char *e = o.i == &Context::debug_flags ? nullptr : getenv(env.c_str());
        if (e && option_store(o, atoll(e)) != GrB_SUCCESS)
            fprintf(stderr, "libgrb_mi355x: %s=%s rejected (not a valid value of option \"%s\"): the default stays\n", env.c_str(), e, o.name);
        option_initial[k] = option_load(o);  // (what GrX_options_reset returns to)
    }
    return GrB_SUCCESS;
}

// SuiteSparse's initialiser with the caller's allocator (python-graphblas: graphblas/__init__.py:170-173 via
// suitesparse_graphblas.initialize(memory_manager="numpy")): this library allocates nothing on the host for the caller, but the GxB
// import / pack entries take OWNERSHIP of host arrays and release them with `user_free`.
extern "C" GrB_Info GxB_init(GrB_Mode mode, void *(*user_malloc)(size_t), void *(*user_calloc)(size_t, size_t),
                             void *(*user_realloc)(void *, size_t), void (*user_free)(void *))
{
    (void)user_malloc;
    (void)user_calloc;
    (void)user_realloc;
    const GrB_Info info = GrB_init(mode);
    if (info == GrB_SUCCESS) ctx().host_free = user_free;
    return info;
}

extern "C" GrB_Info GrB_finalize(void)
{
    Context &c = ctx();
    if (!c.initialized) return GrB_SUCCESS;
    if (c.push_counters) dev_free(c.push_counters);
    c.push_counters = nullptr;
    dev_cache_release();
    (void)hipStreamSynchronize(c.stream);
    if (c.host_pinned) (void)hipHostFree(c.host_pinned);
    c.host_pinned = nullptr;
    if (c.host_stage) (void)hipHostFree(c.host_stage);
    c.host_stage = nullptr;
    c.host_stage_failed = false;
    if (c.ev0) (void)hipEventDestroy(c.ev0);
    if (c.ev1) (void)hipEventDestroy(c.ev1);
    c.ev0 = c.ev1 = nullptr;
    c.initialized = false;
    return GrB_SUCCESS;
}

extern "C" GrB_Info GrB_getVersion(unsigned int *version, unsigned int *subversion)
{
    if (!version || !subversion) return GrB_NULL_POINTER;
    *version = GRB_VERSION;
    *subversion = GRB_SUBVERSION;
    return GrB_SUCCESS;
}

extern "C" GrB_Info GrX_set_stream(void *hip_stream)
{
    GRB_TRY
    require_init();
    dev_cache_release();  // cached blocks were last used on the old stream
    sync_stream();
    ctx().stream = static_cast<hipStream_t>(hip_stream);
    GRB_CATCH(nullptr)
}

extern "C" GrB_Info GrX_get_stream(void **hip_stream)
{
    GRB_TRY
    require_init();
    if (!hip_stream) fail(GrB_NULL_POINTER, "hip_stream is NULL");
    *hip_stream = (void *)ctx().stream;
    GRB_CATCH(nullptr)
}

extern "C" GrB_Info GrX_synchronize(void)
{
    GRB_TRY
    require_init();
    sync_stream();
    GRB_CATCH(nullptr)
}

extern "C" GrB_Info GrX_trim_memory(void)
{
    GRB_TRY
    require_init();
    sync_stream();
    dev_cache_release();
    sync_stream();
    int dev = 0;
    hipMemPool_t pool;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) (void)hipMemPoolTrimTo(pool, 0);
    (void)hipGetLastError();
    GRB_CATCH(nullptr)
}

extern "C" GrB_Info GrX_timer_start(void)
{
    GRB_TRY
    require_init();
    GRB_HIP(hipEventRecord(ctx().ev0, ctx().stream));
    GRB_CATCH(nullptr)
}

extern "C" GrB_Info GrX_timer_stop(float *elapsed_ms)
{
    GRB_TRY
    require_init();
    if (!elapsed_ms) fail(GrB_NULL_POINTER, "elapsed_ms is NULL");
    GRB_HIP(hipEventRecord(ctx().ev1, ctx().stream));
    GRB_HIP(hipEventSynchronize(ctx().ev1));
    GRB_HIP(hipEventElapsedTime(elapsed_ms, ctx().ev0, ctx().ev1));
    GRB_CATCH(nullptr)
}

extern "C" GrB_Info GrX_last_stats(GrX_Stats *stats)
{
    if (!stats) return GrB_NULL_POINTER;
    *stats = ctx().stats;
    return GrB_SUCCESS;
}

extern "C" GrB_Info GrX_option_set(const char *name, int64_t value)
{
    if (!name) return GrB_NULL_POINTER;
    const Option *o = option_find(name);
    return o ? option_store(*o, value) : GrB_INVALID_VALUE;
}

extern "C" GrB_Info GrX_option_get(const char *name, int64_t *value)
{
    if (!name || !value) return GrB_NULL_POINTER;
    const Option *o = option_find(name);
    if (!o) return GrB_INVALID_VALUE;
    *value = option_load(*o);
    return GrB_SUCCESS;
}

extern "C" GrB_Info GrX_options_reset(void)
{
    if (!ctx().initialized) return GrB_PANIC;
    for (size_t k = 0; k < N_OPTIONS; k++)
        if (option_store(OPTIONS[k], option_initial[k]) != GrB_SUCCESS) return GrB_PANIC;  // (a stored value is a valid value)
    return GrB_SUCCESS;
}

extern "C" const char *GrX_version_string(void) { return "grb-mi355x 0.1 (gfx950, GraphBLAS C API 2.0 subset)"; }
