// gradus_mi355x.hip -- host side of libgradus_mi355x.so: the C ABI of include/gradus_mi355x.h, contexts, staging and the
// dispatch to the per-metric kernel objects (kernels_tu.hip, one translation unit per metric id and precision).
//
// Two launch shapes for the same per-lane integrator (gr_device.hpp):
//   kernel 0  "lane"        one ray per work-item, 8x8-pixel tiles per wave; a wave lives as
//                           long as its slowest ray.
//   kernel 1  "persistent"  a resident grid pulls rays from a global counter; when enough lanes
//                           of a wave have finished (wave ballot), their results are written and
//                           they are refilled with new rays, so lanes stay busy although step
//                           counts differ ~4x between rays.
// Output is one double per ray (fused PointFunction) or one 152-byte GeodesicPoint per ray.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#define GR_NS gr
#define GR_RADTRANS_LAYOUT 1      // Cold with the two pointers of the TraceRadiativeTransfer kernels behind everything else (gr_device.hpp)
#include "gr_device.hpp"
#include "gr_stats_fold.hpp"
#include "gr_tile_order.hpp"
#include "gr_mesh_grid.hpp"
#include "gr_lagbin.hpp"
#include "gr_tfint.hpp"
#include "gr_tftd.hpp"
#include "gr_ringarm.hpp"
#include "gr_skygrid.hpp"
#include "gr_planegrid.hpp"
#include "gr_offsetsolve.hpp"

using namespace gr;

// ---- the per-metric kernel objects (kernels_tu.hip) ----
#define GR_DECLARE_METRIC(ID)                                                                                          \
    hipError_t gr64_launch_trace_m##ID(int, int, int, int, unsigned long long*, const void*, hipStream_t);             \
    hipError_t gr32_launch_trace_m##ID(int, int, int, int, unsigned long long*, const void*, hipStream_t);             \
    hipError_t grt_launch_trace_m##ID(int, int, int, int, unsigned long long*, const void*, hipStream_t);              \
    hipError_t grt1_launch_trace_m##ID(int, int, int, int, unsigned long long*, const void*, hipStream_t);             \
    hipError_t grts_launch_trace_m##ID(int, int, int, int, unsigned long long*, const void*, hipStream_t);             \
    hipError_t grts1_launch_trace_m##ID(int, int, int, int, unsigned long long*, const void*, hipStream_t);            \
    hipError_t gr64_launch_path_m##ID(const void*, double*, int64_t, unsigned long long*, hipStream_t);                \
    hipError_t gr64_launch_apply_m##ID(const void*, const gr_point*, double, double*, hipStream_t);                     \
    hipError_t gr64_launch_classify_m##ID(const void*, uint8_t*, int64_t, hipStream_t);                                \
    hipError_t gr64_launch_areafactor_m##ID(const void*, const double*, double*, hipStream_t);                         \
    hipError_t grv1_launch_offset_m##ID(const void*, const void*, int, hipStream_t);
GR_DECLARE_METRIC(0) GR_DECLARE_METRIC(1) GR_DECLARE_METRIC(2) GR_DECLARE_METRIC(3) GR_DECLARE_METRIC(4) GR_DECLARE_METRIC(5)
GR_DECLARE_METRIC(6) GR_DECLARE_METRIC(7) GR_DECLARE_METRIC(8) GR_DECLARE_METRIC(9) GR_DECLARE_METRIC(10)
#undef GR_DECLARE_METRIC
// GR_METRIC_TABULATED (11): every flavour of the trace kernels (the fp32 ones evaluate the fp64 table in double, gr_device.hpp)
hipError_t gr64_launch_trace_m11(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t gr32_launch_trace_m11(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grt_launch_trace_m11(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grt1_launch_trace_m11(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grts_launch_trace_m11(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grts1_launch_trace_m11(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t gr64_launch_path_m11(const void*, double*, int64_t, unsigned long long*, hipStream_t);
hipError_t gr64_launch_apply_m11(const void*, const gr_point*, double, double*, hipStream_t);
hipError_t gr64_launch_classify_m11(const void*, uint8_t*, int64_t, hipStream_t);
hipError_t gr64_launch_areafactor_m11(const void*, const double*, double*, hipStream_t);
hipError_t grv1_launch_offset_m11(const void*, const void*, int, hipStream_t);
// TraceRadiativeTransfer (kernels_tu.hip -DGR_TU_RT -> kernelsrt_m<id>.o): the catalogue metrics that have an ISCO
hipError_t grrt_launch_trace_m0(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grrt_launch_trace_m1(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grrt_launch_trace_m3(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grrt_launch_trace_m4(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grrt_launch_trace_m5(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grrt_launch_trace_m6(int, int, int, int, unsigned long long*, const void*, hipStream_t);
hipError_t grrt_launch_trace_m9(int, int, int, int, unsigned long long*, const void*, hipStream_t);
static_assert(GR_METRIC_NOZ == 10 && GR_METRIC_TABULATED == 11, "one kernel object per metric id 0..11: extend the tables below with the catalogue");

namespace {
struct LaunchKnobs {
    int kernel;              // 0 = lane, 1 = persistent
    int block;
    int n_cu;
    int waves_per_simd;      // 0 = from the occupancy query
    unsigned long long* queue;   // work counter of the persistent kernel (zeroed by the launcher)
};
typedef hipError_t (*trace_fn)(int, int, int, int, unsigned long long*, const void*, hipStream_t);
typedef hipError_t (*path_fn)(const void*, double*, int64_t, unsigned long long*, hipStream_t);
typedef hipError_t (*apply_fn)(const void*, const gr_point*, double, double*, hipStream_t);
typedef hipError_t (*classify_fn)(const void*, uint8_t*, int64_t, hipStream_t);
typedef hipError_t (*areafactor_fn)(const void*, const double*, double*, hipStream_t);
typedef hipError_t (*offset_fn)(const void*, const void*, int, hipStream_t);
#define GR_ROW(F, LAST) { F##0, F##1, F##2, F##3, F##4, F##5, F##6, F##7, F##8, F##9, F##10, LAST }
const trace_fn kTrace64[12] = GR_ROW(gr64_launch_trace_m, gr64_launch_trace_m11);
const trace_fn kTrace32[12] = GR_ROW(gr32_launch_trace_m, gr32_launch_trace_m11);
const trace_fn kTraceTan[12] = GR_ROW(grt_launch_trace_m, grt_launch_trace_m11);      // value + ∂/∂α + ∂/∂β (out_mode 5): one lane per ray
const trace_fn kTraceTan1[12] = GR_ROW(grt1_launch_trace_m, grt1_launch_trace_m11);   // the same with a PAIR of lanes per ray (kernels_tu.hip)
const trace_fn kTraceSky[12] = GR_ROW(grts_launch_trace_m, grts_launch_trace_m11);     // the same two shapes with the sky-cell branches (out_mode 6,
const trace_fn kTraceSky1[12] = GR_ROW(grts1_launch_trace_m, grts1_launch_trace_m11);  // gr_sky_cells): instantiations of their own (kernels_tu.hip)
const path_fn kPath64[12] = GR_ROW(gr64_launch_path_m, gr64_launch_path_m11);
const apply_fn kApply64[12] = GR_ROW(gr64_launch_apply_m, gr64_launch_apply_m11);
const classify_fn kClassify64[12] = GR_ROW(gr64_launch_classify_m, gr64_launch_classify_m11);      // the live-first tile order's flags (gr_tile_order.hpp)
const areafactor_fn kAreaFactor64[12] = GR_ROW(gr64_launch_areafactor_m, gr64_launch_areafactor_m11);      // γ(r) A(r) of the disc (kernelsarea_m<id>.o)
const offset_fn kOffsetSolve1[12] = GR_ROW(grv1_launch_offset_m, grv1_launch_offset_m11);      // k_offset_solve / k_offset_search (kernelssolve1_m<id>.o)
#undef GR_ROW
// the radiative-transfer kernels, null where the metric has no ISCO (Morris-Thorne, flat space, Kerr with dark matter, no-Z) and for a table
const trace_fn kTraceRT[12] = { grrt_launch_trace_m0, grrt_launch_trace_m1, nullptr, grrt_launch_trace_m3, grrt_launch_trace_m4, grrt_launch_trace_m5,
                                grrt_launch_trace_m6, nullptr, nullptr, grrt_launch_trace_m9, nullptr, nullptr };
// Metric::kEscapeRadiusM per metric id, in units of params[0] (escape_cull_radius)
#define GR_ESC(ID) MetricOf<ID>::type::kEscapeRadiusM
const double kEscapeRadiusM[12] = { GR_ESC(0), GR_ESC(1), GR_ESC(2), GR_ESC(3), GR_ESC(4), GR_ESC(5), GR_ESC(6), GR_ESC(7),
                                    GR_ESC(8), GR_ESC(9), GR_ESC(10), GR_ESC(11) };
#undef GR_ESC
}  // namespace

namespace {

thread_local std::string g_last_error;
int32_t fail(int32_t code, const std::string& msg);

// ---- GR_METRIC_COMPILED: kernel modules loaded at run time (gr_metric_module_load; kernels_tu.hip -DGR_TU_USER) ----
// what was hashed into this unit at build time (__graft_entry__.csrc_hash): a module compiled against other sources is refused
#ifndef GR_CSRC_HASH
#define GR_CSRC_HASH 0, 0, 0, 0
#endif
const int64_t kCsrcHash[4] = { GR_CSRC_HASH };
std::string hash_hex(const int64_t* w)
{
    char buf[65];
    std::snprintf(buf, sizeof buf, "%016llx%016llx%016llx%016llx", (unsigned long long)w[0], (unsigned long long)w[1],
                  (unsigned long long)w[2], (unsigned long long)w[3]);
    return buf;
}
typedef hipError_t (*attrs_fn)(int, int, hipFuncAttributes*);
// the launchers of one metric: a row of the tables above, or a module's
struct MetricKernels {
    trace_fn trace64 = nullptr, trace32 = nullptr, tan = nullptr, tan1 = nullptr, sky = nullptr, sky1 = nullptr;
    path_fn path = nullptr;
    apply_fn apply = nullptr;
    classify_fn classify = nullptr;
    areafactor_fn area = nullptr;
    offset_fn offset = nullptr;
    attrs_fn attrs64 = nullptr, attrs_tan = nullptr, attrs_tan1 = nullptr;      // modules only
    int64_t build_id = 0;                                                       // modules only: what caches key on
};
struct ModuleSlot {
    bool used = false;
    void* handle = nullptr;
    MetricKernels k;
};
std::mutex g_modules_mu;
ModuleSlot g_modules[GR_METRIC_MODULE_SLOTS];

// THE accessor of every per-metric dispatch: false for an id that names neither a catalogue metric nor a loaded module
bool metric_kernels(int32_t id, MetricKernels& out)
{
    if (id >= GR_METRIC_KERR && id <= GR_METRIC_TABULATED) {
        out = MetricKernels{};
        out.trace64 = kTrace64[id]; out.trace32 = kTrace32[id]; out.tan = kTraceTan[id]; out.tan1 = kTraceTan1[id];
        out.sky = kTraceSky[id]; out.sky1 = kTraceSky1[id]; out.path = kPath64[id]; out.apply = kApply64[id];
        out.classify = kClassify64[id]; out.area = kAreaFactor64[id]; out.offset = kOffsetSolve1[id];
        return true;
    }
    if (id < GR_METRIC_COMPILED || id >= GR_METRIC_COMPILED + GR_METRIC_MODULE_SLOTS) return false;
    std::lock_guard<std::mutex> lock(g_modules_mu);
    const ModuleSlot& m = g_modules[id - GR_METRIC_COMPILED];
    if (!m.used) return false;
    out = m.k;
    return true;
}
bool metric_known(int32_t id)
{
    MetricKernels k;
    return metric_kernels(id, k);
}
// the build id of a compiled metric's module, 0 for the catalogue: part of every cache key that holds a metric (slots are reused)
int64_t metric_build_id(int32_t id)
{
    MetricKernels k;
    return (id >= GR_METRIC_COMPILED && metric_kernels(id, k)) ? k.build_id : 0;
}
// Metric::kEscapeRadiusM of a metric id: a compiled metric is never culled (GenericMetricT)
double metric_escape_radius_m(int32_t id) { return (id >= 0 && id <= GR_METRIC_TABULATED) ? kEscapeRadiusM[id] : HUGE_VAL; }
// a flavour the metric has no kernel for (a module without the tangent objects, say)
#define GR_NEED_KERNEL(fn, what)                                                                                       \
    do {                                                                                                               \
        if (!(fn)) return fail(GR_ERR_UNSUPPORTED, std::string("this metric has no ") + (what) + " kernels");         \
    } while (0)

std::atomic<int> g_live_ctx{ 0 };     // contexts alive: the pool of page-locked blocks is emptied when the last one goes

int32_t fail(int32_t code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

}  // namespace
// for the library's other host units (metric_table.hip)
int32_t gr_set_last_error(int32_t code, const char* msg) { return fail(code, msg); }
int32_t gr_metric_table_check(const double* table, int64_t table_n);      // metric_table.hip
namespace {

#define GR_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? GR_ERR_OUT_OF_MEMORY : GR_ERR_HIP,            \
                        std::string(#call) + ": " + hipGetErrorString(e_));                       \
    } while (0)

}  // namespace

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
struct gr_ctx {
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr;          // used by the host-buffer entry points
    unsigned long long* d_queue = nullptr; // ring of work counters (one per in-flight launch)
    int queue_slots = 64, queue_next = 0;
    unsigned long long* d_stats = nullptr; // for host-buffer entry points
    unsigned long long* d_stat_part = nullptr; // ring of partials blocks (gr_stats_fold.hpp), one per in-flight launch: all zero between launches
    int stat_next = 0;
    double* d_disc_table = nullptr;        // device copy of a tabulated disc profile
    size_t disc_table_bytes = 0;
    double* d_mesh = nullptr;              // GR_DISC_MESH: the grid-sorted triangle table (gr_mesh_grid.hpp), kept while the
    size_t mesh_bytes = 0;                 //   caller passes the same mesh (fingerprint of its table)
    uint64_t mesh_fp = 0;
    int64_t mesh_n = -1;
    std::vector<double> mesh_host;
    double* d_sky = nullptr;               // a sky source's (x, v) arrays, written by k_sky_velocities for the trace kernels
    unsigned* d_sky_table = nullptr;       // ... dealt by cost: counts, then offsets, per (class, chunk) (k_sky_velocities_dealt)
    size_t sky_table_bytes = 0;
    size_t sky_bytes = 0;
    int64_t sky_first = 0, sky_total = 0;  // the share of a sky source the launch being prepared traces (rays_params -> sky_prepare)
    bool sky_any_order = false;            // ... whose rows may come in any order (gr_corona_trace): the rays are dealt by predicted cost
    const double* sky_rows = nullptr;      // ... and its per-sample rows (gr_rayset.sky_rows, device) or null
    double* d_corona = nullptr;            // gr_corona_trace: (g, ρ, t, status) per ray, kept for gr_corona_bin
    size_t corona_bytes = 0;
    int64_t corona_n = -1, corona_hits = 0;
    double corona_gmax = 0.0, corona_tmax = 0.0;
    double* d_lag = nullptr;               // gr_lagtransfer_trace: (g, ρ, t, area) per ray of the observer's plane, kept for gr_lagtransfer_bin
    size_t lag_bytes = 0;
    int64_t lag_n = -1, lag_hits = 0;
    double* d_metric_table = nullptr;      // GR_METRIC_TABULATED: device copy of the caller's table, kept while its build id stays
    size_t metric_table_bytes = 0;
    double metric_table_id = 0.0;
    double* d_chart_table = nullptr;       // device copy of a PoloidalShapeChart table
    size_t chart_table_bytes = 0;
    Cold* d_cold = nullptr;                // ring of per-launch cold blocks
    gr_transfer* d_transfer = nullptr;     // ring of per-launch medium blocks of the gr_transfer_* calls (made at the first of them)
    int transfer_next = 0;
    int cold_next = 0;
    double* d_plunge = nullptr;            // 4 x n_plunge
    int64_t plunge_cap = 0;
    void* d_scratch = nullptr;             // staging for host-buffer entry points
    size_t scratch_bytes = 0;
    void* d_in = nullptr;
    size_t in_bytes = 0;
    double* d_offset_work = nullptr;       // gr_offset_solve / gr_offset_search: α | β | row of the ray every problem is tracing
    size_t offset_work_bytes = 0;
    // knobs
    int64_t kernel = 2;                    // 0 lane, 1 persistent, 2 auto (by launch depth)
    int64_t lpt_lane = 0;                  // also order tiles longest-first for the lane kernel
    int64_t block = 0;                    // 0 = auto: 64 for the one-ray-per-lane kernel, 256 for the persistent one
    int64_t refill_threshold = 0;          // idle lanes that trigger a refill; 0 = auto: 16 for the fp64 kernels, 32 for the fp32 ones
    int64_t waves_per_simd = 0;            // 0 = from occupancy query
    int64_t swizzle = 1;
    int64_t tile_rows = 8;                 // rows of the pixel tile of a wave: 8 (8 x 8) or 16 (16 x 4: whole 128-B lines per store)
    int64_t precision = 64;                // 64 = fp64 kernels, 32 = fp32 kernels (tolerance sweeps)
    int64_t lds = 1;                       // stage the plunging table / line-profile histogram in LDS
    int64_t lpt = 1;                       // longest-first tile order learned from the previous render
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_k = nullptr;             // end of the last trace kernel of a host call (gr_stats.kernel_ms vs call_ms)
    int64_t hugepages = 1;                 // madvise(MADV_HUGEPAGE) on large caller-owned result buffers before pre-faulting
    int64_t lds_points = 1;                // one-ray-per-lane kernel: a wave's end-point records leave through LDS as whole runs
    int64_t direct_host = 1;               // gr_render_endpoints into a gr_host_alloc block: the kernel stores across the link itself
    int64_t tangent_pairs = 2;             // tangent kernels: 0 = one lane per ray, 1 = a pair of lanes per ray, 2 = by launch size
    int64_t tf_chunk = 0;                  // gr_tf_lineprofile / gr_tf_lagtransfer: annuli per workgroup, 0 = auto (the launch shape only)
    int64_t sky_deal = 1;                  // gr_corona_trace: the sky rays of a source dealt to the waves by predicted cost (k_sky_velocities_dealt)
    int64_t xcd_spread = 1;                // one-ray-per-lane kernel, rays in caller order: chunks dealt over the XCDs by digit sum
    int64_t tangent_norm = 1;              // tangent kernels: the tangents are part of the error norm (DiffEqBase on Dual state); 0 = values only
    // LPT state for one (config, plane, range) key
    std::vector<unsigned char> lpt_key;
    uint32_t* d_tile_cost = nullptr;
    uint32_t* d_tile_perm = nullptr;
    int64_t lpt_tiles = 0, lpt_cap = 0;
    bool lpt_have_perm = false, lpt_cost_pending = false;
    hipEvent_t ev_cost = nullptr;
    // live-first tile order (gr_tile_order.hpp): a ring of permutations (live_cap + 1 words each: the live count behind the tiles)
    // and of flag blocks (live_cap bytes each), one per in-flight launch like the cold blocks, written and read under stream order
    int64_t live_first = 1;                // 0 off, 1 auto (launch_trace), 2 always (tests)
    uint32_t* d_live_perm = nullptr;
    uint8_t* d_live_flags = nullptr;
    int64_t live_cap = 0;                  // tiles per slot, a multiple of 8
    int live_next = 0;
    const uint32_t* live_last = nullptr;   // the permutation of the last trace launch (null: it kept its order) and its tiles
    int64_t live_last_tiles = 0;
    // The staged tables (plunging table, disc profile, chart) are single ctx-owned buffers.  A launch that reads
    // them records `ev_tables` on its stream; the next staging on a DIFFERENT stream first waits for that event,
    // so a table is never overwritten under a kernel that is still reading it (launches without tables -- Kerr
    // with a thin disc, the bench workload -- never wait on each other).
    hipEvent_t ev_tables = nullptr;
    hipStream_t tables_stream = nullptr;
    bool tables_busy = false;
    // host-buffer entry points that return 152 B per ray: the result goes back in bands on a second stream while later
    // bands are still being traced (see Bands)
    hipStream_t copy_stream = nullptr;
    hipStream_t band_stream = nullptr;     // odd bands are traced here, even ones on `stream`: the tail of one band's launch
                                           // (SIMDs draining) overlaps the head of the next
    hipEvent_t ev_fork = nullptr;
    hipEvent_t ev_band[8] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    bool lpt_suspend = false;              // banded launches do not learn / use a tile order (their ranges differ)
    int64_t pipeline = 4;                  // bands of the end-point return (0 / 1: one launch + one copy)
    bool counted = false;                  // this context is in g_live_ctx
};

namespace {

int32_t ensure(void** buf, size_t* cap, size_t need)
{
    if (*cap >= need) return GR_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    GR_HIP(hipMalloc(buf, need));
    *cap = need;
    return GR_OK;
}

// make `stream` wait for the last launch that read the ctx-owned staged tables (if it ran on another stream)
int32_t tables_acquire(gr_ctx* ctx, hipStream_t stream)
{
    if (ctx->tables_busy && ctx->tables_stream != stream) GR_HIP(hipStreamWaitEvent(stream, ctx->ev_tables, 0));
    return GR_OK;
}
// called after a launch that reads staged tables
int32_t tables_release(gr_ctx* ctx, hipStream_t stream)
{
    GR_HIP(hipEventRecord(ctx->ev_tables, stream));
    ctx->tables_stream = stream;
    ctx->tables_busy = true;
    return GR_OK;
}

int32_t validate_cfg(const gr_config* cfg)
{
    if (!cfg) return fail(GR_ERR_INVALID_ARGUMENT, "config is null");
    if (!metric_known(cfg->metric_id))      // the catalogue, or a module that is loaded now (gr_metric_module_load)
        return fail(GR_ERR_UNSUPPORTED, "unknown metric_id " + std::to_string(cfg->metric_id)
                                        + (cfg->metric_id >= GR_METRIC_COMPILED ? " (no kernel module is loaded under it)" : ""));
    if (cfg->metric_id == GR_METRIC_TABULATED) {
        const int32_t trc = gr_metric_table_check(cfg->metric_table, cfg->metric_table_n);
        if (trc != GR_OK) return trc;
        // The table is polynomials: outside [r_min, r_max] they extrapolate to garbage (g_tt = -3e4 at ten times r_max).  A ray
        // lives between the chart's boundaries, so the chart has to lie inside the table (a hair of slack: the Python and Julia
        // hosts plan r_min a part in a thousand inside the chart's inner radius).
        const double t_min = cfg->metric_table[gr_tab::H_RMIN], t_max = cfg->metric_table[gr_tab::H_RMAX];
        double c_in = cfg->r_inner;
        if (cfg->chart_table_n > 1 && cfg->chart_table)
            for (int64_t k = 0; k < cfg->chart_table_n; ++k) c_in = k == 0 ? cfg->chart_table[k] : std::fmin(c_in, cfg->chart_table[k]);
        if (!(c_in >= t_min - 1e-9 * std::fabs(t_min) - 1e-12) || !(cfg->r_outer <= t_max + 1e-9 * std::fabs(t_max)))
            return fail(GR_ERR_INVALID_ARGUMENT, "GR_METRIC_TABULATED: the chart [" + std::to_string(c_in) + ", " + std::to_string(cfg->r_outer)
                                                 + "] leaves the radial range of the metric table [" + std::to_string(t_min) + ", "
                                                 + std::to_string(t_max) + "]: fit the table on a range that contains the chart");
    }
    if (cfg->disc_id < GR_DISC_NONE || cfg->disc_id > GR_DISC_MESH)
        return fail(GR_ERR_UNSUPPORTED, "unknown disc_id " + std::to_string(cfg->disc_id));
    if (cfg->disc_id == GR_DISC_COMPOSITE) {
        if (cfg->comp_n < 2 || cfg->comp_n > GR_COMP_MAX)
            return fail(GR_ERR_INVALID_ARGUMENT, "a composite geometry has 2.." + std::to_string(GR_COMP_MAX) + " components");
        for (int k = 0; k < cfg->comp_n; ++k) {
            const int id = cfg->comp[k].disc_id;
            if (id != GR_DISC_THIN && id != GR_DISC_SHAKURA_SUNYAEV && id != GR_DISC_ELLIPTICAL && id != GR_DISC_DATUM)
                return fail(GR_ERR_UNSUPPORTED, "composite geometry: component " + std::to_string(k) + " must be a thin disc, a Shakura-Sunyaev "
                                                "disc, an elliptical disc or a datum plane");
            if (id == GR_DISC_THIN && !(cfg->comp[k].disc_r_out >= cfg->comp[k].disc_r_in))
                return fail(GR_ERR_INVALID_ARGUMENT, "composite geometry: disc outer radius below inner radius");
        }
    }
    if (!(cfg->abstol > 0.0) || !(cfg->reltol > 0.0))
        return fail(GR_ERR_INVALID_ARGUMENT, "abstol and reltol must be positive");
    if (!(cfg->lambda1 > cfg->lambda0))
        return fail(GR_ERR_INVALID_ARGUMENT, "λ domain must be increasing");
    if (cfg->maxiters <= 0) return fail(GR_ERR_INVALID_ARGUMENT, "maxiters must be positive");
    if (cfg->disc_id == GR_DISC_TABULATED && (!cfg->disc_table || cfg->disc_table_n < 2 || !(cfg->disc_params[1] > cfg->disc_params[0])))
        return fail(GR_ERR_INVALID_ARGUMENT, "tabulated disc needs >= 2 samples on an increasing ρ grid");
    if (cfg->disc_id == GR_DISC_MESH && (!cfg->disc_table || cfg->disc_table_n < 1 || cfg->disc_table_n > (int64_t)1 << 24))
        return fail(GR_ERR_INVALID_ARGUMENT, "a mesh geometry needs its bounding box and 1 .. 2^24 triangles in disc_table");
    if (cfg->chart_table_n < 0 || cfg->chart_table_n == 1 || (cfg->chart_table_n > 1 && (!cfg->chart_table || !(cfg->chart_theta1 > cfg->chart_theta0))))
        return fail(GR_ERR_INVALID_ARGUMENT, "chart table needs >= 2 samples on an increasing θ grid");
    if (cfg->disc_id == GR_DISC_THIN && !(cfg->disc_r_out >= cfg->disc_r_in))
        return fail(GR_ERR_INVALID_ARGUMENT, "disc outer radius below inner radius");
    return GR_OK;
}

int32_t validate_plane(const gr_plane* pl, const gr_range* rg)
{
    if (!pl || !rg) return fail(GR_ERR_INVALID_ARGUMENT, "plane/range is null");
    if (pl->width <= 0 || pl->height <= 0) return fail(GR_ERR_INVALID_ARGUMENT, "image dimensions must be positive");
    // @assert issorted(αlims), rendering.jl:148-149
    if (pl->alpha0 > pl->alpha1) return fail(GR_ERR_INVALID_ARGUMENT, "α limits must be sorted");
    if (pl->beta0 > pl->beta1) return fail(GR_ERR_INVALID_ARGUMENT, "β limits must be sorted");
    if (rg->count < 0 || rg->first < 0 || rg->block <= 0 || rg->stride_blocks <= 0)
        return fail(GR_ERR_INVALID_ARGUMENT, "bad ray range");
    if (rg->count > 0) {
        const int64_t last = rg->count - 1;
        const int64_t b = last / rg->block;
        const int64_t i = rg->first + b * rg->stride_blocks * rg->block + (last - b * rg->block);
        if (i >= pl->width * pl->height) return fail(GR_ERR_INVALID_ARGUMENT, "ray range exceeds the image");
    }
    return GR_OK;
}

// device copies of the tabulated chart and disc profile (cfg.chart_table / cfg.disc_table are host
// pointers); records "PoloidalShapeChart active" in bit 1 and "count windings" in bit 2 of the private copy of
// cfg.upper_hemisphere
// GR_METRIC_TABULATED: the device copy of the caller's table (uploaded when its build id changes), its header into cfg.params
// and its device address into the private copy of cfg.metric_table -- what TabulatedMetric::load reads
int32_t stage_metric_table(gr_ctx* ctx, Params& p, hipStream_t stream)
{
    if (p.cfg.metric_id != GR_METRIC_TABULATED) return GR_OK;
    const double* t = p.cfg.metric_table;
    const size_t bytes = sizeof(double) * (size_t)p.cfg.metric_table_n;
    const double id = t[gr_tab::H_BUILD_ID];
    if (!ctx->d_metric_table || ctx->metric_table_id != id || ctx->metric_table_bytes < bytes) {
        const int32_t arc = tables_acquire(ctx, stream);
        if (arc != GR_OK) return arc;
        ctx->metric_table_id = 0.0;
        const int32_t rc = ensure((void**)&ctx->d_metric_table, &ctx->metric_table_bytes, bytes);
        if (rc != GR_OK) return rc;
        GR_HIP(hipMemcpyAsync(ctx->d_metric_table, t, bytes, hipMemcpyHostToDevice, stream));
        GR_HIP(hipStreamSynchronize(stream));      // the caller's table may be pageable and gone after the call; once per table
        ctx->metric_table_id = id;
    }
    gr_tab::stage_params(t, p.cfg.params);
    p.cfg.metric_table = ctx->d_metric_table;
    return GR_OK;
}

int32_t stage_disc_table(gr_ctx* ctx, Params& p, hipStream_t stream)
{
    {
        const int32_t mrc = stage_metric_table(ctx, p, stream);
        if (mrc != GR_OK) return mrc;
    }
    p.chart_table = nullptr;
    p.cfg.upper_hemisphere = p.cfg.upper_hemisphere ? 1 : 0;
    if (p.cfg.chart_table_n > 1 || p.cfg.disc_id == GR_DISC_TABULATED || p.cfg.disc_id == GR_DISC_MESH) {
        const int32_t arc = tables_acquire(ctx, stream);
        if (arc != GR_OK) return arc;
    }
    if (p.cfg.chart_table_n > 1) {
        const size_t cb = sizeof(double) * (size_t)p.cfg.chart_table_n;
        int32_t crc = ensure((void**)&ctx->d_chart_table, &ctx->chart_table_bytes, cb);
        if (crc != GR_OK) return crc;
        GR_HIP(hipMemcpyAsync(ctx->d_chart_table, p.cfg.chart_table, cb, hipMemcpyHostToDevice, stream));
        p.chart_table = ctx->d_chart_table;
        p.cfg.upper_hemisphere |= 2;
    }
    if (p.cfg.count_windings) p.cfg.upper_hemisphere |= 4;     // TraceWindings: bit 2
    p.disc_table = nullptr;
    if (p.cfg.disc_id == GR_DISC_MESH) {
        // the caller's triangles -> the grid-sorted table the kernels walk; rebuilt only when the mesh changes
        const int64_t n = p.cfg.disc_table_n;
        const uint64_t fp = gr_mesh::fingerprint(p.cfg.disc_table, n);
        if (ctx->mesh_n != n || ctx->mesh_fp != fp || !ctx->d_mesh) {
            if (!gr_mesh::vertices_finite(p.cfg.disc_table, n)) return fail(GR_ERR_INVALID_ARGUMENT, "the mesh has a vertex that is not finite");
            gr_mesh::build_table(p.cfg.disc_table, n, ctx->mesh_host);
            const size_t mb = sizeof(double) * ctx->mesh_host.size();
            ctx->mesh_n = -1;
            const int32_t mrc = ensure((void**)&ctx->d_mesh, &ctx->mesh_bytes, mb);
            if (mrc != GR_OK) return mrc;
            GR_HIP(hipMemcpyAsync(ctx->d_mesh, ctx->mesh_host.data(), mb, hipMemcpyHostToDevice, stream));
            // mesh_host is rebuilt in place by the next mesh: the copy out of it must have finished by then (the device entry
            // points run on a caller's stream that nothing else would wait for).  Once per mesh.
            GR_HIP(hipStreamSynchronize(stream));
            ctx->mesh_n = n;
            ctx->mesh_fp = fp;
        }
        p.disc_table = ctx->d_mesh;
        return GR_OK;
    }
    if (p.cfg.disc_id != GR_DISC_TABULATED) return GR_OK;
    const size_t tb = sizeof(double) * (size_t)p.cfg.disc_table_n;
    int32_t rc = ensure((void**)&ctx->d_disc_table, &ctx->disc_table_bytes, tb);
    if (rc != GR_OK) return rc;
    GR_HIP(hipMemcpyAsync(ctx->d_disc_table, p.cfg.disc_table, tb, hipMemcpyHostToDevice, stream));
    p.disc_table = ctx->d_disc_table;
    return GR_OK;
}

// Longest-processing-time-first order of the 8x8 tiles.  The first render of a plane records the
// step count of one ray per tile; the next render of the SAME (config, plane, range) sorts the
// tiles by that cost, longest first, so the rays started last are the short ones and the tail of
// the launch (queue empty, waves draining) shrinks.  Only the ORDER of the work queue is learned:
// every ray is traced in full every time and results are bit-identical with or without it.
// Which launch shape a launch of n rays gets under kernel = 2 (auto).  Measured on MI355X with
// Launch shape when the caller leaves it to the library (kernel = 2, block = 0).  Measured on MI355X
// (scripts/kernel_shapes.py, bench.py --emulate-shard):
//  * image planes (8x8 pixel tiles per wave): one ray per lane in ONE-WAVE workgroups.  The hardware
//    dispatcher then refills a SIMD the moment a single wave retires, which beats the persistent
//    kernel's wave-ballot refill at every depth (2048²: 23.3 vs 23.8 ms; 1/8 shard: 3.3 vs 3.7 ms;
//    Johannsen 1024²: 8.5 vs 9.6 ms), and 256-thread workgroups of the same kernel by 5-10 %.
//  * line profiles: persistent (every workgroup flushes its LDS histogram at exit; a quarter of a
//    million one-wave workgroups would turn that into 5e7 global atomics: 31 vs 21 ms at 2048² rays).
//  * ray arrays in caller order (no tiles, neighbours may differ wildly in length): persistent with
//    wave-ballot refill, except for launches only a few rays per resident lane deep.
//  * a tabulated metric: the lane kernel whatever the source of the rays.  Refilled lanes take rays from anywhere in the set, a
//    wave's rays then sit in as many patches as it has lanes and most evaluations leave the patch cache for global memory
//    (10⁶ sky rays of a corona: 170 ms against 84; 2²⁰ rays in random order: 179 against 138).
int resolve_kernel(const gr_ctx* ctx, int64_t n, const Cold& cold, int metric_id = -1)
{
    if (ctx->kernel != 2) return (int)ctx->kernel;
    // a tabulated metric: one ray per lane whatever the launch -- a refilled wave's rays sit in more patches than its cache has
    // slots (BinningMethod line profile, 4096² rays at tolerance 1e-5: 69 ms against 158 through the persistent kernel; 203 either
    // way at 1e-9; scripts/sibling_workloads.py tabc5lo)
    if (metric_id == GR_METRIC_TABULATED) return 0;
    if (cold.out_mode == 2) return 1;
    if (cold.src_mode == 0 && cold.swizzle) return 0;
    const int64_t resident_lanes = (int64_t)ctx->n_cu * 8 * 64;
    return n < 6 * resident_lanes ? 0 : 1;
}
int resolve_block(const gr_ctx* ctx, int kernel)
{
    if (ctx->block) return (int)ctx->block;
    return kernel == 0 ? 64 : 256;
}

int32_t lpt_prepare(gr_ctx* ctx, const Params& p, Cold& cold, hipStream_t stream, bool* record)
{
    *record = false;
    cold.tile_perm = nullptr;
    cold.tile_cost = nullptr;
    const int kern = resolve_kernel(ctx, p.n, cold, p.cfg.metric_id);
    // (a tabulated metric's lane kernel orders its tiles longest-first by default: its waves' lifetimes spread 9x around their
    // mean -- the fused kernels' 2.7x -- and the cost it learns is the wave's lifetime, not a step count)
    const bool tab = p.cfg.metric_id == GR_METRIC_TABULATED;
    if (!ctx->lpt || ctx->lpt_suspend || (kern != 1 && !ctx->lpt_lane && !tab) || !cold.swizzle || cold.src_mode != 0) return GR_OK;
    const int64_t tiles = p.n >> 6;
    // Measured on MI355X before the miss culls (DESIGN_measurements.md §M14): longest-first paid when a launch was only a few
    // tiles per resident wave deep (the 1/8 shard of a 2048² image: 4.0 -> 3.7 ms on the rank holding the α≈0 columns, whose
    // rays take up to 430 steps) and cost 2-4 % on deep launches (2048²: 17.3 -> 17.8 ms).  Those launches are four times
    // shorter now and the thresholds below have not been measured again; lpt = 2 forces it.  The order is learned from the
    // previous render of the SAME (config, plane, range) with host synchronisations, so it serves repeated renders only; a
    // launch it leaves alone may get the live-first order made on the device from its own inputs (launch_trace).
    const int64_t resident_waves = (int64_t)ctx->n_cu * 8;
    if (tiles < resident_waves) return GR_OK;
    if (ctx->lpt == 1 && tiles >= (tab ? 24 : 6) * resident_waves) return GR_OK;
    // (a tabulated metric: the table's build id is part of the key -- the config itself holds only a pointer, and two metrics
    // fitted into the same buffer on the same grid would otherwise share one learned order)
    // (a compiled metric: its module's build id is part of the key and its slot number is not -- a slot is reused after an unload)
    std::vector<unsigned char> key(sizeof(gr_config) + sizeof(gr_plane) + sizeof(gr_range) + sizeof(double) + sizeof(int64_t));
    const double table_id = tab && p.cfg.metric_table ? p.cfg.metric_table[gr_tab::H_BUILD_ID] : 0.0;
    const int64_t module_id = metric_build_id(p.cfg.metric_id);
    std::memcpy(key.data() + sizeof(gr_config) + sizeof(gr_plane) + sizeof(gr_range), &table_id, sizeof(double));
    std::memcpy(key.data() + sizeof(gr_config) + sizeof(gr_plane) + sizeof(gr_range) + sizeof(double), &module_id, sizeof(int64_t));
    {
        gr_config keyed = p.cfg;
        if (keyed.metric_id >= GR_METRIC_COMPILED) keyed.metric_id = GR_METRIC_COMPILED;
        std::memcpy(key.data(), &keyed, sizeof(gr_config));
    }
    std::memcpy(key.data() + sizeof(gr_config), &cold.plane, sizeof(gr_plane));
    std::memcpy(key.data() + sizeof(gr_config) + sizeof(gr_plane), &cold.range, sizeof(gr_range));
    if (key != ctx->lpt_key) {
        ctx->lpt_key = key;
        ctx->lpt_have_perm = false;
        ctx->lpt_cost_pending = false;
        if (ctx->lpt_cap < tiles) {
            if (ctx->d_tile_cost) (void)hipFree(ctx->d_tile_cost);
            if (ctx->d_tile_perm) (void)hipFree(ctx->d_tile_perm);
            ctx->d_tile_cost = ctx->d_tile_perm = nullptr;
            ctx->lpt_cap = 0;
            GR_HIP(hipMalloc((void**)&ctx->d_tile_cost, sizeof(uint32_t) * tiles));
            GR_HIP(hipMalloc((void**)&ctx->d_tile_perm, sizeof(uint32_t) * tiles));
            ctx->lpt_cap = tiles;
        }
        ctx->lpt_tiles = tiles;
    }
    if (!ctx->lpt_have_perm && ctx->lpt_cost_pending) {
        // the recording launch has to be complete before its costs can be sorted (one-time)
        GR_HIP(hipEventSynchronize(ctx->ev_cost));
        std::vector<uint32_t> cost((size_t)tiles), perm((size_t)tiles);
        GR_HIP(hipMemcpy(cost.data(), ctx->d_tile_cost, sizeof(uint32_t) * tiles, hipMemcpyDeviceToHost));
        // counting sort, descending cost, stable in tile index
        uint32_t cmax = 0;
        for (uint32_t c : cost) cmax = c > cmax ? c : cmax;
        if (cmax < (1u << 24)) {
            std::vector<uint32_t> start((size_t)cmax + 2, 0);
            for (uint32_t c : cost) start[(size_t)(cmax - c) + 1]++;
            for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
            for (int64_t t = 0; t < tiles; ++t) perm[start[(size_t)(cmax - cost[(size_t)t])]++] = (uint32_t)t;
            GR_HIP(hipMemcpyAsync(ctx->d_tile_perm, perm.data(), sizeof(uint32_t) * tiles, hipMemcpyHostToDevice, stream));
            GR_HIP(hipStreamSynchronize(stream));   // perm is a local vector
            ctx->lpt_have_perm = true;
        }
        ctx->lpt_cost_pending = false;
    }
    if (ctx->lpt_have_perm) {
        cold.tile_perm = ctx->d_tile_perm;
    } else {
        GR_HIP(hipMemsetAsync(ctx->d_tile_cost, 0, sizeof(uint32_t) * tiles, stream));
        cold.tile_cost = ctx->d_tile_cost;
        *record = true;
    }
    return GR_OK;
}

#ifdef GR_WAVE_TIMELINE
unsigned long long* g_debug_timeline = nullptr;
#endif

extern "C++" {
namespace {
// Rays from a source into its sky (gr_rayset.sky_*): sample_position_direction_velocity for a source at one position
// (corona-models.jl:1-33).  Sample number j + 1 -> (θ, ϕ) on the source's sky (samplers.jl:30-44) -> k̂ -> v = Mx (1, k̂)
// (sky_angles_to_velocity, samplers.jl:81-99, the tetrad and the Jacobian folded into Mx on the host).  A kernel of its own
// that writes x (once) and v (32 B per ray) for the trace kernels to read as ray arrays: inside Ray::initial_conditions the
// branch -- libm's double-precision sin / cos / acos / atan / fmod -- cost every persistent kernel 6 % whether taken or not
// (C5 through the persistent kernel 58.2 -> 61.5 ms: SGPR spills in the refill path); 32 MB through HBM at 10⁶ rays cost 10 µs.
struct SkyParams {
    double x_obs[4], Mx[16];
    int64_t n;
    int64_t first, total;      // this launch's rays are samples first + 1 .. first + n of `total` (gr_rayset.sky_first / sky_total)
    const double* rows;        // gr_rayset.sky_rows (device) or null: per-sample position, matrix and lowered source velocity
    int32_t sampler, both, generator, reserved;
    double resolution;
    const double* sky_i;
};
// sample jl of the launch -> its direction on the source's sky (samplers.jl:30-44) and the four-velocity v = Mx (1, k̂)
__device__ __forceinline__ void sky_sample(const SkyParams& p, int64_t jl, double& el, double& az, double v[4], double x[4], double& f)
{
    const double n = (double)p.total;
    const double idx = (double)(p.first + jl + 1);
    const double i = p.generator == 0 ? idx : p.generator == 1 ? idx / n : p.sky_i[jl];
    if (p.sampler == 2) {
        const double ph = 2.0 * ::atan(::sqrt(p.resolution / i));
        const bool even = (::floor(i) == i) && (::fmod(i, 2.0) == 0.0);
        el = (!p.both || even) ? ph : 3.14159265358979323846 - ph;
    } else {
        const double u = i / n;
        el = p.both ? ::acos(1.0 - 2.0 * u) : ::acos(1.0 - u);
    }
    const double az_raw = (p.generator == 0 ? 3.14159265358979323846 * (1.0 + 2.2360679774997896964) : 6.28318530717958647692) * i;
    az = ::fmod(az_raw, 6.28318530717958647692);
    if (az < 0.0) az += 6.28318530717958647692;
    const double se = ::sin(el), ce = ::cos(el), sa = ::sin(az), ca = ::cos(az);
    const double pb[4] = { 1.0, -(se * ca), -(se * sa), -ce };
    f = 1.0;
    if (p.rows) {
        // a sample with a position of its own: its matrix, and the factor that turns the ratio against the static observer
        // (g_tμ v^μ) into the ratio against the source's own velocity (u_μ v^μ)
        const double* row = p.rows + GR_SKY_ROW * jl;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            x[q] = row[q];
            v[q] = row[4 + q * 4 + 0] * pb[0] + row[4 + q * 4 + 1] * pb[1] + row[4 + q * 4 + 2] * pb[2] + row[4 + q * 4 + 3] * pb[3];
        }
        double eu = 0.0, et = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { eu += row[20 + q] * v[q]; et += row[24 + q] * v[q]; }
        f = eu / et;
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        x[q] = p.x_obs[q];
        v[q] = p.Mx[q * 4 + 0] * pb[0] + p.Mx[q * 4 + 1] * pb[1] + p.Mx[q * 4 + 2] * pb[2] + p.Mx[q * 4 + 3] * pb[3];
    }
}
// out: x_obs[4], v[n][4] -- and for a source of many positions (SkyParams.rows) x[n][4] and f[n] behind them
__device__ __forceinline__ void sky_store(const SkyParams& p, double* out, int64_t slot, const double v[4], const double x[4], double f)
{
    double* o = out + 4 + 4 * slot;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = v[q];
    if (p.rows) {
        double* ox = out + 4 + 4 * p.n + 4 * slot;
#pragma unroll
        for (int q = 0; q < 4; ++q) ox[q] = x[q];
        out[4 + 8 * p.n + slot] = f;
    }
}
__global__ void __launch_bounds__(256) k_sky_velocities(const SkyParams p, double* out)
{
    const int64_t jl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (jl == 0)
        for (int q = 0; q < 4; ++q) out[q] = p.x_obs[q];
    if (jl >= p.n) return;
    double el, az, v[4], x[4], f;
    sky_sample(p, jl, el, az, v, x, f);
    sky_store(p, out, jl, v, x, f);
}
// rows (g, ρ, t, status) of a source of many positions: g against the sample's own source velocity
__global__ void __launch_bounds__(256) k_sky_scale_g(double* rows, const double* f, int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) rows[4 * j] *= f[j];
}
// The cells of a source's adaptive sky (gr_sky_cells; AdaptiveSky, adaptive-sample.jl:43-81): cell j is the direction
// (θ = acos(cos θ_j), ϕ_j), v = Mx (1, -k̂) with k̂ = (sin θ cos ϕ, sin θ sin ϕ, cos θ) (sky_angles_to_velocity, samplers.jl:75-97),
// and next to it the seed of the tangent kernels (Cold::v_tan): ∂v/∂θ = -Mx (0, ∂k̂/∂θ), ∂v/∂ϕ = -Mx (0, ∂k̂/∂ϕ), then sin θ.
// out: x_src[4], v[n][4], seed[n][GR_SKYCELL_SEED]
struct SkyCellParams {
    double x_src[4], Mx[16];
    const double* cos_theta;   // device, n
    const double* phi;         // device, n
    int64_t n;
};
__global__ void __launch_bounds__(256) k_skycell_velocities(const SkyCellParams p, double* out)
{
    const int64_t jl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (jl == 0)
        for (int q = 0; q < 4; ++q) out[q] = p.x_src[q];
    if (jl >= p.n) return;
    const double ct = p.cos_theta[jl], th = ::acos(ct), ph = p.phi[jl];
    const double st = ::sin(th), sp = ::sin(ph), cp = ::cos(ph);
    const double k[3] = { st * cp, st * sp, ct };
    const double kt[3] = { ct * cp, ct * sp, -st };
    const double kp[3] = { -st * sp, st * cp, 0.0 };
    double* v = out + 4 + 4 * jl;
    double* seed = out + 4 + 4 * p.n + GR_SKYCELL_SEED * jl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double* row = p.Mx + 4 * q;
        v[q] = row[0] - (row[1] * k[0] + row[2] * k[1] + row[3] * k[2]);
        seed[q] = -(row[1] * kt[0] + row[2] * kt[1] + row[3] * kt[2]);
        seed[4 + q] = -(row[1] * kp[0] + row[2] * kp[1] + row[3] * kp[2]);
    }
    seed[8] = st;
}
// The same rays DEALT BY WHAT THEY WILL COST (gr_corona_trace: the order of its rows is free -- min / max and integer bins do not
// know it).  How many steps a ray takes is known, to a constant per polar angle of emission, BEFORE it is traced: the integrator
// resolves the ray's passage round the polar axis of the coordinates, and along the flat-space straight line from the source the
// azimuth sweeps Δϕ and ln sin θ runs down to the line's closest angular approach to the axis and back --
//     steps ≈ base(polar angle of emission) + 16 Δϕ + 36 ln(sin θ₀ / sin θ_min)
// follows the oracle's step counts of the lamp-post scene (h = 10, 0.01 rad off the axis: 53 ... 519 steps within one polar angle)
// with a residual of 4 steps rms (scripts/corona_lanes.py, DESIGN_measurements.md §M19).  The rays are counting-sorted by that
// number in classes of 12 steps, the most expensive class first, inside a class by chunk of kSkyChunk consecutive samples (one polar
// angle to 1 %: one base): the 64 rays of a wave then take the same number of steps to a few per cent AND the launch starts with its
// longest waves -- a wave of 500-step rays takes 2 ms alone whenever it starts, and consecutive samples put one into every chunk.
// Three launches: count per (class, chunk), one-workgroup exclusive scan, scatter.
// A source with a position per sample (SkyParams.rows: DiscCorona) has no "one base per chunk": its base depends on where the sample
// sits -- oracle step counts of a disc corona (r = 10, h = 5): +90 steps for positions next to the axis, -20 far from it.  Such rays
// are sorted by (class, bucket of |sin θ| of the POSITION, chunk): eight buckets, the one next to the axis first.  Lane utilisation of
// 64-ray waves by the oracle's counts, four chunks: 0.17 ... 0.56 in sample order, 0.21 ... 0.71 by class alone, 0.40 ... 0.83 with
// the position bucket (DESIGN_measurements.md §M19).
constexpr int kSkyChunk = 4096;
constexpr int kSkyClasses = 32;
constexpr int kSkyPosBuckets = 8;
__device__ __forceinline__ int sky_cost_class(const double x[4], const double v[4], int nb, int& pos_bucket)
{
    const double r = x[1], s = ::sin(x[2]), c = ::cos(x[2]);
    {
        const int b = (int)(::fabs(s) * (double)nb);
        pos_bucket = b < 0 ? 0 : b >= nb ? nb - 1 : b;
    }
    double er = v[1], et = r * v[2], ep = r * s * v[3];
    const double nrm = ::sqrt(er * er + et * et + ep * ep);
    if (!(nrm > 0.0) || !(nrm < 1e300)) return 0;
    er /= nrm; et /= nrm; ep /= nrm;
    // the source in the x-z plane, the ray's direction in Cartesian components
    const double Px = r * s, Pz = r * c;
    const double dx = er * s + et * c, dy = ep, dz = er * c - et * s;
    const double dphi = ::atan2(::fabs(dy), dx);
    // the directions origin -> points of the line run along a great circle from P̂ to d̂ (normal n = P x d): sin θ on it has an
    // extremum |n_z| / |n|, reached on the way iff cos θ moves towards that pole at the start and away from it at the end
    const double Pd = Px * dx + Pz * dz;
    const double nx = -Pz * dy, ny = Pz * dx - Px * dz, nz = Px * dy;
    const double nn = ::sqrt(nx * nx + ny * ny + nz * nz);
    const double a0 = dz * r * r - Pz * Pd, a1 = Pz - Pd * dz;
    double tv = 0.0;
    if (((a0 > 0.0 && a1 > 0.0) || (a0 < 0.0 && a1 < 0.0)) && nn > 0.0) {
        const double s_ext = ::fabs(nz) / nn, s0 = ::fabs(s);
        if (s_ext < s0) tv = ::log(s0 / (s_ext > 1e-12 ? s_ext : 1e-12));
    }
    const double cost = 16.0 * dphi + 36.0 * tv;
    const int cls = (int)(cost * (1.0 / 12.0));
    return cls < 0 ? 0 : cls >= kSkyClasses ? kSkyClasses - 1 : cls;      // (NaN -> 0)
}
// counts / offsets: [kSkyClasses - 1 - class][position bucket][chunks - 1 - chunk] -- the order of the dealt array (the last samples
// of a sky leave upwards, away from the disc, and have the larger base: first within their class and bucket)
template <bool COUNT>
__global__ void __launch_bounds__(1024) k_sky_velocities_dealt(const SkyParams p, double* out, unsigned* table)
{
    __shared__ int cnt[kSkyClasses * kSkyPosBuckets];
    const int nb = p.rows ? kSkyPosBuckets : 1;
    const int64_t base = (int64_t)blockIdx.x * kSkyChunk;
    const int64_t left = p.n - base;
    const int nloc = left < kSkyChunk ? (int)left : kSkyChunk;
    if (threadIdx.x < kSkyClasses * kSkyPosBuckets) cnt[threadIdx.x] = 0;
    if (!COUNT && blockIdx.x == 0 && threadIdx.x == 0)
        for (int q = 0; q < 4; ++q) out[q] = p.x_obs[q];
    __syncthreads();
    double v[kSkyChunk / 1024][4], x[kSkyChunk / 1024][4], f[kSkyChunk / 1024];
    int cls[kSkyChunk / 1024], pos[kSkyChunk / 1024];
#pragma unroll
    for (int k = 0; k < kSkyChunk / 1024; ++k) {
        const int j = (int)threadIdx.x + 1024 * k;
        cls[k] = -1;
        if (j < nloc) {
            double el, az;
            sky_sample(p, base + j, el, az, v[k], x[k], f[k]);
            int pb;
            const int c = sky_cost_class(x[k], v[k], nb, pb);
            cls[k] = (kSkyClasses - 1 - c) * nb + pb;          // the cell's row in the table: expensive classes first
            pos[k] = atomicAdd(&cnt[cls[k]], 1);
        }
    }
    const unsigned chunks = gridDim.x;
    const unsigned col = chunks - 1u - blockIdx.x;
    if (COUNT) {
        __syncthreads();
        if ((int)threadIdx.x < kSkyClasses * nb) table[(size_t)threadIdx.x * chunks + col] = (unsigned)cnt[threadIdx.x];
        return;
    }
#pragma unroll
    for (int k = 0; k < kSkyChunk / 1024; ++k) {
        if (cls[k] < 0) continue;
        sky_store(p, out, (int64_t)table[(size_t)cls[k] * chunks + col] + pos[k], v[k], x[k], f[k]);
    }
}
// in-place exclusive scan of `n` counts by one workgroup (n = 32 x chunks: 7808 for 10⁶ samples)
__global__ void __launch_bounds__(1024) k_sky_scan(unsigned* table, int64_t n)
{
    __shared__ unsigned part[1024];
    const int64_t per = (n + 1023) / 1024;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    unsigned sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += table[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned run = part[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) { const unsigned c = table[i]; table[i] = run; run += c; }
}
}  // namespace
}  // extern "C++"

// are the rays of this launch's sky source dealt by cost? (offsets are 32-bit)
static bool sky_dealt(const gr_ctx* ctx, int64_t n)
{
    return ctx->sky_any_order && ctx->sky_deal && n >= 4 * kSkyChunk && n < ((int64_t)1 << 32);
}
// a sky source -> ray arrays in the context's sky buffer (ordered against earlier launches that read it like the staged tables)
static int32_t sky_prepare(gr_ctx* ctx, Params& p, Cold& cold, hipStream_t stream)
{
    int32_t rc;
    if ((rc = tables_acquire(ctx, stream)) != GR_OK) return rc;
    if ((rc = ensure((void**)&ctx->d_sky, &ctx->sky_bytes, sizeof(double) * (4 + (ctx->sky_rows ? 9 : 4) * (size_t)p.n))) != GR_OK) return rc;
    SkyParams sp;
    std::memcpy(sp.x_obs, cold.plane.x_obs, sizeof sp.x_obs);
    std::memcpy(sp.Mx, cold.plane.Mx, sizeof sp.Mx);
    sp.n = p.n;
    sp.first = ctx->sky_first;
    sp.total = ctx->sky_total > 0 ? ctx->sky_total : p.n;
    sp.sampler = cold.sky_sampler; sp.both = cold.sky_both; sp.generator = cold.sky_generator; sp.reserved = 0;
    sp.resolution = cold.sky_resolution;
    sp.sky_i = cold.sky_i;
    sp.rows = ctx->sky_rows;
    if (sky_dealt(ctx, p.n)) {
        const unsigned chunks = (unsigned)((p.n + kSkyChunk - 1) / kSkyChunk);
        const int64_t cells = (int64_t)kSkyClasses * (sp.rows ? kSkyPosBuckets : 1) * chunks;
        if ((rc = ensure((void**)&ctx->d_sky_table, &ctx->sky_table_bytes, sizeof(unsigned) * (size_t)cells)) != GR_OK) return rc;
        hipLaunchKernelGGL(k_sky_velocities_dealt<true>, dim3(chunks), dim3(1024), 0, stream, sp, ctx->d_sky, ctx->d_sky_table);
        hipLaunchKernelGGL(k_sky_scan, dim3(1), dim3(1024), 0, stream, ctx->d_sky_table, cells);
        hipLaunchKernelGGL(k_sky_velocities_dealt<false>, dim3(chunks), dim3(1024), 0, stream, sp, ctx->d_sky, ctx->d_sky_table);
    } else
        hipLaunchKernelGGL(k_sky_velocities, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, stream, sp, ctx->d_sky);
    GR_HIP(hipGetLastError());
    cold.src_mode = 1;
    cold.x = ctx->sky_rows ? ctx->d_sky + 4 + 4 * p.n : ctx->d_sky;
    cold.x_stride = ctx->sky_rows ? 4 : 0;
    cold.v = ctx->d_sky + 4;
    cold.sky_i = nullptr;
    return GR_OK;
}

// The culls' gating radius for one launch (Params::r_cull for Ray::step's escape and polar-rate culls, Params::r_cull_start for
// Ray::init's start cull); +inf leaves every ray to run to its end.
// Finite only where each condition of the proofs in Ray::step and Ray::init holds:
//   output:    finalize reads nothing but the status of a ray that misses -- a fused point function behind filter_intersected
//              (out_mode 0), BinningMethod (2: only rays that hit are binned) or (g, ρ) pairs (3: NaN pairs).  Never for end points
//              (1), ray summaries (4, 5), filter_early_term or an unfiltered point function;
//   geometry:  one GR_DISC_THIN disc (no composite, precessing, mesh or thick one) with a finite outer radius and gtol < 1;
//   metric:    a finite Metric::kEscapeRadiusM -- the fused Kerr (not Kerr-Newman, not a tabulated Kerr) with |a| <= M; null rays
//              (μ = 0) traced forward (λ1 > λ0);
//   callbacks: no hemisphere, PoloidalShapeChart or winding callback (any of them can set a status after the cull point);
//   precision: the fp64 kernels (lane and persistent); not fp32, not the tangent kernels.
// Five switches in the environment, read at every launch (A/B of one build), each on its own mechanism (launch_trace):
// GRADUS_MI355X_ESCAPE_CULL=0 -- no ray ends early inside the step loop (the escape, polar-rate and entry culls);
// GRADUS_MI355X_START_CULL=0 -- no ray is decided at its start (the start cull and the pass cull, Params::r_pass = pass_cull_radius);
// GRADUS_MI355X_PASS_CULL=0 -- the pass cull alone is off.  The entry cull (Ray::step) asks the pass cull's question inside the step
// loop and is armed at the start, so each of the three turns it off as well; GRADUS_MI355X_ENTRY_CULL=0 (Params::entry_cull) turns
// it off alone.  The defer cull (Ray::start_decided, Ray::step) is decided by the pass cull at the start and ends its rays in the
// step loop: each of the three turns it off too, and GRADUS_MI355X_DEFER_CULL=0 (Params::defer_cull) turns it off alone.
// The statistics of a launch: the trace kernel's waves have added their sums to the rows of one partials block (LaneStats::flush);
// this adds the column sums to the caller's nine counters -- with atomics, as the waves themselves did before: launches on other
// streams may be adding to the same counters -- and leaves the block zero for the launch that draws it next.  One workgroup.
__global__ void __launch_bounds__(64) k_stats_fold(unsigned long long* part, unsigned long long* counters)
{
    const int t = (int)threadIdx.x;
    unsigned long long s = 0;
    if (t < gr_fold::kStatCols) s = gr_fold::column_sum(part, gr_fold::kStatRows, gr_fold::kStatStride, t);
    __syncthreads();
    if (t < gr_fold::kStatCols && s) atomicAdd(counters + t, s);
    for (int i = t; i < gr_fold::kStatWords; i += 64) part[i] = 0;
}

// The live-first tile order (gr_tile_order.hpp): the stable partition of the tiles by their flags.  Workgroup b places the tiles
// [1024 b, 1024 b + 1024), one per thread.  It counts for itself how many flags are set before its tiles and in all -- every
// workgroup reads the whole flag block, 64 KB for the 2048² bench render, eight bytes per load -- so no workgroup waits for
// another and nothing is placed by an atomic: the order is the same at every launch.  perm[tiles] receives the number of live
// tiles (gr_debug_tile_order).  (One workgroup of 1024 threads with 64 tiles each took 42 µs: 65 536 single-word stores to
// 65 536 cache lines from one CU.)
__global__ void __launch_bounds__(gr_order::kPartitionThreads) k_tile_partition(const uint8_t* flags, int64_t tiles, uint32_t* perm)
{
    constexpr int T = gr_order::kPartitionThreads, W = T / 64;
    __shared__ uint32_t s_before[W], s_total[W], s_wave[W];
    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * T;          // a multiple of 8: a word of eight flags lies before it or behind it
    uint32_t before = 0, total = 0;
    const int64_t words = tiles >> 3;
    for (int64_t k = t; k < words; k += T) {
        const uint32_t c = gr_order::chunk_ones(flags, 8 * k, 8 * k + 8);
        total += c;
        if (8 * k < base) before += c;
    }
    for (int64_t i = 8 * words + t; i < tiles; i += T) total += gr_order::chunk_ones(flags, i, i + 1);      // (behind every base)
    // this thread's tile among its wave's
    const int64_t i = base + t;
    const bool in = i < tiles;
    const unsigned long long set = __ballot(in && flags[in ? i : 0] != 0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        before += (uint32_t)__shfl_xor((int)before, off, 64);
        total += (uint32_t)__shfl_xor((int)total, off, 64);
    }
    if (lane == 0) { s_before[w] = before; s_total[w] = total; s_wave[w] = (uint32_t)__popcll(set); }
    __syncthreads();
    uint32_t ones_before = 0, ones_total = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        ones_before += s_before[k] + (k < w ? s_wave[k] : 0u);
        ones_total += s_total[k];
    }
    ones_before += (uint32_t)__popcll(set & ((1ull << lane) - 1ull));
    const uint32_t zeros_total = (uint32_t)tiles - ones_total;
    if (in) gr_order::chunk_place(flags, i, i + 1, ones_before, zeros_total, perm);
    if (blockIdx.x == 0 && t == 0) perm[tiles] = zeros_total;
}

static bool cull_switched_off(const char* name)
{
    const char* sw = std::getenv(name);
    return sw && std::strcmp(sw, "0") == 0;
}
static double escape_cull_radius(const gr_ctx* ctx, const Params& p, const Cold& cold, bool tangent)
{
    const double off = HUGE_VAL;
    if (tangent || ctx->precision == 32) return off;
    const bool misses_ignored = (cold.out_mode == 0 && cold.pf.filter_id == GR_FILTER_INTERSECTED) || cold.out_mode == 2 || cold.out_mode == 3;
    const gr_config& c = p.cfg;
    if (!misses_ignored || c.metric_id < 0) return off;
    const double esc = metric_escape_radius_m(c.metric_id);
    if (!(esc < HUGE_VAL)) return off;      // never culled: every compiled metric, and what the table above says
    return cull_gate_radius(c, esc);      // the conditions on the configuration: gr_device.hpp
}

int32_t launch_trace(gr_ctx* ctx, Params& p, const Cold& cold_in, hipStream_t stream)
{
    Cold cold = cold_in;
    cold.winding_plane = p.cfg.winding_plane;
    // the metric's launchers: a row of the catalogue's tables or a loaded module's (validate_cfg has seen the id; a module may have
    // been unloaded since by another thread -- refused here, not crashed on)
    MetricKernels mk;
    if (!metric_kernels(p.cfg.metric_id, mk)) return fail(GR_ERR_UNSUPPORTED, "unknown metric_id " + std::to_string(p.cfg.metric_id));
    if (p.cfg.metric_id >= GR_METRIC_COMPILED && ctx->precision == 32)
        return fail(GR_ERR_UNSUPPORTED, "a compiled metric has no fp32 kernels (\"precision\" 32): trace it with the fp64 kernels");
    if (p.cfg.metric_id == GR_METRIC_TABULATED && cold_in.src_mode != 1 && !(cold_in.src_mode == 3 && ctx->sky_rows)) {
        // (validate_cfg has compared the chart with the table's range; p.cfg.metric_table is still the caller's host table here.)
        // The observer / source position the rays start from must lie inside the table as well.  (A sky source with sky_rows has no
        // such position -- x_obs is not read: the host-pointer entry points have checked every row's radius, sky_rows_in_table.)
        const double r_obs = cold_in.plane.x_obs[1], t_min = p.cfg.metric_table[gr_tab::H_RMIN], t_max = p.cfg.metric_table[gr_tab::H_RMAX];
        if (!(r_obs >= t_min - 1e-9 * std::fabs(t_min) - 1e-12) || !(r_obs <= t_max + 1e-9 * std::fabs(t_max)))
            return fail(GR_ERR_INVALID_ARGUMENT, "GR_METRIC_TABULATED: the rays start at r = " + std::to_string(r_obs) + ", outside the radial range of the "
                                                 "metric table [" + std::to_string(t_min) + ", " + std::to_string(t_max) + "]");
    }
    const bool sky = cold.src_mode == 3;
    if (sky && p.n > 0) {
        const int32_t src = sky_prepare(ctx, p, cold, stream);
        if (src != GR_OK) return src;
    }
    bool lpt_record = false;
    if (p.n > 0) {
        const int32_t lrc = lpt_prepare(ctx, p, cold, stream, &lpt_record);
        if (lrc != GR_OK) return lrc;
    }
    if (p.n == 0) return GR_OK;
    {
        const int32_t trc = stage_disc_table(ctx, p, stream);
        if (trc != GR_OK) return trc;
    }
    // the cold block goes into the next ring slot (staged below, once the tile order is settled: stream-ordered before the kernel)
    Cold* slot = ctx->d_cold + ctx->cold_next;
    ctx->cold_next = (ctx->cold_next + 1) % ctx->queue_slots;
    p.cold = slot;
    // (fp32 line profile, 4096² rays: 21.2 ms at 32 against 22.3 at 16 and 24.2 at 8; fp64: 50.8 either way -- profiles/r5n_c5f32_knobs.log)
    p.refill_threshold = (int32_t)(ctx->refill_threshold ? ctx->refill_threshold : (ctx->precision == 32 ? 32 : 16));
    // the tangent objects carry the one-ray-per-lane kernel only: settle kernel and block BEFORE anything is sized by them
    const bool tangent = cold.out_mode == 5 || cold.out_mode == 6;
    if (p.cfg.disc_id == GR_DISC_MESH && (tangent || ctx->precision == 32))
        return fail(GR_ERR_UNSUPPORTED, "a mesh geometry is traced by the fp64 kernels only (not with \"precision\" 32, not by the tangent entry points)");
    // A sky source whose rays were dealt by predicted cost (sky_prepare): a wave's 64 rays take nearly the same number of steps
    // (lane utilisation 0.93 against 0.5 for consecutive samples) and the array begins with the longest, which the persistent
    // kernel's refill would mix again -- one ray per lane, four waves to a workgroup (10⁶ lamp-post samples: 5.9 ms against 7.6
    // persistent, 6.6 with one-wave workgroups, 8.4 in sample order; profiles/r6_corona_cost_ab.log)
    const bool dealt = sky && sky_dealt(ctx, p.n) && !tangent;
    const bool transfer = cold.transfer != nullptr;      // the gr_transfer_* calls: the one-ray-per-lane kernel of kernelsrt_m<id>.o
    const int kern_sel = (tangent || transfer) ? 0 : (dealt && ctx->kernel == 2) ? 0 : resolve_kernel(ctx, p.n, cold, p.cfg.metric_id);
    const int block_sel = tangent ? (ctx->block ? (int)ctx->block : 64) : (dealt && ctx->kernel == 2 && !ctx->block) ? 256 : resolve_block(ctx, kern_sel);
    // LDS staging: the plunging table (<= 2048 rows = 64 KB) and the line-profile histogram (<= 4096 bins).
    // A table is staged per workgroup: with one-wave workgroups a CU holds 8 copies, so it is staged
    // only while those fit the 160 KB of LDS without capping the occupancy (<= 640 rows of 32 B).
    // The table is read at finalize only: on the Johannsen 1024² render (605 rows) staged and
    // L2-served lookups are within run-to-run noise of each other (8.5-8.7 ms).
    const int64_t lds_rows_max = block_sel >= 256 ? 2048 : 640;
    p.lds_plunge_rows = (ctx->lds && cold_in.pf.pf_id == GR_PF_REDSHIFT && cold_in.out_mode != 1
                         && cold_in.pf.n_plunge > 0
                         && cold_in.pf.n_plunge <= lds_rows_max) ? (int32_t)cold_in.pf.n_plunge : 0;
    p.lds_bins = (ctx->lds && cold_in.out_mode == 2 && cold_in.lp_nbins <= 4096) ? (int32_t)cold_in.lp_nbins : 0;
    p.lds_points = (ctx->lds_points && cold.out_mode == 1 && kern_sel == 0) ? 1 : 0;
    // rays in caller order on the one-ray-per-lane kernel: deal the chunks of 64 rays over the XCDs (gr_kernels.hpp, xcd_chunk);
    // image planes are tiled and their tile order already mixes (gr_ctx_set "xcd_spread" 0 switches it off)
    p.xcd_spread = (ctx->xcd_spread && kern_sel == 0 && cold.src_mode != 0) ? 1 : 0;
    derive_params(p);
    {
        const double r_gate = escape_cull_radius(ctx, p, cold, tangent);
        p.r_cull = cull_switched_off("GRADUS_MI355X_ESCAPE_CULL") ? HUGE_VAL : r_gate;
        p.r_cull_start = cull_switched_off("GRADUS_MI355X_START_CULL") ? HUGE_VAL : r_gate;
        p.r_pass = cull_switched_off("GRADUS_MI355X_PASS_CULL") ? HUGE_VAL : pass_cull_radius(p.r_cull_start);
        p.entry_cull = cull_switched_off("GRADUS_MI355X_ENTRY_CULL") ? 0 : 1;
        p.defer_cull = cull_switched_off("GRADUS_MI355X_DEFER_CULL") ? 0 : 1;
    }
    // LIVE-FIRST TILE ORDER (gr_tile_order.hpp): an image launch of the one-ray-per-lane kernel under the start cull
    // takes its live tiles first and the tiles decided at the start last.  The order is made on the device from this launch's own
    // parameters by two small kernels ahead of the trace kernel on its stream -- no host synchronisation, no host copy -- so it
    // serves a configuration that changes from call to call, which the learned order (lpt_prepare) does not; where that one is
    // in use or being recorded it stays.  gr_ctx_set "live_first": 0 = off, 1 [default] = launches of at
    // least as many tiles as the device holds waves (below that every wave is resident at once and the order decides nothing)
    // and at most 2^20, 2 = any size; GRADUS_MI355X_LIVE_FIRST=0 | 1 | 2 in the environment, read at every launch
    // like the culls' switches, takes the knob's place (A/B of one build through a program that does not set the knob).
    const int64_t tiles = p.n >> 6;
    uint8_t* live_flags = nullptr;
    ctx->live_last = nullptr;
    ctx->live_last_tiles = 0;
    int64_t live_mode = ctx->live_first;
    if (const char* sw = std::getenv("GRADUS_MI355X_LIVE_FIRST"))
        if ((sw[0] == '0' || sw[0] == '1' || sw[0] == '2') && sw[1] == 0) live_mode = sw[0] - '0';
    if (live_mode && kern_sel == 0 && cold.src_mode == 0 && cold.swizzle && p.r_cull_start < HUGE_VAL && !cold.tile_perm && !lpt_record
        && tiles > 0 && tiles < ((int64_t)1 << 29)
        && (live_mode == 2 || (tiles >= (int64_t)ctx->n_cu * 8 && tiles <= ((int64_t)1 << 20)))) {
        if (ctx->live_cap < tiles) {
            // (a smaller ring may still be read by launches in flight: hipFree waits for the device)
            if (ctx->d_live_perm) (void)hipFree(ctx->d_live_perm);
            if (ctx->d_live_flags) (void)hipFree(ctx->d_live_flags);
            ctx->d_live_perm = nullptr;
            ctx->d_live_flags = nullptr;
            ctx->live_cap = 0;
            const int64_t cap = (tiles + 7) & ~(int64_t)7;
            GR_HIP(hipMalloc((void**)&ctx->d_live_perm, sizeof(uint32_t) * (size_t)(cap + 1) * (size_t)ctx->queue_slots));
            GR_HIP(hipMalloc((void**)&ctx->d_live_flags, (size_t)cap * (size_t)ctx->queue_slots));
            ctx->live_cap = cap;
        }
        uint32_t* const perm = ctx->d_live_perm + (size_t)ctx->live_next * (size_t)(ctx->live_cap + 1);
        live_flags = ctx->d_live_flags + (size_t)ctx->live_next * (size_t)ctx->live_cap;
        ctx->live_next = (ctx->live_next + 1) % ctx->queue_slots;
        cold.tile_perm = perm;
        ctx->live_last = perm;
        ctx->live_last_tiles = tiles;
    }
    GR_HIP(hipMemcpyAsync(slot, &cold, sizeof(Cold), hipMemcpyHostToDevice, stream));
    if (live_flags) {
        GR_NEED_KERNEL(mk.classify, "tile classification");
        const hipError_t ce = mk.classify(&p, live_flags, tiles, stream);
        if (ce != hipSuccess) return fail(GR_ERR_HIP, std::string("tile classification launch: ") + hipGetErrorString(ce));
        hipLaunchKernelGGL(k_tile_partition, dim3((unsigned)((tiles + gr_order::kPartitionThreads - 1) / gr_order::kPartitionThreads)),
                           dim3(gr_order::kPartitionThreads), 0, stream, live_flags, tiles,
                           const_cast<uint32_t*>(cold.tile_perm));
        GR_HIP(hipGetLastError());
    }
    LaunchKnobs knobs{ kern_sel, block_sel, ctx->n_cu, (int)ctx->waves_per_simd,
                       ctx->d_queue + ctx->queue_next };
    ctx->queue_next = (ctx->queue_next + 1) % ctx->queue_slots;
    // validate_cfg() has pinned metric_id to [GR_METRIC_KERR, GR_METRIC_NOZ]
    // Tangent launches come in two shapes (kernels_tu.hip): a pair of lanes per ray has the shorter step (latency), one lane
    // per ray does less work in all (throughput).  A launch whose pairs fit the machine at one wave per SIMD -- 2 n / 64 waves
    // on 4 SIMDs per CU -- cannot keep the SIMDs busy either way and is as long as its longest ray: it takes the pairs.
    const bool pairs = tangent && (ctx->tangent_pairs == 1 || (ctx->tangent_pairs == 2 && 2 * p.n <= (int64_t)ctx->n_cu * 4 * 64));
    const bool skycell = cold.out_mode == 6;
    const trace_fn fn = transfer ? ((p.cfg.metric_id >= 0 && p.cfg.metric_id < 12) ? kTraceRT[p.cfg.metric_id] : nullptr)
                        : skycell ? (pairs ? mk.sky1 : mk.sky) : tangent ? (pairs ? mk.tan1 : mk.tan) : ctx->precision == 32 ? mk.trace32 : mk.trace64;
    GR_NEED_KERNEL(fn, transfer ? "radiative-transfer" : skycell ? "sky-cell" : tangent ? "tangent" : ctx->precision == 32 ? "fp32" : "fp64 trace");
    p.tangent_norm = (tangent && ctx->tangent_norm) ? 1 : 0;
#ifdef GR_WAVE_TIMELINE
    p.queue = g_debug_timeline;      // debug builds: 4 x u64 per wave of a one-ray-per-lane launch (gr_kernels.hpp)
#endif
    // statistics: the waves add to a partials block of the context, k_stats_fold adds that to the caller's counters
    unsigned long long* const caller_stats = p.stats;
    if (caller_stats) {
        p.stats = ctx->d_stat_part + (size_t)ctx->stat_next * gr_fold::kStatWords;
        ctx->stat_next = (ctx->stat_next + 1) % ctx->queue_slots;
    }
    const hipError_t le = fn(knobs.kernel, knobs.block, knobs.n_cu, knobs.waves_per_simd, knobs.queue, &p, stream);
    if (le != hipSuccess) return fail(GR_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(le));
    if (caller_stats) {
        hipLaunchKernelGGL(k_stats_fold, dim3(1), dim3(64), 0, stream, p.stats, caller_stats);
        GR_HIP(hipGetLastError());
        p.stats = caller_stats;
    }
    if (stream == ctx->stream) GR_HIP(hipEventRecord(ctx->ev_k, stream));      // host variants: where the kernel ends
    if (p.disc_table || p.chart_table || cold.pf.n_plunge > 0 || p.cfg.metric_id == GR_METRIC_TABULATED || sky || cold.v_tan) {
        const int32_t trc = tables_release(ctx, stream);
        if (trc != GR_OK) return trc;
    }
    if (lpt_record) {
        GR_HIP(hipEventRecord(ctx->ev_cost, stream));
        ctx->lpt_cost_pending = true;
    }
    return GR_OK;
}

// copy the plunging table (host pointers) into the context and fill the device-side pf
int32_t stage_pf(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf, PfDev& out, hipStream_t stream)
{
    if (!pf) return fail(GR_ERR_INVALID_ARGUMENT, "point function is null");
    if (pf->pf_id < GR_PF_AFFINE_TIME || pf->pf_id > GR_PF_WINDING)
        return fail(GR_ERR_UNSUPPORTED, "unknown pf_id " + std::to_string(pf->pf_id));
    if (pf->filter_id < GR_FILTER_NONE || pf->filter_id > GR_FILTER_INTERSECTED)
        return fail(GR_ERR_UNSUPPORTED, "unknown filter_id " + std::to_string(pf->filter_id));
    out.pf_id = pf->pf_id;
    out.filter_id = pf->filter_id;
    out.fill = pf->fill;
    out.r_isco = pf->r_isco;
    out.n_plunge = 0;
    out.plunge_r = out.plunge_vt = out.plunge_vr = out.plunge_vphi = nullptr;
    out.has_u_src = pf->has_u_src ? 1 : 0;
    out.pad_u = 0;
    for (int q = 0; q < 4; ++q) out.u_src[q] = pf->has_u_src ? pf->u_src[q] : (q == 0 ? 1.0 : 0.0);
    if (pf->pf_id == GR_PF_REDSHIFT && pf->n_plunge > 0) {
        if (pf->n_plunge < 2 || !pf->plunge_r || !pf->plunge_vt || !pf->plunge_vr || !pf->plunge_vphi)
            return fail(GR_ERR_INVALID_ARGUMENT, "plunging table needs >= 2 rows and four arrays");
        const int64_t n = pf->n_plunge;
        {
            const int32_t arc = tables_acquire(ctx, stream);
            if (arc != GR_OK) return arc;
        }
        if (ctx->plunge_cap < n) {
            // a smaller table may still be read by a launch in flight on this very stream: hipFree waits for the device
            if (ctx->d_plunge) (void)hipFree(ctx->d_plunge);
            ctx->d_plunge = nullptr;
            ctx->plunge_cap = 0;
            GR_HIP(hipMalloc((void**)&ctx->d_plunge, sizeof(double) * 4 * n));
            ctx->plunge_cap = n;
        }
        const double* src[4] = { pf->plunge_r, pf->plunge_vt, pf->plunge_vr, pf->plunge_vphi };
        for (int q = 0; q < 4; ++q)
            GR_HIP(hipMemcpyAsync(ctx->d_plunge + q * ctx->plunge_cap, src[q], sizeof(double) * n, hipMemcpyHostToDevice, stream));
        out.n_plunge = n;
        out.plunge_r = ctx->d_plunge;
        out.plunge_vt = ctx->d_plunge + ctx->plunge_cap;
        out.plunge_vr = ctx->d_plunge + 2 * ctx->plunge_cap;
        out.plunge_vphi = ctx->d_plunge + 3 * ctx->plunge_cap;
    }
    if (pf->pf_id == GR_PF_REDSHIFT && !(pf->r_isco > 0.0))
        return fail(GR_ERR_INVALID_ARGUMENT, "redshift needs r_isco > 0");
    // n_plunge = 0 selects the analytic Cunningham plunge, which exists for Kerr only (redshift.jl:93-164); every
    // other metric interpolates a tabulated plunge inside its ISCO (redshift.jl:246-276) and must bring the table
    if (pf->pf_id == GR_PF_REDSHIFT && cfg->metric_id != GR_METRIC_KERR && pf->n_plunge < 2)
        return fail(GR_ERR_INVALID_ARGUMENT, "redshift of a non-Kerr metric needs a plunging table (n_plunge >= 2)");
    return GR_OK;
}

void plane_params(gr_ctx* ctx, Params& pp, Cold& p, const gr_config* cfg, const gr_plane* plane, const gr_range* range)
{
    std::memset(&pp, 0, sizeof pp);
    std::memset(&p, 0, sizeof p);
    pp.cfg = *cfg;
    pp.n = range->count;
    p.src_mode = 0;
    p.plane = *plane;
    p.range = *range;
    // tiles of R rows x 64/R columns need whole, column-aligned groups of 64/R columns in the local index space
    const int64_t H = plane->height;
    auto tiles_ok = [&](int64_t rows) {
        const int64_t cols = 64 / rows;
        return (H % rows == 0) && (range->first % H == 0) && (range->block % (cols * H) == 0) && (range->count % (cols * H) == 0);
    };
    p.swizzle = 0;
    if (ctx->swizzle) {
        if (ctx->tile_rows == 16 && tiles_ok(16)) p.swizzle = 4;
        else if (tiles_ok(8)) p.swizzle = 3;
    }
    const int64_t lim = (int64_t)1 << 31;
    p.idx32 = (plane->width * plane->height < lim && range->count < lim && range->block < lim) ? 1 : 0;
}

void stats_to_host(const unsigned long long* h, gr_stats* s)
{
    s->rays = (int64_t)h[0];
    s->accepted_steps = (int64_t)h[1];
    s->rejected_steps = (int64_t)h[2];
    s->rhs_evals = (int64_t)h[3];
    s->flagged_rays = (int64_t)h[4];
    for (int i = 0; i < 4; ++i) s->status_count[i] = (int64_t)h[5 + i];
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int32_t gr_abi_version(void) { return GR_ABI_VERSION; }

#ifdef GR_WAVE_TIMELINE
// debug builds only (not in the header): device buffer of 4 x u64 per wave for the next launches, or NULL
void gr_debug_set_timeline(void* device_buffer) { g_debug_timeline = (unsigned long long*)device_buffer; }
#endif

// For the tests (not in the header): the live-first tile order of the context's last trace launch as the device built it
// (gr_tile_order.hpp).  *tiles = 0: that launch kept its order.  Else min(*tiles, cap) entries of the permutation (queue position
// -> tile) go to `perm` and the number of tiles in the live class to *live.  Waits for the device.
int32_t gr_debug_tile_order(gr_ctx* c, uint32_t* perm, int64_t cap, int64_t* tiles, int64_t* live)
{
    if (!c || !tiles || !live) return fail(GR_ERR_INVALID_ARGUMENT, "ctx/tiles/live is null");
    *tiles = 0;
    *live = 0;
    if (!c->live_last) return GR_OK;
    GR_HIP(hipSetDevice(c->device));
    GR_HIP(hipDeviceSynchronize());
    uint32_t n_live = 0;
    GR_HIP(hipMemcpy(&n_live, c->live_last + c->live_last_tiles, sizeof n_live, hipMemcpyDeviceToHost));
    const int64_t n = cap < c->live_last_tiles ? cap : c->live_last_tiles;
    if (perm && n > 0) GR_HIP(hipMemcpy(perm, c->live_last, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    *tiles = c->live_last_tiles;
    *live = (int64_t)n_live;
    return GR_OK;
}

const char* gr_last_error(void) { return g_last_error.c_str(); }

// ---- GR_METRIC_COMPILED: the registry of kernel modules (include/gradus_mi355x.h, "compiled metrics") ----
int32_t gr_metric_module_load(const char* path, int64_t* metric_id)
{
    if (!path || !metric_id) return fail(GR_ERR_INVALID_ARGUMENT, "gr_metric_module_load: path or metric_id is null");
    *metric_id = -1;
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        const char* why = dlerror();
        return fail(GR_ERR_INVALID_ARGUMENT, std::string("gr_metric_module_load: ") + (why ? why : "dlopen failed"));
    }
    typedef const gr_user_module_info_t* (*info_fn)(void);
    const info_fn info_of = reinterpret_cast<info_fn>(dlsym(h, "gr_user_module_info"));
    if (!info_of) {
        dlclose(h);
        return fail(GR_ERR_INVALID_ARGUMENT, std::string("gr_metric_module_load: ") + path + " exports no gr_user_module_info: not a metric module");
    }
    const gr_user_module_info_t* info = info_of();
    if (!info || info->abi_version != GR_ABI_VERSION || info->metric_id != GR_METRIC_COMPILED) {
        const std::string got = info ? std::to_string(info->abi_version) : std::string("none");
        dlclose(h);
        return fail(GR_ERR_INVALID_ARGUMENT, std::string("gr_metric_module_load: ") + path + " was compiled for ABI " + got + ", this library is ABI "
                                             + std::to_string(GR_ABI_VERSION));
    }
    if (std::memcmp(info->header_hash, kCsrcHash, sizeof kCsrcHash) != 0) {
        const std::string got = hash_hex(info->header_hash);
        dlclose(h);
        return fail(GR_ERR_INVALID_ARGUMENT, std::string("gr_metric_module_load: ") + path + " was compiled against other kernel sources (hash " + got
                                             + ") than this library (" + hash_hex(kCsrcHash) + "): compile it again");
    }
    MetricKernels k;
    k.build_id = info->build_id;
    k.trace64 = reinterpret_cast<trace_fn>(dlsym(h, "gr64_launch_trace_m12"));
    k.path = reinterpret_cast<path_fn>(dlsym(h, "gr64_launch_path_m12"));
    k.apply = reinterpret_cast<apply_fn>(dlsym(h, "gr64_launch_apply_m12"));
    k.classify = reinterpret_cast<classify_fn>(dlsym(h, "gr64_launch_classify_m12"));
    k.area = reinterpret_cast<areafactor_fn>(dlsym(h, "gr64_launch_areafactor_m12"));
    k.tan = reinterpret_cast<trace_fn>(dlsym(h, "grt_launch_trace_m12"));
    k.tan1 = reinterpret_cast<trace_fn>(dlsym(h, "grt1_launch_trace_m12"));
    k.sky = reinterpret_cast<trace_fn>(dlsym(h, "grts_launch_trace_m12"));
    k.sky1 = reinterpret_cast<trace_fn>(dlsym(h, "grts1_launch_trace_m12"));
    k.offset = reinterpret_cast<offset_fn>(dlsym(h, "grv1_launch_offset_m12"));
    k.attrs64 = reinterpret_cast<attrs_fn>(dlsym(h, "gr64_kernel_attrs_m12"));
    k.attrs_tan = reinterpret_cast<attrs_fn>(dlsym(h, "grt_kernel_attrs_m12"));
    k.attrs_tan1 = reinterpret_cast<attrs_fn>(dlsym(h, "grt1_kernel_attrs_m12"));
    // the fp64 set is what every entry point needs; the other flavours may be absent (their entry points then refuse the metric)
    if (!k.trace64 || !k.path || !k.apply || !k.classify) {
        dlclose(h);
        return fail(GR_ERR_INVALID_ARGUMENT, std::string("gr_metric_module_load: ") + path + " lacks a launcher of the fp64 set "
                                             "(gr64_launch_trace_m12, _path_, _apply_, _classify_)");
    }
    std::lock_guard<std::mutex> lock(g_modules_mu);
    for (int slot = 0; slot < GR_METRIC_MODULE_SLOTS; ++slot) {
        if (g_modules[slot].used) continue;
        g_modules[slot].used = true;
        g_modules[slot].handle = h;
        g_modules[slot].k = k;
        *metric_id = GR_METRIC_COMPILED + slot;
        return GR_OK;
    }
    dlclose(h);
    return fail(GR_ERR_UNSUPPORTED, "gr_metric_module_load: all " + std::to_string(GR_METRIC_MODULE_SLOTS) + " module slots are taken: unload one");
}

int32_t gr_metric_module_unload(int32_t metric_id)
{
    std::lock_guard<std::mutex> lock(g_modules_mu);
    const int slot = metric_id - GR_METRIC_COMPILED;
    if (slot < 0 || slot >= GR_METRIC_MODULE_SLOTS || !g_modules[slot].used)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_metric_module_unload: no module is loaded under metric_id " + std::to_string(metric_id));
    // the slot is free; the code stays mapped (no dlclose): a launch in flight may still run it, and its kernels stay registered
    g_modules[slot] = ModuleSlot{};
    return GR_OK;
}

int32_t gr_metric_module_build_id(int32_t metric_id, int64_t* build_id)
{
    if (!build_id) return fail(GR_ERR_INVALID_ARGUMENT, "gr_metric_module_build_id: build_id is null");
    *build_id = 0;
    MetricKernels k;
    if (metric_id < GR_METRIC_COMPILED || !metric_kernels(metric_id, k))
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_metric_module_build_id: no module is loaded under metric_id " + std::to_string(metric_id));
    *build_id = k.build_id;
    return GR_OK;
}

int32_t gr_metric_module_resources(int32_t metric_id, const gr_config* cfg, gr_metric_resources* out)
{
    if (!out) return fail(GR_ERR_INVALID_ARGUMENT, "gr_metric_module_resources: out is null");
    std::memset(out, 0, sizeof(gr_metric_resources) * GR_MODULE_KERNEL_COUNT);
    MetricKernels k;
    if (metric_id < GR_METRIC_COMPILED || !metric_kernels(metric_id, k))
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_metric_module_resources: no module is loaded under metric_id " + std::to_string(metric_id));
    const int disc = cfg ? cfg->disc_id : GR_DISC_THIN;
    const attrs_fn fns[GR_MODULE_KERNEL_COUNT] = { k.attrs64, k.attrs64, k.attrs_tan, k.attrs_tan1 };
    for (int q = 0; q < GR_MODULE_KERNEL_COUNT; ++q) {
        if (!fns[q]) continue;
        hipFuncAttributes a;
        std::memset(&a, 0, sizeof(a));
        GR_HIP(fns[q](q == GR_MODULE_KERNEL_TRACE_PERSISTENT ? 1 : 0, disc, &a));
        out[q].vgprs = a.numRegs;
        out[q].scratch_bytes = (int32_t)a.localSizeBytes;
        out[q].lds_bytes = (int32_t)a.sharedSizeBytes;
        out[q].max_threads = a.maxThreadsPerBlock;
    }
    return GR_OK;
}

int32_t gr_ctx_create(int32_t device, gr_ctx** out)
{
    if (!out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(GR_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= count)
        return fail(GR_ERR_INVALID_ARGUMENT, "device index out of range");
    GR_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    GR_HIP(hipGetDeviceProperties(&prop, device));
    gr_ctx* c = new gr_ctx();
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    int32_t rc = GR_OK;
    do {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(GR_ERR_HIP, "hipStreamCreate failed"); break; }
        if (hipMalloc((void**)&c->d_queue, sizeof(unsigned long long) * c->queue_slots) != hipSuccess) { rc = fail(GR_ERR_OUT_OF_MEMORY, "hipMalloc(queue) failed"); break; }
        if (hipMalloc((void**)&c->d_stats, sizeof(unsigned long long) * N_STAT) != hipSuccess) { rc = fail(GR_ERR_OUT_OF_MEMORY, "hipMalloc(stats) failed"); break; }
        if (hipMalloc((void**)&c->d_cold, sizeof(Cold) * c->queue_slots) != hipSuccess) { rc = fail(GR_ERR_OUT_OF_MEMORY, "hipMalloc(cold) failed"); break; }
        {
            const size_t part_bytes = sizeof(unsigned long long) * gr_fold::kStatWords * (size_t)c->queue_slots;
            if (hipMalloc((void**)&c->d_stat_part, part_bytes) != hipSuccess) { rc = fail(GR_ERR_OUT_OF_MEMORY, "hipMalloc(stats partials) failed"); break; }
            // (zero before any stream of the caller's can reach it: the wait is for that)
            if (hipMemsetAsync(c->d_stat_part, 0, part_bytes, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
                rc = fail(GR_ERR_HIP, "hipMemset(stats partials) failed");
                break;
            }
        }
        if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess || hipEventCreate(&c->ev_k) != hipSuccess
            || hipEventCreateWithFlags(&c->ev_cost, hipEventDisableTiming) != hipSuccess
            || hipEventCreateWithFlags(&c->ev_tables, hipEventDisableTiming) != hipSuccess) { rc = fail(GR_ERR_HIP, "hipEventCreate failed"); break; }
    } while (0);
    if (rc != GR_OK) {
        gr_ctx_destroy(c);
        return rc;
    }
    c->counted = true;
    g_live_ctx.fetch_add(1);
    *out = c;
    return GR_OK;
}

static void pool_drop_all();
static void sky_drop_ctx(gr_ctx* c);      // the resident skies a context owns go with it (gr_sky_*, at the end of this file)

int32_t gr_ctx_destroy(gr_ctx* c)
{
    if (!c) return GR_OK;
    // the last context takes the pool of page-locked blocks with it (blocks still HELD by the caller stay: their finalizers
    // may run later, gr_host_free needs no context)
    if (c->counted && g_live_ctx.fetch_sub(1) == 1) pool_drop_all();
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    sky_drop_ctx(c);
    if (c->d_queue) (void)hipFree(c->d_queue);
    if (c->d_stats) (void)hipFree(c->d_stats);
    if (c->d_stat_part) (void)hipFree(c->d_stat_part);
    if (c->d_cold) (void)hipFree(c->d_cold);
    if (c->d_transfer) (void)hipFree(c->d_transfer);
    if (c->d_disc_table) (void)hipFree(c->d_disc_table);
    if (c->d_mesh) (void)hipFree(c->d_mesh);
    if (c->d_chart_table) (void)hipFree(c->d_chart_table);
    if (c->d_metric_table) (void)hipFree(c->d_metric_table);
    if (c->d_corona) (void)hipFree(c->d_corona);
    if (c->d_lag) (void)hipFree(c->d_lag);
    if (c->d_sky) (void)hipFree(c->d_sky);
    if (c->d_sky_table) (void)hipFree(c->d_sky_table);
    if (c->d_tile_cost) (void)hipFree(c->d_tile_cost);
    if (c->d_tile_perm) (void)hipFree(c->d_tile_perm);
    if (c->d_live_perm) (void)hipFree(c->d_live_perm);
    if (c->d_live_flags) (void)hipFree(c->d_live_flags);
    if (c->ev_cost) (void)hipEventDestroy(c->ev_cost);
    if (c->ev_tables) (void)hipEventDestroy(c->ev_tables);
    if (c->d_plunge) (void)hipFree(c->d_plunge);
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->d_offset_work) (void)hipFree(c->d_offset_work);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_k) (void)hipEventDestroy(c->ev_k);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    for (hipEvent_t e : c->ev_band)
        if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->band_stream) (void)hipStreamDestroy(c->band_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    delete c;
    return GR_OK;
}

// Pinned result blocks are registered process-wide, not per context: the caller's array (a Julia Vector with a finalizer)
// may outlive the context that allocated it, and finalizers run in no particular order.
//
// How a block is made (round 3, scripts/microbench/host_register_thp.hip on the GPU box, 608 MiB = the end points of a 2048² plane):
//   hipHostMalloc 122-365 ms, hipHostFree 82-97 ms -- page-locking 155 000 4-KiB pages, ten times the call the block serves;
//   mmap + MADV_HUGEPAGE + first touch from 8 threads 11-12 ms, hipHostRegister (Portable | Mapped) of those 304 huge pages
//   1.3 ms, hipHostUnregister 0.0 ms, munmap 28-42 ms; device-to-host copies and the kernel's own stores reach the same
//   56 GB/s either way.
// So blocks of 8 MiB and more are anonymous mappings on transparent huge pages that the library registers (13 ms instead of
// 122-365); smaller ones, and any block for which one of those steps fails, come from hipHostMalloc as before.
// Freed blocks still go to a small process-wide POOL first and the next gr_host_alloc of a similar size takes one from there
// (no cost at all).  Bounded (4 blocks, 4 GiB in all by default: gr_ctx_set(ctx, "pinned_pool_mib", MiB); 0 empties and
// disables it); a pooled block is handed out for requests between half its size and its size.
namespace {
struct PinnedMem {
    void* p;          // what the caller holds
    size_t size;      // usable bytes
    void* map;        // base of the anonymous mapping (null: the block came from hipHostMalloc)
    size_t map_len;
};
std::mutex g_pinned_mutex;
std::vector<PinnedMem> g_pinned;      // blocks handed out
std::vector<PinnedMem> g_pool;        // page-locked blocks waiting for the next gr_host_alloc
size_t g_pool_cap = (size_t)1 << 30;  // freed blocks kept page-locked: 1 GiB (one 2048² end-point block and change); "pinned_pool_mib"
constexpr size_t kPoolBlocks = 4;
constexpr size_t kHugeMin = (size_t)8 << 20;
std::atomic<bool> g_pinned_huge{ true };   // gr_ctx_set(ctx, "pinned_huge", 0): every block from hipHostMalloc (process-wide)
// A garbage-collected caller (Julia, Python) sees a 100-byte wrapper, not the block behind it, and may pile up page-locked
// memory long before a collection runs: the bytes handed out and not yet freed are counted, and gr_host_alloc REFUSES
// (GR_ERR_OUT_OF_MEMORY) a request that would take them past this cap -- the bindings then collect and retry, or fall back to
// an ordinary pageable array.  gr_ctx_set(ctx, "pinned_max_mib", MiB), default 8 GiB.
size_t g_pinned_max = (size_t)8 << 30;
size_t g_pinned_out = 0;              // bytes of g_pinned (under g_pinned_mutex)

void prefault_threads(char* base, size_t bytes);     // below: first touch from up to 8 threads

bool pinned_make(size_t want, PinnedMem& out)
{
    if (g_pinned_huge.load(std::memory_order_relaxed) && want >= kHugeMin) {
        const size_t two = (size_t)2 << 20, len = (want + two - 1) / two * two;
        void* m = mmap(nullptr, len + two, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m != MAP_FAILED) {
            char* al = (char*)(((size_t)m + two - 1) / two * two);
            (void)madvise(al, len, MADV_HUGEPAGE);          // refused or unavailable: 4-KiB pages, a slower registration, same result
            prefault_threads(al, len);
            if (hipHostRegister(al, len, hipHostRegisterPortable | hipHostRegisterMapped) == hipSuccess) {
                out = PinnedMem{ al, len, m, len + two };
                return true;
            }
            (void)hipGetLastError();
            (void)munmap(m, len + two);
        }
    }
    void* p = nullptr;
    // page-locked and mapped for every device (hipHostMallocPortable): a multi-device render may write into one block
    if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess) return false;
    out = PinnedMem{ p, want, nullptr, 0 };
    return true;
}
hipError_t pinned_release(const PinnedMem& b)
{
    if (!b.map) return hipHostFree(b.p);      // waits for work that still targets the block
    const hipError_t e = hipHostUnregister(b.p);
    (void)munmap(b.map, b.map_len);
    return e;
}

size_t pool_bytes_locked()
{
    size_t t = 0;
    for (const auto& q : g_pool) t += q.size;
    return t;
}
// release pooled blocks until the pool fits `cap` (call with g_pinned_mutex held; trims are rare)
void pool_trim_locked(size_t cap)
{
    while (!g_pool.empty() && (pool_bytes_locked() > cap || g_pool.size() > kPoolBlocks)) {
        (void)pinned_release(g_pool.front());
        g_pool.erase(g_pool.begin());
    }
}
}

static void pool_drop_all()
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    pool_trim_locked(0);
}

int32_t gr_ctx_set(gr_ctx* c, const char* key, int64_t value)
{
    if (!c || !key) return fail(GR_ERR_INVALID_ARGUMENT, "ctx/key is null");
    const std::string k(key);
    if (k == "pipeline") {
        if (value < 0 || value > 8) return fail(GR_ERR_INVALID_ARGUMENT, "pipeline must be 0..8 bands");
        c->pipeline = value;
        return GR_OK;
    }
    if (k == "kernel") {
        if (value < 0 || value > 2) return fail(GR_ERR_INVALID_ARGUMENT, "kernel must be 0 (lane), 1 (persistent) or 2 (auto)");
        c->kernel = value;
    } else if (k == "block") {
        if (value != 0 && (value < 64 || value > 256 || value % 64)) return fail(GR_ERR_INVALID_ARGUMENT, "block must be 0 (auto) or a multiple of 64 in [64, 256]");
        c->block = value;
    } else if (k == "refill_threshold") {
        if (value < 0 || value > 64) return fail(GR_ERR_INVALID_ARGUMENT, "refill_threshold must be in [0, 64] (0 = auto)");
        c->refill_threshold = value;
    } else if (k == "waves_per_simd") {
        if (value < 0 || value > 8) return fail(GR_ERR_INVALID_ARGUMENT, "waves_per_simd must be in [0, 8]");
        c->waves_per_simd = value;
    } else if (k == "swizzle") {
        c->swizzle = value ? 1 : 0;
    } else if (k == "tile_rows") {
        if (value != 8 && value != 16) return fail(GR_ERR_INVALID_ARGUMENT, "tile_rows must be 8 or 16");
        c->tile_rows = value;
        c->lpt_key.clear();
    } else if (k == "lpt_lane") {
        c->lpt_lane = value ? 1 : 0;
        c->lpt_key.clear();
    } else if (k == "lds") {
        c->lds = value ? 1 : 0;
    } else if (k == "precision") {
        if (value != 32 && value != 64) return fail(GR_ERR_INVALID_ARGUMENT, "precision must be 32 or 64");
        c->precision = value;
    } else if (k == "lpt") {
        if (value < 0 || value > 2) return fail(GR_ERR_INVALID_ARGUMENT, "lpt must be 0 (off), 1 (auto) or 2 (always)");
        c->lpt = value;
        c->lpt_key.clear();
    } else if (k == "live_first") {
        if (value < 0 || value > 2) return fail(GR_ERR_INVALID_ARGUMENT, "live_first must be 0 (off), 1 (auto) or 2 (always)");
        c->live_first = value;
    } else if (k == "hugepages") {
        c->hugepages = value ? 1 : 0;
    } else if (k == "tangent_norm") {
        c->tangent_norm = value ? 1 : 0;
    } else if (k == "tangent_pairs") {
        if (value < 0 || value > 2) return fail(GR_ERR_INVALID_ARGUMENT, "tangent_pairs must be 0 (one lane per ray), 1 (a pair of lanes per ray) or 2 (by launch size)");
        c->tangent_pairs = value;
    } else if (k == "xcd_spread") {
        c->xcd_spread = value ? 1 : 0;
    } else if (k == "sky_deal") {
        c->sky_deal = value ? 1 : 0;
    } else if (k == "tf_chunk") {
        if (value < 0 || value > 65536) return fail(GR_ERR_INVALID_ARGUMENT, "tf_chunk must be in [0, 65536] (0 = auto)");
        c->tf_chunk = value;
    } else if (k == "lds_points") {
        c->lds_points = value ? 1 : 0;
    } else if (k == "direct_host") {
        c->direct_host = value ? 1 : 0;
    } else if (k == "pinned_huge") {
        g_pinned_huge.store(value != 0);
    } else if (k == "pinned_max_mib") {
        if (value < 0) return fail(GR_ERR_INVALID_ARGUMENT, "pinned_max_mib must be non-negative");
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        g_pinned_max = (size_t)value << 20;        // process-wide: bytes of gr_host_alloc blocks that may be outstanding at once
    } else if (k == "pinned_pool_mib") {
        if (value < 0) return fail(GR_ERR_INVALID_ARGUMENT, "pinned_pool_mib must be non-negative");
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        g_pool_cap = (size_t)value << 20;          // process-wide, like the blocks themselves
        pool_trim_locked(g_pool_cap);
    } else {
        return fail(GR_ERR_INVALID_ARGUMENT, "unknown knob '" + k + "'");
    }
    return GR_OK;
}

int32_t gr_host_alloc(gr_ctx* ctx, int64_t bytes, void** out)
{
    if (!ctx || !out) return fail(GR_ERR_INVALID_ARGUMENT, "ctx/out is null");
    *out = nullptr;
    if (bytes < 0) return fail(GR_ERR_INVALID_ARGUMENT, "bytes must be non-negative");
    const size_t want = (size_t)(bytes > 0 ? bytes : 1);
    try {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        if (g_pinned_out + want > g_pinned_max)
            return fail(GR_ERR_OUT_OF_MEMORY, "gr_host_alloc: " + std::to_string((g_pinned_out + want) >> 20) + " MiB of page-locked results would be "
                        "outstanding (cap " + std::to_string(g_pinned_max >> 20) + " MiB, gr_ctx_set \"pinned_max_mib\"): free or finalize earlier results");
        // best fit among the pooled blocks that are large enough and not more than twice as large
        auto best = g_pool.end();
        for (auto it = g_pool.begin(); it != g_pool.end(); ++it)
            if (it->size >= want && it->size / 2 <= want && (best == g_pool.end() || it->size < best->size)) best = it;
        if (best != g_pool.end()) {
            g_pinned.push_back(*best);
            g_pinned_out += best->size;
            *out = best->p;
            g_pool.erase(best);
            return GR_OK;
        }
    } catch (...) {
        return fail(GR_ERR_OUT_OF_MEMORY, "gr_host_alloc: registry");
    }
    GR_HIP(hipSetDevice(ctx->device));
    PinnedMem b{};
    if (!pinned_make(want, b)) {
        const hipError_t e = hipGetLastError();
        return fail(GR_ERR_OUT_OF_MEMORY, std::string("gr_host_alloc: ") + hipGetErrorString(e));
    }
    try {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        g_pinned.push_back(b);
        g_pinned_out += b.size;
    } catch (...) {
        (void)pinned_release(b);
        return fail(GR_ERR_OUT_OF_MEMORY, "gr_host_alloc: registry");
    }
    *out = b.p;
    return GR_OK;
}

int32_t gr_host_free(gr_ctx* /* may be NULL or already destroyed: not dereferenced */, void* p)
{
    if (!p) return GR_OK;
    PinnedMem b{};
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        auto it = std::find_if(g_pinned.begin(), g_pinned.end(), [p](const PinnedMem& q) { return q.p == p; });
        if (it == g_pinned.end()) return fail(GR_ERR_INVALID_ARGUMENT, "pointer was not allocated by gr_host_alloc");
        b = *it;
        g_pinned.erase(it);
        g_pinned_out -= b.size <= g_pinned_out ? b.size : g_pinned_out;
        // every entry point that writes a block is blocking, so nothing targets it any more: it can wait for the next request
        if (b.size <= g_pool_cap && g_live_ctx.load() > 0) {      // no context left: nobody to hand the block to
            // the newest block is the likeliest to be asked for again: older ones make room (least recently freed first)
            while (!g_pool.empty() && (g_pool.size() >= kPoolBlocks || pool_bytes_locked() + b.size > g_pool_cap)) {
                (void)pinned_release(g_pool.front());
                g_pool.erase(g_pool.begin());
            }
            try {
                g_pool.push_back(b);
                return GR_OK;
            } catch (...) {
            }
        }
    }
    GR_HIP(pinned_release(b));
    return GR_OK;
}

// Do the `bytes` bytes at p lie inside ONE block the library pinned itself?  (No page faults to prepare, no huge-page advice to
// give -- and the only memory a kernel may store into across the link: the whole extent is checked, a pointer near the end of a
// block or a pooled block handed out for a smaller request must not send the GPU past the registered mapping.)
static bool is_pinned(const void* p, size_t bytes)
{
    if (!p) return false;
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    for (const auto& q : g_pinned)
        if ((const char*)p >= (const char*)q.p && (const char*)p + (bytes ? bytes : 1) <= (const char*)q.p + q.size) return true;
    return false;
}

// out_global: pixel / record of local ray j goes to index range_map(j) of d_image / d_points (the whole plane's buffer, which
// several devices fill together) instead of to index j of a buffer holding this range only
static int32_t render_device_impl(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf,
                                  const gr_range* range, double* d_image, gr_stats* d_stats, void* hip_stream, bool out_global)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if ((rc = validate_plane(plane, range)) != GR_OK) return rc;
    if (!d_image && range->count > 0) return fail(GR_ERR_INVALID_ARGUMENT, "image is null");
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    plane_params(ctx, p, cd, cfg, plane, range);
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    cd.out_mode = 0;
    cd.image = d_image;
    cd.out_global = out_global ? 1 : 0;
    p.stats = (unsigned long long*)d_stats;   // same layout: 9 x 64-bit counters then kernel_ms
    return launch_trace(ctx, p, cd, stream);
}

int32_t gr_render_device(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf,
                         const gr_range* range, double* d_image, gr_stats* d_stats, void* hip_stream)
{
    return render_device_impl(ctx, cfg, plane, pf, range, d_image, d_stats, hip_stream, false);
}

static int32_t render_endpoints_device_impl(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_range* range,
                                            gr_point* d_points, gr_stats* d_stats, void* hip_stream, bool out_global)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if ((rc = validate_plane(plane, range)) != GR_OK) return rc;
    if (!d_points && range->count > 0) return fail(GR_ERR_INVALID_ARGUMENT, "points is null");
    GR_HIP(hipSetDevice(ctx->device));
    Params p;
    Cold cd;
    plane_params(ctx, p, cd, cfg, plane, range);
    cd.out_mode = 1;
    cd.points = d_points;
    cd.out_global = out_global ? 1 : 0;
    p.stats = (unsigned long long*)d_stats;
    return launch_trace(ctx, p, cd, (hipStream_t)hip_stream);
}

int32_t gr_render_endpoints_device(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_range* range,
                                   gr_point* d_points, gr_stats* d_stats, void* hip_stream)
{
    return render_endpoints_device_impl(ctx, cfg, plane, range, d_points, d_stats, hip_stream, false);
}

int32_t gr_trace_endpoints_device(gr_ctx* ctx, const gr_config* cfg, const double* d_x, int64_t x_stride,
                                  const double* d_v, int64_t n, gr_point* d_points, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (x_stride != 0 && x_stride != 4) return fail(GR_ERR_INVALID_ARGUMENT, "x_stride must be 0 or 4");
    if (n > 0 && (!d_x || !d_v || !d_points)) return fail(GR_ERR_INVALID_ARGUMENT, "x/v/points is null");
    GR_HIP(hipSetDevice(ctx->device));
    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = n;
    p.stats = (unsigned long long*)d_stats;
    cd.src_mode = 1;
    cd.out_mode = 1;
    cd.x = d_x;
    cd.x_stride = x_stride;
    cd.v = d_v;
    cd.points = d_points;
    cd.range = gr_range{ 0, n, n > 0 ? n : 1, 1 };
    cd.swizzle = 0;
    return launch_trace(ctx, p, cd, (hipStream_t)hip_stream);
}

int32_t gr_apply_pointfunction_device(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf,
                                      const gr_point* d_points, int64_t n, double max_time, double* d_out, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (n > 0 && (!d_points || !d_out)) return fail(GR_ERR_INVALID_ARGUMENT, "points/out is null");
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = n;
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    if (n == 0) return GR_OK;
    if ((rc = stage_metric_table(ctx, p, stream)) != GR_OK) return rc;
    Cold* slot = ctx->d_cold + ctx->cold_next;
    ctx->cold_next = (ctx->cold_next + 1) % ctx->queue_slots;
    GR_HIP(hipMemcpyAsync(slot, &cd, sizeof(Cold), hipMemcpyHostToDevice, stream));
    p.cold = slot;
    {
        MetricKernels mk;
        if (!metric_kernels(cfg->metric_id, mk)) return fail(GR_ERR_UNSUPPORTED, "unknown metric_id " + std::to_string(cfg->metric_id));
        GR_NEED_KERNEL(mk.apply, "point-function");
        GR_HIP(mk.apply(&p, d_points, max_time, d_out, stream));
    }
    GR_HIP(hipGetLastError());
    if ((cd.pf.n_plunge > 0 || cfg->metric_id == GR_METRIC_TABULATED) && (rc = tables_release(ctx, stream)) != GR_OK) return rc;
    return GR_OK;
}

// γ(r) A(r) of the disc at n radii (k_disc_area_factor): the velocity branches are those of the REDSHIFT point function, so pf is
// staged as a launch of it stages it
int32_t gr_disc_area_factor_device(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf, const double* d_r, int64_t n,
                                   double* d_out, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (n > 0 && (!d_r || !d_out)) return fail(GR_ERR_INVALID_ARGUMENT, "r/out is null");
    if (!pf || pf->pf_id != GR_PF_REDSHIFT)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_disc_area_factor: the disc's velocity is the redshift point function's: pf->pf_id must be GR_PF_REDSHIFT");
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = n;
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    const bool tables = cd.pf.n_plunge > 0 || cfg->metric_id == GR_METRIC_TABULATED;
    if (n == 0) return GR_OK;
    if ((rc = stage_metric_table(ctx, p, stream)) != GR_OK) return rc;
    Cold* slot = ctx->d_cold + ctx->cold_next;
    ctx->cold_next = (ctx->cold_next + 1) % ctx->queue_slots;
    GR_HIP(hipMemcpyAsync(slot, &cd, sizeof(Cold), hipMemcpyHostToDevice, stream));
    p.cold = slot;
    {
        MetricKernels mk;
        if (!metric_kernels(cfg->metric_id, mk)) return fail(GR_ERR_UNSUPPORTED, "unknown metric_id " + std::to_string(cfg->metric_id));
        GR_NEED_KERNEL(mk.area, "area-factor");
        GR_HIP(mk.area(&p, d_r, d_out, stream));
    }
    GR_HIP(hipGetLastError());
    if (tables && (rc = tables_release(ctx, stream)) != GR_OK) return rc;
    return GR_OK;
}

static void prefault_output(void* dst, size_t bytes, bool huge);

int32_t gr_trace_paths(gr_ctx* ctx, const gr_config* cfg, const double* x, int64_t x_stride, const double* v, int64_t n,
                       int64_t cap, double* path, int64_t* n_rows, gr_point* endpoints)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (!x || !v || !path || !n_rows || cap < 2 || n < 0 || (x_stride != 0 && x_stride != 4))
        return fail(GR_ERR_INVALID_ARGUMENT, "x/v/path/n_rows is null, cap < 2, n < 0 or x_stride not 0 / 4");
    if (n == 0) return GR_OK;
    GR_HIP(hipSetDevice(ctx->device));
    const size_t path_bytes = sizeof(double) * 9 * (size_t)cap * (size_t)n;
    const size_t pt_bytes = sizeof(gr_point) * (size_t)n;
    if ((rc = ensure(&ctx->d_scratch, &ctx->scratch_bytes, path_bytes + pt_bytes + 8 * (size_t)n + 16)) != GR_OK) return rc;
    const size_t nx = x_stride ? (size_t)n : 1;
    if ((rc = ensure(&ctx->d_in, &ctx->in_bytes, sizeof(double) * 4 * (nx + (size_t)n) + 8)) != GR_OK) return rc;
    double* d_path = (double*)ctx->d_scratch;
    gr_point* d_pt = (gr_point*)((char*)ctx->d_scratch + path_bytes);
    unsigned long long* d_n = (unsigned long long*)((char*)d_pt + pt_bytes);
    double* d_x = (double*)ctx->d_in;
    double* d_v = d_x + 4 * nx;
    GR_HIP(hipMemcpyAsync(d_x, x, sizeof(double) * 4 * nx, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(d_v, v, sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = n;
    derive_params(p);
    cd.src_mode = 1;
    cd.out_mode = 1;
    cd.winding_plane = p.cfg.winding_plane;
    cd.x = d_x;
    cd.x_stride = x_stride;
    cd.v = d_v;
    cd.points = d_pt;
    cd.range = gr_range{ 0, n, n, 1 };
    if ((rc = stage_disc_table(ctx, p, ctx->stream)) != GR_OK) return rc;
    Cold* slot = ctx->d_cold + ctx->cold_next;
    ctx->cold_next = (ctx->cold_next + 1) % ctx->queue_slots;
    GR_HIP(hipMemcpyAsync(slot, &cd, sizeof(Cold), hipMemcpyHostToDevice, ctx->stream));
    p.cold = slot;
    {
        MetricKernels mk;
        if (!metric_kernels(cfg->metric_id, mk)) return fail(GR_ERR_UNSUPPORTED, "unknown metric_id " + std::to_string(cfg->metric_id));
        GR_NEED_KERNEL(mk.path, "path");
        GR_HIP(mk.path(&p, d_path, cap, d_n, ctx->stream));
    }
    GR_HIP(hipGetLastError());
    if ((p.disc_table || p.chart_table || cfg->metric_id == GR_METRIC_TABULATED) && (rc = tables_release(ctx, ctx->stream)) != GR_OK) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "row counters are copied as int64");
    if (!is_pinned(path, path_bytes)) prefault_output(path, path_bytes, ctx->hugepages != 0);          // while the kernel runs (the path buffer of 16 384 geodesics is 600 MB)
    GR_HIP(hipMemcpyAsync(n_rows, d_n, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipMemcpyAsync(path, d_path, path_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (endpoints) GR_HIP(hipMemcpyAsync(endpoints, d_pt, pt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    return GR_OK;
}

int32_t gr_trace_path(gr_ctx* ctx, const gr_config* cfg, const double* x, const double* v, int64_t cap, double* path,
                      int64_t* n_rows, gr_point* endpoint)
{
    return gr_trace_paths(ctx, cfg, x, 0, v, 1, cap, path, n_rows, endpoint);
}

// A source without one position (gr_rayset.sky_rows) brings a source velocity per sample: only gr_ray_summary / gr_corona_trace scale a
// row's g with its sample's factor (k_sky_scale_g).  The line profile, the (g, ρ) pairs and the ray tangents would return g against
// the static observer instead: they refuse such a set, before anything of it is staged.
static int32_t refuse_sky_rows(const gr_rayset* rays, const char* who)
{
    if (rays && rays->sky_sampler && rays->sky_rows)
        return fail(GR_ERR_INVALID_ARGUMENT, std::string(who) + ": a sky source with sky_rows (a source velocity per sample) is traced by gr_ray_summary / "
                                             "gr_corona_trace, the only calls that form g against each sample's own velocity");
    return GR_OK;
}

// GR_METRIC_TABULATED under a source without one position: EVERY sample's start radius (sky_rows[28 j + 1], host memory here) must lie
// inside the table's radial range, with the slack of launch_trace's guard on x_obs -- which is not read for such a set.
static int32_t sky_rows_in_table(const gr_config* cfg, const gr_rayset* rays)
{
    if (!cfg || cfg->metric_id != GR_METRIC_TABULATED || !rays || !rays->sky_sampler || !rays->sky_rows || rays->n <= 0) return GR_OK;
    const int32_t trc = gr_metric_table_check(cfg->metric_table, cfg->metric_table_n);
    if (trc != GR_OK) return trc;
    const double t_min = cfg->metric_table[gr_tab::H_RMIN], t_max = cfg->metric_table[gr_tab::H_RMAX];
    double lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    for (int64_t j = 0; j < rays->n; ++j) {
        const double r = rays->sky_rows[GR_SKY_ROW * j + 1];
        nan = nan || !(r == r);
        lo = std::fmin(lo, r);
        hi = std::fmax(hi, r);
    }
    const bool below = !(lo >= t_min - 1e-9 * std::fabs(t_min) - 1e-12), above = !(hi <= t_max + 1e-9 * std::fabs(t_max));
    if (nan || below || above)
        return fail(GR_ERR_INVALID_ARGUMENT, "GR_METRIC_TABULATED: a sample of the sky source starts at r = " + (nan ? std::string("nan") : std::to_string(below ? lo : hi))
                                             + ", outside the radial range of the metric table [" + std::to_string(t_min) + ", " + std::to_string(t_max) + "]");
    return GR_OK;
}

static int32_t rays_params(gr_ctx* ctx, Params& p, Cold& cd, const gr_config* cfg, const gr_rayset* rays)
{
    if (!rays) return fail(GR_ERR_INVALID_ARGUMENT, "rayset is null");
    if (rays->n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (rays->sky_sampler) {
        // rays from a source into its sky (gr_rayset.sky_*): nothing per ray crosses but, for a caller's generator, its numbers
        if (rays->sky_sampler < 1 || rays->sky_sampler > 2 || rays->sky_generator < 0 || rays->sky_generator > 2)
            return fail(GR_ERR_INVALID_ARGUMENT, "sky source: unknown sampler / generator");
        if (rays->sky_generator == 2 && rays->n > 0 && !rays->sky_i) return fail(GR_ERR_INVALID_ARGUMENT, "sky source: generator 2 needs sky_i");
        if (rays->sky_sampler == 2 && !(rays->sky_resolution > 0.0)) return fail(GR_ERR_INVALID_ARGUMENT, "sky source: WeierstrassSampler needs a resolution > 0");
        if (rays->sep_r || rays->height) return fail(GR_ERR_INVALID_ARGUMENT, "sky source: separable tables / per-ray heights do not apply");
        if (rays->sky_first < 0 || rays->sky_total < 0 || (rays->sky_total > 0 && rays->sky_first + rays->n > rays->sky_total))
            return fail(GR_ERR_INVALID_ARGUMENT, "sky source: the share sky_first .. sky_first + n runs past sky_total");
        ctx->sky_first = rays->sky_total > 0 ? rays->sky_first : 0;
        ctx->sky_total = rays->sky_total > 0 ? rays->sky_total : rays->n;
        ctx->sky_rows = rays->sky_rows;
        std::memset(&p, 0, sizeof p);
        std::memset(&cd, 0, sizeof cd);
        p.cfg = *cfg;
        p.n = rays->n;
        cd.src_mode = 3;
        std::memcpy(cd.plane.x_obs, rays->x_obs, sizeof cd.plane.x_obs);
        std::memcpy(cd.plane.Mx, rays->Mx, sizeof cd.plane.Mx);
        cd.plane.width = rays->n; cd.plane.height = 1;
        cd.range = gr_range{ 0, rays->n, rays->n > 0 ? rays->n : 1, 1 };
        cd.sky_sampler = rays->sky_sampler; cd.sky_both = rays->sky_both ? 1 : 0; cd.sky_generator = rays->sky_generator;
        cd.sky_resolution = rays->sky_resolution;
        cd.sky_i = rays->sky_generator == 2 ? rays->sky_i : nullptr;
        cd.swizzle = 0;
        return GR_OK;
    }
    if (rays->sep_r) {
        if (!rays->sep_cos || !rays->sep_sin || rays->sep_nr < 1 || rays->sep_nt < 1)
            return fail(GR_ERR_INVALID_ARGUMENT, "separable ray set: tables missing or empty");
        if (rays->sep_nr > (int64_t)1 << 31 || rays->sep_nt > (int64_t)1 << 31 || rays->sep_first < 0 || rays->sep_block < 0
            || (rays->sep_block > 0 && rays->sep_stride < rays->sep_block))
            return fail(GR_ERR_INVALID_ARGUMENT, "separable ray set: bad sep_first / sep_block / sep_stride");
        if (rays->n > 0) {
            const int64_t j = rays->n - 1;
            const int64_t last = rays->sep_block > 0
                                     ? rays->sep_first + (j / rays->sep_block) * rays->sep_stride + j % rays->sep_block
                                     : rays->sep_first + j;
            if (last >= rays->sep_nr * rays->sep_nt)
                return fail(GR_ERR_INVALID_ARGUMENT, "separable ray set: the launch's rays run past sep_nr * sep_nt");
        }
        if (rays->height) return fail(GR_ERR_INVALID_ARGUMENT, "separable ray set: per-ray heights are not supported");
    } else if (rays->n > 0 && (!rays->alpha || !rays->beta)) return fail(GR_ERR_INVALID_ARGUMENT, "alpha/beta is null");
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = rays->n;
    cd.src_mode = 2;
    std::memcpy(cd.plane.x_obs, rays->x_obs, sizeof cd.plane.x_obs);
    std::memcpy(cd.plane.Mx, rays->Mx, sizeof cd.plane.Mx);
    cd.plane.width = rays->n; cd.plane.height = 1;
    cd.range = gr_range{ 0, rays->n, rays->n > 0 ? rays->n : 1, 1 };
    cd.alpha = rays->alpha; cd.beta = rays->beta; cd.area = rays->area;
    cd.height = cfg->disc_id == GR_DISC_DATUM ? rays->height : nullptr;
    if (rays->sep_r) {
        cd.sep_r = rays->sep_r; cd.sep_cos = rays->sep_cos; cd.sep_sin = rays->sep_sin;
        cd.sep_nr = rays->sep_nr; cd.sep_nt = rays->sep_nt;
        cd.sep_first = rays->sep_first; cd.sep_block = rays->sep_block; cd.sep_stride = rays->sep_stride;
        const bool tiled = rays->sep_tiled && rays->sep_nr >= 8 && rays->sep_nt >= 8;
        cd.sep_core_rows = tiled ? (rays->sep_nr / 8) * 8 : 0;
        cd.sep_core_cols = tiled ? (rays->sep_nt / 8) * 8 : 0;
        if (!tiled) { cd.sep_core_rows = 0; cd.sep_core_cols = 0; }
        cd.alpha = cd.beta = cd.area = nullptr;
    }
    cd.swizzle = 0;
    (void)ctx;
    return GR_OK;
}

int32_t gr_lineprofile_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              const gr_binning* b, double* d_flux, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = refuse_sky_rows(rays, "gr_lineprofile_device")) != GR_OK) return rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (!b || b->n_bins < 1 || !b->bin_edges || !d_flux) return fail(GR_ERR_INVALID_ARGUMENT, "binning/flux is null or empty");
    if (!(b->r_max >= b->r_min)) return fail(GR_ERR_INVALID_ARGUMENT, "maxrₑ below minrₑ");
    if (cfg->disc_id == GR_DISC_NONE) return fail(GR_ERR_INVALID_ARGUMENT, "a line profile needs accretion geometry");
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    if ((rc = rays_params(ctx, p, cd, cfg, rays)) != GR_OK) return rc;
    if (!pf || pf->pf_id != GR_PF_REDSHIFT) return fail(GR_ERR_INVALID_ARGUMENT, "line profiles use the redshift point function");
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    cd.out_mode = 2;
    if (b->eps_n != 0 && (b->eps_n < 2 || !b->eps_r || !b->eps_v))
        return fail(GR_ERR_INVALID_ARGUMENT, "tabulated emissivity: needs eps_n >= 2 radii and values");
    cd.lp_rmin = b->r_min; cd.lp_rmax = b->r_max; cd.lp_q = b->emissivity_index;
    cd.lp_eps_r = b->eps_n >= 2 ? b->eps_r : nullptr; cd.lp_eps_v = b->eps_n >= 2 ? b->eps_v : nullptr;
    cd.lp_eps_n = b->eps_n >= 2 ? b->eps_n : 0;
    cd.lp_nbins = b->n_bins; cd.lp_edges = b->bin_edges; cd.lp_flux = d_flux;
    p.stats = (unsigned long long*)d_stats;
    GR_HIP(hipMemsetAsync(d_flux, 0, sizeof(double) * (size_t)b->n_bins, stream));
    return launch_trace(ctx, p, cd, stream);
}

int32_t gr_redshift_radius_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                                  double r_min, double r_max, double* d_pairs, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = refuse_sky_rows(rays, "gr_redshift_radius_device")) != GR_OK) return rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    if ((rc = rays_params(ctx, p, cd, cfg, rays)) != GR_OK) return rc;
    if (rays->n > 0 && !d_pairs) return fail(GR_ERR_INVALID_ARGUMENT, "pairs is null");
    if (!pf || pf->pf_id != GR_PF_REDSHIFT) return fail(GR_ERR_INVALID_ARGUMENT, "needs the redshift point function");
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    cd.out_mode = 3;
    cd.lp_rmin = r_min; cd.lp_rmax = r_max;
    cd.lp_pairs = d_pairs;
    p.stats = (unsigned long long*)d_stats;
    return launch_trace(ctx, p, cd, stream);
}

int32_t gr_ray_summary_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              double* d_out, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    if ((rc = rays_params(ctx, p, cd, cfg, rays)) != GR_OK) return rc;
    if (rays->n > 0 && !d_out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    if (!pf || pf->pf_id != GR_PF_REDSHIFT) return fail(GR_ERR_INVALID_ARGUMENT, "needs the redshift point function");
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    cd.out_mode = 4;
    cd.lp_rmin = 0.0;
    cd.lp_rmax = INFINITY;
    cd.lp_pairs = d_out;
    p.stats = (unsigned long long*)d_stats;
    const bool per_sample = rays->sky_sampler && rays->sky_rows;
    if (per_sample && pf->has_u_src)
        return fail(GR_ERR_INVALID_ARGUMENT, "a sky source with sky_rows brings a source velocity per ray: pf->has_u_src must be 0");
    if ((rc = launch_trace(ctx, p, cd, stream)) != GR_OK) return rc;
    if (per_sample && rays->n > 0) {
        // g of every row against ITS sample's source velocity (the factors were formed with the rays, sky_prepare)
        hipLaunchKernelGGL(k_sky_scale_g, dim3((unsigned)((rays->n + 255) / 256)), dim3(256), 0, stream, d_out, ctx->d_sky + 4 + 8 * rays->n, rays->n);
        GR_HIP(hipGetLastError());
    }
    return GR_OK;
}

int32_t gr_ray_tangent_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              double* d_out, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = refuse_sky_rows(rays, "gr_ray_tangent_device")) != GR_OK) return rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (cfg->disc_id == GR_DISC_NONE) return fail(GR_ERR_INVALID_ARGUMENT, "ray tangents are taken where the ray meets the geometry: none given");
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    if ((rc = rays_params(ctx, p, cd, cfg, rays)) != GR_OK) return rc;
    if (rays->n > 0 && !d_out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    if (!pf || pf->pf_id != GR_PF_REDSHIFT) return fail(GR_ERR_INVALID_ARGUMENT, "needs the redshift point function");
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    cd.out_mode = 5;
    cd.lp_rmin = 0.0;
    cd.lp_rmax = INFINITY;
    cd.lp_pairs = d_out;
    p.stats = (unsigned long long*)d_stats;
    return launch_trace(ctx, p, cd, stream);
}

// ---- gr_offset_solve / gr_offset_search: the iterations around gr_ray_tangent's rays, one problem per lane pair (gr_offsetsolve.hpp) ----
extern "C++" {
namespace {
// gr_offset_problems and gr_offset_searches as one: a (cos θ, sin θ | lower, upper), sign for a search alone
struct OffsetCall {
    int64_t n;
    const double *r_target, *a, *b, *sign, *height;
    gr_os::Setup st;
    int64_t max_iter, iterations, per_wave;
    bool search;
    int64_t out_stride() const { return search ? gr_os::search_stride(iterations) : gr_os::kSolveOut; }
};
int32_t offset_call(const gr_offset_problems* q, OffsetCall& c)
{
    if (!q) return fail(GR_ERR_INVALID_ARGUMENT, "gr_offset_solve: problems is null");
    c = OffsetCall{ q->n, q->r_target, q->cos_theta, q->sin_theta, nullptr, q->height,
                    gr_os::Setup{ q->alpha0, q->beta0, q->zero_atol, q->r_min, q->contrapoint_bias, 0, 0 }, q->max_iter, 0, q->per_wave, false };
    return GR_OK;
}
int32_t offset_call(const gr_offset_searches* q, OffsetCall& c)
{
    if (!q) return fail(GR_ERR_INVALID_ARGUMENT, "gr_offset_search: searches is null");
    c = OffsetCall{ q->n, q->r_target, q->lower, q->upper, q->sign, q->height,
                    gr_os::Setup{ q->alpha0, q->beta0, q->zero_atol, q->r_min, q->contrapoint_bias, 0, 0 }, q->max_iter, q->iterations, q->per_wave, true };
    return GR_OK;
}
// what every form refuses before anything touches the device
int32_t offset_check(const gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, OffsetCall& c, const void* out)
{
    const std::string who = c.search ? "gr_offset_search" : "gr_offset_solve";
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!rays) return fail(GR_ERR_INVALID_ARGUMENT, "rayset is null");
    if (rays->sky_sampler || rays->sky_rows) return fail(GR_ERR_UNSUPPORTED, who + ": the rays leave an observer's image plane, not a source's sky");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (cfg->disc_id != GR_DISC_THIN && cfg->disc_id != GR_DISC_DATUM)
        return fail(GR_ERR_UNSUPPORTED, who + ": the offsets are solved against a thin disc or a datum plane (disc_id " + std::to_string(cfg->disc_id) + ")");
    if (ctx->precision == 32) return fail(GR_ERR_UNSUPPORTED, who + ": the tangent kernels are fp64 (precision 32 is set)");
    if (c.n < 0 || c.n > (int64_t)INT32_MAX) return fail(GR_ERR_INVALID_ARGUMENT, who + ": n in 0 ... 2^31 - 1");
    if (c.n > 0 && (!c.r_target || !c.a || !c.b || (c.search && !c.sign) || !out)) return fail(GR_ERR_INVALID_ARGUMENT, who + ": a null pointer");
    if (c.max_iter < 0 || c.max_iter > (int64_t)1 << 20) return fail(GR_ERR_INVALID_ARGUMENT, who + ": max_iter in 0 ... 2^20");
    if (c.iterations < 0 || c.iterations > 4096) return fail(GR_ERR_INVALID_ARGUMENT, who + ": iterations in 0 ... 4096");
    if (c.per_wave < 0 || c.per_wave > 32) return fail(GR_ERR_INVALID_ARGUMENT, who + ": per_wave in 0 ... 32");
    if (!pf || pf->pf_id != GR_PF_REDSHIFT) return fail(GR_ERR_INVALID_ARGUMENT, who + ": needs the redshift point function");
    c.st.max_iter = (int32_t)c.max_iter;
    c.st.iterations = (int32_t)c.iterations;
    return GR_OK;
}

// the launch: every pointer of `c` and `d_out` on the device
int32_t offset_launch(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, const OffsetCall& c,
                      double* d_out, gr_stats* d_stats, hipStream_t stream)
{
    if (c.n == 0) return GR_OK;
    int32_t rc;
    // The work block -- α, β and the row of the ray every problem is tracing -- is the context's, like its staged tables: a launch on
    // another stream waits for the one that used it last.
    if ((rc = tables_acquire(ctx, stream)) != GR_OK) return rc;
    const size_t n = (size_t)c.n;
    if ((rc = ensure((void**)&ctx->d_offset_work, &ctx->offset_work_bytes, sizeof(double) * 10 * n)) != GR_OK) return rc;
    gr_os::OffsetDev d;
    d.r_target = c.r_target; d.a = c.a; d.b = c.b; d.sign = c.sign;
    d.alpha = ctx->d_offset_work; d.beta = d.alpha + n; d.rows = d.alpha + 2 * n;
    d.out = d_out;
    d.st = c.st;
    // problems per wave: full waves.  Measured on the default line profile's 8000 solves (DESIGN_measurements.md §M38): 63 ms at 32
    // and at 16 pairs per wave, 77 at 8 (one wave on every SIMD), 104 at 4, 207 at 1; its 200 searches take the same time at every
    // value.  A wave's step costs the same for one pair as for thirty-two, and fewer waves share a CU's caches.
    d.per_wave = (int32_t)(c.per_wave > 0 ? c.per_wave : 32);

    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = c.n;
    cd.src_mode = 2;
    cd.out_mode = 5;
    std::memcpy(cd.plane.x_obs, rays->x_obs, sizeof cd.plane.x_obs);
    std::memcpy(cd.plane.Mx, rays->Mx, sizeof cd.plane.Mx);
    cd.plane.width = c.n; cd.plane.height = 1;
    cd.range = gr_range{ 0, c.n, c.n, 1 };
    cd.alpha = d.alpha; cd.beta = d.beta;
    cd.height = cfg->disc_id == GR_DISC_DATUM ? c.height : nullptr;
    cd.lp_rmin = 0.0; cd.lp_rmax = INFINITY; cd.lp_pairs = d.rows;
    cd.winding_plane = p.cfg.winding_plane;
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    if (p.cfg.metric_id == GR_METRIC_TABULATED) {      // as launch_trace: the observer must lie inside the table
        const double r_obs = rays->x_obs[1], t_min = p.cfg.metric_table[gr_tab::H_RMIN], t_max = p.cfg.metric_table[gr_tab::H_RMAX];
        if (!(r_obs >= t_min - 1e-9 * std::fabs(t_min) - 1e-12) || !(r_obs <= t_max + 1e-9 * std::fabs(t_max)))
            return fail(GR_ERR_INVALID_ARGUMENT, "GR_METRIC_TABULATED: the rays start at r = " + std::to_string(r_obs) + ", outside the radial range of the "
                                                 "metric table [" + std::to_string(t_min) + ", " + std::to_string(t_max) + "]");
    }
    if ((rc = stage_disc_table(ctx, p, stream)) != GR_OK) return rc;
    Cold* slot = ctx->d_cold + ctx->cold_next;
    ctx->cold_next = (ctx->cold_next + 1) % ctx->queue_slots;
    p.cold = slot;
    // one-wave workgroups: the plunging table is staged per workgroup while 8 copies fit a CU's LDS (launch_trace)
    p.lds_plunge_rows = (ctx->lds && cd.pf.n_plunge > 0 && cd.pf.n_plunge <= 640) ? (int32_t)cd.pf.n_plunge : 0;
    derive_params(p);      // every cull off, as for gr_ray_tangent
    p.tangent_norm = ctx->tangent_norm ? 1 : 0;
    GR_HIP(hipMemcpyAsync(slot, &cd, sizeof(Cold), hipMemcpyHostToDevice, stream));
    unsigned long long* const caller_stats = (unsigned long long*)d_stats;
    if (caller_stats) {
        p.stats = ctx->d_stat_part + (size_t)ctx->stat_next * gr_fold::kStatWords;
        ctx->stat_next = (ctx->stat_next + 1) % ctx->queue_slots;
    }
    MetricKernels mk;
    if (!metric_kernels(p.cfg.metric_id, mk)) return fail(GR_ERR_UNSUPPORTED, "unknown metric_id " + std::to_string(p.cfg.metric_id));
    GR_NEED_KERNEL(mk.offset, "offset-solve");
    const hipError_t le = mk.offset(&p, &d, c.search ? 1 : 0, stream);
    if (le != hipSuccess) return fail(GR_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(le));
    if (caller_stats) {
        hipLaunchKernelGGL(k_stats_fold, dim3(1), dim3(64), 0, stream, p.stats, caller_stats);
        GR_HIP(hipGetLastError());
    }
    if (stream == ctx->stream) GR_HIP(hipEventRecord(ctx->ev_k, stream));
    return tables_release(ctx, stream);
}

template <class Q>
int32_t offset_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, const Q* q, double* d_out,
                      gr_stats* d_stats, void* hip_stream)
{
    OffsetCall c;
    int32_t rc;
    if ((rc = offset_call(q, c)) != GR_OK) return rc;
    if ((rc = offset_check(ctx, cfg, rays, pf, c, d_out)) != GR_OK) return rc;
    GR_HIP(hipSetDevice(ctx->device));
    return offset_launch(ctx, cfg, rays, pf, c, d_out, d_stats, (hipStream_t)hip_stream);
}
}  // namespace
}  // extern "C++"

int32_t gr_offset_solve_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                               const gr_offset_problems* problems, double* d_out, gr_stats* d_stats, void* hip_stream)
{
    return offset_device(ctx, cfg, rays, pf, problems, d_out, d_stats, hip_stream);
}

int32_t gr_offset_search_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                                const gr_offset_searches* searches, double* d_out, gr_stats* d_stats, void* hip_stream)
{
    return offset_device(ctx, cfg, rays, pf, searches, d_out, d_stats, hip_stream);
}

// ---- the cells of a source's adaptive sky (AdaptiveSky, adaptive-sample.jl:43-81): gr_sky_cells ----

// what every gr_sky_cells* refuses before anything touches the device; `host_angles`: cos_theta / phi can be read here
static int32_t skycells_check(const gr_config* cfg, const gr_skycells* cells, const gr_pointfunction* pf, bool host_angles)
{
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (!cells) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: cells is null");
    if (cells->n < 0 || cells->n > (int64_t)INT32_MAX) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: n in 0 ... 2^31 - 1");
    if (cells->n > 0 && (!cells->cos_theta || !cells->phi)) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: cos_theta / phi is null");
    if (cfg->disc_id == GR_DISC_NONE) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: the Jacobian is taken where the ray meets the geometry: none given");
    if (!pf || pf->pf_id != GR_PF_REDSHIFT) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: needs the redshift point function");
    if (!pf->has_u_src) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: g is the energy ratio against the source's velocity: pf->has_u_src must be 1");
    if (cfg->metric_id == GR_METRIC_TABULATED) {
        const double r = cells->x_src[1], t_min = cfg->metric_table[gr_tab::H_RMIN], t_max = cfg->metric_table[gr_tab::H_RMAX];
        if (!(r >= t_min - 1e-9 * std::fabs(t_min) - 1e-12) || !(r <= t_max + 1e-9 * std::fabs(t_max)))
            return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: the source at r = " + std::to_string(r) + " lies outside the radial range of the metric table ["
                                                 + std::to_string(t_min) + ", " + std::to_string(t_max) + "]");
    }
    if (host_angles)
        for (int64_t j = 0; j < cells->n; ++j)
            if (!(std::fabs(cells->cos_theta[j]) < 1.0))
                return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_cells: |cos θ| must lie below 1 (cell " + std::to_string(j) + "): J divides by sin θ");
    return GR_OK;
}

int32_t gr_sky_cells_device(gr_ctx* ctx, const gr_config* cfg, const gr_skycells* cells, const gr_pointfunction* pf,
                            double* d_out, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = skycells_check(cfg, cells, pf, false)) != GR_OK) return rc;
    if (cells->n > 0 && !d_out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t n = cells->n;
    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = n;
    if ((rc = stage_pf(ctx, cfg, pf, cd.pf, stream)) != GR_OK) return rc;
    if (n == 0) return GR_OK;
    // the rays and their seeds go into the context's sky buffer (ordered against earlier launches that read it: sky_prepare)
    if ((rc = tables_acquire(ctx, stream)) != GR_OK) return rc;
    if ((rc = ensure((void**)&ctx->d_sky, &ctx->sky_bytes, sizeof(double) * (4 + (size_t)(4 + GR_SKYCELL_SEED) * (size_t)n))) != GR_OK) return rc;
    SkyCellParams sp;
    std::memcpy(sp.x_src, cells->x_src, sizeof sp.x_src);
    std::memcpy(sp.Mx, cells->Mx, sizeof sp.Mx);
    sp.cos_theta = cells->cos_theta;
    sp.phi = cells->phi;
    sp.n = n;
    hipLaunchKernelGGL(k_skycell_velocities, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sp, ctx->d_sky);
    GR_HIP(hipGetLastError());
    cd.src_mode = 1;
    cd.out_mode = 6;
    cd.x = ctx->d_sky;
    cd.x_stride = 0;
    cd.v = ctx->d_sky + 4;
    cd.v_tan = ctx->d_sky + 4 + 4 * n;
    std::memcpy(cd.plane.x_obs, cells->x_src, sizeof cd.plane.x_obs);
    cd.range = gr_range{ 0, n, n, 1 };
    cd.swizzle = 0;
    cd.lp_rmin = 0.0;
    cd.lp_rmax = INFINITY;
    cd.lp_pairs = d_out;
    p.stats = (unsigned long long*)d_stats;
    return launch_trace(ctx, p, cd, stream);
}

// ---- the cells of an observer's adaptive image plane (AdaptivePlane, adaptive-plane.jl:60-91): gr_plane_cells ----

// Cell j is the ray of impact parameters (α_j, β_j): v = Mx local_momentum(x_obs[1], -α, β) (utility.jl:13-20; the sign of α:
// adaptive-plane.jl:81) in the arithmetic of tracing.map_impact_parameters, unconstrained.  out: x_obs[4], v[n][4]
struct PlaneCellParams {
    double x_obs[4], Mx[16];
    const double* alpha;       // device, n
    const double* beta;        // device, n
    int64_t n;
};
__global__ void __launch_bounds__(256) k_plane_velocities(const PlaneCellParams p, double* out)
{
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p.n; j += (int64_t)gridDim.x * 256) {
        if (j == 0)
            for (int q = 0; q < 4; ++q) out[q] = p.x_obs[q];
        const double a = -p.alpha[j] / p.x_obs[1], b = p.beta[j] / p.x_obs[1];
        const double pr = -1.0 / sqrt(1.0 + a * a + b * b);
        const double pb[4] = { 1.0, pr, b * pr, a * pr };
        double* v = out + 4 + 4 * j;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = p.Mx[q * 4 + 0] * pb[0] + p.Mx[q * 4 + 1] * pb[1] + p.Mx[q * 4 + 2] * pb[2] + p.Mx[q * 4 + 3] * pb[3];
    }
}

// what every gr_plane_cells* and gr_sky_create_plane refuse before anything touches the device
static int32_t planecells_check(const gr_config* cfg, const gr_plane* plane)
{
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (!plane) return fail(GR_ERR_INVALID_ARGUMENT, "gr_plane_cells: plane is null");
    if (cfg->metric_id == GR_METRIC_TABULATED) {
        const double r = plane->x_obs[1], t_min = cfg->metric_table[gr_tab::H_RMIN], t_max = cfg->metric_table[gr_tab::H_RMAX];
        if (!(r >= t_min - 1e-9 * std::fabs(t_min) - 1e-12) || !(r <= t_max + 1e-9 * std::fabs(t_max)))
            return fail(GR_ERR_INVALID_ARGUMENT, "gr_plane_cells: the observer at r = " + std::to_string(r) + " lies outside the radial range of the metric table ["
                                                 + std::to_string(t_min) + ", " + std::to_string(t_max) + "]");
    }
    return GR_OK;
}
static int32_t planecells_args(const double* alpha, const double* beta, int64_t n, const gr_point* out)
{
    if (n < 0 || n > (int64_t)INT32_MAX) return fail(GR_ERR_INVALID_ARGUMENT, "gr_plane_cells: n in 0 ... 2^31 - 1");
    if (n > 0 && (!alpha || !beta || !out)) return fail(GR_ERR_INVALID_ARGUMENT, "gr_plane_cells: alpha / beta / out is null");
    return GR_OK;
}

int32_t gr_plane_cells_device(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const double* d_alpha, const double* d_beta, int64_t n,
                              gr_point* d_out, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = planecells_check(cfg, plane)) != GR_OK) return rc;
    if ((rc = planecells_args(d_alpha, d_beta, n, d_out)) != GR_OK) return rc;
    GR_HIP(hipSetDevice(ctx->device));
    if (n == 0) return GR_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    // the rays go into the context's sky buffer (ordered against earlier launches that read it: sky_prepare)
    if ((rc = tables_acquire(ctx, stream)) != GR_OK) return rc;
    if ((rc = ensure((void**)&ctx->d_sky, &ctx->sky_bytes, sizeof(double) * (4 + 4 * (size_t)n))) != GR_OK) return rc;
    PlaneCellParams pp;
    std::memcpy(pp.x_obs, plane->x_obs, sizeof pp.x_obs);
    std::memcpy(pp.Mx, plane->Mx, sizeof pp.Mx);
    pp.alpha = d_alpha;
    pp.beta = d_beta;
    pp.n = n;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048));
    hipLaunchKernelGGL(k_plane_velocities, dim3(blocks), dim3(256), 0, stream, pp, ctx->d_sky);
    GR_HIP(hipGetLastError());
    if ((rc = gr_trace_endpoints_device(ctx, cfg, ctx->d_sky, 0, ctx->d_sky + 4, n, d_out, d_stats, hip_stream)) != GR_OK) return rc;
    return tables_release(ctx, stream);
}

int32_t gr_rayset_endpoints_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, gr_point* d_points,
                                   gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    if ((rc = rays_params(ctx, p, cd, cfg, rays)) != GR_OK) return rc;
    if (rays->n > 0 && !d_points) return fail(GR_ERR_INVALID_ARGUMENT, "points is null");
    cd.out_mode = 1;
    cd.points = d_points;
    p.stats = (unsigned long long*)d_stats;
    return launch_trace(ctx, p, cd, stream);
}

// ---- host-buffer variants: stage through the context, block until done ----

namespace {
// first touch of every page of a buffer from up to 8 threads (its content is about to be overwritten)
void prefault_threads(char* base, size_t bytes)
{
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4 : (nt > 8 ? 8 : nt);
    const size_t page = 4096;
    std::vector<std::thread> th;
    // thread creation can throw (std::system_error: out of threads) and nothing may unwind through the C ABI: pre-faulting
    // is an optimisation, so whatever threads exist do their stripes and the copy (or the registration) faults the rest in itself
    try {
        th.reserve(nt);
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([=]() {
                // every thread sweeps front to back (pages t, t + nt, ...): the first band's pages are ready first
                for (size_t off = (size_t)t * page; off < bytes; off += (size_t)nt * page) ((volatile char*)base)[off] = 0;
            });
    } catch (...) {
    }
    for (auto& x : th) x.join();
}
}
// Touch every page of an output buffer (from 64 MB up).  A freshly allocated destination -- numpy's `empty`, Julia's
// `Vector{GeodesicPoint}(undef, n)` -- is not backed by pages yet, and taking those faults inside the device-to-host copy
// costs as much again as the copy (637 MB of end points at 2048²: 35 ms into touched memory, 60 ms into fresh memory); taken
// here they overlap the kernel that is already running.
static void prefault_output(void* dst, size_t bytes, bool huge)
{
    if (bytes < ((size_t)64 << 20)) return;
    if (huge) {   // ask for transparent huge pages on the 2 MB-aligned interior: 300 faults instead of 155 000 for 637 MB
        // (measured on the GPU box, THP mode "madvise": 10.7 ms instead of 27-64 ms with 8 threads; errors are ignored;
        // gr_ctx_set(ctx, "hugepages", 0) leaves the caller's mapping alone)
        const size_t two = (size_t)2 << 20;
        const size_t a0 = ((size_t)dst + two - 1) / two * two, a1 = ((size_t)dst + bytes) / two * two;
        if (a1 > a0) (void)madvise((void*)a0, a1 - a0, MADV_HUGEPAGE);
    }
    prefault_threads((char*)dst, bytes);
}
struct BackgroundPrefault {
    static constexpr unsigned kMax = 8;
    std::atomic<size_t> progress[kMax];
    std::vector<std::thread> th;
    unsigned nt = 0;
    size_t bytes = 0;
    void start(void* dst, size_t n, bool huge)
    {
        bytes = n;
        if (n < ((size_t)64 << 20)) return;
        const size_t two = (size_t)2 << 20;
        const size_t a0 = ((size_t)dst + two - 1) / two * two, a1 = ((size_t)dst + n) / two * two;
        if (huge && a1 > a0) (void)madvise((void*)a0, a1 - a0, MADV_HUGEPAGE);
        unsigned want = std::thread::hardware_concurrency();
        want = want == 0 ? 4 : (want > kMax ? kMax : want);
        char* base = (char*)dst;
        const unsigned n_threads = want;
        for (unsigned t = 0; t < kMax; ++t) progress[t].store(0, std::memory_order_relaxed);
        // no exception may cross the C ABI: if a thread cannot be created, the ones that exist sweep their stripes and
        // wait_until() waits for those only (nt counts the threads that really run)
        try {
            th.reserve(want);
            for (unsigned t = 0; t < want; ++t) {
                th.emplace_back([this, base, n, t, n_threads]() {
                    const size_t page = 4096;
                    size_t since = 0;
                    for (size_t off = (size_t)t * page; off < n; off += (size_t)n_threads * page) {
                        ((volatile char*)base)[off] = 0;
                        if (++since == 256) { progress[t].store(off, std::memory_order_release); since = 0; }
                    }
                    progress[t].store(n, std::memory_order_release);
                });
                nt = t + 1;
            }
        } catch (...) {
        }
    }
    void wait_until(size_t off) const
    {
        if (nt == 0) return;
        if (off > bytes) off = bytes;
        for (unsigned t = 0; t < nt; ++t)
            while (progress[t].load(std::memory_order_acquire) < off) std::this_thread::yield();
    }
    void finish()
    {
        for (auto& x : th) x.join();
        th.clear();
        nt = 0;
    }
    ~BackgroundPrefault() { finish(); }
};

static int32_t ensure_copy_stream(gr_ctx* ctx)
{
    if (!ctx->copy_stream) GR_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (!ctx->band_stream) GR_HIP(hipStreamCreateWithFlags(&ctx->band_stream, hipStreamNonBlocking));
    if (!ctx->ev_fork) GR_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    for (hipEvent_t& e : ctx->ev_band)
        if (!e) GR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return GR_OK;
}

// How many bands a result of n records is returned in (1: not worth it), each a multiple of `unit` records.
static int band_count(const gr_ctx* ctx, int64_t n, int64_t unit, bool pinned)
{
    if (ctx->pipeline <= 1 || unit <= 0 || n < ((int64_t)1 << 21)) return 1;
    // into page-locked memory the copies run at the link's rate and need no page faults: more, smaller bands leave a
    // shorter last copy exposed (the only one nothing overlaps)
    int nb = (int)(ctx->pipeline > 8 ? 8 : ctx->pipeline);
    if (pinned && nb < 8) nb = 8;
    while (nb > 1 && (n / nb) < unit) --nb;
    return nb;
}

static int32_t begin_host_call(gr_ctx* ctx, gr_stats* stats)
{
    GR_HIP(hipSetDevice(ctx->device));
    if (stats) GR_HIP(hipMemsetAsync(ctx->d_stats, 0, sizeof(unsigned long long) * N_STAT, ctx->stream));
    GR_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    GR_HIP(hipEventRecord(ctx->ev_k, ctx->stream));      // re-recorded behind every trace kernel of the call (launch_trace)
    return GR_OK;
}

static int32_t end_host_call(gr_ctx* ctx, gr_stats* stats)
{
    GR_HIP(hipSetDevice(ctx->device));
    GR_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    unsigned long long h[N_STAT];
    if (stats) GR_HIP(hipMemcpyAsync(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    if (stats) {
        stats_to_host(h, stats);
        float ms = 0.f;
        GR_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev_k));
        stats->kernel_ms = ms;      // start of the call's device work -> end of its last trace kernel (input staging included)
        GR_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        stats->call_ms = ms;        // ... -> end of the last copy back to the caller's buffer
        stats->enqueue_ms = 0.0;    // the *_multi entry points fill it in
    }
    return GR_OK;
}

// would this render of a plane run on the one-ray-per-lane kernel (whose waves store whole runs: 64-byte image segments of an
// 8 x 8 tile, 1216-byte runs of end-point records)?  Only those stores are worth sending across the link directly.
static bool plane_on_lane_kernel(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_range* range, int out_mode)
{
    if (validate_cfg(cfg) != GR_OK || validate_plane(plane, range) != GR_OK) return false;   // the regular path reports it
    Params p;
    Cold cd;
    plane_params(ctx, p, cd, cfg, plane, range);
    cd.out_mode = out_mode;
    return resolve_kernel(ctx, range->count, cd, cfg->metric_id) == 0;
}

// ---------------------------------------------------------------------------------------
// ONE host thread, SEVERAL devices (include/gradus_mi355x.h, "*_multi"): enqueue on every context, queue the copies home,
// wait for all.
// ---------------------------------------------------------------------------------------
extern "C++" {
namespace {
double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

int32_t validate_ctxs(gr_ctx* const* ctxs, int32_t n)
{
    if (!ctxs || n < 1) return fail(GR_ERR_INVALID_ARGUMENT, "no contexts");
    for (int k = 0; k < n; ++k) {
        if (!ctxs[k]) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
        for (int q = 0; q < k; ++q)
            if (ctxs[q] == ctxs[k]) return fail(GR_ERR_INVALID_ARGUMENT, "the same context twice: every share needs its own stream and staging buffers");
    }
    return GR_OK;
}

// Wait for everything a host call may have queued on a context -- its stream and, once a banded return has made them, the two
// streams beside it: nothing may be in flight, reading or writing the caller's buffers, when a failed call returns.  Errors are
// ignored and the message of the failure that brought us here is left alone (nothing below sets one).
void drain(gr_ctx* ctx)
{
    (void)hipSetDevice(ctx->device);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->band_stream) (void)hipStreamSynchronize(ctx->band_stream);
    (void)hipStreamSynchronize(ctx->stream);
}

// The one path of a host call that has a *_multi form: the one-context entry point is the same implementation on `&ctx, 1`.
// enq(k): stage and launch context k's share (begins with begin_host_call, before it stages: kernel_ms / call_ms count the
// staging); copy(k): queue its copy home -- no enq queues a copy to the host, so every share is queued before any is waited for.
// Whatever was started is waited for before the call returns, also on an error: the buffers belong to the caller.
template <class Enqueue, class CopyBack>
int32_t multi_drive(gr_ctx* const* ctxs, int32_t n, gr_stats* stats, Enqueue enq, CopyBack copy)
{
    double t_enq[64];
    int32_t rc = GR_OK;
    int started = 0;
    for (int k = 0; k < n && rc == GR_OK; ++k) {
        const double t0 = now_ms();
        rc = enq(k);
        if (k < 64) t_enq[k] = now_ms() - t0;
        started = k + 1;      // begin_host_call may have queued work even if a later step of enq failed
    }
    for (int k = 0; k < n && rc == GR_OK; ++k) rc = copy(k);
    for (int k = 0; k < started; ++k) {
        gr_stats* st = stats ? &stats[k] : nullptr;
        if (rc == GR_OK) rc = end_host_call(ctxs[k], st);
        else drain(ctxs[k]);      // an earlier failure: its message stands
        if (st && rc == GR_OK) st->enqueue_ms = k < 64 ? t_enq[k] : 0.0;
    }
    return rc;
}

// what a one-context entry point returns of its shared implementation's result: enqueue_ms is the *_multi forms' to report
int32_t one_context(int32_t rc, gr_stats* stats)
{
    if (rc == GR_OK && stats) stats->enqueue_ms = 0.0;
    return rc;
}

// the block-cyclic deal of an image's columns over n contexts: `block` rays per block, `n_blocks` blocks = `count` rays each
int32_t plane_deal(const gr_plane* plane, int32_t n, int64_t block_cols, int64_t* block, int64_t* n_blocks, int64_t* count)
{
    if (!plane) return fail(GR_ERR_INVALID_ARGUMENT, "plane is null");
    const int64_t W = plane->width, H = plane->height;
    if (W <= 0 || H <= 0) return fail(GR_ERR_INVALID_ARGUMENT, "image dimensions must be positive");
    int64_t bc = block_cols > 0 ? block_cols : 8;
    while (bc > 1 && W % (bc * n) != 0) bc /= 2;
    if (W % (bc * n) != 0) return fail(GR_ERR_INVALID_ARGUMENT, "image width cannot be dealt in column blocks over the contexts");
    *block = bc * H;
    *n_blocks = W / (bc * n);
    *count = *n_blocks * *block;
    return GR_OK;
}

// the device-side address of a block the library pinned, as the CURRENT device sees it (blocks are registered portable)
void* pinned_device_pointer(void* host)
{
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, host, 0) == hipSuccess && dp) return dp;
    (void)hipGetLastError();
    return nullptr;
}

// contiguous shares of n_rays rays over n contexts, in multiples of 64 rays (the last may be short or empty)
void contiguous_share(int64_t n_rays, int32_t n, int k, int64_t* off, int64_t* cnt)
{
    int64_t per = (n_rays + n - 1) / n;
    per = (per + 63) / 64 * 64;
    int64_t a = (int64_t)k * per, b = a + per;
    if (a > n_rays) a = n_rays;
    if (b > n_rays) b = n_rays;
    *off = a;
    *cnt = b - a;
}
}  // namespace
}  // extern "C++"

// ---- the image plane: gr_render, gr_render_endpoints and their *_multi forms are one implementation ----
extern "C++" {
namespace {
// banded launches do not learn / use a tile order (their ranges differ)
struct LptSuspend {
    gr_ctx* ctx;
    explicit LptSuspend(gr_ctx* c) : ctx(c) { ctx->lpt_suspend = true; }
    ~LptSuspend() { ctx->lpt_suspend = false; }
    LptSuspend(const LptSuspend&) = delete;
    LptSuspend& operator=(const LptSuspend&) = delete;
};

// ONE context returns the end points of a contiguous range of a large plane in bands of whole 8-column tile strips: band k is
// copied back on a second stream while bands k+1.. are traced (2048²: 20 ms of kernel + 15 ms of copy become 25 ms), and the
// destination's pages are faulted in by helper threads meanwhile.  It is one context's enqueue and copy strategy and is not
// offered to several: whether bands help when several devices share a link has never been measured (the test box has one).
struct Bands {
    int64_t j0[9];      // band k is rays j0[k] ... j0[k + 1] of the range
    int used = 0;       // 0: the range goes out in one launch and one copy

    // the launches, on two streams; begin_host_call has run
    int32_t enqueue(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_range* range, int nb, int64_t unit, gr_stats* d_stats)
    {
        int32_t rc;
        if ((rc = ensure_copy_stream(ctx)) != GR_OK) return rc;
        // equal bands except the last, which is half a band: its copy is the only one nothing overlaps
        const int64_t per = ((2 * range->count / (2 * nb - 1) + unit - 1) / unit) * unit;
        for (int64_t j = 0; j < range->count && used < 8; j += per) j0[used++] = j;
        j0[used] = range->count;
        {
            LptSuspend no_tile_order(ctx);
            // Bands alternate between two streams: a launch ends when its slowest wave does, and on ONE stream the next band would
            // only start then (four bands: 22.5 ms of kernels against 19.6 ms for the plane in one launch).  Side by side the next
            // band's waves fill the SIMDs the draining one leaves idle.  The second stream starts behind the call's begin marker
            // (the statistics counters are zeroed on the first).
            GR_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
            GR_HIP(hipStreamWaitEvent(ctx->band_stream, ctx->ev_fork, 0));
            for (int k = 0; k < used; ++k) {
                hipStream_t s = (k & 1) ? ctx->band_stream : ctx->stream;
                const gr_range band{ range->first + j0[k], j0[k + 1] - j0[k], j0[k + 1] - j0[k], 1 };
                if ((rc = gr_render_endpoints_device(ctx, cfg, plane, &band, (gr_point*)ctx->d_scratch + j0[k], d_stats, s)) != GR_OK) return rc;
                GR_HIP(hipEventRecord(ctx->ev_band[k], s));
            }
        }
        // join: everything the second stream did is ordered before the call's end marker on the first
        if (used > 1) GR_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_band[(used - 1) & 1 ? used - 1 : used - 2], 0));
        GR_HIP(hipEventRecord(ctx->ev_k, ctx->stream));
        return GR_OK;
    }

    // the copies, each behind its band, on a third stream; all of them have landed when this returns
    int32_t copy(gr_ctx* ctx, gr_point* points, bool pinned) const
    {
        BackgroundPrefault pf;
        if (!pinned) pf.start(points, sizeof(gr_point) * (size_t)j0[used], ctx->hugepages != 0);
        for (int k = 0; k < used; ++k) {
            pf.wait_until(sizeof(gr_point) * (size_t)j0[k + 1]);
            GR_HIP(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_band[k], 0));
            GR_HIP(hipMemcpyAsync(points + j0[k], (gr_point*)ctx->d_scratch + j0[k], sizeof(gr_point) * (size_t)(j0[k + 1] - j0[k]),
                                  hipMemcpyDeviceToHost, ctx->copy_stream));
        }
        GR_HIP(hipStreamSynchronize(ctx->copy_stream));
        return GR_OK;
    }
};

// One row per ray of an image plane -- a pixel (out_mode 0, 8 bytes) or an end-point record (out_mode 1, 152 bytes) -- for one
// context or several.  Context k traces `first` moved on by k * step rays.
//   dealt = false (the one-context calls): `out` holds the rows of the range alone, in the range's order, and they go home with
//           one contiguous copy -- or, end points of a large contiguous range, in Bands;
//   dealt = true (the *_multi calls): `out` is the whole plane, context k's blocks go to their places in it with one 2-D copy.
// Into a block the library pinned (gr_host_alloc) the kernels store the rows themselves: no staging copy in HBM, no copy engine,
// nothing for the host to wait on but the kernels.  The wave-transposed stores of records (points_epilogue, hence lds_points)
// cross the link as full-size packets -- 637 MB spread over the 20 ms of the 2048² trace is about half the link's rate.  A dealt
// kernel then addresses the plane globally (out_global).
int32_t plane_rows(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf,
                   const gr_range& first, int64_t step, bool dealt, int out_mode, void* out, gr_stats* stats)
{
    const bool records = out_mode == 1;
    const size_t row = records ? sizeof(gr_point) : sizeof(double);
    const int64_t count = first.count > 0 ? first.count : 0;
    const size_t bytes = row * (size_t)count;                                                 // of one context's rows
    const size_t extent = dealt ? row * (size_t)(plane->width * plane->height) : bytes;       // of the caller's buffer
    auto range_of = [&](int k) {
        gr_range rg = first;
        rg.first += (int64_t)k * step;
        return rg;
    };
    const bool pinned = is_pinned(out, extent);
    // the direct route is all contexts' or none's: only waves of the lane kernel store whole runs (plane_on_lane_kernel)
    bool direct = pinned && extent;
    for (int k = 0; k < n && direct; ++k) {
        const gr_range rg = range_of(k);
        direct = ctxs[k]->direct_host && (!records || ctxs[k]->lds_points) && plane_on_lane_kernel(ctxs[k], cfg, plane, &rg, out_mode);
    }
    int nb = 1;
    const int64_t unit = plane ? 8 * plane->height : 0;
    if (n == 1 && !dealt && records && unit > 0 && first.first % unit == 0 && (first.stride_blocks == 1 || first.count <= first.block))
        nb = band_count(ctxs[0], first.count, unit, pinned);
    Bands bands;
    bool global[64] = {};      // context k's kernel stores into the caller's block itself: nothing of its to copy
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int32_t r;
        GR_HIP(hipSetDevice(c->device));      // before any allocation: ensure() mallocs on the current device
        void* dst = direct ? pinned_device_pointer(out) : nullptr;
        global[k] = dst != nullptr;
        if (!dst) {      // only the staged routes need the copy of the rows in HBM (637 MB of records at 2048²)
            if ((r = ensure(&c->d_scratch, &c->scratch_bytes, bytes ? bytes : 8)) != GR_OK) return r;
            dst = c->d_scratch;
        }
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        const gr_range rg = range_of(k);
        gr_stats* d_stats = stats ? (gr_stats*)c->d_stats : nullptr;
        if (!global[k] && nb > 1) return bands.enqueue(c, cfg, plane, &rg, nb, unit, d_stats);
        return records ? render_endpoints_device_impl(c, cfg, plane, &rg, (gr_point*)dst, d_stats, c->stream, global[k] && dealt)
                       : render_device_impl(c, cfg, plane, pf, &rg, (double*)dst, d_stats, c->stream, global[k] && dealt);
    };
    bool faulted = false;
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        if (global[k] || count == 0) return GR_OK;
        GR_HIP(hipSetDevice(c->device));
        if (bands.used) return bands.copy(c, (gr_point*)out, pinned);
        // every kernel is running by now: the pages of a fresh pageable destination are faulted in under them, once
        if (records && !faulted && !pinned) prefault_output(out, extent, c->hugepages != 0);
        faulted = true;
        if (!dealt) {
            GR_HIP(hipMemcpyAsync(out, c->d_scratch, bytes, hipMemcpyDeviceToHost, c->stream));
        } else {
            // local block b of context k is block b * n + k of the plane: one 2-D copy places all of them
            const gr_range rg = range_of(k);
            GR_HIP(hipMemcpy2DAsync((char*)out + row * (size_t)rg.first, row * (size_t)(rg.stride_blocks * rg.block), c->d_scratch,
                                    row * (size_t)rg.block, row * (size_t)rg.block, (size_t)(rg.count / rg.block),
                                    hipMemcpyDeviceToHost, c->stream));
        }
        return GR_OK;
    };
    return multi_drive(ctxs, n, stats, enq, copy);
}

// the *_multi forms: the block-cyclic deal of the plane's columns
int32_t plane_rows_dealt(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf,
                         int64_t block_cols, int out_mode, void* out, gr_stats* stats)
{
    int32_t rc;
    int64_t block, n_blocks, count;
    if ((rc = plane_deal(plane, n, block_cols, &block, &n_blocks, &count)) != GR_OK) return rc;
    return plane_rows(ctxs, n, cfg, plane, pf, gr_range{ 0, count, block, (int64_t)n }, block, true, out_mode, out, stats);
}
}  // namespace
}  // extern "C++"

int32_t gr_render(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf,
                  const gr_range* range, double* image, gr_stats* stats)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!range) return fail(GR_ERR_INVALID_ARGUMENT, "range is null");
    if (!image && range->count > 0) return fail(GR_ERR_INVALID_ARGUMENT, "image is null");
    return one_context(plane_rows(&ctx, 1, cfg, plane, pf, *range, 0, false, 0, image, stats), stats);
}

int32_t gr_render_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_plane* plane,
                        const gr_pointfunction* pf, int64_t block_cols, double* image, gr_stats* stats)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    if (!image) return fail(GR_ERR_INVALID_ARGUMENT, "image is null");
    return plane_rows_dealt(ctxs, n, cfg, plane, pf, block_cols, 0, image, stats);
}

int32_t gr_render_endpoints(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const gr_range* range,
                            gr_point* points, gr_stats* stats)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!range) return fail(GR_ERR_INVALID_ARGUMENT, "range is null");
    if (!points && range->count > 0) return fail(GR_ERR_INVALID_ARGUMENT, "points is null");
    return one_context(plane_rows(&ctx, 1, cfg, plane, nullptr, *range, 0, false, 1, points, stats), stats);
}

int32_t gr_render_endpoints_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_plane* plane,
                                  int64_t block_cols, gr_point* points, gr_stats* stats)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    if (!points) return fail(GR_ERR_INVALID_ARGUMENT, "points is null");
    return plane_rows_dealt(ctxs, n, cfg, plane, nullptr, block_cols, 1, points, stats);
}

// n items in, n doubles out on one context: stage the items, `launch(d_in, d_out)`, copy the doubles home, wait
extern "C++" {
template <class Launch>
static int32_t items_to_doubles(gr_ctx* ctx, const void* in, size_t item_bytes, int64_t n, double* out, Launch launch)
{
    int32_t rc;
    const size_t in_bytes = item_bytes * (size_t)n, out_bytes = sizeof(double) * (size_t)n;
    GR_HIP(hipSetDevice(ctx->device));      // before any allocation: ensure() mallocs on the current device
    if ((rc = ensure(&ctx->d_in, &ctx->in_bytes, in_bytes ? in_bytes : 8)) != GR_OK) return rc;
    if ((rc = ensure(&ctx->d_scratch, &ctx->scratch_bytes, out_bytes ? out_bytes : 8)) != GR_OK) return rc;
    if (n > 0) GR_HIP(hipMemcpyAsync(ctx->d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch(ctx->d_in, (double*)ctx->d_scratch)) != GR_OK) return rc;
    if (n > 0) GR_HIP(hipMemcpyAsync(out, ctx->d_scratch, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    return GR_OK;
}
}  // extern "C++"

int32_t gr_apply_pointfunction(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf, const gr_point* points,
                               int64_t n, double max_time, double* out)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (n > 0 && (!points || !out)) return fail(GR_ERR_INVALID_ARGUMENT, "points/out is null");
    return items_to_doubles(ctx, points, sizeof(gr_point), n, out, [&](const void* d_in, double* d_out) {
        return gr_apply_pointfunction_device(ctx, cfg, pf, (const gr_point*)d_in, n, max_time, d_out, ctx->stream);
    });
}

int32_t gr_disc_area_factor(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf, const double* r, int64_t n, double* out)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (n > 0 && (!r || !out)) return fail(GR_ERR_INVALID_ARGUMENT, "r/out is null");
    return items_to_doubles(ctx, r, sizeof(double), n, out, [&](const void* d_in, double* d_out) {
        return gr_disc_area_factor_device(ctx, cfg, pf, (const double*)d_in, n, d_out, ctx->stream);
    });
}

// stage a host rayset on the device: alpha | beta | area | height contiguous in ctx->d_in
static int32_t stage_rays(gr_ctx* ctx, const gr_rayset* rays, gr_rayset& dev, size_t extra_bytes, void** extra)
{
    if (!rays) return fail(GR_ERR_INVALID_ARGUMENT, "rayset is null");
    if (rays->n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (rays->sky_sampler) {
        // a source's sky: only a caller's generator has per-ray input (8 B per ray)
        const size_t n = (rays->sky_generator == 2) ? (size_t)rays->n : 0;
        if (n && !rays->sky_i) return fail(GR_ERR_INVALID_ARGUMENT, "sky source: generator 2 needs sky_i");
        // ... and a source of many positions its rows (GR_SKY_ROW doubles per ray)
        const size_t nr = rays->sky_rows ? (size_t)rays->n * GR_SKY_ROW : 0;
        int32_t rcs;
        if ((rcs = ensure(&ctx->d_in, &ctx->in_bytes, sizeof(double) * (n + nr) + extra_bytes + 64)) != GR_OK) return rcs;
        double* b = (double*)ctx->d_in;
        dev = *rays;
        dev.alpha = dev.beta = dev.area = dev.height = nullptr;
        dev.sky_i = n ? b : nullptr;
        dev.sky_rows = nr ? b + n : nullptr;
        if (n) GR_HIP(hipMemcpyAsync(b, rays->sky_i, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
        if (nr) GR_HIP(hipMemcpyAsync(b + n, rays->sky_rows, sizeof(double) * nr, hipMemcpyHostToDevice, ctx->stream));
        if (extra) *extra = (void*)(b + n + nr);
        return GR_OK;
    }
    if (rays->sep_r) {
        // separable set: three small tables instead of 24 B per ray
        if (!rays->sep_cos || !rays->sep_sin || rays->sep_nr < 1 || rays->sep_nt < 1)
            return fail(GR_ERR_INVALID_ARGUMENT, "separable ray set: tables missing or empty");
        if (rays->height) return fail(GR_ERR_INVALID_ARGUMENT, "separable ray set: per-ray heights are not supported");
        const size_t nr = (size_t)rays->sep_nr, nt = (size_t)rays->sep_nt;
        int32_t rcs;
        if ((rcs = ensure(&ctx->d_in, &ctx->in_bytes, sizeof(double) * (nr + 2 * nt) + extra_bytes + 64)) != GR_OK) return rcs;
        double* b = (double*)ctx->d_in;
        dev = *rays;
        dev.alpha = dev.beta = dev.area = dev.height = nullptr;
        dev.sep_r = b; dev.sep_cos = b + nr; dev.sep_sin = b + nr + nt;
        GR_HIP(hipMemcpyAsync(b, rays->sep_r, sizeof(double) * nr, hipMemcpyHostToDevice, ctx->stream));
        GR_HIP(hipMemcpyAsync(b + nr, rays->sep_cos, sizeof(double) * nt, hipMemcpyHostToDevice, ctx->stream));
        GR_HIP(hipMemcpyAsync(b + nr + nt, rays->sep_sin, sizeof(double) * nt, hipMemcpyHostToDevice, ctx->stream));
        if (extra) *extra = (void*)(b + nr + 2 * nt);
        return GR_OK;
    }
    if (rays->n > 0 && (!rays->alpha || !rays->beta)) return fail(GR_ERR_INVALID_ARGUMENT, "alpha/beta is null");
    const size_t n = (size_t)rays->n;
    int32_t rc;
    if ((rc = ensure(&ctx->d_in, &ctx->in_bytes, sizeof(double) * 4 * n + extra_bytes + 64)) != GR_OK) return rc;
    double* base = (double*)ctx->d_in;
    dev = *rays;
    dev.alpha = base; dev.beta = base + n; dev.area = rays->area ? base + 2 * n : nullptr;
    dev.height = rays->height ? base + 3 * n : nullptr;
    if (n) {
        GR_HIP(hipMemcpyAsync(base, rays->alpha, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
        GR_HIP(hipMemcpyAsync(base + n, rays->beta, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
        if (rays->area) GR_HIP(hipMemcpyAsync(base + 2 * n, rays->area, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
        if (rays->height) GR_HIP(hipMemcpyAsync(base + 3 * n, rays->height, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    }
    if (extra) *extra = (void*)(base + 4 * n);
    return GR_OK;
}

// ---- corona -> disc: the reductions of emissivity_profile (src/corona/radial.jl:38-100) on the summaries gr_corona_trace keeps ----
extern "C++" {
namespace {
// Over the rays that hit (finite g): min and max of ρ, max |g| and max |t| -- as ordered bit patterns (non-negative doubles: the
// order of the bits is the order of the values) -- and their number.  red[0] = min ρ, [1] = max ρ, [2] = count, [3] = max |g|,
// [4] = max |t|.
__global__ void __launch_bounds__(256) k_corona_minmax(const double* __restrict__ rows, int64_t n, unsigned long long* red)
{
    unsigned long long lo = ~0ull, hi = 0ull, cnt = 0ull, gm = 0ull, tm = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double g = rows[4 * i], rho = rows[4 * i + 1], t = rows[4 * i + 2];
        if (g == g) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(rho);
            const unsigned long long bg = (unsigned long long)__double_as_longlong(fabs(g));
            const unsigned long long bt = (unsigned long long)__double_as_longlong(fabs(t));
            lo = b < lo ? b : lo;
            hi = b > hi ? b : hi;
            gm = bg > gm ? bg : gm;
            tm = bt > tm ? bt : tm;
            ++cnt;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64), c2 = __shfl_down(cnt, off, 64);
        const unsigned long long g2 = __shfl_down(gm, off, 64), t2 = __shfl_down(tm, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        gm = g2 > gm ? g2 : gm;
        tm = t2 > tm ? t2 : tm;
        cnt += c2;
    }
    // one set of atomics per workgroup (per wave, 8192 waves on five addresses, the atomics WERE the kernel: 0.48 ms of a 9 ms call)
    __shared__ unsigned long long part[4][5];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[w][0] = lo; part[w][1] = hi; part[w][2] = cnt; part[w][3] = gm; part[w][4] = tm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            lo = part[k][0] < lo ? part[k][0] : lo;
            hi = part[k][1] > hi ? part[k][1] : hi;
            cnt += part[k][2];
            gm = part[k][3] > gm ? part[k][3] : gm;
            tm = part[k][4] > tm ? part[k][4] : tm;
        }
        if (cnt) {
            atomicMin(red, lo);
            atomicMax(red + 1, hi);
            atomicAdd(red + 2, cnt);
            atomicMax(red + 3, gm);
            atomicMax(red + 4, tm);
        }
    }
}

// The fixed-point grid of the sums (CoronaScale, corona_split, CoronaGrid, corona_grid) lives in gr_lagbin.hpp, which the lag-energy
// bins below share with their host harness: integer sums do not depend on the order of the additions.
using gr_lag::CoronaGrid;
using gr_lag::CoronaScale;
using gr_lag::corona_grid;
using gr_lag::corona_split;

// bucket(Simple(), ρ, ...) per hit: the last edge <= ρ, clamped to the first / last bin (the rule the reference's golden emissivity
// vector pins, test/unit/emissivity.jl:27-48); per bin the count and the fixed-point sums of g and t.  acc: 5 x nb integers
// (count, g hi, g lo, t hi, t lo).  LDS = 1: the histograms are private to the workgroup in LDS and leave as one global atomic
// per non-empty entry; LDS = 0 (more bins than 40 KB of LDS hold): global atomics.
template <int LDS>
__global__ void __launch_bounds__(256) k_corona_bin(const double* __restrict__ rows, int64_t n, const double* __restrict__ edges, int nb,
                                                    CoronaScale sg, CoronaScale st, unsigned long long* acc)
{
    extern __shared__ unsigned long long hist[];
    unsigned long long* h = LDS ? hist : acc;
    if (LDS) {
        for (int i = threadIdx.x; i < 5 * nb; i += blockDim.x) hist[i] = 0ull;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double g = rows[4 * i], rho = rows[4 * i + 1], t = rows[4 * i + 2];
        if (g == g) {
            int lo = 0, hi = nb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (edges[mid] <= rho) lo = mid + 1; else hi = mid;
            }
            lo = lo > 0 ? lo - 1 : 0;
            long long gh, gl, th, tl;
            corona_split(g, sg, gh, gl);
            corona_split(t, st, th, tl);
            atomicAdd(h + lo, 1ull);
            atomicAdd(h + nb + lo, (unsigned long long)gh);
            atomicAdd(h + 2 * nb + lo, (unsigned long long)gl);
            atomicAdd(h + 3 * nb + lo, (unsigned long long)th);
            atomicAdd(h + 4 * nb + lo, (unsigned long long)tl);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < 5 * nb; i += blockDim.x)
            if (hist[i] != 0ull) atomicAdd(acc + i, hist[i]);
    }
}

// ---- observer -> disc: the reduction and the bins of binflux (transfer-functions-2d.jl:98-121,211-241) on the rows
// gr_lagtransfer_trace keeps; the arithmetic per row is gr_lagbin.hpp ----

// Row preparation: the ray's area into the status column, so that a row is (g, ρ, t, area) and needs nothing of the staged ray
// set any more (g is already NaN unless the ray met the geometry); counts the hits.  The area is area[j], r_i² of a separable
// plane (gr_lag::sep_row) or 1.
using gr_lag::LagSep;
__global__ void __launch_bounds__(256) k_lag_prepare(double* __restrict__ rows, int64_t n, const double* __restrict__ area, LagSep sep,
                                                     unsigned long long* hits)
{
    unsigned long long cnt = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double a = 1.0;
        if (sep.r) {
            const double rr = sep.r[gr_lag::sep_row(sep, i)];
            a = rr * rr;
        } else if (area) {
            a = area[i];
        }
        const double g = rows[4 * i];
        rows[4 * i + 3] = a;
        cnt += (g == g) ? 1ull : 0ull;
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt = part[0] + part[1] + part[2] + part[3];
        if (cnt) atomicAdd(hits, cnt);
    }
}

// Over the hits: min / max of E and of t (as ordered bit patterns, gr_lag::ordered_bits), their number and max |f| (the bits of a
// non-negative double).  red[0] = min E, [1] = max E, [2] = min t, [3] = max t, [4] = count, [5] = max |f|.  Per-wave reduction,
// then one set of atomics per workgroup (k_corona_minmax).
__global__ void __launch_bounds__(256) k_lag_extrema(const double* __restrict__ rows, int64_t n, gr_lag::Profile prof, unsigned long long* red)
{
    unsigned long long v[6] = { ~0ull, 0ull, ~0ull, 0ull, 0ull, 0ull };
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        gr_lag::Hit h;
        if (gr_lag::hit_of(prof, rows + 4 * i, h)) {
            const unsigned long long be = gr_lag::ordered_bits(h.E), bt = gr_lag::ordered_bits(h.t);
            const double af = fabs(h.f);
            const unsigned long long bf = af < INFINITY ? (unsigned long long)__double_as_longlong(af) : 0ull;      // (a NaN or infinite f adds nothing)
            v[0] = be < v[0] ? be : v[0];
            v[1] = be > v[1] ? be : v[1];
            v[2] = bt < v[2] ? bt : v[2];
            v[3] = bt > v[3] ? bt : v[3];
            v[4] += 1ull;
            v[5] = bf > v[5] ? bf : v[5];
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = __shfl_down(v[k], off, 64);
        v[0] = o[0] < v[0] ? o[0] : v[0];
        v[1] = o[1] > v[1] ? o[1] : v[1];
        v[2] = o[2] < v[2] ? o[2] : v[2];
        v[3] = o[3] > v[3] ? o[3] : v[3];
        v[4] += o[4];
        v[5] = o[5] > v[5] ? o[5] : v[5];
    }
    __shared__ unsigned long long part[4][6];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) part[w][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            v[0] = part[k][0] < v[0] ? part[k][0] : v[0];
            v[1] = part[k][1] > v[1] ? part[k][1] : v[1];
            v[2] = part[k][2] < v[2] ? part[k][2] : v[2];
            v[3] = part[k][3] > v[3] ? part[k][3] : v[3];
            v[4] += part[k][4];
            v[5] = part[k][5] > v[5] ? part[k][5] : v[5];
        }
        if (v[4]) {
            atomicMin(red, v[0]);
            atomicMax(red + 1, v[1]);
            atomicMin(red + 2, v[2]);
            atomicMax(red + 3, v[3]);
            atomicAdd(red + 4, v[4]);
            atomicMax(red + 5, v[5]);
        }
    }
}

// Σ f per (E, t) cell as two integers on the fixed-point grid `sf`: acc[cell] = Σ hi, acc[cells + cell] = Σ lo with
// cell = i_E n_t + i_t.  LDS = 1: the histogram is private to the workgroup in LDS (2 x 8 x cells bytes, at most 40 KB) and leaves
// as one global atomic per non-empty entry; LDS = 0 (the default 300 x 300 matrix): global atomics.
template <int LDS>
__global__ void __launch_bounds__(256) k_lag_bin(const double* __restrict__ rows, int64_t n, gr_lag::Profile prof,
                                                 const double* __restrict__ e_edges, int n_e, const double* __restrict__ t_edges, int n_t,
                                                 CoronaScale sf, unsigned long long* acc)
{
    extern __shared__ unsigned long long lag_hist[];
    const int cells = n_e * n_t;
    unsigned long long* h = LDS ? lag_hist : acc;
    if (LDS) {
        for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x) lag_hist[i] = 0ull;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        gr_lag::Hit hit;
        if (gr_lag::hit_of(prof, rows + 4 * i, hit) && fabs(hit.f) < INFINITY) {
            const int cell = gr_lag::bucket(e_edges, n_e, hit.E) * n_t + gr_lag::bucket(t_edges, n_t, hit.t);
            long long fh, fl;
            corona_split(hit.f, sf, fh, fl);
            atomicAdd(h + cell, (unsigned long long)fh);
            atomicAdd(h + cells + cell, (unsigned long long)fl);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x)
            if (lag_hist[i] != 0ull) atomicAdd(acc + i, lag_hist[i]);
    }
}

// ---- transfer functions into flux per bin: integrate_lineprofile / integrate_lagtransfer (integration.jl:336-453); the
// arithmetic per (annulus, g bin) is gr_tfint.hpp ----
// Workgroup b serves set b / n_chunks and the annuli [c chunk, (c + 1) chunk) of it, c = b % n_chunks: a wave takes one annulus
// at a time (its radial blend and weight are wave-uniform), its lanes the g bins.  PASS 0: the largest |deposit| of every set
// (red[set], the bits of a non-negative double).  PASS 1: every deposit as two integers on the set's fixed-point grid sc[set],
// acc[set][cell] = Σ hi, acc[set][cells + cell] = Σ lo with cell = j (line profile) or j n_t + i_t (LAG) -- integer sums do
// not depend on the order of the additions, so the launch shape does not show in the result.  LDS = 1: the set's histogram is
// private to the workgroup in LDS (2 x 8 x cells bytes, at most 40 KB) and leaves as one global atomic per non-empty entry.
template <int LAG, int PASS, int LDS>
__global__ void __launch_bounds__(256) k_tf(const gr_tf::Set* __restrict__ sets, gr_tf::Quad quad, const double* __restrict__ g_edges, int n_g,
                                            const double* __restrict__ t_edges, int n_t, int chunk, int n_chunks,
                                            unsigned long long* red, const CoronaScale* __restrict__ sc, unsigned long long* acc)
{
    extern __shared__ unsigned long long tf_hist[];
    const int set = (int)(blockIdx.x / (unsigned)n_chunks), c = (int)(blockIdx.x % (unsigned)n_chunks);
    const gr_tf::Set s = sets[set];
    const int cells = LAG ? n_g * n_t : n_g;
    unsigned long long* h = nullptr;
    CoronaScale scale{};
    if (PASS == 1) {
        acc += (size_t)set * 2 * (size_t)cells;
        h = LDS ? tf_hist : acc;
        scale = sc[set];
        if (LDS) {
            for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x) tf_hist[i] = 0ull;
            __syncthreads();
        }
    }
    const int64_t a0 = (int64_t)c * chunk, a1 = a0 + chunk < s.n_int ? a0 + chunk : s.n_int;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long vmax = 0ull;
    for (int64_t ia = a0 + wave; ia < a1; ia += 4) {
        const gr_tf::Annulus an = gr_tf::annulus_of(s, ia);
        for (int j = lane; j < n_g - 1; j += 64) {
            double v[2];
            int cell[2] = { -1, -1 };
            if (LAG) {
                int it[2];
                if (gr_tf::lag_deposits(s, an, quad, g_edges, j, t_edges, n_t, v, it)) {
                    if (it[0] < n_t) cell[0] = j * n_t + it[0];
                    if (it[1] < n_t) cell[1] = j * n_t + it[1];
                }
            } else if (gr_tf::line_deposit(s, an, quad, g_edges, j, v[0])) {
                cell[0] = j;
            }
#pragma unroll
            for (int k = 0; k < (LAG ? 2 : 1); ++k) {
                if (cell[k] < 0) continue;
                if (PASS == 0) {
                    const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(v[k]));
                    vmax = b > vmax ? b : vmax;
                } else {
                    long long fh, fl;
                    corona_split(v[k], scale, fh, fl);
                    atomicAdd(h + cell[k], (unsigned long long)fh);
                    atomicAdd(h + cells + cell[k], (unsigned long long)fl);
                }
            }
        }
    }
    if (PASS == 0) {
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(vmax, off, 64);
            vmax = o > vmax ? o : vmax;
        }
        if (lane == 0 && vmax) atomicMax(red + set, vmax);
    } else if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x)
            if (tf_hist[i] != 0ull) atomicAdd(acc + i, tf_hist[i]);
    }
}

// ---- the lag transfer function of a time-dependent emissivity (RingCoronaProfile / DiscCoronaProfile; ring.jl:857-950); the
// arithmetic is gr_tftd.hpp ----
// k_tftd_em: workgroup ia forms what annulus ia needs of the profile, em[ia] = (t_lo, t_hi, ε(time_k) for k < n_time).
// Pass A: a wave per arm, lanes over its slices: the extrema of the slices' t at ρ by shuffles, folded into the wave's limits
// and then across the four waves.  Pass B, arm by arm in ring order: the slices' (t, ε) into LDS, each slice's rank by counting
// (a stable sort, NaN last), the sorted knots into LDS, and thread k adds the arm at time_k - dt to the samples it owns:
// (left + right) w_i, ring by ring, the order of the host route.  Every em[ia][k] has one writer and one order of additions.
__global__ void __launch_bounds__(256) k_tftd_em(const gr_tf::Set* __restrict__ set, const gr_tftd::Profile* __restrict__ profile, int n_time,
                                                 double* __restrict__ em)
{
    GR_LAG_NO_CONTRACT
    __shared__ double raw_t[gr_tftd::kMaxCurves], raw_e[gr_tftd::kMaxCurves], knot_t[gr_tftd::kMaxCurves], knot_e[gr_tftd::kMaxCurves];
    __shared__ double wave_lo[4], wave_hi[4];
    __shared__ int wave_any[4];
    const gr_tftd::Profile p = *profile;
    const int64_t ia = blockIdx.x;
    const double rho = set->r_int[ia];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n_arms = 2 * (int)p.n_rings;
    // pass A
    double w_lo = 0.0, w_hi = 0.0;
    bool w_any = false;
    for (int arm = wave; arm < n_arms; arm += 4) {
        const int64_t c0 = p.arm_off[arm], nc = p.arm_off[arm + 1] - c0;
        double lo = INFINITY, hi = -INFINITY;
        int count = 0;
        for (int64_t j = lane; j < nc; j += 64) {
            double t, e;
            gr_tftd::slice_at(p, c0 + j, rho, t, e);
            if (t == t) {
                lo = fmin(lo, t);
                hi = fmax(hi, t);
                ++count;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, off, 64));
            hi = fmax(hi, __shfl_xor(hi, off, 64));
            count += __shfl_xor(count, off, 64);
        }
        gr_tftd::fold_limits(lo, hi, count, p.dt[arm >> 1], !w_any, w_lo, w_hi);
        w_any = true;
    }
    if (lane == 0) {
        wave_lo[wave] = w_lo;
        wave_hi[wave] = w_hi;
        wave_any[wave] = w_any ? 1 : 0;
    }
    __syncthreads();
    double t_lo = wave_lo[0], t_hi = wave_hi[0];             // (wave 0 always has an arm: n_arms >= 2)
    for (int k = 1; k < 4; ++k)
        if (wave_any[k]) {
            t_lo = fmin(t_lo, wave_lo[k]);
            t_hi = fmax(t_hi, wave_hi[k]);
        }
    double* row = em + (size_t)ia * (size_t)(2 + n_time);
    if (tid == 0) {
        row[0] = t_lo;
        row[1] = t_hi;
    }
    // pass B
    constexpr int kOwn = (int)(gr_tftd::kMaxTime / 256);
    double sum[kOwn], left[kOwn], time[kOwn];
#pragma unroll
    for (int s = 0; s < kOwn; ++s) {
        const int k = tid + 256 * s;
        sum[s] = left[s] = 0.0;
        time[s] = k < n_time ? gr_tftd::time_sample(t_lo, t_hi, n_time, k) : 0.0;
    }
    for (int arm = 0; arm < n_arms; ++arm) {
        const int64_t c0 = p.arm_off[arm];
        const int nc = (int)(p.arm_off[arm + 1] - c0);
        for (int j = tid; j < nc; j += 256) gr_tftd::slice_at(p, c0 + j, rho, raw_t[j], raw_e[j]);
        __syncthreads();
        for (int j = tid; j < nc; j += 256) {
            const int r = gr_tftd::rank_of(raw_t, nc, j);
            knot_t[r] = raw_t[j];
            knot_e[r] = raw_e[j];
        }
        __syncthreads();
        const double dt = p.dt[arm >> 1], w = p.w[arm >> 1];
#pragma unroll
        for (int s = 0; s < kOwn; ++s) {
            if (tid + 256 * s >= n_time) continue;
            const double v = gr_tftd::arm_at(knot_t, knot_e, nc, time[s] - dt);
            if (arm & 1) {
                const double both = left[s] + v, term = both * w;
                sum[s] += term;
            } else {
                left[s] = v;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < kOwn; ++s)
        if (tid + 256 * s < n_time) row[2 + tid + 256 * s] = sum[s];
}

// k_tftd: the launch shape of k_tf -- workgroup c serves the annuli [c chunk, (c + 1) chunk), a wave one annulus at a time, its
// lanes the (g bin, fine bin) pairs -- and each lane walks the n_time samples of em[ia].  PASS 0: the largest |deposit| (red[0]).
// PASS 1: every deposit as two integers on the grid sc[0], into the workgroup's LDS histogram (LDS = 1) or into acc.  The
// samples ascend, so consecutive deposits of a branch mostly share a t cell: the lane keeps the cell's running integer pair
// and adds it once when the cell changes -- integer sums, so the result does not see it.
template <int PASS, int LDS>
__global__ void __launch_bounds__(256) k_tftd(const gr_tf::Set* __restrict__ set, gr_tf::Quad quad, const double* __restrict__ g_edges, int n_g,
                                              const double* __restrict__ t_edges, int n_t, int upscale, int n_time, double t0,
                                              const double* __restrict__ em, int chunk, unsigned long long* red,
                                              const CoronaScale* __restrict__ sc, unsigned long long* acc)
{
    GR_LAG_NO_CONTRACT
    extern __shared__ unsigned long long tftd_hist[];
    const gr_tf::Set s = *set;
    const int cells = n_g * n_t;
    unsigned long long* h = nullptr;
    CoronaScale scale{};
    if (PASS == 1) {
        h = LDS ? tftd_hist : acc;
        scale = sc[0];
        if (LDS) {
            for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x) tftd_hist[i] = 0ull;
            __syncthreads();
        }
    }
    const int64_t a0 = (int64_t)blockIdx.x * chunk, a1 = a0 + chunk < s.n_int ? a0 + chunk : s.n_int;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_fine = (n_g - 1) * upscale;
    unsigned long long vmax = 0ull;
    for (int64_t ia = a0 + wave; ia < a1; ia += 4) {
        const gr_tf::Annulus an = gr_tf::annulus_of(s, ia);
        const double* row = em + (size_t)ia * (size_t)(2 + n_time);
        const double t_lo = row[0], t_hi = row[1];
        const double dt_step = (t_hi - t_lo) / (double)n_time;
        for (int idx = lane; idx < n_fine; idx += 64) {
            const int j = idx / upscale, i = idx - j * upscale;
            const double glo = gr_tf::clampd(g_edges[j] / s.g_scale, an.gmin, an.gmax), ghi = gr_tf::clampd(g_edges[j + 1] / s.g_scale, an.gmin, an.gmax);
            if (glo == ghi) continue;
            double lo, hi;
            gr_tftd::fine_bin(glo, ghi, upscale, i, lo, hi);
            const gr_tftd::FineBin fb = gr_tftd::fine_bin_of(s, an, quad, lo, hi);
            int cur[2] = { -1, -1 };
            long long run_hi[2] = { 0, 0 }, run_lo[2] = { 0, 0 };
            for (int k = 0; k < n_time; ++k) {
                const double time = gr_tftd::time_sample(t_lo, t_hi, n_time, k), e = row[2 + k];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    double v;
                    int it;
                    if (!gr_tftd::deposit(fb.k[b], fb.tb[b], time, e, dt_step, t0, t_edges, n_t, v, it)) continue;
                    if (PASS == 0) {
                        const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(v));
                        vmax = bits > vmax ? bits : vmax;
                    } else {
                        const int cell = j * n_t + it;
                        if (cell != cur[b]) {
                            if (cur[b] >= 0) {
                                atomicAdd(h + cur[b], (unsigned long long)run_hi[b]);
                                atomicAdd(h + cells + cur[b], (unsigned long long)run_lo[b]);
                            }
                            cur[b] = cell;
                            run_hi[b] = run_lo[b] = 0;
                        }
                        long long fh, fl;
                        corona_split(v, scale, fh, fl);
                        run_hi[b] += fh;
                        run_lo[b] += fl;
                    }
                }
            }
            if (PASS == 1) {
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    if (cur[b] >= 0) {
                        atomicAdd(h + cur[b], (unsigned long long)run_hi[b]);
                        atomicAdd(h + cells + cur[b], (unsigned long long)run_lo[b]);
                    }
            }
        }
    }
    if (PASS == 0) {
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(vmax, off, 64);
            vmax = o > vmax ? o : vmax;
        }
        if (lane == 0 && vmax) atomicMax(red, vmax);
    } else if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x)
            if (tftd_hist[i] != 0ull) atomicAdd(acc + i, tftd_hist[i]);
    }
}

int32_t rayset_share(const gr_rayset* rays, int32_t n, int k, gr_rayset& out, int64_t* off_out);      // (below, with the other *_multi helpers)
}  // namespace
}  // extern "C++"

// gr_corona_trace[_multi]: every context stages its share of the samples, traces it into its d_corona and reduces it there
// (k_corona_minmax: min ρ, max ρ, hits, max |g|, max |t|); the 40 bytes of each come home in the driver's second phase and the
// host folds them.  Whatever fails, no context of the call keeps rows to bin (corona_n = -1).
static int32_t corona_trace_on(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                               double* rho_min_max, int64_t* n_hits, gr_stats* stats, const char* who)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    for (int k = 0; k < n; ++k) ctxs[k]->corona_n = -1;
    if (!rays || !rays->sky_sampler) return fail(GR_ERR_INVALID_ARGUMENT, std::string(who) + " traces a sky source (gr_rayset.sky_sampler != 0)");
    if (!rho_min_max || !n_hits) return fail(GR_ERR_INVALID_ARGUMENT, "rho_min_max / n_hits is null");
    if (cfg && cfg->disc_id == GR_DISC_NONE) return fail(GR_ERR_INVALID_ARGUMENT, "a corona illuminates accretion geometry: none given");
    if ((rc = sky_rows_in_table(cfg, rays)) != GR_OK) return rc;
    std::vector<unsigned long long> h(5 * (size_t)n);
    std::vector<gr_rayset> share((size_t)n);
    for (int k = 0; k < n; ++k) {
        int64_t off;
        if ((rc = rayset_share(rays, n, k, share[(size_t)k], &off)) != GR_OK) return rc;
    }
    auto red_of = [&](int k) { return (unsigned long long*)(ctxs[k]->d_corona + 4 * (size_t)share[(size_t)k].n); };
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        const gr_rayset& sh = share[(size_t)k];
        int32_t r;
        GR_HIP(hipSetDevice(c->device));
        gr_rayset dev;
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        if ((r = stage_rays(c, &sh, dev, 0, nullptr)) != GR_OK) return r;
        if ((r = ensure((void**)&c->d_corona, &c->corona_bytes, sizeof(double) * 4 * (size_t)sh.n + 64)) != GR_OK) return r;
        static const unsigned long long init[5] = { ~0ull, 0ull, 0ull, 0ull, 0ull };
        GR_HIP(hipMemcpyAsync(red_of(k), init, sizeof init, hipMemcpyHostToDevice, c->stream));
        c->sky_any_order = true;      // (the rows are reduced and binned: their order is the library's to choose)
        r = gr_ray_summary_device(c, cfg, &dev, pf, c->d_corona, stats ? (gr_stats*)c->d_stats : nullptr, c->stream);
        c->sky_any_order = false;
        if (r != GR_OK) return r;
        if (sh.n > 0) {
            int64_t blocks = (sh.n + 255) / 256;
            blocks = blocks > 512 ? 512 : blocks;
            hipLaunchKernelGGL(k_corona_minmax, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->d_corona, sh.n, red_of(k));
            GR_HIP(hipGetLastError());
        }
        return GR_OK;
    };
    auto copy = [&](int k) -> int32_t {
        GR_HIP(hipSetDevice(ctxs[k]->device));
        GR_HIP(hipMemcpyAsync(h.data() + 5 * (size_t)k, red_of(k), sizeof(unsigned long long) * 5, hipMemcpyDeviceToHost, ctxs[k]->stream));
        return GR_OK;
    };
    if ((rc = multi_drive(ctxs, n, stats, enq, copy)) != GR_OK) return rc;
    double lo = INFINITY, hi = -INFINITY, gmax = 0.0, tmax = 0.0;
    int64_t hits = 0;
    for (int k = 0; k < n; ++k) {
        double v[5];
        std::memcpy(v, h.data() + 5 * (size_t)k, sizeof v);
        const int64_t hk = (int64_t)h[5 * (size_t)k + 2];
        if (hk) { lo = std::fmin(lo, v[0]); hi = std::fmax(hi, v[1]); }
        gmax = std::fmax(gmax, v[3]);
        tmax = std::fmax(tmax, v[4]);
        hits += hk;
    }
    // the fixed-point grid of the bins is formed from these: every context gets the values of ALL shares
    for (int k = 0; k < n; ++k) {
        ctxs[k]->corona_gmax = gmax;
        ctxs[k]->corona_tmax = tmax;
        ctxs[k]->corona_hits = hits;
        ctxs[k]->corona_n = share[(size_t)k].n;
    }
    *n_hits = hits;
    rho_min_max[0] = hits ? lo : NAN;
    rho_min_max[1] = hits ? hi : NAN;
    return GR_OK;
}

int32_t gr_corona_trace(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                        double* rho_min_max, int64_t* n_hits, gr_stats* stats)
{
    return one_context(corona_trace_on(&ctx, 1, cfg, rays, pf, rho_min_max, n_hits, stats, "gr_corona_trace"), stats);
}

int32_t gr_corona_trace_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              double* rho_min_max, int64_t* n_hits, gr_stats* stats)
{
    return corona_trace_on(ctxs, n, cfg, rays, pf, rho_min_max, n_hits, stats, "gr_corona_trace_multi");
}

// gr_corona_bin[_multi]: every context bins its rows into integer accumulators (count, Σg hi / lo, Σt hi / lo) on the grid of the
// trace's corona_gmax / corona_tmax / corona_hits; the 5 nb accumulators of each come home in the driver's second phase.
static int32_t corona_bin_on(gr_ctx* const* ctxs, int32_t n, const double* edges, int64_t n_edges, double* out, bool multi)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    const gr_ctx* c0 = ctxs[0];
    for (int k = 0; k < n; ++k) {
        if (ctxs[k]->corona_n < 0)
            return fail(GR_ERR_INVALID_ARGUMENT, multi ? "gr_corona_bin_multi bins the rays of the contexts' last gr_corona_trace_multi: there is none"
                                                       : "gr_corona_bin bins the rays of the context's last gr_corona_trace: there is none");
        if (ctxs[k]->corona_gmax != c0->corona_gmax || ctxs[k]->corona_tmax != c0->corona_tmax || ctxs[k]->corona_hits != c0->corona_hits)
            return fail(GR_ERR_INVALID_ARGUMENT, "gr_corona_bin_multi: the contexts do not hold the shares of ONE gr_corona_trace_multi");
    }
    if (!edges || !out || n_edges < 1 || n_edges > 65536) return fail(GR_ERR_INVALID_ARGUMENT, "edges / out is null or n_edges not in 1..65536");
    for (int64_t i = 1; i < n_edges; ++i)
        if (!(edges[i] >= edges[i - 1])) return fail(GR_ERR_INVALID_ARGUMENT, "bin edges must ascend");
    const size_t nb = (size_t)n_edges;
    const CoronaGrid gg = corona_grid(c0->corona_gmax, c0->corona_hits), gt = corona_grid(c0->corona_tmax, c0->corona_hits);
    std::vector<long long> acc(5 * nb * (size_t)n);
    // (no statistics and no timing here: the call begins with its staging, the driver's wait ends it)
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int32_t r;
        GR_HIP(hipSetDevice(c->device));
        if ((r = ensure(&c->d_in, &c->in_bytes, sizeof(double) * 6 * nb + 64)) != GR_OK) return r;
        double* d_edges = (double*)c->d_in;
        unsigned long long* d_acc = (unsigned long long*)(d_edges + nb);
        GR_HIP(hipMemcpyAsync(d_edges, edges, sizeof(double) * nb, hipMemcpyHostToDevice, c->stream));
        GR_HIP(hipMemsetAsync(d_acc, 0, sizeof(unsigned long long) * 5 * nb, c->stream));
        if (c->corona_n > 0) {
            int64_t blocks = (c->corona_n + 255) / 256;
            blocks = blocks > 1024 ? 1024 : blocks;
            if (nb <= 1024) {
                hipLaunchKernelGGL(k_corona_bin<1>, dim3((unsigned)blocks), dim3(256), sizeof(unsigned long long) * 5 * nb, c->stream,
                                   c->d_corona, c->corona_n, d_edges, (int)nb, gg.sc, gt.sc, d_acc);
            } else {
                hipLaunchKernelGGL(k_corona_bin<0>, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->d_corona, c->corona_n,
                                   d_edges, (int)nb, gg.sc, gt.sc, d_acc);
            }
            GR_HIP(hipGetLastError());
        }
        return GR_OK;
    };
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        GR_HIP(hipSetDevice(c->device));
        GR_HIP(hipMemcpyAsync(acc.data() + 5 * nb * (size_t)k, (const double*)c->d_in + nb, sizeof(long long) * 5 * nb, hipMemcpyDeviceToHost, c->stream));
        return GR_OK;
    };
    if ((rc = multi_drive(ctxs, n, nullptr, enq, copy)) != GR_OK) return rc;
    // integer addition is associative: the sums of the shares are the sums one context would have formed of all rays
    for (int k = 1; k < n; ++k)
        for (size_t i = 0; i < 5 * nb; ++i) acc[i] += acc[5 * nb * (size_t)k + i];
    for (size_t i = 0; i < nb; ++i) {
        out[i] = (double)acc[i];
        out[nb + i] = (double)(((long double)acc[nb + i] + (long double)acc[2 * nb + i] * (long double)gg.lo_unit) * (long double)gg.step);
        out[2 * nb + i] = (double)(((long double)acc[3 * nb + i] + (long double)acc[4 * nb + i] * (long double)gt.lo_unit) * (long double)gt.step);
    }
    return GR_OK;
}

int32_t gr_corona_bin(gr_ctx* ctx, const double* edges, int64_t n_edges, double* out)
{
    return corona_bin_on(&ctx, 1, edges, n_edges, out, false);
}

int32_t gr_corona_bin_multi(gr_ctx* const* ctxs, int32_t n, const double* edges, int64_t n_edges, double* out)
{
    return corona_bin_on(ctxs, n, edges, n_edges, out, true);
}

// ---- observer -> disc on the device: lagtransfer's second half and binflux (transfer-functions-2d.jl:141-242) ----
// the checks of gr_lagtransfer_extrema / _bin that need no device come first, so that a bad argument is reported as such
static int32_t lag_profile_args(const gr_lagprofile* p)
{
    if (!p) return fail(GR_ERR_INVALID_ARGUMENT, "profile is null");
    if (p->time_n < 2 || !p->time_r || !p->time_v)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_lagprofile: the coordtime table needs time_n >= 2 radii and times");
    if (p->eps_n != 0 && (p->eps_n < 2 || !p->eps_r || !p->eps_v))
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_lagprofile: a tabulated emissivity needs eps_n >= 2 radii and values");
    for (int64_t i = 1; i < p->time_n; ++i)
        if (!(p->time_r[i] >= p->time_r[i - 1])) return fail(GR_ERR_INVALID_ARGUMENT, "gr_lagprofile: the radii of the coordtime table must ascend");
    for (int64_t i = 1; i < p->eps_n; ++i)
        if (!(p->eps_r[i] >= p->eps_r[i - 1])) return fail(GR_ERR_INVALID_ARGUMENT, "gr_lagprofile: the radii of the emissivity table must ascend");
    return GR_OK;
}
static int32_t lag_edge_args(const double* edges, int64_t n, const char* axis)
{
    if (!edges) return fail(GR_ERR_INVALID_ARGUMENT, std::string(axis) + " edges are null");
    if (n < 2) return fail(GR_ERR_INVALID_ARGUMENT, std::string(axis) + " axis: at least two edges");
    if (n > ((int64_t)1 << 22)) return fail(GR_ERR_INVALID_ARGUMENT, "at most 2^22 cells (n_E * n_t)");
    for (int64_t i = 1; i < n; ++i)
        if (!(edges[i] >= edges[i - 1])) return fail(GR_ERR_INVALID_ARGUMENT, std::string(axis) + " edges must ascend");
    return GR_OK;
}
static int32_t lag_have_trace(const gr_ctx* ctx, const char* who)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (ctx->lag_n < 0)
        return fail(GR_ERR_INVALID_ARGUMENT, std::string(who) + " bins the rays of the context's last gr_lagtransfer_trace: there is none");
    return GR_OK;
}

// the profile's tables into ctx->d_in, followed by `extra` doubles for the caller (edges, accumulators, reductions)
static int32_t lag_stage(gr_ctx* ctx, const gr_lagprofile* p, size_t extra, gr_lag::Profile& dev, double** d_extra)
{
    int32_t rc;
    const size_t nt = (size_t)p->time_n, ne = p->eps_n >= 2 ? (size_t)p->eps_n : 0;
    if ((rc = ensure(&ctx->d_in, &ctx->in_bytes, sizeof(double) * (2 * nt + 2 * ne + extra) + 64)) != GR_OK) return rc;
    double* b = (double*)ctx->d_in;
    GR_HIP(hipMemcpyAsync(b, p->time_r, sizeof(double) * nt, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(b + nt, p->time_v, sizeof(double) * nt, hipMemcpyHostToDevice, ctx->stream));
    if (ne) {
        GR_HIP(hipMemcpyAsync(b + 2 * nt, p->eps_r, sizeof(double) * ne, hipMemcpyHostToDevice, ctx->stream));
        GR_HIP(hipMemcpyAsync(b + 2 * nt + ne, p->eps_v, sizeof(double) * ne, hipMemcpyHostToDevice, ctx->stream));
    }
    dev.E0 = p->E0;
    dev.q = p->emissivity_index;
    dev.time_r = b; dev.time_v = b + nt; dev.time_n = p->time_n;
    dev.eps_r = ne ? b + 2 * nt : nullptr; dev.eps_v = ne ? b + 2 * nt + ne : nullptr; dev.eps_n = (int64_t)ne;
    *d_extra = b + 2 * nt + 2 * ne;
    return GR_OK;
}

// k_lag_extrema over the context's rows; waits for it: v = (E_min, E_max, t_min, t_max, max |f|)
static int32_t lag_extrema(gr_ctx* ctx, const gr_lag::Profile& dev, unsigned long long* d_red /* 6 */, double v[5])
{
    static const unsigned long long init[6] = { ~0ull, 0ull, ~0ull, 0ull, 0ull, 0ull };
    unsigned long long h[6];
    GR_HIP(hipMemcpyAsync(d_red, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    int64_t blocks = (ctx->lag_n + 255) / 256;
    blocks = blocks > 512 ? 512 : blocks;
    hipLaunchKernelGGL(k_lag_extrema, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, ctx->d_lag, ctx->lag_n, dev, d_red);
    GR_HIP(hipGetLastError());
    GR_HIP(hipMemcpyAsync(h, d_red, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; ++k) v[k] = gr_lag::ordered_value(h[k]);
    std::memcpy(&v[4], &h[5], sizeof(double));
    return GR_OK;
}

// k_lag_bin over the context's rows into `acc` (host, 2 x cells integers); waits for it
static int32_t lag_bin(gr_ctx* ctx, const gr_lag::Profile& dev, const double* d_e, int64_t n_e, const double* d_t, int64_t n_t,
                       const CoronaGrid& gf, unsigned long long* d_acc, long long* acc)
{
    const size_t cells = (size_t)(n_e * n_t);
    GR_HIP(hipMemsetAsync(d_acc, 0, sizeof(unsigned long long) * 2 * cells, ctx->stream));
    int64_t blocks = (ctx->lag_n + 255) / 256;
    blocks = blocks > 1024 ? 1024 : blocks;
    const size_t lds = sizeof(unsigned long long) * 2 * cells;
    if (lds <= 40 * 1024) {
        hipLaunchKernelGGL(k_lag_bin<1>, dim3((unsigned)blocks), dim3(256), lds, ctx->stream, ctx->d_lag, ctx->lag_n, dev, d_e, (int)n_e,
                           d_t, (int)n_t, gf.sc, d_acc);
    } else {
        hipLaunchKernelGGL(k_lag_bin<0>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, ctx->d_lag, ctx->lag_n, dev, d_e, (int)n_e,
                           d_t, (int)n_t, gf.sc, d_acc);
    }
    GR_HIP(hipGetLastError());
    GR_HIP(hipMemcpyAsync(acc, d_acc, sizeof(long long) * 2 * cells, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    return GR_OK;
}

int32_t gr_lagtransfer_trace(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, int64_t* n_hits,
                             gr_stats* stats)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    ctx->lag_n = -1;      // (a refused trace leaves none)
    if (!rays || !n_hits) return fail(GR_ERR_INVALID_ARGUMENT, "rayset / n_hits is null");
    if (rays->sky_sampler) return fail(GR_ERR_INVALID_ARGUMENT, "gr_lagtransfer_trace traces an observer's plane, not a sky source (gr_rayset.sky_sampler = 0)");
    if (cfg && cfg->disc_id == GR_DISC_NONE) return fail(GR_ERR_INVALID_ARGUMENT, "a lag transfer function needs accretion geometry: none given");
    int32_t rc;
    GR_HIP(hipSetDevice(ctx->device));
    gr_rayset dev;
    if ((rc = begin_host_call(ctx, stats)) != GR_OK) return rc;
    if ((rc = stage_rays(ctx, rays, dev, 0, nullptr)) != GR_OK) return rc;
    const size_t n = (size_t)rays->n;
    if ((rc = ensure((void**)&ctx->d_lag, &ctx->lag_bytes, sizeof(double) * 4 * n + 64)) != GR_OK) return rc;
    unsigned long long* d_hits = (unsigned long long*)(ctx->d_lag + 4 * n);
    GR_HIP(hipMemsetAsync(d_hits, 0, sizeof(unsigned long long), ctx->stream));
    if ((rc = gr_ray_summary_device(ctx, cfg, &dev, pf, ctx->d_lag, stats ? (gr_stats*)ctx->d_stats : nullptr, ctx->stream)) != GR_OK) return rc;
    if (n > 0) {
        LagSep sep{};
        if (dev.sep_r) {
            const bool tiled = dev.sep_tiled && dev.sep_nr >= 8 && dev.sep_nt >= 8;      // (as rays_params lays the rays out)
            sep.r = dev.sep_r; sep.nr = dev.sep_nr;
            sep.core_rows = tiled ? (dev.sep_nr / 8) * 8 : 0;
            sep.core_cols = tiled ? (dev.sep_nt / 8) * 8 : 0;
            sep.first = dev.sep_first; sep.block = dev.sep_block; sep.stride = dev.sep_stride;
        }
        int64_t blocks = ((int64_t)n + 255) / 256;
        blocks = blocks > 1024 ? 1024 : blocks;
        hipLaunchKernelGGL(k_lag_prepare, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, ctx->d_lag, (int64_t)n, dev.area, sep, d_hits);
        GR_HIP(hipGetLastError());
    }
    unsigned long long h = 0ull;
    GR_HIP(hipMemcpyAsync(&h, d_hits, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = end_host_call(ctx, stats)) != GR_OK) return rc;      // (synchronises the stream)
    ctx->lag_hits = (int64_t)h;
    ctx->lag_n = rays->n;
    *n_hits = (int64_t)h;
    return GR_OK;
}

int32_t gr_lagtransfer_extrema(gr_ctx* ctx, const gr_lagprofile* profile, double* lims, double* flux_sum)
{
    int32_t rc;
    if ((rc = lag_profile_args(profile)) != GR_OK) return rc;
    if (!lims || !flux_sum) return fail(GR_ERR_INVALID_ARGUMENT, "lims / flux_sum is null");
    if ((rc = lag_have_trace(ctx, "gr_lagtransfer_extrema")) != GR_OK) return rc;
    if (ctx->lag_hits == 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_lagtransfer_extrema: no ray of the context's last gr_lagtransfer_trace met the geometry");
    GR_HIP(hipSetDevice(ctx->device));
    gr_lag::Profile dev;
    double* x;
    if ((rc = lag_stage(ctx, profile, 2 + 2 + 6, dev, &x)) != GR_OK) return rc;
    double v[5];
    if ((rc = lag_extrema(ctx, dev, (unsigned long long*)(x + 4), v)) != GR_OK) return rc;
    for (int k = 0; k < 4; ++k) lims[k] = v[k];
    // Σ f: every hit into the one cell of a 1 x 1 matrix (whatever its edge holds, the cell is clamped to it)
    GR_HIP(hipMemsetAsync(x, 0, sizeof(double) * 2, ctx->stream));
    const CoronaGrid gf = corona_grid(v[4], ctx->lag_hits);
    long long acc[2];
    if ((rc = lag_bin(ctx, dev, x, 1, x + 1, 1, gf, (unsigned long long*)(x + 2), acc)) != GR_OK) return rc;
    *flux_sum = gr_lag::corona_sum(acc[0], acc[1], gf);
    return GR_OK;
}

int32_t gr_lagtransfer_bin(gr_ctx* ctx, const gr_lagprofile* profile, const double* E_edges, int64_t n_E, const double* t_edges,
                           int64_t n_t, double* out)
{
    int32_t rc;
    if ((rc = lag_profile_args(profile)) != GR_OK) return rc;
    if ((rc = lag_edge_args(E_edges, n_E, "energy")) != GR_OK) return rc;
    if ((rc = lag_edge_args(t_edges, n_t, "time")) != GR_OK) return rc;
    if (n_E * n_t > ((int64_t)1 << 22)) return fail(GR_ERR_INVALID_ARGUMENT, "at most 2^22 cells (n_E * n_t)");
    if (!out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    if ((rc = lag_have_trace(ctx, "gr_lagtransfer_bin")) != GR_OK) return rc;
    const size_t cells = (size_t)(n_E * n_t);
    if (ctx->lag_hits == 0) {
        std::fill(out, out + cells, 0.0);
        return GR_OK;
    }
    GR_HIP(hipSetDevice(ctx->device));
    gr_lag::Profile dev;
    double* x;
    if ((rc = lag_stage(ctx, profile, (size_t)(n_E + n_t) + 2 * cells + 6, dev, &x)) != GR_OK) return rc;
    double *d_e = x, *d_t = x + n_E;
    unsigned long long* d_acc = (unsigned long long*)(x + n_E + n_t);
    GR_HIP(hipMemcpyAsync(d_e, E_edges, sizeof(double) * (size_t)n_E, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(d_t, t_edges, sizeof(double) * (size_t)n_t, hipMemcpyHostToDevice, ctx->stream));
    double v[5];
    if ((rc = lag_extrema(ctx, dev, d_acc + 2 * cells, v)) != GR_OK) return rc;      // (max |f| of THIS profile: the grid of the sums)
    const CoronaGrid gf = corona_grid(v[4], ctx->lag_hits);
    std::vector<long long> acc(2 * cells);
    if ((rc = lag_bin(ctx, dev, d_e, n_E, d_t, n_t, gf, d_acc, acc.data())) != GR_OK) return rc;
    for (size_t c = 0; c < cells; ++c) out[c] = gr_lag::corona_sum(acc[c], acc[cells + c], gf);
    return GR_OK;
}

int32_t gr_lagtransfer_rows(gr_ctx* ctx, double* out)
{
    int32_t rc;
    if ((rc = lag_have_trace(ctx, "gr_lagtransfer_rows")) != GR_OK) return rc;
    if (ctx->lag_n > 0 && !out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    GR_HIP(hipSetDevice(ctx->device));
    if (ctx->lag_n > 0) GR_HIP(hipMemcpyAsync(out, ctx->d_lag, sizeof(double) * 4 * (size_t)ctx->lag_n, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    return GR_OK;
}

// ---- transfer functions integrated on the device: gr_tf_lineprofile / gr_tf_lagtransfer ----
// the checks that read only the arguments, before anything touches the device
static int32_t tf_args(const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges, int64_t n_g,
                       const double* t_edges, int64_t n_t, bool lag, const double* out, bool annulus_values = true)
{
    if (!sets) return fail(GR_ERR_INVALID_ARGUMENT, "sets is null");
    if (!quad) return fail(GR_ERR_INVALID_ARGUMENT, "quad is null");
    if (!g_edges) return fail(GR_ERR_INVALID_ARGUMENT, "g edges are null");
    if (lag && !t_edges) return fail(GR_ERR_INVALID_ARGUMENT, "t edges are null");
    if (!out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    if (n_sets < 1) return fail(GR_ERR_INVALID_ARGUMENT, "n_sets must be at least 1");
    if (n_g < 2) return fail(GR_ERR_INVALID_ARGUMENT, "g axis: at least two edges");
    if (lag && n_t < 2) return fail(GR_ERR_INVALID_ARGUMENT, "t axis: at least two edges");
    const int64_t lim = (int64_t)1 << 24;
    if (n_sets > lim || n_g > lim || n_t > lim || n_sets * n_g > lim || n_sets * n_g * n_t > lim)
        return fail(GR_ERR_INVALID_ARGUMENT, "at most 2^24 cells (n_sets * n_g * n_t)");
    if (!quad->x || !quad->w) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfquad: nodes / weights are null");
    if (quad->n_q < 1 || quad->n_q > gr_tf::kMaxQuad) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfquad: n_q must be in 1 ... 32");
    for (int64_t k = 0; k < n_sets; ++k) {
        const gr_tfset& s = sets[k];
        const std::string who = "gr_tfset " + std::to_string(k) + ": ";
        if (s.n_r < 2) return fail(GR_ERR_INVALID_ARGUMENT, who + "n_r >= 2 emission radii are needed");
        if (s.n_int < 2) return fail(GR_ERR_INVALID_ARGUMENT, who + "n_int >= 2 annuli are needed");
        if (s.n_r > lim || s.n_int > lim) return fail(GR_ERR_INVALID_ARGUMENT, who + "at most 2^24 radii / annuli");
        if (!s.radii || !s.gmin || !s.gmax || !s.off || !s.knot_g || !s.knot_f || !s.knot_t)
            return fail(GR_ERR_INVALID_ARGUMENT, who + "a transfer-function array is null");
        if (!s.r_int || (annulus_values && (!s.eps_int || (lag && !s.tsd_int)))) return fail(GR_ERR_INVALID_ARGUMENT, who + "an annulus array is null");
        if (s.off[0] < 0) return fail(GR_ERR_INVALID_ARGUMENT, who + "offsets must ascend from off[0] >= 0");
        for (int64_t i = 0; i < 2 * s.n_r; ++i) {
            const int64_t n = s.off[i + 1] - s.off[i];
            if (s.off[i + 1] < s.off[i]) return fail(GR_ERR_INVALID_ARGUMENT, who + "offsets must ascend");
            if (n < 2 || n > gr_tf::kMaxKnots) return fail(GR_ERR_INVALID_ARGUMENT, who + "a branch needs 2 ... 1024 knots");
        }
    }
    return GR_OK;
}

// Both calls: stage every set in one block (descriptors, edges, arrays), find each set's largest deposit, accumulate on the
// grids that gives, read the integers back.  The block is the context's input scratch or, beyond 32 MiB, a buffer of this call.
static int32_t tf_integrate(gr_ctx* ctx, const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges, int64_t n_g,
                            const double* t_edges, int64_t n_t, bool lag, double* out)
{
    int32_t rc;
    if ((rc = tf_args(sets, n_sets, quad, g_edges, n_g, t_edges, n_t, lag, out)) != GR_OK) return rc;
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!lag) n_t = 1;
    GR_HIP(hipSetDevice(ctx->device));
    const size_t ns = (size_t)n_sets, cells = (size_t)(n_g * n_t);
    // layout in units of 8 bytes: descriptors | g edges | t edges | per set: radii gmin gmax r_int eps tsd off kg kf kt
    static_assert(sizeof(gr_tf::Set) % 8 == 0 && sizeof(CoronaScale) == 16, "8-byte units");
    const size_t desc_w = ns * (sizeof(gr_tf::Set) / 8);
    size_t words = desc_w + (size_t)n_g + (lag ? (size_t)n_t : 0);
    int64_t max_int = 0;
    for (size_t k = 0; k < ns; ++k) {
        const gr_tfset& s = sets[k];
        words += 3 * (size_t)s.n_r + 3 * (size_t)s.n_int + (2 * (size_t)s.n_r + 1) + 3 * (size_t)(s.off[2 * s.n_r] - s.off[0]);
        max_int = s.n_int > max_int ? s.n_int : max_int;
    }
    const size_t up_w = words;                                   // what is uploaded; behind it: red | scales | acc
    const size_t red_w = up_w, sc_w = red_w + ns, acc_w = sc_w + 2 * ns;
    const size_t bytes = 8 * (acc_w + 2 * ns * cells) + 64;
    void* own = nullptr;
    struct Free { void*& p; ~Free() { if (p) (void)hipFree(p); } } free_own{own};
    char* base;
    if (bytes > ((size_t)32 << 20)) {
        GR_HIP(hipMalloc(&own, bytes));
        base = (char*)own;
    } else {
        if ((rc = ensure(&ctx->d_in, &ctx->in_bytes, bytes)) != GR_OK) return rc;
        base = (char*)ctx->d_in;
    }
    std::vector<uint64_t> blob(up_w);
    const double* d0 = (const double*)base;
    size_t at = desc_w;
    auto put = [&](const void* src, size_t n) {
        std::memcpy(blob.data() + at, src, 8 * n);
        const double* d = d0 + at;
        at += n;
        return d;
    };
    const double* d_g = put(g_edges, (size_t)n_g);
    const double* d_t = lag ? put(t_edges, (size_t)n_t) : d_g;
    for (size_t k = 0; k < ns; ++k) {
        const gr_tfset& s = sets[k];
        const size_t nr = (size_t)s.n_r, ni = (size_t)s.n_int, nk = (size_t)(s.off[2 * s.n_r] - s.off[0]);
        gr_tf::Set d;
        d.n_r = s.n_r; d.n_int = s.n_int; d.r_min = s.r_min; d.g_scale = s.g_scale;
        d.radii = put(s.radii, nr); d.gmin = put(s.gmin, nr); d.gmax = put(s.gmax, nr);
        d.r_int = put(s.r_int, ni); d.eps = put(s.eps_int, ni);
        d.tsd = lag ? put(s.tsd_int, ni) : d.eps;
        int64_t* off = (int64_t*)(blob.data() + at);
        d.off = (const int64_t*)put(s.off, 2 * nr + 1);
        for (size_t i = 0; i <= 2 * nr; ++i) off[i] -= s.off[0];             // (the staged knots begin at the set's first)
        d.kg = put(s.knot_g + s.off[0], nk); d.kf = put(s.knot_f + s.off[0], nk); d.kt = put(s.knot_t + s.off[0], nk);
        std::memcpy(blob.data() + k * (sizeof(gr_tf::Set) / 8), &d, sizeof d);
    }
    gr_tf::Quad q{};
    q.h = quad->h; q.n = (int)quad->n_q;
    for (int i = 0; i < q.n; ++i) { q.x[i] = quad->x[i]; q.w[i] = quad->w[i]; }
    unsigned long long* d_red = (unsigned long long*)base + red_w;
    CoronaScale* d_sc = (CoronaScale*)((unsigned long long*)base + sc_w);
    unsigned long long* d_acc = (unsigned long long*)base + acc_w;
    GR_HIP(hipMemcpyAsync(base, blob.data(), 8 * up_w, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemsetAsync(d_red, 0, 8 * (acc_w - red_w + 2 * ns * cells), ctx->stream));
    // annuli per workgroup: one per wave unless that makes more than 2^16 workgroups
    int64_t chunk = ctx->tf_chunk;
    if (chunk <= 0) {
        chunk = 4;
        while ((int64_t)ns * ((max_int + chunk - 1) / chunk) > 65536) chunk *= 2;
    }
    const int64_t n_chunks = (max_int + chunk - 1) / chunk;
    if ((int64_t)ns * n_chunks > ((int64_t)1 << 30)) return fail(GR_ERR_INVALID_ARGUMENT, "tf_chunk: more than 2^30 workgroups");
    const dim3 grid((unsigned)((int64_t)ns * n_chunks)), block(256);
    const gr_tf::Set* d_sets = (const gr_tf::Set*)base;
    if (lag) hipLaunchKernelGGL((k_tf<1, 0, 0>), grid, block, 0, ctx->stream, d_sets, q, d_g, (int)n_g, d_t, (int)n_t, (int)chunk, (int)n_chunks, d_red, d_sc, d_acc);
    else     hipLaunchKernelGGL((k_tf<0, 0, 0>), grid, block, 0, ctx->stream, d_sets, q, d_g, (int)n_g, d_t, (int)n_t, (int)chunk, (int)n_chunks, d_red, d_sc, d_acc);
    GR_HIP(hipGetLastError());
    std::vector<unsigned long long> red(ns);
    GR_HIP(hipMemcpyAsync(red.data(), d_red, 8 * ns, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<CoronaGrid> grids(ns);
    std::vector<CoronaScale> scales(ns);
    for (size_t k = 0; k < ns; ++k) {
        double vmax;
        std::memcpy(&vmax, &red[k], sizeof vmax);
        grids[k] = corona_grid(vmax, 2 * sets[k].n_int);         // a cell takes at most two deposits per annulus
        scales[k] = grids[k].sc;
    }
    GR_HIP(hipMemcpyAsync(d_sc, scales.data(), sizeof(CoronaScale) * ns, hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = sizeof(unsigned long long) * 2 * cells;
    if (lds <= 40 * 1024) {
        if (lag) hipLaunchKernelGGL((k_tf<1, 1, 1>), grid, block, lds, ctx->stream, d_sets, q, d_g, (int)n_g, d_t, (int)n_t, (int)chunk, (int)n_chunks, d_red, d_sc, d_acc);
        else     hipLaunchKernelGGL((k_tf<0, 1, 1>), grid, block, lds, ctx->stream, d_sets, q, d_g, (int)n_g, d_t, (int)n_t, (int)chunk, (int)n_chunks, d_red, d_sc, d_acc);
    } else {
        if (lag) hipLaunchKernelGGL((k_tf<1, 1, 0>), grid, block, 0, ctx->stream, d_sets, q, d_g, (int)n_g, d_t, (int)n_t, (int)chunk, (int)n_chunks, d_red, d_sc, d_acc);
        else     hipLaunchKernelGGL((k_tf<0, 1, 0>), grid, block, 0, ctx->stream, d_sets, q, d_g, (int)n_g, d_t, (int)n_t, (int)chunk, (int)n_chunks, d_red, d_sc, d_acc);
    }
    GR_HIP(hipGetLastError());
    std::vector<long long> acc(2 * ns * cells);
    GR_HIP(hipMemcpyAsync(acc.data(), d_acc, 8 * acc.size(), hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < ns; ++k) {
        const long long* a = acc.data() + 2 * cells * k;
        for (size_t c = 0; c < cells; ++c) out[k * cells + c] = gr_lag::corona_sum(a[c], a[cells + c], grids[k]);
    }
    return GR_OK;
}

int32_t gr_tf_lineprofile(gr_ctx* ctx, const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges, int64_t n_g,
                          double* out)
{
    return tf_integrate(ctx, sets, n_sets, quad, g_edges, n_g, nullptr, 1, false, out);
}

int32_t gr_tf_lagtransfer(gr_ctx* ctx, const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges, int64_t n_g,
                          const double* t_edges, int64_t n_t, double* out)
{
    return tf_integrate(ctx, sets, n_sets, quad, g_edges, n_g, t_edges, n_t, true, out);
}

// ---- gr_tf_lagtransfer_td: the lag transfer function of a time-dependent emissivity ----
// the checks that read only the arguments
static int32_t tftd_args(const gr_tfprofile* p, int64_t g_upscale, int64_t n_time)
{
    if (!p) return fail(GR_ERR_INVALID_ARGUMENT, "prof is null");
    if (n_time < 2 || n_time > gr_tftd::kMaxTime) return fail(GR_ERR_INVALID_ARGUMENT, "n_time must be in 2 ... 1024");
    if (g_upscale < 1 || g_upscale > gr_tftd::kMaxUpscale) return fail(GR_ERR_INVALID_ARGUMENT, "g_upscale must be in 1 ... 64");
    if (p->n_rings < 1 || p->n_rings > gr_tftd::kMaxRings) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: n_rings must be in 1 ... 1024");
    if (!p->ring_weight || !p->ring_dt || !p->arm_off || !p->curve_off || !p->knot_r || !p->knot_t || !p->knot_e)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: an array is null");
    if (p->arm_off[0] < 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: arm offsets must ascend from arm_off[0] >= 0");
    for (int64_t a = 0; a < 2 * p->n_rings; ++a) {
        const int64_t n = p->arm_off[a + 1] - p->arm_off[a];
        if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: arm offsets must ascend");
        if (n < 2 || n > gr_tftd::kMaxCurves) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: an arm needs 2 ... 1024 curves");
    }
    const int64_t c0 = p->arm_off[0], c1 = p->arm_off[2 * p->n_rings];
    if (p->curve_off[c0] < 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: curve offsets must ascend from an offset >= 0");
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t n = p->curve_off[c + 1] - p->curve_off[c];
        if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: curve offsets must ascend");
        if (n < 2) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: a curve needs at least 2 knots");
    }
    if (p->curve_off[c1] - p->curve_off[c0] > ((int64_t)1 << 28)) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tfprofile: at most 2^28 knots");
    return GR_OK;
}

// One block as tf_integrate stages it: descriptors | edges | the set's arrays (ε = 1) | the profile's arrays, behind them
// em | red | scale | acc.  k_tftd_em fills em, k_tftd<0> finds the largest deposit, k_tftd<1> accumulates on the grid it gives.
int32_t gr_tf_lagtransfer_td(gr_ctx* ctx, const gr_tfset* set, const gr_tfprofile* prof, const gr_tfquad* quad, const double* g_edges,
                             int64_t n_g, const double* t_edges, int64_t n_t, int64_t g_upscale, int64_t n_time, double t0, double* out,
                             double* em_out)
{
    int32_t rc;
    if ((rc = tf_args(set, 1, quad, g_edges, n_g, t_edges, n_t, true, out, false)) != GR_OK) return rc;
    if ((rc = tftd_args(prof, g_upscale, n_time)) != GR_OK) return rc;
    if (n_g * g_upscale > ((int64_t)1 << 24)) return fail(GR_ERR_INVALID_ARGUMENT, "at most 2^24 fine g bins (n_g * g_upscale)");
    if (set->n_int * g_upscale * n_time > ((int64_t)1 << 38)) return fail(GR_ERR_INVALID_ARGUMENT, "at most 2^38 deposits per cell (n_int * g_upscale * n_time)");
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    GR_HIP(hipSetDevice(ctx->device));
    const gr_tfset& s = *set;
    const gr_tfprofile& p = *prof;
    const size_t cells = (size_t)(n_g * n_t);
    const size_t nr = (size_t)s.n_r, ni = (size_t)s.n_int, nk = (size_t)(s.off[2 * s.n_r] - s.off[0]);
    const size_t rings = (size_t)p.n_rings;
    const int64_t c0 = p.arm_off[0], c1 = p.arm_off[2 * p.n_rings], k0 = p.curve_off[c0];
    const size_t n_curves = (size_t)(c1 - c0), n_knots = (size_t)(p.curve_off[c1] - k0);
    static_assert(sizeof(gr_tf::Set) % 8 == 0 && sizeof(gr_tftd::Profile) % 8 == 0, "8-byte units");
    const size_t set_w = sizeof(gr_tf::Set) / 8, desc_w = set_w + sizeof(gr_tftd::Profile) / 8;
    const size_t up_w = desc_w + (size_t)n_g + (size_t)n_t + 3 * nr + 2 * ni + (2 * nr + 1) + 3 * nk
                        + 2 * rings + (2 * rings + 1) + (n_curves + 1) + 3 * n_knots;
    const size_t em_row = 2 + (size_t)n_time;
    const size_t em_w = up_w, red_w = em_w + ni * em_row, sc_w = red_w + 1, acc_w = sc_w + 2;
    const size_t bytes = 8 * (acc_w + 2 * cells) + 64;
    void* own = nullptr;
    struct Free { void*& p; ~Free() { if (p) (void)hipFree(p); } } free_own{own};
    char* base;
    if (bytes > ((size_t)32 << 20)) {
        GR_HIP(hipMalloc(&own, bytes));
        base = (char*)own;
    } else {
        if ((rc = ensure(&ctx->d_in, &ctx->in_bytes, bytes)) != GR_OK) return rc;
        base = (char*)ctx->d_in;
    }
    std::vector<uint64_t> blob(up_w);
    const double* d0 = (const double*)base;
    size_t at = desc_w;
    auto put = [&](const void* src, size_t n) {
        std::memcpy(blob.data() + at, src, 8 * n);
        const double* d = d0 + at;
        at += n;
        return d;
    };
    const double* d_g = put(g_edges, (size_t)n_g);
    const double* d_t = put(t_edges, (size_t)n_t);
    gr_tf::Set d;
    d.n_r = s.n_r; d.n_int = s.n_int; d.r_min = s.r_min; d.g_scale = s.g_scale;
    d.radii = put(s.radii, nr); d.gmin = put(s.gmin, nr); d.gmax = put(s.gmax, nr);
    d.r_int = put(s.r_int, ni);
    {
        const std::vector<double> ones(ni, 1.0);                 // the annulus weight has no ε: annulus_of multiplies by 1
        d.eps = d.tsd = put(ones.data(), ni);
    }
    {
        int64_t* off = (int64_t*)(blob.data() + at);
        d.off = (const int64_t*)put(s.off, 2 * nr + 1);
        for (size_t i = 0; i <= 2 * nr; ++i) off[i] -= s.off[0];
    }
    d.kg = put(s.knot_g + s.off[0], nk); d.kf = put(s.knot_f + s.off[0], nk); d.kt = put(s.knot_t + s.off[0], nk);
    std::memcpy(blob.data(), &d, sizeof d);
    gr_tftd::Profile dp;
    dp.n_rings = p.n_rings;
    dp.w = put(p.ring_weight, rings); dp.dt = put(p.ring_dt, rings);
    {
        int64_t* off = (int64_t*)(blob.data() + at);
        dp.arm_off = (const int64_t*)put(p.arm_off, 2 * rings + 1);
        for (size_t i = 0; i <= 2 * rings; ++i) off[i] -= c0;
        off = (int64_t*)(blob.data() + at);
        dp.curve_off = (const int64_t*)put(p.curve_off + c0, n_curves + 1);
        for (size_t i = 0; i <= n_curves; ++i) off[i] -= k0;
    }
    dp.kr = put(p.knot_r + k0, n_knots); dp.kt = put(p.knot_t + k0, n_knots); dp.ke = put(p.knot_e + k0, n_knots);
    std::memcpy(blob.data() + set_w, &dp, sizeof dp);
    if (at != up_w) return fail(GR_ERR_INVALID_ARGUMENT, "gr_tf_lagtransfer_td: the staged block does not match its layout");
    gr_tf::Quad q{};
    q.h = quad->h; q.n = (int)quad->n_q;
    for (int i = 0; i < q.n; ++i) { q.x[i] = quad->x[i]; q.w[i] = quad->w[i]; }
    double* d_em = (double*)base + em_w;
    unsigned long long* d_red = (unsigned long long*)base + red_w;
    CoronaScale* d_sc = (CoronaScale*)((unsigned long long*)base + sc_w);
    unsigned long long* d_acc = (unsigned long long*)base + acc_w;
    const gr_tf::Set* d_set = (const gr_tf::Set*)base;
    const gr_tftd::Profile* d_prof = (const gr_tftd::Profile*)((const uint64_t*)base + set_w);
    GR_HIP(hipMemcpyAsync(base, blob.data(), 8 * up_w, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemsetAsync(d_red, 0, 8 * (acc_w - red_w + 2 * cells), ctx->stream));
    hipLaunchKernelGGL(k_tftd_em, dim3((unsigned)ni), dim3(256), 0, ctx->stream, d_set, d_prof, (int)n_time, d_em);
    GR_HIP(hipGetLastError());
    int64_t chunk = ctx->tf_chunk;
    if (chunk <= 0) {
        chunk = 4;
        while ((s.n_int + chunk - 1) / chunk > 65536) chunk *= 2;
    }
    const int64_t n_chunks = (s.n_int + chunk - 1) / chunk;
    const dim3 grid((unsigned)n_chunks), block(256);              // (n_int <= 2^24 annuli, a chunk holds at least one)
    hipLaunchKernelGGL((k_tftd<0, 0>), grid, block, 0, ctx->stream, d_set, q, d_g, (int)n_g, d_t, (int)n_t, (int)g_upscale, (int)n_time, t0,
                       (const double*)d_em, (int)chunk, d_red, d_sc, d_acc);
    GR_HIP(hipGetLastError());
    unsigned long long red = 0ull;
    GR_HIP(hipMemcpyAsync(&red, d_red, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (em_out) GR_HIP(hipMemcpyAsync(em_out, d_em, 8 * ni * em_row, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    double vmax;
    std::memcpy(&vmax, &red, sizeof vmax);
    // a cell takes at most two deposits per annulus, fine bin and time sample
    const CoronaGrid grd = corona_grid(vmax, 2 * s.n_int * g_upscale * n_time);
    GR_HIP(hipMemcpyAsync(d_sc, &grd.sc, sizeof(CoronaScale), hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = sizeof(unsigned long long) * 2 * cells;
    if (lds <= 40 * 1024)
        hipLaunchKernelGGL((k_tftd<1, 1>), grid, block, lds, ctx->stream, d_set, q, d_g, (int)n_g, d_t, (int)n_t, (int)g_upscale, (int)n_time, t0,
                           (const double*)d_em, (int)chunk, d_red, d_sc, d_acc);
    else
        hipLaunchKernelGGL((k_tftd<1, 0>), grid, block, 0, ctx->stream, d_set, q, d_g, (int)n_g, d_t, (int)n_t, (int)g_upscale, (int)n_time, t0,
                           (const double*)d_em, (int)chunk, d_red, d_sc, d_acc);
    GR_HIP(hipGetLastError());
    std::vector<long long> acc(2 * cells);
    GR_HIP(hipMemcpyAsync(acc.data(), d_acc, 8 * acc.size(), hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t c = 0; c < cells; ++c) out[c] = gr_lag::corona_sum(acc[c], acc[cells + c], grd);
    return GR_OK;
}

// ---- the longitudinal arms of ring coronae (corona_arms, src/corona/models/ring.jl:1-485): gr_ring_rays / gr_ring_arms ----
// The arithmetic is gr_ringarm.hpp's; the trace is launch_trace's ray-summary launch on (x, v) arrays, as a sky source's.
extern "C++" {
namespace {
struct RingDev {      // a staged gr_ringset
    const double *frames, *betas, *base;
    int32_t n_rings, n_slices, n_base, extrema_iter;
};
// ray j -> x, v and the factor of its g.  With a list: (ring, slice) = ring_slice[j], θ = angles[j]; without: the base rays,
// ray j = (ring * n_slices + slice) * n_base + i at base angle i
__global__ void __launch_bounds__(256) k_ring_rays(const RingDev r, int64_t n, const int64_t* ring_slice, const double* angles,
                                                   double* x, double* v, double* f)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    int ring, slice;
    double th;
    if (ring_slice) {
        ring = (int)ring_slice[2 * j];
        slice = (int)ring_slice[2 * j + 1];
        th = angles[j];
    } else {
        const int64_t s = j / r.n_base;
        ring = (int)(s / r.n_slices);
        slice = (int)(s % r.n_slices);
        th = r.base[j % r.n_base];
    }
    const double* fr = r.frames + (size_t)gr_ring::kFrame * ring;
    double vv[4], ff;
    gr_ring::form_ray(fr, r.betas[slice], th, vv, ff);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        x[4 * j + q] = fr[q];
        v[4 * j + q] = vv[q];
    }
    f[j] = ff;
}
// one lane per search q = 2 (ring * n_slices + slice) + target: the bracket from the slice's base rows.  A slice without a
// hit has no search: done from the start, its count -1.
__global__ void __launch_bounds__(64) k_ring_bracket(const RingDev r, int n_search, const double* rows, gr_ring::Search* searches, int32_t* cnt)
{
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= n_search) return;
    gr_ring::Search s;
    const bool have = gr_ring::bracket(rows + (size_t)4 * r.n_base * (q >> 1), r.base, r.n_base, q & 1, s.a, s.b, s.best);
    s.n = s.iters = s.too_many = 0;
    s.done = have ? 0 : 1;
    searches[q] = s;
    cnt[q] = have ? 0 : -1;
}
// one lane per search: a live one takes the next slot of this iteration's list and forms its two probe rays there
__global__ void __launch_bounds__(64) k_ring_probe(const RingDev r, int n_search, const gr_ring::Search* searches, unsigned long long* live,
                                                   int32_t* list, double* x, double* v, double* f)
{
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= n_search) return;
    const gr_ring::Search s = searches[q];
    if (s.done) return;
    const size_t slot = (size_t)atomicAdd(live, 1ull);          // < n_search: every search adds at most once
    list[slot] = q;
    const int sl = q >> 1;
    const double* fr = r.frames + (size_t)gr_ring::kFrame * (sl / r.n_slices);
    const double beta = r.betas[sl % r.n_slices];
    double th[2];
    gr_ring::probes(s, th[0], th[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double vv[4], ff;
        gr_ring::form_ray(fr, beta, th[k], vv, ff);
        const size_t j = 2 * slot + k;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            x[4 * j + c] = fr[c];
            v[4 * j + c] = vv[c];
        }
        f[j] = ff;
    }
}
// one lane per slot of the list: the golden update of its search from the two probe rows; a kept probe joins the search's run
// app[q][extrema_iter][5] = (θ, g, ρ, t, status) (n <= extrema_iter counts every kept probe: the run cannot overflow)
__global__ void __launch_bounds__(64) k_ring_update(const RingDev r, int n_live, const int32_t* list, const double* prows, gr_ring::Search* searches,
                                                    int32_t* cnt, double* app)
{
    const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (slot >= n_live) return;
    const int q = list[slot];
    gr_ring::Search s = searches[q];
    double th[2];
    gr_ring::probes(s, th[0], th[1]);
    const double* pc = prows + 8 * (size_t)slot;
    const int append = gr_ring::golden_update(s, q & 1, r.extrema_iter, (int)pc[3], pc[1], (int)pc[7], pc[5]);
    searches[q] = s;
    if (append) {
        const int at = cnt[q];
        if (at < r.extrema_iter) {
            const double* row = pc + 4 * (append - 1);
            double* o = app + 5 * ((size_t)q * r.extrema_iter + at);
            o[0] = th[append - 1];
#pragma unroll
            for (int c = 0; c < 4; ++c) o[1 + c] = row[c];
            cnt[q] = at + 1;
        }
    }
}
// one lane per (slice, slot of its cache): base rows, then what the minima search kept, then the maxima search's; zeros behind
__global__ void __launch_bounds__(256) k_ring_pack(const RingDev r, int64_t n, const double* rows, const int32_t* cnt, const double* app, double* out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int width = r.n_base + 2 * r.extrema_iter;
    const int64_t sl = j / width;
    const int slot = (int)(j % width);
    const int c_min = cnt[2 * sl] > 0 ? cnt[2 * sl] : 0, c_max = cnt[2 * sl + 1] > 0 ? cnt[2 * sl + 1] : 0;
    double o[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    const double* src = nullptr;
    if (slot < r.n_base) {
        o[0] = r.base[slot];
        src = rows + 4 * ((size_t)sl * r.n_base + slot);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[1 + c] = src[c];
    } else {
        const int k = slot - r.n_base;
        if (k < c_min) src = app + 5 * ((size_t)(2 * sl) * r.extrema_iter + k);
        else if (k < c_min + c_max) src = app + 5 * ((size_t)(2 * sl + 1) * r.extrema_iter + (k - c_min));
        if (src) {
#pragma unroll
            for (int c = 0; c < 5; ++c) o[c] = src[c];
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) out[5 * j + c] = o[c];
}
}  // namespace
}  // extern "C++"

static int32_t ring_args(gr_ctx* ctx, const gr_config* cfg, const gr_ringset* rings, const gr_pointfunction* pf)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!cfg || !rings || !pf) return fail(GR_ERR_INVALID_ARGUMENT, "config / ring set / point function is null");
    if (cfg->disc_id != GR_DISC_THIN) return fail(GR_ERR_UNSUPPORTED, "the arms of a ring corona are traced onto a ThinDisc only");
    if (rings->n_rings < 1 || rings->n_slices < 1 || rings->n_rings > (1 << 20) || rings->n_slices > (1 << 20) || !rings->frames || !rings->betas)
        return fail(GR_ERR_INVALID_ARGUMENT, "ring set: n_rings and n_slices in 1 ... 2^20, frames and betas");
    if (pf->pf_id != GR_PF_REDSHIFT) return fail(GR_ERR_INVALID_ARGUMENT, "needs the redshift point function");
    if (pf->has_u_src) return fail(GR_ERR_INVALID_ARGUMENT, "a ring set brings a source velocity per ring: pf->has_u_src must be 0");
    return GR_OK;
}
// the ray-summary launch on n rays written as x[n][4], v[n][4]: rows (g, ρ, t, status), g against each ray's own source (f)
static int32_t ring_trace(gr_ctx* ctx, const gr_config* cfg, const PfDev& pfd, const double* d_x, const double* d_v, const double* d_f,
                          int64_t n, double* d_rows, gr_stats* d_stats)
{
    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = n;
    p.stats = (unsigned long long*)d_stats;
    cd.src_mode = 1;
    cd.out_mode = 4;
    cd.x = d_x;
    cd.x_stride = 4;
    cd.v = d_v;
    cd.pf = pfd;
    cd.lp_rmin = 0.0;
    cd.lp_rmax = INFINITY;
    cd.lp_pairs = d_rows;
    cd.range = gr_range{ 0, n, n > 0 ? n : 1, 1 };
    cd.swizzle = 0;
    int32_t rc;
    if ((rc = launch_trace(ctx, p, cd, ctx->stream)) != GR_OK) return rc;
    hipLaunchKernelGGL(k_sky_scale_g, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_rows, d_f, n);
    GR_HIP(hipGetLastError());
    return GR_OK;
}

int32_t gr_ring_rays(gr_ctx* ctx, const gr_config* cfg, const gr_ringset* rings, const gr_pointfunction* pf, int64_t n,
                     const int64_t* ring_slice, const double* angles, double* rows_out, double* v_out, gr_stats* stats)
{
    int32_t rc;
    if ((rc = ring_args(ctx, cfg, rings, pf)) != GR_OK) return rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (n < 0 || n > INT32_MAX) return fail(GR_ERR_INVALID_ARGUMENT, "gr_ring_rays: n in 0 ... 2^31 - 1");
    if (n > 0 && (!ring_slice || !angles || !rows_out)) return fail(GR_ERR_INVALID_ARGUMENT, "gr_ring_rays: ring_slice / angles / rows_out is null");
    for (int64_t j = 0; j < n; ++j)
        if (ring_slice[2 * j] < 0 || ring_slice[2 * j] >= rings->n_rings || ring_slice[2 * j + 1] < 0 || ring_slice[2 * j + 1] >= rings->n_slices)
            return fail(GR_ERR_INVALID_ARGUMENT, "gr_ring_rays: ray " + std::to_string(j) + " names a ring or a slice the set does not have");
    GR_HIP(hipSetDevice(ctx->device));
    if (n == 0) return GR_OK;
    const size_t R = (size_t)rings->n_rings, NS = (size_t)rings->n_slices, N = (size_t)n;
    const size_t in_w = gr_ring::kFrame * R + NS + N + 2 * N;      // frames | betas | angles | ring_slice (2 n int64)
    if ((rc = ensure(&ctx->d_in, &ctx->in_bytes, 8 * in_w + 64)) != GR_OK) return rc;
    if ((rc = ensure(&ctx->d_scratch, &ctx->scratch_bytes, 8 * 13 * N + 64)) != GR_OK) return rc;
    double* d_frames = (double*)ctx->d_in;
    double* d_betas = d_frames + gr_ring::kFrame * R;
    double* d_angles = d_betas + NS;
    int64_t* d_rs = (int64_t*)(d_angles + N);
    double* d_x = (double*)ctx->d_scratch;
    double *d_v = d_x + 4 * N, *d_f = d_v + 4 * N, *d_rows = d_f + N;
    if ((rc = begin_host_call(ctx, stats)) != GR_OK) return rc;
    GR_HIP(hipMemcpyAsync(d_frames, rings->frames, 8 * gr_ring::kFrame * R, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(d_betas, rings->betas, 8 * NS, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(d_angles, angles, 8 * N, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(d_rs, ring_slice, 8 * 2 * N, hipMemcpyHostToDevice, ctx->stream));
    Cold staged;
    std::memset(&staged, 0, sizeof staged);
    if ((rc = stage_pf(ctx, cfg, pf, staged.pf, ctx->stream)) != GR_OK) return rc;
    const RingDev rd{ d_frames, d_betas, nullptr, (int32_t)R, (int32_t)NS, 0, 0 };
    hipLaunchKernelGGL(k_ring_rays, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, rd, n, (const int64_t*)d_rs,
                       (const double*)d_angles, d_x, d_v, d_f);
    GR_HIP(hipGetLastError());
    if ((rc = ring_trace(ctx, cfg, staged.pf, d_x, d_v, d_f, n, d_rows, stats ? (gr_stats*)ctx->d_stats : nullptr)) != GR_OK) return rc;
    GR_HIP(hipMemcpyAsync(rows_out, d_rows, 8 * 4 * N, hipMemcpyDeviceToHost, ctx->stream));
    if (v_out) GR_HIP(hipMemcpyAsync(v_out, d_v, 8 * 4 * N, hipMemcpyDeviceToHost, ctx->stream));
    return end_host_call(ctx, stats);
}

int32_t gr_ring_arms(gr_ctx* ctx, const gr_config* cfg, const gr_ringset* rings, const gr_pointfunction* pf, double* rows_out,
                     int64_t* counts_out, gr_stats* stats)
{
    int32_t rc;
    if ((rc = ring_args(ctx, cfg, rings, pf)) != GR_OK) return rc;
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (!rings->base_angles || !rows_out || !counts_out) return fail(GR_ERR_INVALID_ARGUMENT, "gr_ring_arms: base_angles / rows_out / counts_out is null");
    if (rings->n_base < 2 || rings->extrema_iter < 1 || rings->n_base > (1 << 24) || rings->extrema_iter > (1 << 20))
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_ring_arms: n_base in 2 ... 2^24, extrema_iter in 1 ... 2^20");
    const size_t R = (size_t)rings->n_rings, NS = (size_t)rings->n_slices, NB = (size_t)rings->n_base, E = (size_t)rings->extrema_iter;
    const size_t S = R * NS, W = NB + 2 * E, n0 = S * NB, Q = 2 * S;
    if (n0 > (size_t)INT32_MAX || S * W > (size_t)INT32_MAX) return fail(GR_ERR_INVALID_ARGUMENT, "gr_ring_arms: at most 2^31 - 1 base rays and cache rows");
    GR_HIP(hipSetDevice(ctx->device));
    static_assert(sizeof(gr_ring::Search) == 40, "five 8-byte units");
    // frames | betas | base | x0 v0 f0 rows0 | probe x v f rows (2 Q rays) | app | out | searches | cnt | list | live
    const size_t max_it = 2 * E + 1;
    const size_t o_frames = 0, o_betas = o_frames + gr_ring::kFrame * R, o_base = o_betas + NS, o_x0 = o_base + NB, o_v0 = o_x0 + 4 * n0,
                 o_f0 = o_v0 + 4 * n0, o_rows0 = o_f0 + n0, o_px = o_rows0 + 4 * n0, o_pv = o_px + 8 * Q, o_pf = o_pv + 8 * Q, o_prows = o_pf + 2 * Q,
                 o_app = o_prows + 8 * Q, o_out = o_app + 5 * Q * E, o_search = o_out + 5 * S * W, o_cnt = o_search + 5 * Q, o_list = o_cnt + S,
                 o_live = o_list + S, total = o_live + max_it + 1;
    if ((rc = ensure(&ctx->d_scratch, &ctx->scratch_bytes, 8 * total + 64)) != GR_OK) return rc;
    double* base = (double*)ctx->d_scratch;
    gr_ring::Search* d_search = (gr_ring::Search*)(base + o_search);
    int32_t* d_cnt = (int32_t*)(base + o_cnt);
    int32_t* d_list = (int32_t*)(base + o_list);
    unsigned long long* d_live = (unsigned long long*)(base + o_live);
    if ((rc = begin_host_call(ctx, stats)) != GR_OK) return rc;
    gr_stats* d_stats = stats ? (gr_stats*)ctx->d_stats : nullptr;
    GR_HIP(hipMemcpyAsync(base + o_frames, rings->frames, 8 * gr_ring::kFrame * R, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(base + o_betas, rings->betas, 8 * NS, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemcpyAsync(base + o_base, rings->base_angles, 8 * NB, hipMemcpyHostToDevice, ctx->stream));
    GR_HIP(hipMemsetAsync(d_live, 0, 8 * (max_it + 1), ctx->stream));
    Cold staged;
    std::memset(&staged, 0, sizeof staged);
    if ((rc = stage_pf(ctx, cfg, pf, staged.pf, ctx->stream)) != GR_OK) return rc;
    const RingDev rd{ base + o_frames, base + o_betas, base + o_base, (int32_t)R, (int32_t)NS, (int32_t)NB, (int32_t)E };
    // 1. the base rays of every slice, one launch
    hipLaunchKernelGGL(k_ring_rays, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, ctx->stream, rd, (int64_t)n0, (const int64_t*)nullptr,
                       (const double*)nullptr, base + o_x0, base + o_v0, base + o_f0);
    GR_HIP(hipGetLastError());
    if ((rc = ring_trace(ctx, cfg, staged.pf, base + o_x0, base + o_v0, base + o_f0, (int64_t)n0, base + o_rows0, d_stats)) != GR_OK) return rc;
    // 2. the brackets
    const dim3 q_grid((unsigned)((Q + 63) / 64));
    hipLaunchKernelGGL(k_ring_bracket, q_grid, dim3(64), 0, ctx->stream, rd, (int)Q, (const double*)(base + o_rows0), d_search, d_cnt);
    GR_HIP(hipGetLastError());
    // 3. the searches in lock-step: probe rays of the live ones, trace, update
    for (size_t it = 0; it < max_it; ++it) {
        hipLaunchKernelGGL(k_ring_probe, q_grid, dim3(64), 0, ctx->stream, rd, (int)Q, (const gr_ring::Search*)d_search, d_live + it, d_list,
                           base + o_px, base + o_pv, base + o_pf);
        GR_HIP(hipGetLastError());
        unsigned long long n_live = 0;
        GR_HIP(hipMemcpyAsync(&n_live, d_live + it, 8, hipMemcpyDeviceToHost, ctx->stream));
        GR_HIP(hipStreamSynchronize(ctx->stream));
        if (n_live == 0) break;
        if (n_live > Q) return fail(GR_ERR_HIP, "gr_ring_arms: more live searches than searches");
        if ((rc = ring_trace(ctx, cfg, staged.pf, base + o_px, base + o_pv, base + o_pf, (int64_t)(2 * n_live), base + o_prows, d_stats)) != GR_OK) return rc;
        hipLaunchKernelGGL(k_ring_update, dim3((unsigned)((n_live + 63) / 64)), dim3(64), 0, ctx->stream, rd, (int)n_live, (const int32_t*)d_list,
                           (const double*)(base + o_prows), d_search, d_cnt, base + o_app);
        GR_HIP(hipGetLastError());
    }
    // 4. every slice's cache in the reference's order
    hipLaunchKernelGGL(k_ring_pack, dim3((unsigned)((S * W + 255) / 256)), dim3(256), 0, ctx->stream, rd, (int64_t)(S * W), (const double*)(base + o_rows0),
                       (const int32_t*)d_cnt, (const double*)(base + o_app), base + o_out);
    GR_HIP(hipGetLastError());
    std::vector<int32_t> cnt(Q);
    GR_HIP(hipMemcpyAsync(rows_out, base + o_out, 8 * 5 * S * W, hipMemcpyDeviceToHost, ctx->stream));
    GR_HIP(hipMemcpyAsync(cnt.data(), d_cnt, 4 * Q, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = end_host_call(ctx, stats)) != GR_OK) return rc;
    for (size_t s = 0; s < S; ++s) {
        counts_out[3 * s] = (int64_t)NB;
        counts_out[3 * s + 1] = cnt[2 * s];
        counts_out[3 * s + 2] = cnt[2 * s + 1];
    }
    return GR_OK;
}

// ---- ray arrays and ray sets: one context, or contiguous shares of the rays over several ----

int32_t gr_trace_endpoints_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const double* x, int64_t x_stride,
                                 const double* v, int64_t n_rays, gr_point* points, gr_stats* stats)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    if (n_rays < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (x_stride != 0 && x_stride != 4) return fail(GR_ERR_INVALID_ARGUMENT, "x_stride must be 0 or 4");
    if (n_rays > 0 && (!x || !v || !points)) return fail(GR_ERR_INVALID_ARGUMENT, "x/v/points is null");
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    const bool pinned = is_pinned(points, sizeof(gr_point) * (size_t)n_rays);
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(n_rays, n, k, &off, &cnt);
        int32_t r;
        GR_HIP(hipSetDevice(c->device));
        const size_t nx = (size_t)(x_stride == 0 ? 4 : 4 * cnt), nv = (size_t)(4 * cnt);
        const size_t out_bytes = sizeof(gr_point) * (size_t)cnt;
        if ((r = ensure(&c->d_scratch, &c->scratch_bytes, out_bytes ? out_bytes : 8)) != GR_OK) return r;
        if ((r = ensure(&c->d_in, &c->in_bytes, sizeof(double) * (nx + nv) + 8)) != GR_OK) return r;
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        if (cnt == 0) return GR_OK;
        double* d_x = (double*)c->d_in;
        double* d_v = d_x + nx;
        GR_HIP(hipMemcpyAsync(d_x, x_stride == 0 ? x : x + 4 * off, sizeof(double) * nx, hipMemcpyHostToDevice, c->stream));
        GR_HIP(hipMemcpyAsync(d_v, v + 4 * off, sizeof(double) * nv, hipMemcpyHostToDevice, c->stream));
        return gr_trace_endpoints_device(c, cfg, d_x, x_stride, d_v, cnt, (gr_point*)c->d_scratch,
                                         stats ? (gr_stats*)c->d_stats : nullptr, c->stream);
    };
    bool faulted = false;
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(n_rays, n, k, &off, &cnt);
        if (cnt == 0) return GR_OK;
        if (!faulted && !pinned) prefault_output(points, sizeof(gr_point) * (size_t)n_rays, c->hugepages != 0);
        faulted = true;
        GR_HIP(hipSetDevice(c->device));
        GR_HIP(hipMemcpyAsync(points + off, c->d_scratch, sizeof(gr_point) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        return GR_OK;
    };
    return multi_drive(ctxs, n, stats, enq, copy);
}

int32_t gr_trace_endpoints(gr_ctx* ctx, const gr_config* cfg, const double* x, int64_t x_stride, const double* v,
                           int64_t n, gr_point* points, gr_stats* stats)
{
    return one_context(gr_trace_endpoints_multi(&ctx, 1, cfg, x, x_stride, v, n, points, stats), stats);
}

// ---- covariant radiative transfer (include/gradus_mi355x.h, gr_transfer): TraceRadiativeTransfer through a thick disc ----
extern "C++" {
namespace {
// what the radiative-transfer kernels are not built for, refused before anything touches the device
int32_t transfer_check(const gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer)
{
    if (!cfg) return fail(GR_ERR_INVALID_ARGUMENT, "config is null");
    if (!transfer) return fail(GR_ERR_INVALID_ARGUMENT, "transfer is null");
    if (cfg->metric_id == GR_METRIC_TABULATED || cfg->metric_id >= GR_METRIC_COMPILED)
        return fail(GR_ERR_UNSUPPORTED, "radiative transfer is traced through the catalogue's metrics only (not GR_METRIC_TABULATED, not a compiled metric)");
    if (cfg->metric_id < 0 || cfg->metric_id >= 12 || !kTraceRT[cfg->metric_id])
        return fail(GR_ERR_UNSUPPORTED, "radiative transfer needs a metric with an ISCO (fluid_velocity): metric_id " + std::to_string(cfg->metric_id) + " has none");
    if (cfg->disc_id != GR_DISC_SHAKURA_SUNYAEV && cfg->disc_id != GR_DISC_TABULATED)
        return fail(GR_ERR_UNSUPPORTED, "radiative transfer is traced through GR_DISC_SHAKURA_SUNYAEV and GR_DISC_TABULATED only (disc_id "
                                        + std::to_string(cfg->disc_id) + ")");
    if (cfg->disc_id == GR_DISC_TABULATED && cfg->disc_params[3] != 0.0)
        return fail(GR_ERR_UNSUPPORTED, "radiative transfer: a warped thin disc's table (disc_params[3] != 0) is an optically thin sheet, not a medium");
    if (ctx->precision == 32) return fail(GR_ERR_UNSUPPORTED, "radiative transfer has fp64 kernels only (\"precision\" 32)");
    if (cfg->q != 0.0) return fail(GR_ERR_UNSUPPORTED, "radiative transfer along charged test particles (q != 0) is not built");
    if (cfg->count_windings) return fail(GR_ERR_UNSUPPORTED, "radiative transfer does not count windings (count_windings)");
    if (!(transfer->r_isco > 0.0)) return fail(GR_ERR_INVALID_ARGUMENT, "transfer->r_isco must be positive");
    return GR_OK;
}

// the caller's medium block into the next slot of the context's ring, ordered on `stream` before the kernel that reads it
int32_t stage_transfer(gr_ctx* ctx, const gr_transfer* transfer, hipStream_t stream, const gr_transfer** d_out)
{
    if (!ctx->d_transfer) GR_HIP(hipMalloc((void**)&ctx->d_transfer, sizeof(gr_transfer) * (size_t)ctx->queue_slots));
    gr_transfer* slot = ctx->d_transfer + ctx->transfer_next;
    ctx->transfer_next = (ctx->transfer_next + 1) % ctx->queue_slots;
    GR_HIP(hipMemcpyAsync(slot, transfer, sizeof(gr_transfer), hipMemcpyHostToDevice, stream));
    *d_out = slot;
    return GR_OK;
}

// rays given by (x, v) on the device: records to d_points, intensities to d_intensity
int32_t transfer_endpoints_device(gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer, const double* d_x, int64_t x_stride,
                                  const double* d_v, int64_t n, gr_point* d_points, double* d_intensity, gr_stats* d_stats, hipStream_t stream)
{
    int32_t rc;
    Params p;
    Cold cd;
    std::memset(&p, 0, sizeof p);
    std::memset(&cd, 0, sizeof cd);
    p.cfg = *cfg;
    p.n = n;
    p.stats = (unsigned long long*)d_stats;
    cd.src_mode = 1;
    cd.out_mode = 1;
    cd.x = d_x;
    cd.x_stride = x_stride;
    cd.v = d_v;
    cd.points = d_points;
    cd.intensity = d_intensity;
    cd.range = gr_range{ 0, n, n > 0 ? n : 1, 1 };
    cd.swizzle = 0;
    if (n == 0) return GR_OK;
    if ((rc = stage_transfer(ctx, transfer, stream, &cd.transfer)) != GR_OK) return rc;
    return launch_trace(ctx, p, cd, stream);
}
}  // namespace
}  // extern "C++"

int32_t gr_transfer_render_device(gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer, const gr_plane* plane,
                                  const gr_pointfunction* pf, const gr_range* range, double* d_image, gr_stats* d_stats, void* hip_stream)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = transfer_check(ctx, cfg, transfer)) != GR_OK) return rc;      // (first: what it refuses, it refuses as unsupported)
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if ((rc = validate_plane(plane, range)) != GR_OK) return rc;
    if (!pf) return fail(GR_ERR_INVALID_ARGUMENT, "point function is null");
    if (pf->pf_id != GR_PF_INTENSITY) return fail(GR_ERR_UNSUPPORTED, "a radiative-transfer render gives GR_PF_INTENSITY (pf_id " + std::to_string(pf->pf_id) + ")");
    if (pf->filter_id < GR_FILTER_NONE || pf->filter_id > GR_FILTER_INTERSECTED) return fail(GR_ERR_UNSUPPORTED, "unknown filter_id " + std::to_string(pf->filter_id));
    if (!d_image && range->count > 0) return fail(GR_ERR_INVALID_ARGUMENT, "image is null");
    GR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    Params p;
    Cold cd;
    plane_params(ctx, p, cd, cfg, plane, range);
    cd.pf.pf_id = pf->pf_id;
    cd.pf.filter_id = pf->filter_id;
    cd.pf.fill = pf->fill;
    cd.pf.r_isco = transfer->r_isco;
    cd.out_mode = 0;
    cd.image = d_image;
    p.stats = (unsigned long long*)d_stats;
    if (range->count == 0) return GR_OK;
    if ((rc = stage_transfer(ctx, transfer, stream, &cd.transfer)) != GR_OK) return rc;
    return launch_trace(ctx, p, cd, stream);
}

int32_t gr_transfer_render(gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer, const gr_plane* plane, const gr_pointfunction* pf,
                           const gr_range* range, double* image, gr_stats* stats)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!range) return fail(GR_ERR_INVALID_ARGUMENT, "range is null");
    if (!image && range->count > 0) return fail(GR_ERR_INVALID_ARGUMENT, "image is null");
    int32_t rc;
    // refusals come before the call's first device work (begin_host_call)
    if ((rc = transfer_check(ctx, cfg, transfer)) != GR_OK) return rc;      // (first: what it refuses, it refuses as unsupported)
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if ((rc = validate_plane(plane, range)) != GR_OK) return rc;
    if (!pf || pf->pf_id != GR_PF_INTENSITY) return fail(GR_ERR_UNSUPPORTED, "a radiative-transfer render gives GR_PF_INTENSITY");
    const size_t bytes = sizeof(double) * (size_t)(range->count > 0 ? range->count : 0);
    auto enq = [&](int) -> int32_t {
        int32_t r;
        GR_HIP(hipSetDevice(ctx->device));
        if ((r = ensure(&ctx->d_scratch, &ctx->scratch_bytes, bytes ? bytes : 8)) != GR_OK) return r;
        if ((r = begin_host_call(ctx, stats)) != GR_OK) return r;
        return gr_transfer_render_device(ctx, cfg, transfer, plane, pf, range, (double*)ctx->d_scratch, stats ? (gr_stats*)ctx->d_stats : nullptr, ctx->stream);
    };
    auto copy = [&](int) -> int32_t {
        if (bytes == 0) return GR_OK;
        GR_HIP(hipSetDevice(ctx->device));
        GR_HIP(hipMemcpyAsync(image, ctx->d_scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GR_OK;
    };
    return one_context(multi_drive(&ctx, 1, stats, enq, copy), stats);
}

int32_t gr_transfer_endpoints(gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer, const double* x, int64_t x_stride,
                              const double* v, int64_t n, gr_point* points, double* intensity, gr_stats* stats)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    int32_t rc;
    if ((rc = transfer_check(ctx, cfg, transfer)) != GR_OK) return rc;      // (first: what it refuses, it refuses as unsupported)
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (x_stride != 0 && x_stride != 4) return fail(GR_ERR_INVALID_ARGUMENT, "x_stride must be 0 or 4");
    if (n > 0 && (!x || !v || !points || !intensity)) return fail(GR_ERR_INVALID_ARGUMENT, "x/v/points/intensity is null");
    const size_t nx = (size_t)(x_stride == 0 ? 4 : 4 * n), nv = (size_t)(4 * n);
    const size_t rec_bytes = sizeof(gr_point) * (size_t)n, int_bytes = sizeof(double) * (size_t)n;
    auto enq = [&](int) -> int32_t {
        int32_t r;
        GR_HIP(hipSetDevice(ctx->device));
        // the records, then the intensities (152 n is a multiple of 8: the doubles behind them are aligned)
        if ((r = ensure(&ctx->d_scratch, &ctx->scratch_bytes, rec_bytes + int_bytes + 8)) != GR_OK) return r;
        if ((r = ensure(&ctx->d_in, &ctx->in_bytes, sizeof(double) * (nx + nv) + 8)) != GR_OK) return r;
        if ((r = begin_host_call(ctx, stats)) != GR_OK) return r;
        if (n == 0) return GR_OK;
        double* d_x = (double*)ctx->d_in;
        double* d_v = d_x + nx;
        GR_HIP(hipMemcpyAsync(d_x, x, sizeof(double) * nx, hipMemcpyHostToDevice, ctx->stream));
        GR_HIP(hipMemcpyAsync(d_v, v, sizeof(double) * nv, hipMemcpyHostToDevice, ctx->stream));
        return transfer_endpoints_device(ctx, cfg, transfer, d_x, x_stride, d_v, n, (gr_point*)ctx->d_scratch,
                                         (double*)((char*)ctx->d_scratch + rec_bytes), stats ? (gr_stats*)ctx->d_stats : nullptr, ctx->stream);
    };
    auto copy = [&](int) -> int32_t {
        if (n == 0) return GR_OK;
        GR_HIP(hipSetDevice(ctx->device));
        GR_HIP(hipMemcpyAsync(points, ctx->d_scratch, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
        GR_HIP(hipMemcpyAsync(intensity, (char*)ctx->d_scratch + rec_bytes, int_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return GR_OK;
    };
    return one_context(multi_drive(&ctx, 1, stats, enq, copy), stats);
}

extern "C++" {
namespace {
// context k's contiguous share of a ray set (host pointers); one context's share is the caller's set as it came -- tiled or
// blocked, with its own sky_first / sky_total: only sharing rays out needs them in ray order
int32_t rayset_share(const gr_rayset* rays, int32_t n, int k, gr_rayset& out, int64_t* off_out)
{
    if (!rays) return fail(GR_ERR_INVALID_ARGUMENT, "rayset is null");
    if (rays->n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "n must be non-negative");
    if (n == 1) {
        out = *rays;
        *off_out = 0;
        return GR_OK;
    }
    if (rays->sep_r && (rays->sep_block != 0 || rays->sep_tiled))
        return fail(GR_ERR_INVALID_ARGUMENT, "*_multi: a separable ray set with one output row per ray must come whole and in ray order "
                                             "(sep_block = 0, sep_tiled = 0)");
    int64_t off, cnt;
    contiguous_share(rays->n, n, k, &off, &cnt);
    out = *rays;
    out.n = cnt;
    if (rays->sky_sampler) {
        // a share of a source's samples: the sample numbers go on counting where the previous share stopped
        out.sky_total = rays->sky_total > 0 ? rays->sky_total : rays->n;
        out.sky_first = (rays->sky_total > 0 ? rays->sky_first : 0) + off;
        if (rays->sky_generator == 2) {
            if (rays->n > 0 && !rays->sky_i) return fail(GR_ERR_INVALID_ARGUMENT, "sky source: generator 2 needs sky_i");
            out.sky_i = rays->sky_i ? rays->sky_i + off : nullptr;
        }
        if (rays->sky_rows) out.sky_rows = rays->sky_rows + GR_SKY_ROW * off;
    } else if (rays->sep_r) {
        out.sep_first = rays->sep_first + off;
    } else if (rays->n > 0) {
        if (!rays->alpha || !rays->beta) return fail(GR_ERR_INVALID_ARGUMENT, "alpha/beta is null");
        out.alpha = rays->alpha + off;
        out.beta = rays->beta + off;
        out.area = rays->area ? rays->area + off : nullptr;
        out.height = rays->height ? rays->height + off : nullptr;
    }
    *off_out = off;
    return GR_OK;
}

// One output row of `row_bytes` per ray, for one context or several: context k stages its share of the rays,
// `launch(ctx, device rayset, d_out, d_stats)` queues the kernel, the rows go home with one contiguous copy.
template <class Launch>
int32_t rayset_rows(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, size_t row_bytes,
                          void* out, gr_stats* stats, Launch launch)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (!rays) return fail(GR_ERR_INVALID_ARGUMENT, "rayset is null");
    if (rays->n > 0 && !out) return fail(GR_ERR_INVALID_ARGUMENT, "output is null");
    if ((rc = sky_rows_in_table(cfg, rays)) != GR_OK) return rc;
    {
        gr_rayset probe;
        int64_t o;
        if ((rc = rayset_share(rays, n, 0, probe, &o)) != GR_OK) return rc;
    }
    const size_t total = row_bytes * (size_t)(rays->n > 0 ? rays->n : 0);
    const bool pinned = is_pinned(out, total);
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        gr_rayset share, dev;
        int64_t off;
        int32_t r;
        if ((r = rayset_share(rays, n, k, share, &off)) != GR_OK) return r;
        GR_HIP(hipSetDevice(c->device));
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        if ((r = stage_rays(c, &share, dev, 0, nullptr)) != GR_OK) return r;
        const size_t bytes = row_bytes * (size_t)share.n;
        if ((r = ensure(&c->d_scratch, &c->scratch_bytes, bytes ? bytes : 8)) != GR_OK) return r;
        if (share.n == 0) return GR_OK;
        return launch(c, &dev, c->d_scratch, stats ? (gr_stats*)c->d_stats : nullptr);
    };
    bool faulted = false;
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(rays->n, n, k, &off, &cnt);
        if (cnt == 0) return GR_OK;
        if (!faulted && !pinned) prefault_output(out, total, c->hugepages != 0);
        faulted = true;
        GR_HIP(hipSetDevice(c->device));
        GR_HIP(hipMemcpyAsync((char*)out + row_bytes * (size_t)off, c->d_scratch, row_bytes * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        return GR_OK;
    };
    return multi_drive(ctxs, n, stats, enq, copy);
}
}  // namespace
}  // extern "C++"

int32_t gr_rayset_endpoints_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, gr_point* points,
                                  gr_stats* stats)
{
    return rayset_rows(ctxs, n, cfg, rays, sizeof(gr_point), points, stats,
                       [&](gr_ctx* c, const gr_rayset* dev, void* d_out, gr_stats* d_st) {
                           return gr_rayset_endpoints_device(c, cfg, dev, (gr_point*)d_out, d_st, c->stream);
                       });
}

int32_t gr_rayset_endpoints(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, gr_point* points, gr_stats* stats)
{
    return one_context(gr_rayset_endpoints_multi(&ctx, 1, cfg, rays, points, stats), stats);
}

int32_t gr_ray_summary_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                             double* out, gr_stats* stats)
{
    return rayset_rows(ctxs, n, cfg, rays, sizeof(double) * 4, out, stats,
                       [&](gr_ctx* c, const gr_rayset* dev, void* d_out, gr_stats* d_st) {
                           return gr_ray_summary_device(c, cfg, dev, pf, (double*)d_out, d_st, c->stream);
                       });
}

int32_t gr_ray_summary(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                       double* out, gr_stats* stats)
{
    return one_context(gr_ray_summary_multi(&ctx, 1, cfg, rays, pf, out, stats), stats);
}

// (the two that refuse a source velocity per sample name the entry point the caller used)
static int32_t ray_tangent_on(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              double* out, gr_stats* stats, const char* who)
{
    int32_t rc;
    if ((rc = refuse_sky_rows(rays, who)) != GR_OK) return rc;
    return rayset_rows(ctxs, n, cfg, rays, sizeof(double) * 8, out, stats,
                       [&](gr_ctx* c, const gr_rayset* dev, void* d_out, gr_stats* d_st) {
                           return gr_ray_tangent_device(c, cfg, dev, pf, (double*)d_out, d_st, c->stream);
                       });
}

int32_t gr_ray_tangent(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                       double* out, gr_stats* stats)
{
    return one_context(ray_tangent_on(&ctx, 1, cfg, rays, pf, out, stats, "gr_ray_tangent"), stats);
}

int32_t gr_ray_tangent_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                             double* out, gr_stats* stats)
{
    return ray_tangent_on(ctxs, n, cfg, rays, pf, out, stats, "gr_ray_tangent_multi");
}

// ---- gr_offset_solve / gr_offset_search: host buffers; one context, or contiguous shares of the problems over several ----
extern "C++" {
namespace {
template <class Q>
int32_t offset_on(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, const Q* q,
                  double* out, gr_stats* stats)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    OffsetCall all;
    if ((rc = offset_call(q, all)) != GR_OK) return rc;
    for (int k = 0; k < n; ++k)
        if ((rc = offset_check(ctxs[k], cfg, rays, pf, all, out)) != GR_OK) return rc;
    const size_t row_bytes = sizeof(double) * (size_t)all.out_stride();
    const size_t total = row_bytes * (size_t)all.n;
    const bool pinned = is_pinned(out, total);
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(all.n, n, k, &off, &cnt);
        int32_t r;
        GR_HIP(hipSetDevice(c->device));
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        if (cnt == 0) return GR_OK;
        // r_target | a | b | sign | height, cnt each, in the context's input block; the results in its scratch block
        const size_t m = (size_t)cnt;
        if ((r = ensure(&c->d_in, &c->in_bytes, sizeof(double) * 5 * m)) != GR_OK) return r;
        if ((r = ensure(&c->d_scratch, &c->scratch_bytes, row_bytes * m)) != GR_OK) return r;
        double* base = (double*)c->d_in;
        OffsetCall share = all;
        share.n = cnt;
        const double* src[5] = { all.r_target, all.a, all.b, all.sign, all.height };
        const double** dst[5] = { &share.r_target, &share.a, &share.b, &share.sign, &share.height };
        for (int f = 0; f < 5; ++f) {
            if (!src[f]) continue;
            GR_HIP(hipMemcpyAsync(base + f * m, src[f] + off, sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
            *dst[f] = base + f * m;
        }
        // a search that ends early leaves its later records unwritten: NaN (all bits set) is what the caller finds there
        if (share.search) GR_HIP(hipMemsetAsync(c->d_scratch, 0xff, row_bytes * m, c->stream));
        return offset_launch(c, cfg, rays, pf, share, (double*)c->d_scratch, stats ? (gr_stats*)c->d_stats : nullptr, c->stream);
    };
    bool faulted = false;
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(all.n, n, k, &off, &cnt);
        if (cnt == 0) return GR_OK;
        if (!faulted && !pinned) prefault_output(out, total, c->hugepages != 0);
        faulted = true;
        GR_HIP(hipSetDevice(c->device));
        GR_HIP(hipMemcpyAsync((char*)out + row_bytes * (size_t)off, c->d_scratch, row_bytes * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        return GR_OK;
    };
    return multi_drive(ctxs, n, stats, enq, copy);
}
}  // namespace
}  // extern "C++"

int32_t gr_offset_solve_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              const gr_offset_problems* problems, double* out, gr_stats* stats)
{
    return offset_on(ctxs, n, cfg, rays, pf, problems, out, stats);
}

int32_t gr_offset_solve(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                        const gr_offset_problems* problems, double* out, gr_stats* stats)
{
    return one_context(offset_on(&ctx, 1, cfg, rays, pf, problems, out, stats), stats);
}

int32_t gr_offset_search_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                               const gr_offset_searches* searches, double* out, gr_stats* stats)
{
    return offset_on(ctxs, n, cfg, rays, pf, searches, out, stats);
}

int32_t gr_offset_search(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                         const gr_offset_searches* searches, double* out, gr_stats* stats)
{
    return one_context(offset_on(&ctx, 1, cfg, rays, pf, searches, out, stats), stats);
}

static int32_t redshift_radius_on(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                                  double r_min, double r_max, double* pairs, gr_stats* stats, const char* who)
{
    int32_t rc;
    if ((rc = refuse_sky_rows(rays, who)) != GR_OK) return rc;
    return rayset_rows(ctxs, n, cfg, rays, sizeof(double) * 2, pairs, stats,
                       [&](gr_ctx* c, const gr_rayset* dev, void* d_out, gr_stats* d_st) {
                           return gr_redshift_radius_device(c, cfg, dev, pf, r_min, r_max, (double*)d_out, d_st, c->stream);
                       });
}

int32_t gr_redshift_radius(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                           double r_min, double r_max, double* pairs, gr_stats* stats)
{
    return one_context(redshift_radius_on(&ctx, 1, cfg, rays, pf, r_min, r_max, pairs, stats, "gr_redshift_radius"), stats);
}

int32_t gr_redshift_radius_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                                 const gr_pointfunction* pf, double r_min, double r_max, double* pairs, gr_stats* stats)
{
    return redshift_radius_on(ctxs, n, cfg, rays, pf, r_min, r_max, pairs, stats, "gr_redshift_radius_multi");
}

// One histogram per context, added on the host.  The two entry points differ in the deal alone: gr_lineprofile takes the set as
// it is given (a shard of gradus.jl_amd/distributed.py comes with its own sep_block / sep_stride), gr_lineprofile_multi deals a
// separable plane in strips itself.
static int32_t lineprofile_on(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              const gr_binning* b, double* flux, gr_stats* stats, bool multi)
{
    const char* who = multi ? "gr_lineprofile_multi" : "gr_lineprofile";
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    if ((rc = validate_cfg(cfg)) != GR_OK) return rc;
    if (!rays) return fail(GR_ERR_INVALID_ARGUMENT, "rayset is null");
    if ((rc = refuse_sky_rows(rays, who)) != GR_OK) return rc;
    if (!b || b->n_bins < 1 || !b->bin_edges || !flux) return fail(GR_ERR_INVALID_ARGUMENT, "binning/flux is null or empty");
    if (multi && rays->sep_r && rays->sep_block != 0)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_lineprofile_multi: a separable ray set must come whole (sep_block = 0): the call deals it itself");
    const size_t nb = (size_t)b->n_bins;
    const size_t ne = (b->eps_n >= 2 && b->eps_r && b->eps_v) ? (size_t)b->eps_n : 0;
    // the deal of a separable plane: blocks of one strip of 8 x 8 tiles (all radii of 8 neighbouring angles) in the set's
    // visiting order, block k, k + n, ... to context k -- every context sees every radius and an even sample of the angles
    // (gradus.jl_amd/distributed.py: ray_shard does the same across processes)
    const int64_t N = rays->n;
    int64_t sep_blk = 0;
    if (rays->sep_r) {
        const int64_t nr = rays->sep_nr, nt = rays->sep_nt;
        sep_blk = (nr >= 8 && nt >= 8) ? 8 * ((nr / 8) * 8) : std::max<int64_t>(64, (N + (int64_t)n * 8 - 1) / ((int64_t)n * 8));
    }
    std::vector<double> part;
    try {
        part.assign(nb * (size_t)n, 0.0);
    } catch (...) {
        return fail(GR_ERR_OUT_OF_MEMORY, std::string(who) + ": partial histograms");
    }
    auto share_of = [&](int k, gr_rayset& sh) -> int32_t {
        if (!multi || !rays->sep_r) {
            int64_t off;
            return rayset_share(rays, n, k, sh, &off);
        }
        sh = *rays;
        const int64_t blocks = (N + sep_blk - 1) / sep_blk;
        const int64_t mine = k < blocks ? (blocks - 1 - k) / n + 1 : 0;
        int64_t cnt = 0;
        if (mine > 0) {
            const int64_t last = k + (mine - 1) * n;
            cnt = (mine - 1) * sep_blk + std::min<int64_t>(sep_blk, N - last * sep_blk);
        }
        sh.n = cnt;
        sh.sep_first = rays->sep_first + (int64_t)k * sep_blk;
        sh.sep_block = sep_blk;
        sh.sep_stride = (int64_t)n * sep_blk;
        return GR_OK;
    };
    std::vector<double*> d_part((size_t)n, nullptr);
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        gr_rayset sh, dev;
        int32_t r;
        if ((r = share_of(k, sh)) != GR_OK) return r;
        GR_HIP(hipSetDevice(c->device));
        void* extra = nullptr;
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        if ((r = stage_rays(c, &sh, dev, sizeof(double) * (2 * nb + 2 * ne), &extra)) != GR_OK) return r;
        double* d_edges = (double*)extra;
        double* d_flux = d_edges + nb;
        GR_HIP(hipMemcpyAsync(d_edges, b->bin_edges, sizeof(double) * nb, hipMemcpyHostToDevice, c->stream));
        gr_binning db = *b;
        db.bin_edges = d_edges;
        if (ne) {
            double* d_er = d_flux + nb;
            GR_HIP(hipMemcpyAsync(d_er, b->eps_r, sizeof(double) * ne, hipMemcpyHostToDevice, c->stream));
            GR_HIP(hipMemcpyAsync(d_er + ne, b->eps_v, sizeof(double) * ne, hipMemcpyHostToDevice, c->stream));
            db.eps_r = d_er;
            db.eps_v = d_er + ne;
        }
        d_part[(size_t)k] = d_flux;
        // (a context without rays still zeroes its histogram: gr_lineprofile_device does so before it looks at n)
        return gr_lineprofile_device(c, cfg, &dev, pf, &db, d_flux, stats ? (gr_stats*)c->d_stats : nullptr, c->stream);
    };
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        GR_HIP(hipSetDevice(c->device));
        GR_HIP(hipMemcpyAsync(part.data() + nb * (size_t)k, d_part[(size_t)k], sizeof(double) * nb, hipMemcpyDeviceToHost, c->stream));
        return GR_OK;
    };
    if ((rc = multi_drive(ctxs, n, stats, enq, copy)) != GR_OK) return rc;
    for (size_t i = 0; i < nb; ++i) {
        double sum = 0.0;
        for (int k = 0; k < n; ++k) sum += part[nb * (size_t)k + i];     // context order: the same bytes run after run
        flux[i] = sum;
    }
    return GR_OK;
}

int32_t gr_lineprofile(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                       const gr_binning* b, double* flux, gr_stats* stats)
{
    return one_context(lineprofile_on(&ctx, 1, cfg, rays, pf, b, flux, stats, false), stats);
}

int32_t gr_lineprofile_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                             const gr_binning* b, double* flux, gr_stats* stats)
{
    return lineprofile_on(ctxs, n, cfg, rays, pf, b, flux, stats, true);
}

}  // extern "C"

// ---- gr_sky_cells: host buffers; one context, or contiguous shares of the cells over several ----

extern "C++" {
namespace {
// cells [off, off + cnt) of a host cell set -> the context's input buffer; `dev` receives the device pointers
int32_t stage_skycells(gr_ctx* c, const gr_skycells* cells, int64_t off, int64_t cnt, gr_skycells& dev)
{
    int32_t rc;
    if ((rc = ensure(&c->d_in, &c->in_bytes, sizeof(double) * 2 * (size_t)cnt + 64)) != GR_OK) return rc;
    double* b = (double*)c->d_in;
    dev = *cells;
    dev.n = cnt;
    dev.cos_theta = b;
    dev.phi = b + cnt;
    if (cnt > 0) {
        GR_HIP(hipMemcpyAsync(b, cells->cos_theta + off, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
        GR_HIP(hipMemcpyAsync(b + cnt, cells->phi + off, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
    }
    return GR_OK;
}
}  // namespace
}  // extern "C++"

int32_t gr_sky_cells_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_skycells* cells, const gr_pointfunction* pf,
                           double* out, gr_stats* stats)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n)) != GR_OK) return rc;
    if (n > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    if ((rc = skycells_check(cfg, cells, pf, true)) != GR_OK) return rc;
    if (cells->n > 0 && !out) return fail(GR_ERR_INVALID_ARGUMENT, "out is null");
    const size_t row_bytes = sizeof(double) * GR_SKYCELL_ROW;
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(cells->n, n, k, &off, &cnt);
        int32_t r;
        GR_HIP(hipSetDevice(c->device));
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        gr_skycells dev;
        if ((r = stage_skycells(c, cells, off, cnt, dev)) != GR_OK) return r;
        if ((r = ensure(&c->d_scratch, &c->scratch_bytes, cnt ? row_bytes * (size_t)cnt : 8)) != GR_OK) return r;
        if (cnt == 0) return GR_OK;
        return gr_sky_cells_device(c, cfg, &dev, pf, (double*)c->d_scratch, stats ? (gr_stats*)c->d_stats : nullptr, c->stream);
    };
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(cells->n, n, k, &off, &cnt);
        if (cnt == 0) return GR_OK;
        GR_HIP(hipSetDevice(c->device));
        GR_HIP(hipMemcpyAsync((char*)out + row_bytes * (size_t)off, c->d_scratch, row_bytes * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        return GR_OK;
    };
    return multi_drive(ctxs, n, stats, enq, copy);
}

int32_t gr_sky_cells(gr_ctx* ctx, const gr_config* cfg, const gr_skycells* cells, const gr_pointfunction* pf, double* out,
                     gr_stats* stats)
{
    return one_context(gr_sky_cells_multi(&ctx, 1, cfg, cells, pf, out, stats), stats);
}

// ---- gr_plane_cells: host buffers, as gr_sky_cells ----

extern "C++" {
namespace {
// cells [off, off + cnt) of host (α, β) arrays -> the context's input buffer
int32_t stage_planecells(gr_ctx* c, const double* alpha, const double* beta, int64_t off, int64_t cnt)
{
    int32_t rc;
    if ((rc = ensure(&c->d_in, &c->in_bytes, sizeof(double) * 2 * (size_t)cnt + 64)) != GR_OK) return rc;
    if ((rc = ensure(&c->d_scratch, &c->scratch_bytes, cnt ? sizeof(gr_point) * (size_t)cnt : 8)) != GR_OK) return rc;
    double* b = (double*)c->d_in;
    if (cnt > 0) {
        GR_HIP(hipMemcpyAsync(b, alpha + off, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
        GR_HIP(hipMemcpyAsync(b + cnt, beta + off, sizeof(double) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
    }
    return GR_OK;
}
}  // namespace
}  // extern "C++"

int32_t gr_plane_cells_multi(gr_ctx* const* ctxs, int32_t n_ctx, const gr_config* cfg, const gr_plane* plane, const double* alpha,
                             const double* beta, int64_t n, gr_point* out, gr_stats* stats)
{
    int32_t rc;
    if ((rc = validate_ctxs(ctxs, n_ctx)) != GR_OK) return rc;
    if (n_ctx > 64) return fail(GR_ERR_INVALID_ARGUMENT, "at most 64 contexts");
    if ((rc = planecells_check(cfg, plane)) != GR_OK) return rc;
    if ((rc = planecells_args(alpha, beta, n, out)) != GR_OK) return rc;
    auto enq = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(n, n_ctx, k, &off, &cnt);
        int32_t r;
        GR_HIP(hipSetDevice(c->device));
        if ((r = begin_host_call(c, stats ? &stats[k] : nullptr)) != GR_OK) return r;
        if ((r = stage_planecells(c, alpha, beta, off, cnt)) != GR_OK) return r;
        if (cnt == 0) return GR_OK;
        const double* b = (const double*)c->d_in;
        return gr_plane_cells_device(c, cfg, plane, b, b + cnt, cnt, (gr_point*)c->d_scratch, stats ? (gr_stats*)c->d_stats : nullptr, c->stream);
    };
    auto copy = [&](int k) -> int32_t {
        gr_ctx* c = ctxs[k];
        int64_t off, cnt;
        contiguous_share(n, n_ctx, k, &off, &cnt);
        if (cnt == 0) return GR_OK;
        GR_HIP(hipSetDevice(c->device));
        GR_HIP(hipMemcpyAsync(out + off, c->d_scratch, sizeof(gr_point) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        return GR_OK;
    };
    return multi_drive(ctxs, n_ctx, stats, enq, copy);
}

int32_t gr_plane_cells(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const double* alpha, const double* beta, int64_t n, gr_point* out,
                       gr_stats* stats)
{
    return one_context(gr_plane_cells_multi(&ctx, 1, cfg, plane, alpha, beta, n, out, stats), stats);
}

// ---- an adaptive sky resident on the device: gr_sky_* (AdaptiveSky, adaptive-sky.jl; the drivers of adaptive-sample.jl:486-842) ----
// The tree (the arrays of grids.AdaptiveGrid) and the rows stay in device memory between refinement steps; the pair search,
// the refinement and the census of the (r, ϕ) bins are the kernels below around the functions of gr_skygrid.hpp, and the new
// cells of a step go to ONE gr_sky_cells_device launch.  What crosses the link per step is a count.

struct gr_sky {
    gr_ctx* ctx = nullptr;
    gr_config cfg;
    gr_pointfunction pf;
    gr_skycells src;                       // x_src, Mx
    gr_plane pl;                           // a plane sky's x_obs, Mx (gr_sky_create_plane)
    bool plane = false;                    // the rows are gr_points, the cells traced by gr_plane_cells_device
    int row = 6;                           // doubles per row: 6 (t, r, ϕ, g, J, status), or 19 (a gr_point)
    double lim[4] = { 0, 0, 0, 0 };
    int64_t n = 0, cap = 0;                // cells; rows the arrays below hold (cap >= n + 1)
    double* d_pos = nullptr;
    int32_t* d_level = nullptr;
    int64_t* d_children = nullptr;
    int64_t* d_neighbours = nullptr;
    int64_t* d_parent = nullptr;
    int8_t* d_location = nullptr;
    double* d_rows = nullptr;
    // work buffers of cap elements (off: cap + 1), not kept across a growth
    uint8_t* d_mark = nullptr;
    uint32_t* d_cnt = nullptr;
    int64_t* d_off = nullptr;
    int64_t* d_part = nullptr;             // SKY_SCAN_BLOCKS + 1 partial sums, then the refusal flag
    void* d_need = nullptr;                // the list of the last find_need_refine / a host list
    size_t need_bytes = 0;
    int64_t need_n = -1;                   // -1: no list
    void* d_ang = nullptr;                 // (cos θ, ϕ) -- a plane's (α, β) -- of the cells of a launch, then their rows
    size_t ang_bytes = 0;
    void* d_tmp = nullptr;                 // pairs, bin edges and counts, downloads
    size_t tmp_bytes = 0;
    bool traced = false;
};

namespace {

constexpr int SKY_SCAN_BLOCKS = 1024;
constexpr int64_t SKY_MAX_GRID = 2048;     // blocks of a grid-stride launch (256 CUs x 8)

std::mutex g_sky_mutex;
std::vector<gr_sky*> g_skies;              // the skies alive: gr_sky_destroy after the context went is a no-op

gr_skygrid::Grid sky_grid(const gr_sky* s)
{
    gr_skygrid::Grid g;
    g.pos = s->d_pos;
    g.level = s->d_level;
    g.children = s->d_children;
    g.neighbours = s->d_neighbours;
    g.parent = s->d_parent;
    g.location = s->d_location;
    g.n = s->n;
    g.x1 = s->lim[0];
    g.x2 = s->lim[1];
    g.y1 = s->lim[2];
    g.y2 = s->lim[3];
    return g;
}

unsigned sky_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, SKY_MAX_GRID)); }

// ---- an exclusive scan of n counts into n + 1 offsets (off[n] = the sum): block b owns the elements [b per, (b + 1) per) ----
template <class T>
__global__ void __launch_bounds__(256) k_sky_scan_partial(const T* __restrict__ v, int64_t n, int64_t per, int64_t* __restrict__ part)
{
    __shared__ int64_t s[256];
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    int64_t acc = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) acc += (int64_t)v[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}
// part[0 .. nb) -> their exclusive scan, part[nb] = the sum (one block; nb <= SKY_SCAN_BLOCKS)
__global__ void __launch_bounds__(256) k_sky_scan_parts(int64_t* part, int nb)
{
    __shared__ int64_t s[SKY_SCAN_BLOCKS + 1];
    for (int i = threadIdx.x; i < nb; i += 256) s[i] = part[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int i = 0; i < nb; ++i) {
            const int64_t x = s[i];
            s[i] = acc;
            acc += x;
        }
        s[nb] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= nb; i += 256) part[i] = s[i];
}
template <class T>
__global__ void __launch_bounds__(256) k_sky_scan_apply(const T* __restrict__ v, int64_t n, int64_t per, const int64_t* __restrict__ part,
                                                        int64_t* __restrict__ off)
{
    __shared__ int64_t s[256];
    __shared__ int64_t base;
    const int tid = threadIdx.x;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    if (tid == 0) base = part[blockIdx.x];
    __syncthreads();
    for (int64_t t = lo; t < hi; t += 256) {       // (uniform over the block)
        const int64_t i = t + tid;
        const int64_t x = i < hi ? (int64_t)v[i] : 0;
        s[tid] = x;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t y = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += y;
            __syncthreads();
        }
        const int64_t incl = s[tid], b = base;
        if (i < hi) off[i] = b + incl - x;
        __syncthreads();
        if (tid == 255) base = b + incl;
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) off[n] = part[gridDim.x];
}

// off[0 .. n] = the exclusive scan of v[0 .. n); three launches, nothing allocated, no wait
template <class T>
int32_t sky_scan(gr_sky* s, const T* v, int64_t n, hipStream_t stream)
{
    int64_t nb = std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, SKY_SCAN_BLOCKS));
    int64_t per = ((n + nb - 1) / nb + 255) / 256 * 256;
    if (per < 256) per = 256;
    nb = std::max<int64_t>(1, (n + per - 1) / per);
    hipLaunchKernelGGL(k_sky_scan_partial<T>, dim3((unsigned)nb), dim3(256), 0, stream, v, n, per, s->d_part);
    hipLaunchKernelGGL(k_sky_scan_parts, dim3(1), dim3(256), 0, stream, s->d_part, (int)nb);
    hipLaunchKernelGGL(k_sky_scan_apply<T>, dim3((unsigned)nb), dim3(256), 0, stream, v, n, per, (const int64_t*)s->d_part, s->d_off);
    GR_HIP(hipGetLastError());
    return GR_OK;
}

// list[off[c]] = c for every marked cell: the marked cells, ascending (np.unique(i2[need]))
__global__ void __launch_bounds__(256) k_sky_compact(const uint8_t* __restrict__ mark, const int64_t* __restrict__ off, int64_t n_rows,
                                                     int64_t* __restrict__ list)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_rows; c += (int64_t)gridDim.x * 256)
        if (mark[c]) list[off[c]] = c;
}

__global__ void __launch_bounds__(256) k_sky_mark_leaves(const gr_skygrid::Grid g, uint8_t* __restrict__ mark)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= g.n; c += (int64_t)gridDim.x * 256)
        mark[c] = (c >= 1 && gr_skygrid::is_leaf(g, c)) ? 1 : 0;
}

// find_need_refine: one work-item per leaf walks its bordering leaves; a pair the criterion names marks the BORDERING cell with
// a plain byte store of 1 (idempotent: no atomics, no order).  flag: a walk that ran out of stack.
__global__ void __launch_bounds__(256) k_sky_mark_need(const gr_skygrid::Grid g, const double* __restrict__ rows, const gr_sky_criterion cr,
                                                       uint8_t* mark, int32_t* flag)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; c <= g.n; c += (int64_t)gridDim.x * 256) {
        if (!gr_skygrid::is_leaf(g, c)) continue;
        const int k = gr_skygrid::walk_bordering(g, c, [&](int64_t other) {
            if (gr_skygrid::need_refine(cr, g, rows, c, other)) mark[other] = 1;
        });
        if (k < 0) *flag = 5;
    }
}

// ... on a plane sky: the rows are gr_points, the criterion is gr_planegrid::need_refine
__global__ void __launch_bounds__(256) k_plane_mark_need(const gr_skygrid::Grid g, const gr_point* __restrict__ pts, const gr_sky_criterion cr,
                                                         uint8_t* mark, int32_t* flag)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; c <= g.n; c += (int64_t)gridDim.x * 256) {
        if (!gr_skygrid::is_leaf(g, c)) continue;
        const int k = gr_skygrid::walk_bordering(g, c, [&](int64_t other) {
            if (gr_planegrid::need_refine(cr, g, pts, c, other)) mark[other] = 1;
        });
        if (k < 0) *flag = 5;
    }
}

// bordering_pairs: the count pass and the fill pass
__global__ void __launch_bounds__(256) k_sky_pair_count(const gr_skygrid::Grid g, uint32_t* __restrict__ cnt, int32_t* flag)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= g.n; c += (int64_t)gridDim.x * 256) {
        int k = 0;
        if (c >= 1 && gr_skygrid::is_leaf(g, c)) k = gr_skygrid::walk_bordering(g, c, [](int64_t) {});
        if (k < 0) {
            *flag = 5;
            k = 0;
        }
        cnt[c] = (uint32_t)k;
    }
}
__global__ void __launch_bounds__(256) k_sky_pair_fill(const gr_skygrid::Grid g, const int64_t* __restrict__ off, int64_t total,
                                                       int64_t* __restrict__ i1, int64_t* __restrict__ i2)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; c <= g.n; c += (int64_t)gridDim.x * 256) {
        if (!gr_skygrid::is_leaf(g, c)) continue;
        int64_t at = off[c];
        const int64_t end = off[c + 1];
        (void)gr_skygrid::walk_bordering(g, c, [&](int64_t other) {
            if (at < end && at < total) {
                i1[at] = c;
                i2[at] = other;
            }
            ++at;
        });
    }
}

// what refine_many raises on: seen[c] counts how often the list names c (an integer atomic: the old value tells a second naming)
__global__ void __launch_bounds__(256) k_sky_refusals(const gr_skygrid::Grid g, const int64_t* __restrict__ list, int64_t m, uint32_t* seen,
                                                      int32_t* flag)
{
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < m; k += (int64_t)gridDim.x * 256) {
        const int64_t c = list[k];
        int why = gr_skygrid::refine_refusal(g, c);
        if (why == 0 && atomicAdd(&seen[c], 1u) != 0u) why = 4;
        if (why != 0) atomicMax(flag, why);
    }
}

// refine_many on the device: work-item 9 k + c writes child c of the k-th cell of the list into row first + 9 k + c; the middle
// child takes its parent's row (ROW doubles: 6, or the 19 of a plane's whole gr_point), the eight others leave (cos θ, ϕ) for the
// launch, in child order per parent
template <int ROW>
__global__ void __launch_bounds__(256) k_sky_children(const gr_skygrid::Grid g, const int64_t* __restrict__ list, int64_t m, double* rows,
                                                      double* __restrict__ cos_theta, double* __restrict__ phi)
{
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < 9 * m; w += (int64_t)gridDim.x * 256) {
        const int64_t k = w / 9;
        const int c = (int)(w - 9 * k);
        const int64_t cell = list[k], first = g.n + 1 + 9 * k, row = first + c;
        gr_skygrid::write_child(g, cell, first, c);
        if (c == 4) {
            for (int q = 0; q < ROW; ++q) rows[ROW * row + q] = rows[ROW * cell + q];
        } else {
            const int64_t j = 8 * k + (c < 4 ? c : c - 1);
            cos_theta[j] = g.pos[2 * row];
            phi[j] = g.pos[2 * row + 1];
        }
    }
}
// the rows of the launch into the children's slots
template <int ROW>
__global__ void __launch_bounds__(256) k_sky_scatter(const double* __restrict__ traced, int64_t m, int64_t first, double* __restrict__ rows)
{
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < 8 * m; w += (int64_t)gridDim.x * 256) {
        const int64_t k = w / 8;
        const int j = (int)(w - 8 * k);
        const int64_t row = first + 9 * k + (j < 4 ? j : j + 1);
        for (int q = 0; q < ROW; ++q) rows[ROW * row + q] = traced[ROW * w + q];
    }
}
__global__ void __launch_bounds__(256) k_sky_positions(const double* __restrict__ pos, int64_t first, int64_t m, double* __restrict__ cos_theta,
                                                       double* __restrict__ phi)
{
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += (int64_t)gridDim.x * 256) {
        cos_theta[j] = pos[2 * (first + j)];
        phi[j] = pos[2 * (first + j) + 1];
    }
}

// the census of the (r, ϕ) bins: integer atomics, so the counts do not depend on the order
__global__ void __launch_bounds__(256) k_sky_occupancy(const gr_skygrid::Grid g, const double* __restrict__ rows, const double* __restrict__ r_bins,
                                                       int64_t nr, double r_max, const double* __restrict__ phi_bins, int64_t nphi, int has_gamma,
                                                       double gamma, unsigned int* counts)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; c <= g.n; c += (int64_t)gridDim.x * 256) {
        if (!gr_skygrid::is_leaf(g, c)) continue;
        int64_t ri, pi;
        if (!gr_skygrid::bin_of(rows + 6 * c, r_bins, nr, r_max, phi_bins, nphi, ri, pi)) continue;
        if (gr_skygrid::lights(rows + 6 * c, has_gamma != 0, gamma)) atomicAdd(&counts[ri * nphi + pi], 1u);
    }
}

// ---- the (r, ϕ) maps: gr_sky_bin_grid.  The arithmetic per leaf is gr_skygrid.hpp (map_term), the sums are the two-integer
// fixed-point sums of gr_lagbin.hpp: integer atomics, so a map is the same bits on every run and for every grid size ----

// r of every cell, contiguous and indexed by cell, for the γA launch (k_disc_area_factor).  Indexing by cell keeps a compaction
// (a scan and a wait) out of the call; row 0 and the interior cells are given NaN, which the launch passes through without
// evaluating the metric, as it does the leaves that missed the disc.
__global__ void __launch_bounds__(256) k_sky_radii(const gr_skygrid::Grid g, const double* __restrict__ rows, double* __restrict__ r)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= g.n; c += (int64_t)gridDim.x * 256)
        r[c] = (c >= 1 && gr_skygrid::is_leaf(g, c)) ? rows[6 * c + 1] : NAN;
}

// red[0] = max |ΔΩ w|, red[1] = max ΔΩ over the leaves that land in a bin, as the bits of non-negative doubles (a NaN or an
// infinite value adds nothing).  Per-wave reduction, then one pair of atomics per workgroup (k_lag_extrema).
__global__ void __launch_bounds__(256) k_sky_map_extrema(const gr_skygrid::Grid g, const double* __restrict__ rows, const gr_skygrid::MapBins b, int what,
                                                         int has_gamma, double gamma, const double* __restrict__ area, unsigned long long* red)
{
    unsigned long long mt = 0ull, ms = 0ull;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; c <= g.n; c += (int64_t)gridDim.x * 256) {
        if (!gr_skygrid::is_leaf(g, c)) continue;
        int64_t bin;
        double solid, term;
        if (!gr_skygrid::map_term(g, rows, c, b, what, has_gamma != 0, gamma, area, bin, solid, term)) continue;
        const double at = fabs(term), as = fabs(solid);
        const unsigned long long bt = at < INFINITY ? (unsigned long long)__double_as_longlong(at) : 0ull;
        const unsigned long long bs = as < INFINITY ? (unsigned long long)__double_as_longlong(as) : 0ull;
        mt = bt > mt ? bt : mt;
        ms = bs > ms ? bs : ms;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long t2 = __shfl_down(mt, off, 64), s2 = __shfl_down(ms, off, 64);
        mt = t2 > mt ? t2 : mt;
        ms = s2 > ms ? s2 : ms;
    }
    __shared__ unsigned long long part[4][2];
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = mt;
        part[threadIdx.x >> 6][1] = ms;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            mt = part[k][0] > mt ? part[k][0] : mt;
            ms = part[k][1] > ms ? part[k][1] : ms;
        }
        if (mt) atomicMax(red, mt);
        if (ms) atomicMax(red + 1, ms);
    }
}

// Every kept leaf's share of its bin (gr_skygrid::map_accumulate): acc 4 x cells integers, cnt the non-zero finite terms per bin,
// flag 4 x cells bytes set by plain stores of 1 (the idiom of k_sky_mark_need)
__global__ void __launch_bounds__(256) k_sky_map_bin(const gr_skygrid::Grid g, const double* __restrict__ rows, const gr_skygrid::MapBins b, int what,
                                                     int has_gamma, double gamma, const double* __restrict__ area, gr_lag::CoronaScale st, gr_lag::CoronaScale ss,
                                                     int64_t cells, unsigned long long* acc, unsigned int* cnt, uint8_t* flag)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x + 1; c <= g.n; c += (int64_t)gridDim.x * 256) {
        if (!gr_skygrid::is_leaf(g, c)) continue;
        int64_t bin;
        double solid, term;
        if (!gr_skygrid::map_term(g, rows, c, b, what, has_gamma != 0, gamma, area, bin, solid, term)) continue;
        if (bin < 0 || bin >= cells) continue;
        gr_skygrid::map_accumulate(bin, solid, term, cells, st, ss, flag,
                                   [&](int64_t at, long long v) { atomicAdd(acc + at, (unsigned long long)v); },
                                   [&](int64_t at) { atomicAdd(cnt + at, 1u); });
    }
}

// ---- the filled image: gr_sky_fill.  One workgroup per column ϕ_k: the cell of every point (cos θ_j, ϕ_k) into a scratch column,
// the first point of every run of one cell compacted (two block scans that carry across chunks of 256 points, as k_sky_scan_apply
// does: the last non-zero cell before a point, then the number of first points before it), then every point searches the
// compacted column.  A fixed-ϕ line meets the disjoint rectangles of the leaves in contiguous runs, ordered in cos θ, so the
// compacted column IS the sorted set of the reference; the kernel checks that its θ ascend strictly and raises `flag` if not. ----
__global__ void __launch_bounds__(256) k_sky_fill(const gr_skygrid::Grid g, const double* __restrict__ rows, const double* __restrict__ phi,
                                                  const double* __restrict__ theta, const double* __restrict__ cos_theta, int64_t n_theta,
                                                  int64_t n_phi, const int64_t* __restrict__ perm, int64_t* idx_all, int64_t* comp_all, double* col_all,
                                                  double* out, int64_t* cells_out, int32_t* flag)
{
    __shared__ int64_t s[256];
    __shared__ int64_t carry_cell, carry_count;
    const int tid = threadIdx.x;
    for (int64_t k = blockIdx.x; k < n_phi; k += gridDim.x) {      // (uniform over the block)
        int64_t* idx = idx_all + k * n_theta;
        int64_t* comp = comp_all + k * n_theta;
        double* col = col_all + k * n_theta;
        const double ph = phi[k];
        for (int64_t j = tid; j < n_theta; j += 256) idx[j] = gr_skygrid::parent_index(g, cos_theta[j], ph);
        if (tid == 0) {
            carry_cell = 0;
            carry_count = 0;
        }
        __syncthreads();
        for (int64_t t = 0; t < n_theta; t += 256) {
            const int64_t j = t + tid;
            const int64_t c = j < n_theta ? idx[j] : 0;
            s[tid] = c;
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {
                const int64_t y = tid >= d ? s[tid - d] : 0;
                __syncthreads();
                s[tid] = gr_skygrid::last_nonzero(y, s[tid]);
                __syncthreads();
            }
            const int64_t last = s[tid];
            const int64_t before = gr_skygrid::last_nonzero(carry_cell, tid > 0 ? s[tid - 1] : 0);
            const int64_t first = gr_skygrid::first_of_run(c, before) ? 1 : 0;
            const int64_t base = carry_count;
            __syncthreads();
            s[tid] = first;
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {
                const int64_t y = tid >= d ? s[tid - d] : 0;
                __syncthreads();
                s[tid] += y;
                __syncthreads();
            }
            const int64_t incl = s[tid];
            if (first) {
                const int64_t at = base + incl - 1;      // (at < n_theta: at most one first point per point)
                comp[at] = c;
                col[at] = acos(g.pos[2 * c]);
            }
            __syncthreads();
            if (tid == 255) {
                carry_cell = gr_skygrid::last_nonzero(carry_cell, last);
                carry_count = base + incl;
            }
            __syncthreads();
        }
        const int64_t m = carry_count;
        for (int64_t q = tid; q + 1 < m; q += 256)
            if (!(col[q] < col[q + 1])) *flag = 1;
        for (int64_t j = tid; j < n_theta; j += 256) {
            const int64_t at = perm[j] * n_phi + k;      // θ ascends along j (gr_skygrid::theta_order); the point is the caller's perm[j]
            double* o = out + 6 * at;
            int64_t lower = 0, upper = 0;
            if (m < 2) {
                for (int q = 0; q < 6; ++q) o[q] = NAN;
            } else {
                gr_skygrid::fill_point(col, comp, m, rows, theta[j], o, lower, upper);
            }
            cells_out[2 * at] = lower;
            cells_out[2 * at + 1] = upper;
        }
        __syncthreads();      // (the carries are reset for the next column)
    }
}

// ---- the filled image of a plane sky: gr_sky_fill_plane (adaptive-plane.jl:100-181; the arithmetic is gr_planegrid.hpp).  Three
// passes: the cell of every point (x_k, y_j), one work-item per point; the cells a column meets and their values interpolated
// across α, one work-item per column (a serial walk over the column's cell indices: integer compares); every point between two
// cells of its column, one work-item per point. ----
__global__ void __launch_bounds__(256) k_plane_default_values(const gr_point* __restrict__ pts, int64_t n_rows, double* __restrict__ val)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_rows; c += (int64_t)gridDim.x * 256) val[c] = pts[c].x[0];
}
// idx[k n_y + j]: y ascends along j (gr_skygrid::theta_order)
__global__ void __launch_bounds__(256) k_plane_fill_locate(const gr_skygrid::Grid g, const double* __restrict__ x, int64_t n_x,
                                                           const double* __restrict__ y, int64_t n_y, int64_t* __restrict__ idx)
{
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n_x * n_y; w += (int64_t)gridDim.x * 256) {
        const int64_t k = w / n_y, j = w - k * n_y;
        idx[w] = gr_skygrid::parent_index(g, x[k], y[j]);
    }
}
__global__ void __launch_bounds__(256) k_plane_fill_columns(const gr_skygrid::Grid g, const gr_point* __restrict__ pts, const double* __restrict__ val,
                                                            const double* __restrict__ x, int64_t n_x, int64_t n_y, const int64_t* __restrict__ idx,
                                                            int64_t* __restrict__ comp, double* __restrict__ col, double* __restrict__ colval,
                                                            int64_t* __restrict__ count)
{
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n_x; k += (int64_t)gridDim.x * 256)
        count[k] = gr_planegrid::build_column(g, pts, val, x[k], idx + k * n_y, n_y, comp + k * n_y, col + k * n_y, colval + k * n_y);
}
__global__ void __launch_bounds__(256) k_plane_fill(const double* __restrict__ y, int64_t n_x, int64_t n_y, const int64_t* __restrict__ perm,
                                                    const int64_t* __restrict__ comp, const double* __restrict__ col,
                                                    const double* __restrict__ colval, const int64_t* __restrict__ count, double* __restrict__ out,
                                                    int64_t* __restrict__ cells_out)
{
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < n_x * n_y; w += (int64_t)gridDim.x * 256) {
        const int64_t k = w / n_y, j = w - k * n_y;
        const int64_t at = perm[j] * n_x + k;        // the point is the caller's perm[j]
        const int64_t m = count[k];
        int64_t lower = 0, upper = 0;
        out[at] = m < 2 ? NAN : gr_planegrid::fill_point(col + k * n_y, colval + k * n_y, comp + k * n_y, m, y[j], lower, upper);
        cells_out[2 * at] = lower;
        cells_out[2 * at + 1] = upper;
    }
}

// the cells refined since a download and their rows of `children`: every nine cells from `first` on share a parent
__global__ void __launch_bounds__(256) k_sky_refined(const gr_skygrid::Grid g, int64_t first, int64_t groups, int64_t* __restrict__ refined,
                                                     int64_t* __restrict__ kids)
{
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < groups; k += (int64_t)gridDim.x * 256) {
        const int64_t p = g.parent[first + 9 * k];
        refined[k] = p;
        for (int c = 0; c < 9; ++c) kids[9 * k + c] = g.children[9 * p + c];
    }
}

// ---- host side ----

template <class T>
int32_t sky_grow(T** buf, size_t old_count, size_t new_count, hipStream_t stream)
{
    T* fresh = nullptr;
    GR_HIP(hipMalloc((void**)&fresh, sizeof(T) * new_count));
    if (*buf && old_count) GR_HIP(hipMemcpyAsync(fresh, *buf, sizeof(T) * old_count, hipMemcpyDeviceToDevice, stream));
    GR_HIP(hipStreamSynchronize(stream));
    if (*buf) (void)hipFree(*buf);
    *buf = fresh;
    return GR_OK;
}
template <class T>
int32_t sky_fresh(T** buf, size_t count)
{
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    GR_HIP(hipMalloc((void**)buf, sizeof(T) * count));
    return GR_OK;
}

// room for `cells` cells: the arrays grow by doubling (outside any launch function); the work buffers follow
int32_t sky_reserve(gr_sky* s, int64_t cells)
{
    if (cells > (int64_t)INT32_MAX - 16) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky: more than 2^31 cells");
    const size_t need = (size_t)cells + 1;
    if ((size_t)s->cap >= need) return GR_OK;
    const size_t cap = std::max<size_t>(need, std::max<size_t>(2 * (size_t)s->cap, 1024));
    const size_t have = s->cap ? (size_t)s->n + 1 : 0;
    hipStream_t st = s->ctx->stream;
    int32_t rc;
    if ((rc = sky_grow(&s->d_pos, 2 * have, 2 * cap, st)) != GR_OK) return rc;
    if ((rc = sky_grow(&s->d_level, have, cap, st)) != GR_OK) return rc;
    if ((rc = sky_grow(&s->d_children, 9 * have, 9 * cap, st)) != GR_OK) return rc;
    if ((rc = sky_grow(&s->d_neighbours, 4 * have, 4 * cap, st)) != GR_OK) return rc;
    if ((rc = sky_grow(&s->d_parent, have, cap, st)) != GR_OK) return rc;
    if ((rc = sky_grow(&s->d_location, have, cap, st)) != GR_OK) return rc;
    if ((rc = sky_grow(&s->d_rows, (size_t)s->row * have, (size_t)s->row * cap, st)) != GR_OK) return rc;
    if ((rc = sky_fresh(&s->d_mark, cap)) != GR_OK) return rc;
    if ((rc = sky_fresh(&s->d_cnt, cap)) != GR_OK) return rc;
    if ((rc = sky_fresh(&s->d_off, cap + 1)) != GR_OK) return rc;
    if (!s->d_part && (rc = sky_fresh(&s->d_part, (size_t)SKY_SCAN_BLOCKS + 2)) != GR_OK) return rc;
    s->cap = (int64_t)cap;
    return GR_OK;
}

int32_t* sky_flag(gr_sky* s) { return (int32_t*)(s->d_part + SKY_SCAN_BLOCKS + 1); }

void sky_free(gr_sky* s)
{
    (void)hipSetDevice(s->ctx->device);
    if (s->ctx->stream) (void)hipStreamSynchronize(s->ctx->stream);
    void* bufs[] = { s->d_pos, s->d_level, s->d_children, s->d_neighbours, s->d_parent, s->d_location, s->d_rows, s->d_mark,
                     s->d_cnt, s->d_off, s->d_part, s->d_need, s->d_ang, s->d_tmp };
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete s;
}

// launch: the cells whose (cos θ, ϕ) lie in d_ang (m each) -> their rows behind them in d_ang; allocates nothing
int32_t sky_launch_trace(gr_sky* s, int64_t m, gr_stats* stats)
{
    gr_skycells cells = s->src;
    double* ang = (double*)s->d_ang;
    if (s->plane)
        return gr_plane_cells_device(s->ctx, &s->cfg, &s->pl, ang, ang + m, m, (gr_point*)(ang + 2 * m), stats ? (gr_stats*)s->ctx->d_stats : nullptr,
                                     s->ctx->stream);
    cells.cos_theta = ang;
    cells.phi = ang + m;
    cells.n = m;
    return gr_sky_cells_device(s->ctx, &s->cfg, &cells, &s->pf, ang + 2 * m, stats ? (gr_stats*)s->ctx->d_stats : nullptr, s->ctx->stream);
}

// launch: refine the m cells of the device list d_need (checked first) and trace their outer children in one launch.  Room for
// the 9 m children and the launch's angles and rows is there (sky_refine_list): nothing is allocated here, and the host waits
// twice -- for the refusal flag, and at the end of the call.
int32_t sky_refine_launch(gr_sky* s, int64_t m, int64_t* traced, gr_stats* stats)
{
    int32_t rc;
    hipStream_t st = s->ctx->stream;
    const int64_t* list = (const int64_t*)s->d_need;
    const gr_skygrid::Grid g = sky_grid(s);
    // refusals first: nothing has changed when one is found
    GR_HIP(hipMemsetAsync(s->d_cnt, 0, sizeof(uint32_t) * ((size_t)s->n + 1), st));
    GR_HIP(hipMemsetAsync(sky_flag(s), 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_sky_refusals, dim3(sky_blocks(m)), dim3(256), 0, st, g, list, m, s->d_cnt, sky_flag(s));
    GR_HIP(hipGetLastError());
    int32_t why = 0;
    GR_HIP(hipMemcpyAsync(&why, sky_flag(s), sizeof why, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    if (why != 0) {
        static const char* const text[] = { "", "a cell index outside 1 ... n_cells", "a cell is refined already", "a cell at the deepest level (20) cannot be refined",
                                            "a cell is named twice" };
        return fail(GR_ERR_INVALID_ARGUMENT, std::string("gr_sky_refine_and_trace: ") + text[why > 4 ? 0 : why]);
    }
    if ((rc = begin_host_call(s->ctx, stats)) != GR_OK) return rc;
    double* ang = (double*)s->d_ang;
    if (s->plane) hipLaunchKernelGGL(k_sky_children<19>, dim3(sky_blocks(9 * m)), dim3(256), 0, st, g, list, m, s->d_rows, ang, ang + 8 * m);
    else hipLaunchKernelGGL(k_sky_children<6>, dim3(sky_blocks(9 * m)), dim3(256), 0, st, g, list, m, s->d_rows, ang, ang + 8 * m);
    GR_HIP(hipGetLastError());
    if ((rc = sky_launch_trace(s, 8 * m, stats)) != GR_OK) return rc;
    if (s->plane) hipLaunchKernelGGL(k_sky_scatter<19>, dim3(sky_blocks(8 * m)), dim3(256), 0, st, (const double*)(ang + 16 * m), m, s->n + 1, s->d_rows);
    else hipLaunchKernelGGL(k_sky_scatter<6>, dim3(sky_blocks(8 * m)), dim3(256), 0, st, (const double*)(ang + 16 * m), m, s->n + 1, s->d_rows);
    GR_HIP(hipGetLastError());
    if ((rc = end_host_call(s->ctx, stats)) != GR_OK) return rc;
    s->n += 9 * m;
    s->need_n = -1;
    if (traced) *traced = 8 * m;
    return GR_OK;
}

// room first (the arrays grow by doubling, the work buffers follow), then the launch
int32_t sky_refine_list(gr_sky* s, int64_t m, int64_t* traced, gr_stats* stats)
{
    if (traced) *traced = 0;
    if (m == 0) return GR_OK;
    int32_t rc;
    if ((rc = sky_reserve(s, s->n + 9 * m)) != GR_OK) return rc;
    if ((rc = ensure(&s->d_ang, &s->ang_bytes, sizeof(double) * (size_t)(2 + s->row) * 8 * (size_t)m)) != GR_OK) return rc;
    return sky_refine_launch(s, m, traced, stats);
}

int32_t sky_check(gr_sky* sky)
{
    if (!sky) return fail(GR_ERR_INVALID_ARGUMENT, "sky is null");
    GR_HIP(hipSetDevice(sky->ctx->device));
    return GR_OK;
}

}  // namespace

extern "C" {
static void sky_drop_ctx(gr_ctx* c)
{
    std::vector<gr_sky*> mine;
    {
        std::lock_guard<std::mutex> lock(g_sky_mutex);
        for (size_t i = 0; i < g_skies.size();)
            if (g_skies[i]->ctx == c) {
                mine.push_back(g_skies[i]);
                g_skies.erase(g_skies.begin() + (long)i);
            } else
                ++i;
    }
    for (gr_sky* s : mine) sky_free(s);
}
}  // extern "C"

// what gr_sky_create and gr_sky_create_plane share: the limits, room for the nine top cells, the cells themselves and null rows
// (NaN; a plane's: NoStatus points with NaN fields).  `s` is freed on failure.
static int32_t sky_create_common(gr_ctx* ctx, gr_sky* s, const double* limits, int32_t x_periodic, gr_sky** sky)
{
    int32_t rc;
    s->ctx = ctx;
    s->lim[0] = std::min(limits[0], limits[1]);
    s->lim[1] = std::max(limits[0], limits[1]);
    s->lim[2] = std::min(limits[2], limits[3]);
    s->lim[3] = std::max(limits[2], limits[3]);
    if ((rc = sky_reserve(s, 9)) != GR_OK) {
        sky_free(s);
        return rc;
    }
    // the nine top cells, formed here as AdaptiveGrid.__init__ forms them
    double pos[20];
    int32_t level[10];
    int64_t children[90], neighbours[40], parent[10];
    int8_t location[10];
    double rows[190];
    gr_skygrid::Grid g = sky_grid(s);
    g.pos = pos;
    g.level = level;
    g.children = children;
    g.neighbours = neighbours;
    g.parent = parent;
    g.location = location;
    gr_skygrid::top_cells(g, x_periodic != 0);
    for (double& v : rows) v = NAN;
    if (s->plane)
        for (int i = 0; i < 10; ++i) {
            gr_point null_point;
            std::memcpy(&null_point, rows + 19 * i, sizeof null_point);
            null_point.status = GR_STATUS_NO_STATUS;
            null_point.flags = 0;
            std::memcpy(rows + 19 * i, &null_point, sizeof null_point);
        }
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(s->d_pos, pos, sizeof pos, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_level, level, sizeof level, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_children, children, sizeof children, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_neighbours, neighbours, sizeof neighbours, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_parent, parent, sizeof parent, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_location, location, sizeof location, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_rows, rows, sizeof(double) * (size_t)s->row * 10, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        sky_free(s);
        return fail(GR_ERR_HIP, std::string("gr_sky_create: ") + hipGetErrorString(e));
    }
    s->n = 9;
    {
        std::lock_guard<std::mutex> lock(g_sky_mutex);
        g_skies.push_back(s);
    }
    *sky = s;
    return GR_OK;
}

int32_t gr_sky_create(gr_ctx* ctx, const gr_config* cfg, const gr_skycells* source, const gr_pointfunction* pf, const double* limits,
                      int32_t x_periodic, gr_sky** sky)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!sky || !limits) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_create: sky / limits is null");
    *sky = nullptr;
    int32_t rc;
    gr_skycells none;
    if (source) {
        none = *source;
        none.cos_theta = none.phi = nullptr;
        none.n = 0;
    }
    if ((rc = skycells_check(cfg, source ? &none : nullptr, pf, false)) != GR_OK) return rc;
    for (int q = 0; q < 4; ++q)
        if (!std::isfinite(limits[q])) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_create: the limits must be finite");
    GR_HIP(hipSetDevice(ctx->device));
    gr_sky* s = new (std::nothrow) gr_sky;
    if (!s) return fail(GR_ERR_OUT_OF_MEMORY, "gr_sky_create: out of memory");
    s->cfg = *cfg;
    s->pf = *pf;
    s->src = none;
    return sky_create_common(ctx, s, limits, x_periodic, sky);
}

int32_t gr_sky_create_plane(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const double* limits, int32_t x_periodic, gr_sky** sky)
{
    if (!ctx) return fail(GR_ERR_INVALID_ARGUMENT, "ctx is null");
    if (!sky || !limits) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_create_plane: sky / limits is null");
    *sky = nullptr;
    int32_t rc;
    if ((rc = planecells_check(cfg, plane)) != GR_OK) return rc;
    for (int q = 0; q < 4; ++q)
        if (!std::isfinite(limits[q])) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_create_plane: the limits must be finite");
    GR_HIP(hipSetDevice(ctx->device));
    gr_sky* s = new (std::nothrow) gr_sky;
    if (!s) return fail(GR_ERR_OUT_OF_MEMORY, "gr_sky_create_plane: out of memory");
    s->cfg = *cfg;
    std::memset(&s->pf, 0, sizeof s->pf);
    std::memset(&s->src, 0, sizeof s->src);
    s->pl = *plane;
    s->plane = true;
    s->row = 19;
    return sky_create_common(ctx, s, limits, x_periodic, sky);
}

int32_t gr_sky_destroy(gr_sky* sky)
{
    if (!sky) return GR_OK;
    {
        std::lock_guard<std::mutex> lock(g_sky_mutex);
        auto it = std::find(g_skies.begin(), g_skies.end(), sky);
        if (it == g_skies.end()) return GR_OK;      // its context took it along
        g_skies.erase(it);
    }
    sky_free(sky);
    return GR_OK;
}

int32_t gr_sky_size(gr_sky* sky, int64_t* n_cells)
{
    if (!sky || !n_cells) return fail(GR_ERR_INVALID_ARGUMENT, "sky / n_cells is null");
    *n_cells = sky->n;
    return GR_OK;
}

int32_t gr_sky_trace_initial(gr_sky* sky, int32_t level, int64_t* launch_sizes)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (sky->traced || sky->n != 9) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_trace_initial: the sky has been traced already");
    if (level < 1 || level > GR_SKY_MAX_LEVEL) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_trace_initial: level in 1 ... 20");
    hipStream_t st = sky->ctx->stream;
    if ((rc = ensure(&sky->d_ang, &sky->ang_bytes, sizeof(double) * (size_t)(2 + sky->row) * 9)) != GR_OK) return rc;
    double* ang = (double*)sky->d_ang;
    hipLaunchKernelGGL(k_sky_positions, dim3(1), dim3(256), 0, st, (const double*)sky->d_pos, (int64_t)1, (int64_t)9, ang, ang + 9);
    GR_HIP(hipGetLastError());
    if ((rc = sky_launch_trace(sky, 9, nullptr)) != GR_OK) return rc;
    GR_HIP(hipMemcpyAsync(sky->d_rows + sky->row, ang + 18, sizeof(double) * (size_t)sky->row * 9, hipMemcpyDeviceToDevice, st));
    GR_HIP(hipStreamSynchronize(st));
    sky->traced = true;
    if (launch_sizes) launch_sizes[0] = 9;
    for (int32_t l = 1; l < level; ++l) {
        // every leaf: the cells of the last level, ascending
        const int64_t n_rows = sky->n + 1;
        if ((rc = ensure(&sky->d_need, &sky->need_bytes, sizeof(int64_t) * (size_t)n_rows)) != GR_OK) return rc;
        hipLaunchKernelGGL(k_sky_mark_leaves, dim3(sky_blocks(n_rows)), dim3(256), 0, st, sky_grid(sky), sky->d_mark);
        GR_HIP(hipGetLastError());
        if ((rc = sky_scan(sky, (const uint8_t*)sky->d_mark, n_rows, st)) != GR_OK) return rc;
        hipLaunchKernelGGL(k_sky_compact, dim3(sky_blocks(n_rows)), dim3(256), 0, st, (const uint8_t*)sky->d_mark, (const int64_t*)sky->d_off, n_rows,
                           (int64_t*)sky->d_need);
        GR_HIP(hipGetLastError());
        int64_t m = 0;
        GR_HIP(hipMemcpyAsync(&m, sky->d_off + n_rows, sizeof m, hipMemcpyDeviceToHost, st));
        GR_HIP(hipStreamSynchronize(st));
        int64_t traced = 0;
        if ((rc = sky_refine_list(sky, m, &traced, nullptr)) != GR_OK) return rc;
        if (launch_sizes) launch_sizes[l] = traced;
    }
    return GR_OK;
}

int32_t gr_sky_find_need_refine(gr_sky* sky, const gr_sky_criterion* criterion, int64_t* count)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (!criterion || !count) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_find_need_refine: criterion / count is null");
    if (criterion->kind < GR_SKY_CRIT_DEFAULT || criterion->kind > GR_SKY_CRIT_PLANE)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_find_need_refine: unknown criterion kind");
    if (sky->plane && criterion->kind != GR_SKY_CRIT_PLANE && criterion->kind != GR_SKY_CRIT_LEVEL)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_find_need_refine: a plane sky's criteria are GR_SKY_CRIT_PLANE and GR_SKY_CRIT_LEVEL (the others read corona rows)");
    if (!sky->plane && criterion->kind == GR_SKY_CRIT_PLANE)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_find_need_refine: GR_SKY_CRIT_PLANE reads the points of a plane sky (gr_sky_create_plane)");
    if (criterion->n_boxes < 0 || criterion->n_boxes > GR_SKY_MAX_BOXES)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_find_need_refine: n_boxes in 0 ... 8");
    for (int k = 0; k < criterion->n_boxes; ++k)
        if (criterion->boxes[k].n_phi < 0 || criterion->boxes[k].n_phi > 2)
            return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_find_need_refine: a box has zero, one or two ϕ intervals");
    *count = 0;
    sky->need_n = -1;
    hipStream_t st = sky->ctx->stream;
    const int64_t n_rows = sky->n + 1;
    if ((rc = ensure(&sky->d_need, &sky->need_bytes, sizeof(int64_t) * (size_t)n_rows)) != GR_OK) return rc;
    GR_HIP(hipMemsetAsync(sky->d_mark, 0, (size_t)n_rows, st));
    GR_HIP(hipMemsetAsync(sky_flag(sky), 0, sizeof(int32_t), st));
    if (sky->plane)
        hipLaunchKernelGGL(k_plane_mark_need, dim3(sky_blocks(sky->n)), dim3(256), 0, st, sky_grid(sky), (const gr_point*)sky->d_rows, *criterion,
                           sky->d_mark, sky_flag(sky));
    else
        hipLaunchKernelGGL(k_sky_mark_need, dim3(sky_blocks(sky->n)), dim3(256), 0, st, sky_grid(sky), (const double*)sky->d_rows, *criterion, sky->d_mark,
                           sky_flag(sky));
    GR_HIP(hipGetLastError());
    int32_t why = 0;
    GR_HIP(hipMemcpyAsync(&why, sky_flag(sky), sizeof why, hipMemcpyDeviceToHost, st));
    if ((rc = sky_scan(sky, (const uint8_t*)sky->d_mark, n_rows, st)) != GR_OK) return rc;
    hipLaunchKernelGGL(k_sky_compact, dim3(sky_blocks(n_rows)), dim3(256), 0, st, (const uint8_t*)sky->d_mark, (const int64_t*)sky->d_off, n_rows,
                       (int64_t*)sky->d_need);
    GR_HIP(hipGetLastError());
    int64_t m = 0;
    GR_HIP(hipMemcpyAsync(&m, sky->d_off + n_rows, sizeof m, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    if (why != 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_find_need_refine: the tree is deeper than the bordering walk's stack");
    sky->need_n = m;
    *count = m;
    return GR_OK;
}

int32_t gr_sky_need_refine_list(gr_sky* sky, int64_t* cells)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (sky->need_n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_need_refine_list: no list (gr_sky_find_need_refine comes first)");
    if (sky->need_n == 0) return GR_OK;
    if (!cells) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_need_refine_list: cells is null");
    GR_HIP(hipMemcpyAsync(cells, sky->d_need, sizeof(int64_t) * (size_t)sky->need_n, hipMemcpyDeviceToHost, sky->ctx->stream));
    GR_HIP(hipStreamSynchronize(sky->ctx->stream));
    return GR_OK;
}

int32_t gr_sky_pairs(gr_sky* sky, int64_t* i1, int64_t* i2, int64_t cap, int64_t* n)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (!n) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_pairs: n is null");
    hipStream_t st = sky->ctx->stream;
    const int64_t n_rows = sky->n + 1;
    const gr_skygrid::Grid g = sky_grid(sky);
    GR_HIP(hipMemsetAsync(sky_flag(sky), 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_sky_pair_count, dim3(sky_blocks(n_rows)), dim3(256), 0, st, g, sky->d_cnt, sky_flag(sky));
    GR_HIP(hipGetLastError());
    if ((rc = sky_scan(sky, (const uint32_t*)sky->d_cnt, n_rows, st)) != GR_OK) return rc;
    int64_t total = 0;
    int32_t why = 0;
    GR_HIP(hipMemcpyAsync(&total, sky->d_off + n_rows, sizeof total, hipMemcpyDeviceToHost, st));
    GR_HIP(hipMemcpyAsync(&why, sky_flag(sky), sizeof why, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    if (why != 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_pairs: the tree is deeper than the bordering walk's stack");
    *n = total;
    if (!i1 || !i2 || cap < total || total == 0) return GR_OK;
    if ((rc = ensure(&sky->d_tmp, &sky->tmp_bytes, sizeof(int64_t) * 2 * (size_t)total)) != GR_OK) return rc;
    int64_t* d1 = (int64_t*)sky->d_tmp;
    hipLaunchKernelGGL(k_sky_pair_fill, dim3(sky_blocks(sky->n)), dim3(256), 0, st, g, (const int64_t*)sky->d_off, total, d1, d1 + total);
    GR_HIP(hipGetLastError());
    GR_HIP(hipMemcpyAsync(i1, d1, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, st));
    GR_HIP(hipMemcpyAsync(i2, d1 + total, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    return GR_OK;
}

int32_t gr_sky_refine_and_trace(gr_sky* sky, const int64_t* cells, int64_t n, int64_t* traced, gr_stats* stats)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (traced) *traced = 0;
    if (!sky->traced) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_refine_and_trace: gr_sky_trace_initial comes first (the middle children inherit rows)");
    if (!cells) {
        if (sky->need_n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_refine_and_trace: no list (gr_sky_find_need_refine comes first)");
        return sky_refine_list(sky, sky->need_n, traced, stats);
    }
    if (n < 0) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_refine_and_trace: n must be non-negative");
    sky->need_n = -1;
    if (n == 0) return GR_OK;
    if ((rc = ensure(&sky->d_need, &sky->need_bytes, sizeof(int64_t) * (size_t)n)) != GR_OK) return rc;
    GR_HIP(hipMemcpyAsync(sky->d_need, cells, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, sky->ctx->stream));
    return sky_refine_list(sky, n, traced, stats);
}

int32_t gr_sky_occupancy(gr_sky* sky, const double* r_bins, int64_t n_r, const double* phi_bins, int64_t n_phi, const double* gamma,
                         int64_t* counts)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (sky && sky->plane) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_occupancy: a plane sky has no (r, ϕ) rows");
    if (!r_bins || !phi_bins || !counts || n_r < 1 || n_phi < 1 || n_r > 46340 || n_phi > 46340)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_occupancy: r_bins / phi_bins / counts is null, or a count outside 1 ... 46340");
    hipStream_t st = sky->ctx->stream;
    const size_t cells = (size_t)n_r * (size_t)n_phi;
    if ((rc = ensure(&sky->d_tmp, &sky->tmp_bytes, sizeof(double) * (size_t)(n_r + n_phi) + sizeof(unsigned int) * cells)) != GR_OK) return rc;
    double* d_r = (double*)sky->d_tmp;
    double* d_p = d_r + n_r;
    unsigned int* d_c = (unsigned int*)(d_p + n_phi);
    double r_max = r_bins[0];
    for (int64_t k = 1; k < n_r; ++k) r_max = r_bins[k] > r_max ? r_bins[k] : r_max;
    GR_HIP(hipMemcpyAsync(d_r, r_bins, sizeof(double) * (size_t)n_r, hipMemcpyHostToDevice, st));
    GR_HIP(hipMemcpyAsync(d_p, phi_bins, sizeof(double) * (size_t)n_phi, hipMemcpyHostToDevice, st));
    GR_HIP(hipMemsetAsync(d_c, 0, sizeof(unsigned int) * cells, st));
    hipLaunchKernelGGL(k_sky_occupancy, dim3(sky_blocks(sky->n)), dim3(256), 0, st, sky_grid(sky), (const double*)sky->d_rows, (const double*)d_r, n_r,
                       r_max, (const double*)d_p, n_phi, gamma ? 1 : 0, gamma ? *gamma : 0.0, d_c);
    GR_HIP(hipGetLastError());
    std::vector<unsigned int> h;
    try {
        h.resize(cells);
    } catch (...) {
        return fail(GR_ERR_OUT_OF_MEMORY, "gr_sky_occupancy: out of memory");
    }
    GR_HIP(hipMemcpyAsync(h.data(), d_c, sizeof(unsigned int) * cells, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < cells; ++k) counts[k] = (int64_t)h[k];
    return GR_OK;
}

int32_t gr_sky_bin_grid(gr_sky* sky, int32_t what, const double* r_bins, int64_t n_r, const double* phi_bins, int64_t n_phi, const double* gamma,
                        double* out, double* solid_angle)
{
    // refusals first: nothing has touched the device when one is found
    if (!sky) return fail(GR_ERR_INVALID_ARGUMENT, "sky is null");
    if (sky->plane) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_bin_grid: a plane sky has no (r, ϕ) rows");
    if (!r_bins || !phi_bins || !out || n_r < 1 || n_phi < 1 || n_r > 46340 || n_phi > 46340)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_bin_grid: r_bins / phi_bins / out is null, or a count outside 1 ... 46340");
    if (what < GR_SKY_MAP_EMISSIVITY || what > GR_SKY_MAP_TIME) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_bin_grid: unknown map (GR_SKY_MAP_*)");
    if (!sky->traced) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_bin_grid: the sky has not been traced (gr_sky_trace_initial comes first)");
    for (int64_t k = 1; k < n_r; ++k)
        if (!(r_bins[k] >= r_bins[k - 1])) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_bin_grid: the r edges must ascend");
    for (int64_t k = 1; k < n_phi; ++k)
        if (!(phi_bins[k] >= phi_bins[k - 1])) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_bin_grid: the ϕ edges must ascend");
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    hipStream_t st = sky->ctx->stream;
    const size_t cells = (size_t)n_r * (size_t)n_phi, n_rows = (size_t)sky->n + 1;
    const bool emissivity = what == GR_SKY_MAP_EMISSIVITY;
    // edges | per-cell r and γA (emissivity) | max |term|, max ΔΩ | 4 x cells sums | cells counts | 4 x cells flags
    const size_t work = sizeof(unsigned long long) * (2 + 4 * cells) + sizeof(unsigned int) * cells + 4 * cells;
    if ((rc = ensure(&sky->d_tmp, &sky->tmp_bytes, sizeof(double) * ((size_t)(n_r + n_phi) + (emissivity ? 2 * n_rows : 0)) + work)) != GR_OK) return rc;
    double* d_r = (double*)sky->d_tmp;
    double* d_p = d_r + n_r;
    double* d_rad = d_p + n_phi;
    double* d_area = emissivity ? d_rad + n_rows : nullptr;
    unsigned long long* d_red = (unsigned long long*)(d_rad + (emissivity ? 2 * n_rows : 0));
    unsigned long long* d_acc = d_red + 2;
    unsigned int* d_cnt = (unsigned int*)(d_acc + 4 * cells);
    uint8_t* d_flag = (uint8_t*)(d_cnt + cells);
    gr_skygrid::MapBins b;
    b.r_bins = d_r;
    b.nr = n_r;
    b.r_max = r_bins[0];
    for (int64_t k = 1; k < n_r; ++k) b.r_max = r_bins[k] > b.r_max ? r_bins[k] : b.r_max;
    b.phi_bins = d_p;
    b.nphi = n_phi;
    GR_HIP(hipMemcpyAsync(d_r, r_bins, sizeof(double) * (size_t)n_r, hipMemcpyHostToDevice, st));
    GR_HIP(hipMemcpyAsync(d_p, phi_bins, sizeof(double) * (size_t)n_phi, hipMemcpyHostToDevice, st));
    GR_HIP(hipMemsetAsync(d_red, 0, work, st));
    const gr_skygrid::Grid g = sky_grid(sky);
    if (emissivity) {
        hipLaunchKernelGGL(k_sky_radii, dim3(sky_blocks((int64_t)n_rows)), dim3(256), 0, st, g, (const double*)sky->d_rows, d_rad);
        GR_HIP(hipGetLastError());
        if ((rc = gr_disc_area_factor_device(sky->ctx, &sky->cfg, &sky->pf, d_rad, (int64_t)n_rows, d_area, st)) != GR_OK) return rc;
    }
    const int has_gamma = gamma ? 1 : 0;
    const double gam = gamma ? *gamma : 0.0;
    hipLaunchKernelGGL(k_sky_map_extrema, dim3(sky_blocks(sky->n)), dim3(256), 0, st, g, (const double*)sky->d_rows, b, (int)what, has_gamma, gam,
                       (const double*)d_area, d_red);
    GR_HIP(hipGetLastError());
    unsigned long long red[2] = { 0ull, 0ull };
    GR_HIP(hipMemcpyAsync(red, d_red, sizeof red, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    double vmax[2];
    std::memcpy(vmax, red, sizeof vmax);
    const gr_lag::CoronaGrid gt = gr_lag::corona_grid(vmax[0], sky->n), gs = gr_lag::corona_grid(vmax[1], sky->n);
    hipLaunchKernelGGL(k_sky_map_bin, dim3(sky_blocks(sky->n)), dim3(256), 0, st, g, (const double*)sky->d_rows, b, (int)what, has_gamma, gam,
                       (const double*)d_area, gt.sc, gs.sc, (int64_t)cells, d_acc, d_cnt, d_flag);
    GR_HIP(hipGetLastError());
    std::vector<long long> acc;
    std::vector<unsigned int> cnt;
    std::vector<uint8_t> flag;
    try {
        acc.resize(4 * cells);
        cnt.resize(cells);
        flag.resize(4 * cells);
    } catch (...) {
        return fail(GR_ERR_OUT_OF_MEMORY, "gr_sky_bin_grid: out of memory");
    }
    GR_HIP(hipMemcpyAsync(acc.data(), d_acc, sizeof(long long) * 4 * cells, hipMemcpyDeviceToHost, st));
    GR_HIP(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(unsigned int) * cells, hipMemcpyDeviceToHost, st));
    GR_HIP(hipMemcpyAsync(flag.data(), d_flag, 4 * cells, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    const int64_t vanished = gr_skygrid::map_finish(acc.data(), cnt.data(), flag.data(), (int64_t)cells, gt, gs, out, solid_angle);
    if (vanished) {
        char text[320];
        std::snprintf(text, sizeof text, "gr_sky_bin_grid: %lld bins hold non-zero terms that all lie below the resolution %.3g of the fixed-point sums "
                                         "(the map's largest term is %.3g): the dynamic range of the terms is too wide, and the map would be 0 where "
                                         "gr_sky_occupancy counts", (long long)vanished, gt.step * gt.lo_unit, vmax[0]);
        return fail(GR_ERR_UNSUPPORTED, text);
    }
    return GR_OK;
}

int32_t gr_sky_fill(gr_sky* sky, const double* phi_grid, int64_t n_phi, const double* theta_grid, int64_t n_theta, double* out, int64_t* cells)
{
    if (!sky) return fail(GR_ERR_INVALID_ARGUMENT, "sky is null");
    if (sky->plane) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_fill: a plane sky is filled by gr_sky_fill_plane");
    if (!phi_grid || !theta_grid || !out || n_phi < 1 || n_theta < 1 || n_phi > 46340 || n_theta > 46340)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_fill: phi_grid / theta_grid / out is null, or a count outside 1 ... 46340");
    if (!sky->traced) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_fill: the sky has not been traced (gr_sky_trace_initial comes first)");
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    hipStream_t st = sky->ctx->stream;
    const size_t points = (size_t)n_theta * (size_t)n_phi;
    std::vector<double> grids;
    std::vector<int64_t> perm;
    try {
        grids.resize((size_t)n_phi + 2 * (size_t)n_theta);
        perm.resize((size_t)n_theta);
    } catch (...) {
        return fail(GR_ERR_OUT_OF_MEMORY, "gr_sky_fill: out of memory");
    }
    // ϕ | θ ascending | cos θ (formed here, as the reference forms them on the host) | the caller's index of every θ | out | column θ |
    // cells of the points | compacted cells | cells out | flag
    gr_skygrid::theta_order(theta_grid, n_theta, perm.data());
    std::memcpy(grids.data(), phi_grid, sizeof(double) * (size_t)n_phi);
    for (int64_t j = 0; j < n_theta; ++j) {
        const double th = theta_grid[perm[(size_t)j]];
        grids[(size_t)(n_phi + j)] = th;
        grids[(size_t)(n_phi + n_theta + j)] = std::cos(th);
    }
    const size_t bytes = sizeof(double) * (grids.size() + 7 * points) + sizeof(int64_t) * (perm.size() + 4 * points) + 16;
    if ((rc = ensure(&sky->d_tmp, &sky->tmp_bytes, bytes)) != GR_OK) return rc;
    double* d_phi = (double*)sky->d_tmp;
    double* d_theta = d_phi + n_phi;
    double* d_cos = d_theta + n_theta;
    int64_t* d_perm = (int64_t*)(d_cos + n_theta);
    double* d_out = (double*)(d_perm + n_theta);
    double* d_col = d_out + 6 * points;
    int64_t* d_idx = (int64_t*)(d_col + points);
    int64_t* d_comp = d_idx + points;
    int64_t* d_cells = d_comp + points;
    int32_t* d_flag = (int32_t*)(d_cells + 2 * points);
    GR_HIP(hipMemcpyAsync(d_phi, grids.data(), sizeof(double) * grids.size(), hipMemcpyHostToDevice, st));
    GR_HIP(hipMemcpyAsync(d_perm, perm.data(), sizeof(int64_t) * perm.size(), hipMemcpyHostToDevice, st));
    GR_HIP(hipMemsetAsync(d_flag, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_sky_fill, dim3((unsigned)n_phi), dim3(256), 0, st, sky_grid(sky), (const double*)sky->d_rows,
                       (const double*)d_phi, (const double*)d_theta, (const double*)d_cos, n_theta, n_phi, (const int64_t*)d_perm, d_idx, d_comp, d_col, d_out, d_cells, d_flag);
    GR_HIP(hipGetLastError());
    int32_t why = 0;
    GR_HIP(hipMemcpyAsync(&why, d_flag, sizeof why, hipMemcpyDeviceToHost, st));
    GR_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * 6 * points, hipMemcpyDeviceToHost, st));
    if (cells) GR_HIP(hipMemcpyAsync(cells, d_cells, sizeof(int64_t) * 2 * points, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    if (why != 0) return fail(GR_ERR_UNSUPPORTED, "gr_sky_fill: a column does not meet its leaves in ascending θ");
    return GR_OK;
}

int32_t gr_sky_download(gr_sky* sky, int64_t first_cell, int64_t count, double* pos, void* level, int64_t* children, int64_t* neighbours,
                        int64_t* parent, void* location, double* rows, int64_t* refined, int64_t* refined_children)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (first_cell < 0 || count < 0 || first_cell + count > sky->n + 1)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_download: cells first_cell ... first_cell + count - 1 must lie in 0 ... n_cells");
    if (rows && sky->plane) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_download: the rows of a plane sky are gr_points: gr_sky_download_points");
    if (count == 0) return GR_OK;
    hipStream_t st = sky->ctx->stream;
    const size_t f = (size_t)first_cell, c = (size_t)count;
    if (pos) GR_HIP(hipMemcpyAsync(pos, sky->d_pos + 2 * f, sizeof(double) * 2 * c, hipMemcpyDeviceToHost, st));
    if (level) GR_HIP(hipMemcpyAsync(level, sky->d_level + f, sizeof(int32_t) * c, hipMemcpyDeviceToHost, st));
    if (children) GR_HIP(hipMemcpyAsync(children, sky->d_children + 9 * f, sizeof(int64_t) * 9 * c, hipMemcpyDeviceToHost, st));
    if (neighbours) GR_HIP(hipMemcpyAsync(neighbours, sky->d_neighbours + 4 * f, sizeof(int64_t) * 4 * c, hipMemcpyDeviceToHost, st));
    if (parent) GR_HIP(hipMemcpyAsync(parent, sky->d_parent + f, sizeof(int64_t) * c, hipMemcpyDeviceToHost, st));
    if (location) GR_HIP(hipMemcpyAsync(location, sky->d_location + f, sizeof(int8_t) * c, hipMemcpyDeviceToHost, st));
    if (rows) GR_HIP(hipMemcpyAsync(rows, sky->d_rows + 6 * f, sizeof(double) * 6 * c, hipMemcpyDeviceToHost, st));
    if (refined || refined_children) {
        if (!refined || !refined_children) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_download: refined and refined_children come together");
        if (first_cell < 10 || (first_cell - 10) % 9 != 0 || count % 9 != 0)
            return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_download: the refined cells are told from first_cell = 10 + 9 k on, nine cells at a time");
        const int64_t groups = count / 9;
        if ((rc = ensure(&sky->d_tmp, &sky->tmp_bytes, sizeof(int64_t) * 10 * (size_t)groups)) != GR_OK) return rc;
        int64_t* d_ref = (int64_t*)sky->d_tmp;
        hipLaunchKernelGGL(k_sky_refined, dim3(sky_blocks(groups)), dim3(256), 0, st, sky_grid(sky), first_cell, groups, d_ref, d_ref + groups);
        GR_HIP(hipGetLastError());
        GR_HIP(hipMemcpyAsync(refined, d_ref, sizeof(int64_t) * (size_t)groups, hipMemcpyDeviceToHost, st));
        GR_HIP(hipMemcpyAsync(refined_children, d_ref + groups, sizeof(int64_t) * 9 * (size_t)groups, hipMemcpyDeviceToHost, st));
    }
    GR_HIP(hipStreamSynchronize(st));
    return GR_OK;
}

int32_t gr_sky_download_points(gr_sky* sky, int64_t first_cell, int64_t count, gr_point* out)
{
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    if (!sky->plane) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_download_points: the rows of a corona sky are six doubles: gr_sky_download");
    if (first_cell < 0 || count < 0 || first_cell + count > sky->n + 1)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_download_points: cells first_cell ... first_cell + count - 1 must lie in 0 ... n_cells");
    if (count == 0) return GR_OK;
    if (!out) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_download_points: out is null");
    hipStream_t st = sky->ctx->stream;
    GR_HIP(hipMemcpyAsync(out, (const gr_point*)sky->d_rows + first_cell, sizeof(gr_point) * (size_t)count, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    return GR_OK;
}

int32_t gr_sky_fill_plane(gr_sky* sky, const gr_pointfunction* pf, const double* cell_values, const double* x_grid, int64_t n_x, const double* y_grid,
                          int64_t n_y, double* out, int64_t* cells)
{
    if (!sky) return fail(GR_ERR_INVALID_ARGUMENT, "sky is null");
    if (!sky->plane) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_fill_plane: a corona sky is filled by gr_sky_fill");
    if (!x_grid || !y_grid || !out || n_x < 1 || n_y < 1 || n_x > 46340 || n_y > 46340)
        return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_fill_plane: x_grid / y_grid / out is null, or a count outside 1 ... 46340");
    if (pf && cell_values) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_fill_plane: pf or cell_values, not both");
    if (!sky->traced) return fail(GR_ERR_INVALID_ARGUMENT, "gr_sky_fill_plane: the sky has not been traced (gr_sky_trace_initial comes first)");
    int32_t rc;
    if ((rc = sky_check(sky)) != GR_OK) return rc;
    hipStream_t st = sky->ctx->stream;
    const size_t points = (size_t)n_y * (size_t)n_x, n_rows = (size_t)sky->n + 1;
    std::vector<double> grids;
    std::vector<int64_t> perm;
    try {
        grids.resize((size_t)n_x + (size_t)n_y);
        perm.resize((size_t)n_y);
    } catch (...) {
        return fail(GR_ERR_OUT_OF_MEMORY, "gr_sky_fill_plane: out of memory");
    }
    gr_skygrid::theta_order(y_grid, n_y, perm.data());
    std::memcpy(grids.data(), x_grid, sizeof(double) * (size_t)n_x);
    for (int64_t j = 0; j < n_y; ++j) grids[(size_t)(n_x + j)] = y_grid[perm[(size_t)j]];
    // x | y ascending | the values of the cells | out | column y | column values | the caller's index of every y | cells of the points |
    // compacted cells | cells out | cells per column
    const size_t bytes = sizeof(double) * (grids.size() + n_rows + 3 * points) + sizeof(int64_t) * (perm.size() + 4 * points + (size_t)n_x) + 16;
    if ((rc = ensure(&sky->d_tmp, &sky->tmp_bytes, bytes)) != GR_OK) return rc;
    double* d_x = (double*)sky->d_tmp;
    double* d_y = d_x + n_x;
    double* d_val = d_y + n_y;
    double* d_out = d_val + n_rows;
    double* d_col = d_out + points;
    double* d_colval = d_col + points;
    int64_t* d_perm = (int64_t*)(d_colval + points);
    int64_t* d_idx = d_perm + n_y;
    int64_t* d_comp = d_idx + points;
    int64_t* d_cells = d_comp + points;
    int64_t* d_count = d_cells + 2 * points;
    const gr_point* pts = (const gr_point*)sky->d_rows;
    const gr_skygrid::Grid g = sky_grid(sky);
    GR_HIP(hipMemcpyAsync(d_x, grids.data(), sizeof(double) * grids.size(), hipMemcpyHostToDevice, st));
    GR_HIP(hipMemcpyAsync(d_perm, perm.data(), sizeof(int64_t) * perm.size(), hipMemcpyHostToDevice, st));
    if (cell_values) {
        GR_HIP(hipMemcpyAsync(d_val, cell_values, sizeof(double) * n_rows, hipMemcpyHostToDevice, st));
    } else if (pf) {
        // cells 1 ... n; the null cell's value is never read (a cell or a neighbour 0 is no cell)
        GR_HIP(hipMemsetAsync(d_val, 0xFF, sizeof(double), st));
        if ((rc = gr_apply_pointfunction_device(sky->ctx, &sky->cfg, pf, pts + 1, sky->n, sky->cfg.lambda1, d_val + 1, st)) != GR_OK) return rc;
    } else {
        hipLaunchKernelGGL(k_plane_default_values, dim3(sky_blocks((int64_t)n_rows)), dim3(256), 0, st, pts, (int64_t)n_rows, d_val);
    }
    hipLaunchKernelGGL(k_plane_fill_locate, dim3(sky_blocks((int64_t)points)), dim3(256), 0, st, g, (const double*)d_x, n_x, (const double*)d_y, n_y, d_idx);
    hipLaunchKernelGGL(k_plane_fill_columns, dim3(sky_blocks(n_x)), dim3(256), 0, st, g, pts, (const double*)d_val, (const double*)d_x, n_x, n_y,
                       (const int64_t*)d_idx, d_comp, d_col, d_colval, d_count);
    hipLaunchKernelGGL(k_plane_fill, dim3(sky_blocks((int64_t)points)), dim3(256), 0, st, (const double*)d_y, n_x, n_y, (const int64_t*)d_perm,
                       (const int64_t*)d_comp, (const double*)d_col, (const double*)d_colval, (const int64_t*)d_count, d_out, d_cells);
    GR_HIP(hipGetLastError());
    GR_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * points, hipMemcpyDeviceToHost, st));
    if (cells) GR_HIP(hipMemcpyAsync(cells, d_cells, sizeof(int64_t) * 2 * points, hipMemcpyDeviceToHost, st));
    GR_HIP(hipStreamSynchronize(st));
    return GR_OK;
}
