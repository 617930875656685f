// kernels_tu.hip -- the device code of ONE metric: compiled once per metric id and per precision,
//
//     hipcc ... -DGR_TU_METRIC=<GR_METRIC_* id> -c kernels_tu.hip -o kernels_m<id>.o                       (fp64)
//     hipcc ... -DGR_TU_METRIC=<id> -DGR_TU_F32 -Xclang -cl-single-precision-constant ... -o kernels32_m<id>.o   (fp32)
//     hipcc ... -DGR_TU_METRIC=<id> -DGR_TU_TAN -c kernels_tu.hip -o kernelstan_m<id>.o                     (tangent, one lane per ray)
//     hipcc ... -DGR_TU_METRIC=<id> -DGR_TU_TAN1 -c kernels_tu.hip -o kernelstan1_m<id>.o                   (tangent, a pair of lanes per ray)
//     hipcc ... -DGR_TU_METRIC=<id> -DGR_TU_TAN[1] -DGR_TU_SKY -c kernels_tu.hip -o kernelssky[1]_m<id>.o    (the two tangent shapes for sky cells)
//     hipcc ... -DGR_TU_METRIC=<id> -DGR_TU_AREA -c kernels_tu.hip -o kernelsarea_m<id>.o                   (fp64, k_disc_area_factor alone)
//     hipcc ... -DGR_TU_METRIC=<id> -DGR_TU_TAN1 -DGR_TU_SOLVE -c kernels_tu.hip -o kernelssolve1_m<id>.o    (pairs; k_offset_solve, k_offset_search alone)
//     hipcc ... -DGR_TU_METRIC=<id> -DGR_TU_RT -c kernels_tu.hip -o kernelsrt_m<id>.o                       (fp64, TraceRadiativeTransfer; metrics with an ISCO)
//     hipcc ... -DGR_TU_METRIC=12 -DGR_TU_USER -DGR_USER_COMPONENTS_FILE=\"<body>\" [one of the flag sets above but fp32] ...  (a user's metric:
//               gr_usermetric.hpp; the seven objects are linked into a module of their own, not into the library -- metrics.CompiledMetric)
//
// so that every metric's kernels hold only that metric's component function (gr_device.hpp, GenericMetricT) and the
// library builds on all cores at once (__graft_entry__.build_hip).  The fp32 objects are the same source with
// real = float (every floating literal of gr_device.hpp / gr_kernels.hpp is single precision there); they carry the
// trace kernels only: gr_ctx_set(ctx, "precision", 32) selects them for tolerance sweeps.  Inputs, outputs and tables
// stay double in both.
//
// Exports (plain signatures: the host unit, gradus_mi355x.hip, passes its gr::Params by address -- gr32::Params has the
// same layout, its fields are double / integer / pointers only):
//     gr64_launch_trace_m<ID>, gr64_launch_path_m<ID>, gr64_launch_apply_m<ID>, gr64_launch_classify_m<ID>, gr64_launch_areafactor_m<ID> (-DGR_TU_AREA)      gr32_launch_trace_m<ID>      grt_launch_trace_m<ID>      grt1_launch_trace_m<ID>      grts_launch_trace_m<ID>      grts1_launch_trace_m<ID>      grv1_launch_offset_m<ID> (-DGR_TU_SOLVE)      grrt_launch_trace_m<ID> (-DGR_TU_RT)
#ifndef GR_TU_METRIC
#error "compile with -DGR_TU_METRIC=<metric id>"
#endif
#if defined(GR_TU_TAN) || defined(GR_TU_TAN1)
// third flavour: real = value + tangents (gr_tangent.hpp), the one-ray-per-lane kernel only, one wave per SIMD, in TWO shapes
// (round 4; measured with scripts/wave_timeline.py, scripts/lineprofile_tf_time.py; profiles/r4_tangent_*):
//   GR_TU_TAN   namespace grt,  GR_TAN_W = 2: one lane carries a ray with both directions of the Jacobian (455 registers, no
//               scratch).  The THROUGHPUT shape: 1024² rays in 20.9 ms.
//   GR_TU_TAN1  namespace grt1, GR_TAN_W = 1: a PAIR of lanes per ray, one direction each (299 registers, no scratch).  A
//               wave's step is a long dependent chain and a lane with one direction has 1750 instead of 2900 vector
//               instructions in it: 8.8 instead of 10.3 µs per step.  The LATENCY shape: the default line profile of the
//               reference (TransferFunctionMethod: 909 launches of ~126 rays, each as long as its longest ray) takes 1.16 s
//               with it against 1.55 s -- and 24.5 ms against 20.9 for the 1024² launch, where the value part computed
//               twice costs more than the shorter chain saves.
// The host unit picks per launch (gr_ctx_set "tangent_pairs": launches that cannot fill the SIMDs anyway take the pairs).
// A 256-register variant of the pair shape (two waves per SIMD, stage accelerations parked in LDS) was measured and lost
// to both (24.5 ms; 1.31 s).
// Both shapes once more with -DGR_TU_SKY (namespaces grts, grts1): the same kernels with the sky-cell branches of gr_device.hpp
// compiled in (GR_SKYCELL: the (θ, ϕ) seed of src_mode 1, the row of out_mode 6) for gr_sky_cells.  An instantiation of their own
// because the two branches, though outside the step loop, move the register allocation of the kernels above (Kerr, one lane per
// ray: -6 ... +8 VGPRs over the disc types, 439 -> 447 for the datum plane; a tabulated metric's pairs: -32 ... +32 bytes of
// scratch -- DESIGN_measurements.md §M31), which stay as they were.
#define GR_REAL_IS_TAN2 1
#if defined(GR_TU_SKY)
#define GR_SKYCELL 1
#endif
#if defined(GR_TU_TAN1)
#define GR_TAN_W 1
#if defined(GR_TU_SOLVE)
#define GR_NS grv1
#define GR_TU_PREFIX grv1
#elif defined(GR_TU_SKY)
#define GR_NS grts1
#define GR_TU_PREFIX grts1
#else
#define GR_NS grt1
#define GR_TU_PREFIX grt1
#endif
#else
#define GR_TAN_W 2
#if defined(GR_TU_SKY)
#define GR_NS grts
#define GR_TU_PREFIX grts
#else
#define GR_NS grt
#define GR_TU_PREFIX grt
#endif
#endif
#define GR_LANE_ONLY 1
#define GR_LANE_MIN_WAVES 1  // waves per SIMD the tangent kernels are compiled for
#elif defined(GR_TU_RT)
// TraceRadiativeTransfer (namespace grrt; gr_device.hpp, GR_RADTRANS): fp64, the one-ray-per-lane kernel only, for the two
// optically thick discs.  The ray carries a ninth component I with its seven stage derivatives and goes THROUGH the surface.
// An object of its own (the GR_TU_SKY precedent): everything the flavour adds to the headers sits behind GR_RADTRANS, and the
// other objects compile to what they did without it (scripts/isa_compare.py; DESIGN_measurements.md).  Two waves per SIMD: the
// ray's sixteen doubles more do not fit the 168 registers of three (registers, scratch: DESIGN_measurements.md).
#define GR_RADTRANS 1
#define GR_NS grrt
#define GR_TU_PREFIX grrt
#define GR_LANE_ONLY 1
#define GR_LANE_MIN_WAVES 2
#elif defined(GR_TU_F32)
#define GR_REAL_IS_FLOAT 1
#define GR_NS gr32
#define GR_TU_PREFIX gr32
#else
#define GR_NS gr
#define GR_TU_PREFIX gr64
#endif
#include <hip/hip_runtime.h>

#include "gr_kernels.hpp"
#if defined(GR_TU_SOLVE)
#include "gr_offsetsolve.hpp"
#endif
#if defined(GR_TU_USER)
// GR_METRIC_COMPILED: the component function of GenericMetricT<12> comes from the file named on the compile line.  Its explicit
// specialisation has to stand before the launchers below instantiate the kernels with it.
#include "gr_usermetric.hpp"
#endif

#define GR_CAT3_(a, b, c) a##b##c
#define GR_CAT3(a, b, c) GR_CAT3_(a, b, c)
#define GR_TU_NAME(what) GR_CAT3(GR_TU_PREFIX, what, GR_TU_METRIC)
// the library's own objects are linked with the host unit (C++ names); a module is found by dlsym: C names
#if defined(GR_TU_USER)
#define GR_TU_EXPORT extern "C"
#else
#define GR_TU_EXPORT
#endif

namespace {
typedef GR_NS::MetricOf<GR_TU_METRIC>::type TuMetric;
}

#if defined(GR_TU_AREA)
// γ(r) A(r) of the disc at n radii (k_disc_area_factor): the emissivity weight of a resident sky's (r, ϕ) map (gr_sky_bin_grid).
// An object of its own (the GR_TU_SKY precedent): inside the fp64 object it left every trace kernel as it was but moved the
// operands of k_tile_classify (47 of 2004 instructions, Kerr; scripts/isa_compare.py).
GR_TU_EXPORT hipError_t GR_TU_NAME(_launch_areafactor_m)(const void* params, const double* r, double* out, hipStream_t stream)
{
    return GR_NS::launch_areafactor_metric<TuMetric>(*reinterpret_cast<const GR_NS::Params*>(params), r, out, stream);
}
#elif defined(GR_TU_SOLVE)
// The offset solve and the extremum search of the transfer functions, one problem per lane pair (gr_offsetsolve.hpp: k_offset_solve,
// k_offset_search).  An object of its own (the GR_TU_SKY precedent): the pair-shape trace kernel of kernelstan1_m<id>.o stays as
// it is, and this object carries no trace kernel.  `dev` is a gr_os::OffsetDev.
GR_TU_EXPORT hipError_t GR_TU_NAME(_launch_offset_m)(const void* params, const void* dev, int search, hipStream_t stream)
{
    GR_NS::Params p = *reinterpret_cast<const GR_NS::Params*>(params);
    return GR_NS::launch_offset_metric<TuMetric>(p, *reinterpret_cast<const gr_os::OffsetDev*>(dev), search != 0, stream);
}
#else
GR_TU_EXPORT hipError_t GR_TU_NAME(_launch_trace_m)(int kernel, int block, int n_cu, int waves_per_simd, unsigned long long* queue,
                                       const void* params, hipStream_t stream)
{
    GR_NS::Params p = *reinterpret_cast<const GR_NS::Params*>(params);
    GR_NS::LaunchKnobs k{ kernel, block, n_cu, waves_per_simd, queue };
    return GR_NS::launch_metric<TuMetric>(k, p, stream);
}
#endif

#if !defined(GR_TU_F32) && !defined(GR_TU_TAN) && !defined(GR_TU_TAN1) && !defined(GR_TU_AREA) && !defined(GR_TU_RT)
GR_TU_EXPORT hipError_t GR_TU_NAME(_launch_path_m)(const void* params, double* d_path, int64_t cap, unsigned long long* d_n, hipStream_t stream)
{
    return GR_NS::launch_path_metric<TuMetric>(*reinterpret_cast<const GR_NS::Params*>(params), d_path, cap, d_n, stream);
}

GR_TU_EXPORT hipError_t GR_TU_NAME(_launch_apply_m)(const void* params, const gr_point* pts, double max_time, double* out, hipStream_t stream)
{
    return GR_NS::launch_apply_metric<TuMetric>(*reinterpret_cast<const GR_NS::Params*>(params), pts, max_time, out, stream);
}

// the live-first tile order's flags for the launch `params` describes (gr_tile_order.hpp); an error for a metric without the start cull
GR_TU_EXPORT hipError_t GR_TU_NAME(_launch_classify_m)(const void* params, uint8_t* flags, int64_t tiles, hipStream_t stream)
{
    return GR_NS::launch_classify_metric<TuMetric>(*reinterpret_cast<const GR_NS::Params*>(params), flags, tiles, stream);
}
#endif

#if defined(GR_TU_USER) && !defined(GR_TU_AREA) && !defined(GR_TU_SOLVE) && !defined(GR_TU_SKY)
// a module's trace kernels answer for their registers and scratch (gr_metric_module_resources): kernel 0 = lane, 1 = persistent
GR_TU_EXPORT hipError_t GR_TU_NAME(_kernel_attrs_m)(int kernel, int disc_id, hipFuncAttributes* out)
{
    return GR_NS::kernel_attrs_metric<TuMetric>(kernel, disc_id, out);
}
#if !defined(GR_TU_TAN) && !defined(GR_TU_TAN1)
// ... and the fp64 unit says what the module was made from (include/gradus_mi355x.h)
extern "C" const gr_user_module_info_t* gr_user_module_info(void)
{
    static const gr_user_module_info_t info = { GR_ABI_VERSION, GR_METRIC_COMPILED, GR_USER_BUILD_ID, { GR_CSRC_HASH } };
    return &info;
}
#endif
#endif
