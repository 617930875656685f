// gr_usermetric.hpp -- GR_METRIC_COMPILED: a user's metric_components as an instantiation of the library's own kernels.
//
// The catalogue's dual-number form (GenericMetricT<ID>::components on typed duals, eval() + geodesic_contract; gr_device.hpp) is
// what the reference does for ANY metric through ForwardDiff.  This header gives that form a way in for a metric the library was
// not built with: kernels_tu.hip, compiled with
//
//     -DGR_TU_METRIC=12 -DGR_TU_USER -DGR_USER_COMPONENTS_FILE=\"/path/to/body.inc\"
//
// includes it between gr_kernels.hpp and the launchers, and the explicit specialisation below makes the file named on the compile
// line the body of GenericMetricT<GR_METRIC_COMPILED>::components.  MetricOf<12> is the primary template: GenericMetricT<12>,
// kFusedRhs == false, two waves per SIMD, never culled.  Nothing in gr_device.hpp or gr_kernels.hpp changes, and no object of the
// library includes this header: the seven units of a user's metric are linked into a module of their own, which the host unit
// loads at run time (gr_metric_module_load).
//
// What a body may use (it is straight-line code; a metric with branches keeps the table, GR_METRIC_TABULATED):
//     r, s, c          the radius, sin θ, cos θ -- typed duals under eval() (DualR, DualT, DualT), plain `real` under comps()
//     P[0..5]          gr_config.params: run-time parameters, a fit that moves them does not recompile
//     + - *            the operators of DualP / real; a literal is a plain double
//     inv_(x)          the reciprocal (division is written x * inv_(y))
//     dsqrt, dexp, dlog, dpowi<N>        below: each keeps the typed partials (an absent partial stays absent)
//     dput(g[i], x)    stores component i (tt, rr, θθ, ϕϕ, tϕ); a component that depends on neither coordinate is written
//                      (r - r) + k, as the catalogue's flat space does
#pragma once

#ifndef GR_USER_COMPONENTS_FILE
#error "compile with -DGR_USER_COMPONENTS_FILE=\"<file with the body of components()>\""
#endif
#ifdef GR_REAL_IS_FLOAT
#error "a compiled metric has no fp32 flavour"
#endif

namespace GR_NS {

static_assert(GR_METRIC_COMPILED == 12, "the module's launchers are named ..._m12");

// ---- elementary functions on `real`: double in the fp64 kernels, value + tangents in the tangent flavour ----
#ifdef GR_REAL_IS_TAN2
GR_DEV real dsqrt(real x) { return gr_t_sqrt(x); }
GR_DEV real dexp(real x)
{
    const double e = ::exp(x.v);
    x.v = e; x.a *= e; GR_TAN_B(x.b *= e;)
    return x;
}
GR_DEV real dlog(real x)
{
    const double i = gr_d_rcp(x.v);
    x.v = ::log(x.v); x.a *= i; GR_TAN_B(x.b *= i;)
    return x;
}
#else
GR_DEV real dsqrt(real x) { return sqrt_fast(x); }
GR_DEV real dexp(real x) { return ::exp(x); }
GR_DEV real dlog(real x) { return ::log(x); }
#endif

// ---- ... and on typed duals: f(x) carries f'(x) x' in the partials x has ----
template <bool A, bool B>
GR_DEV DualP<A, B> dsqrt(DualP<A, B> x)
{
    const real q = dsqrt(x.v);
    const real h = 0.5 * rcp_full(q);
    return { q, A ? h * x.a : x.a, B ? h * x.b : x.b };
}
template <bool A, bool B>
GR_DEV DualP<A, B> dexp(DualP<A, B> x)
{
    const real e = dexp(x.v);
    return { e, A ? e * x.a : x.a, B ? e * x.b : x.b };
}
template <bool A, bool B>
GR_DEV DualP<A, B> dlog(DualP<A, B> x)
{
    const real i = rcp_full(x.v);
    return { dlog(x.v), A ? i * x.a : x.a, B ? i * x.b : x.b };
}
// x^N for a literal N >= 1 by repeated multiplication, left to right: x, x x, (x x) x, ...
template <int N, class T>
GR_DEV T dpowi(T x)
{
    static_assert(N >= 1, "dpowi<N>: N >= 1 (a negative power is inv_ of a positive one)");
    T y = x;
#pragma unroll
    for (int k = 1; k < N; ++k) y = y * x;
    return y;
}

// ---- the user's component function ----
template <>
template <class TR, class TT, class TG>
GR_DEV void GenericMetricT<GR_METRIC_COMPILED>::components(TR r, TT s, TT c, TG g[5]) const
{
    (void)r; (void)s; (void)c;
#include GR_USER_COMPONENTS_FILE
}

}  // namespace GR_NS

#ifndef GR_HOST_HARNESS
// ---- what a module says about itself (include/gradus_mi355x.h, gr_user_module_info_t): once per module, in the fp64 unit ----
#ifndef GR_USER_BUILD_ID
#define GR_USER_BUILD_ID 0
#endif
#ifndef GR_CSRC_HASH
#define GR_CSRC_HASH 0, 0, 0, 0
#endif
namespace GR_NS {
namespace {
// registers, scratch and LDS of the trace kernel a launch with this disc type would take (hipFuncGetAttributes)
template <class Metric, int DISC>
hipError_t kernel_attrs_tmpl(int kernel, hipFuncAttributes* out)
{
#ifndef GR_LANE_ONLY
    if (kernel != 0) return hipFuncGetAttributes(out, reinterpret_cast<const void*>(&k_trace_persistent<Metric, DISC>));
#endif
    (void)kernel;
    return hipFuncGetAttributes(out, reinterpret_cast<const void*>(&k_trace_lane<Metric, DISC>));
}
template <class Metric>
hipError_t kernel_attrs_metric(int kernel, int disc_id, hipFuncAttributes* out)
{
    switch (disc_id) {
    case GR_DISC_THIN: return kernel_attrs_tmpl<Metric, GR_DISC_THIN>(kernel, out);
    case GR_DISC_SHAKURA_SUNYAEV: return kernel_attrs_tmpl<Metric, GR_DISC_SHAKURA_SUNYAEV>(kernel, out);
    case GR_DISC_TABULATED: return kernel_attrs_tmpl<Metric, GR_DISC_TABULATED>(kernel, out);
    case GR_DISC_DATUM: return kernel_attrs_tmpl<Metric, GR_DISC_DATUM>(kernel, out);
    case GR_DISC_ELLIPTICAL: return kernel_attrs_tmpl<Metric, GR_DISC_ELLIPTICAL>(kernel, out);
    case GR_DISC_PRECESSING_THIN: return kernel_attrs_tmpl<Metric, GR_DISC_PRECESSING_THIN>(kernel, out);
    case GR_DISC_COMPOSITE: return kernel_attrs_tmpl<Metric, GR_DISC_COMPOSITE>(kernel, out);
#if GR_HAS_MESH
    case GR_DISC_MESH: return kernel_attrs_tmpl<Metric, GR_DISC_MESH>(kernel, out);
#endif
    default: return kernel_attrs_tmpl<Metric, GR_DISC_NONE>(kernel, out);
    }
}
}  // namespace
}  // namespace GR_NS
#endif
