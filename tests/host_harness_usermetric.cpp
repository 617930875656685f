// host_harness_usermetric.cpp -- TEST INFRASTRUCTURE.  A generated component body (gradus_jl_amd.compiled_metric) compiled for the
// host with g++ through the header the kernel modules use (gr_usermetric.hpp): GenericMetricT<12>::eval() at a point, and the
// device integrator on it ray by ray.  Built once per body: -DGR_USER_COMPONENTS_FILE="<body>".  Never linked into the library.
#define GR_HOST_HARNESS 1
#include <cmath>
#include <cstring>

#include "../gradus.jl_amd/csrc/gr_device.hpp"
#include "../gradus.jl_amd/csrc/gr_usermetric.hpp"
#include "host_harness_common.hpp"

using namespace GR_NS;

typedef MetricOf<GR_METRIC_COMPILED>::type UserMetric;
static_assert(!UserMetric::kFusedRhs, "a compiled metric takes eval() + geodesic_contract");

template <class Metric, int DISC>
static void run(const Params& p)
{
    Metric m;
    m.load(p.cfg);
    for (int64_t j = 0; j < p.n; ++j) {
        Ray<Metric, DISC> ray;
        ray.init(m, p, j);
        while (!ray.step(m, p)) {}
        ray.finalize(m, p, hh::no_lds());
    }
}

template <class Metric>
static void jac(const gr_config* cfg, double r, double th, double* g, double* dr, double* dth)
{
    Metric m;
    m.load(*cfg);
    double gi[5];
    m.eval(r, std::sin(th), std::cos(th), g, dr, dth, gi);
}

extern "C" {

// (g, ∂r g, ∂θ g) by the typed dual numbers: the generated body for metric ids >= GR_METRIC_COMPILED, the catalogue's own
// component functions through the same eval() otherwise (the yardstick of what rounding order alone costs)
int hu_jacobian(const gr_config* cfg, double r, double th, double* g, double* dr, double* dth)
{
    if (cfg->metric_id >= GR_METRIC_COMPILED) jac<UserMetric>(cfg, r, th, g, dr, dth);
    else if (cfg->metric_id == GR_METRIC_KERR || cfg->metric_id == GR_METRIC_KERR_NEWMAN || cfg->metric_id == GR_METRIC_TABULATED) return -1;
    else jac<GenericMetric>(cfg, r, th, g, dr, dth);
    return 0;
}

// values alone through comps() (plain `real` arguments: the overloads of dsqrt, dexp, dlog, dpowi on real)
int hu_components(const gr_config* cfg, double r, double th, double* g)
{
    UserMetric m;
    m.load(*cfg);
    m.comps(r, std::sin(th), std::cos(th), g);
    return 0;
}

int hu_render_endpoints(const gr_config* cfg, const gr_plane* plane, const gr_range* rg, gr_point* out)
{
    Params p; Cold c;
    hh::fill_plane(p, c, cfg, plane, *rg, 1, nullptr);
    c.points = out;
    p.disc_table = p.cfg.disc_table;
    p.cfg.upper_hemisphere = (p.cfg.upper_hemisphere ? 1 : 0) | (p.cfg.count_windings ? 4 : 0);
    if (p.cfg.disc_id == GR_DISC_THIN) run<UserMetric, GR_DISC_THIN>(p);
    else if (p.cfg.disc_id == GR_DISC_NONE) run<UserMetric, GR_DISC_NONE>(p);
    else return -1;
    return 0;
}

}
