// host_harness_skycell.cpp -- TEST INFRASTRUCTURE.  The device integrator (gr_device.hpp) compiled for the host in its
// TANGENT flavour (real = gr_tan2: value + two tangents) for the cells of a source's sky: rays given as (x, v) with the
// seed ∂v/∂θ, ∂v/∂ϕ, sin θ per ray (Cold::v_tan) -> one (t, r, ϕ, g, J, status) row per ray (out_mode 6), so the CPU suite can
// check the seed, the row and the Jacobian without a GPU.
#define GR_HOST_HARNESS 1
#define GR_REAL_IS_TAN2 1
#define GR_SKYCELL 1
#define GR_NS grt
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../gradus.jl_amd/csrc/gr_device.hpp"
#include "host_harness_common.hpp"

using namespace grt;

template <class Metric, int DISC>
static void run(const Params& p)
{
    Metric m;
    m.load(p.cfg);
    const LdsView no_lds = hh::no_lds();
    for (int64_t j = 0; j < p.n; ++j) {
        Ray<Metric, DISC> ray;
        ray.init(m, p, j);
        while (!ray.step(m, p)) {}
        ray.finalize(m, p, no_lds);
    }
}

extern "C" {

int hhs_row_doubles() { return GR_SKYCELL_ROW; }
int hhs_seed_doubles() { return GR_SKYCELL_SEED; }

// x_src: 4; v: n x 4 (unconstrained); seed: n x GR_SKYCELL_SEED; out: n x GR_SKYCELL_ROW
int hhs_sky_cells(const gr_config* cfg, const gr_pointfunction* pf, const double* x_src, const double* v, const double* seed, int64_t n,
                  int tangent_norm, double* out)
{
    Params p; Cold c;
    hh::fill(p, c, cfg, n, pf);
    c.src_mode = 1; c.out_mode = 6;
    c.x = x_src; c.x_stride = 0; c.v = v; c.v_tan = seed;
    std::memcpy(c.plane.x_obs, x_src, sizeof c.plane.x_obs);
    c.range = gr_range{ 0, n, n > 0 ? n : 1, 1 };
    c.lp_rmin = 0.0; c.lp_rmax = INFINITY; c.lp_pairs = out;
    c.pf.has_u_src = pf->has_u_src ? 1 : 0;
    for (int q = 0; q < 4; ++q) c.pf.u_src[q] = pf->has_u_src ? pf->u_src[q] : (q == 0 ? 1.0 : 0.0);
    p.tangent_norm = tangent_norm ? 1 : 0;
    p.disc_table = p.cfg.disc_table;
    p.cfg.upper_hemisphere = (p.cfg.upper_hemisphere ? 1 : 0);      // (no PoloidalShapeChart, no winding count: as the tangent harness)
    const int disc = p.cfg.disc_id;
#define HH_RUN(M) \
    do { if (disc == GR_DISC_THIN) run<M, GR_DISC_THIN>(p); \
         else return -1; } while (0)
    if (p.cfg.metric_id == GR_METRIC_KERR) HH_RUN(KerrMetric);
    else if (p.cfg.metric_id == GR_METRIC_KERR_NEWMAN) HH_RUN(KerrNewmanMetric);
    else if (p.cfg.metric_id == GR_METRIC_JOHANNSEN) HH_RUN(JohannsenMetric);
    else HH_RUN(GenericMetric);
#undef HH_RUN
    return 0;
}
}
