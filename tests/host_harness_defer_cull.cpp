// host_harness_defer_cull.cpp -- TEST INFRASTRUCTURE.  The device integrator (gr_device.hpp) compiled for the host with g++, for the
// defer cull (Ray::start_decided, Ray::step): whole 8 x 8 tiles traced with the step loop's culls, the decisions at
// the start (at any ζ), the entry cull and the defer cull switched one by one, which rays the start marked for the defer cull,
// which rays it ended, and which rays the entry cull ended.  Built with -DGR_DEFER_CULL_ZETA=... it is the census that chose
// kDeferCullZeta (scripts/cull_census.py --defer-cull).  Never linked into libgradus_mi355x.so.
#define GR_HOST_HARNESS 1
#ifndef GR_DEFER_CULL_ZETA
#define HHD_LIBRARY_CONSTANTS 1      // not a census build: the constants are the library's
#endif
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_device.hpp"

using namespace GR_NS;

#ifdef HHD_LIBRARY_CONSTANTS
static_assert(kEntryCullZeta < kDeferCullZeta && kDeferCullZeta < kPassCullZeta, "ζ_dip < ζ_defer < ζ");
#endif
static_assert(RAY_DEFER_DECIDED < RAY_NO_CULL && RAY_DEFER_DECIDED != RAY_ENTRY_ARMED && RAY_DEFER_DECIDED != RAY_EVENT
                  && (RAY_DEFER_DECIDED & (GR_FLAG_MAXITERS | GR_FLAG_DTMIN | GR_FLAG_NAN)) == 0,
              "the defer cull's bit: below RAY_NO_CULL, apart from the other bits");

namespace {

double gate_radius(const gr_config* c)
{
    if (c->metric_id != GR_METRIC_KERR || c->count_windings != 0) return HUGE_VAL;
    return cull_gate_radius(*c, KerrMetric::kEscapeRadiusM);
}

// zeta < 0: the library's constant (pass_cull_radius); 0: the pass cull off; else R_pass = zeta R_cull
double pass_radius(double gate, double zeta)
{
    if (!(gate < HUGE_VAL) || zeta == 0.0) return HUGE_VAL;
    return zeta < 0.0 ? pass_cull_radius(gate) : zeta * gate;
}

void fill(Params& p, Cold& c, const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf)
{
    std::memset(&p, 0, sizeof p); std::memset(&c, 0, sizeof c);
    const int64_t n = plane->width * plane->height;
    p.cfg = *cfg; p.n = n; p.cold = &c; c.winding_plane = cfg->winding_plane;
    c.src_mode = 0; c.out_mode = 0; c.plane = *plane; c.range = gr_range{ 0, n, n, 1 };
    if (pf) {
        c.pf.pf_id = pf->pf_id; c.pf.filter_id = pf->filter_id; c.pf.fill = pf->fill; c.pf.r_isco = pf->r_isco;
        c.pf.n_plunge = pf->n_plunge; c.pf.plunge_r = pf->plunge_r; c.pf.plunge_vt = pf->plunge_vt;
        c.pf.plunge_vr = pf->plunge_vr; c.pf.plunge_vphi = pf->plunge_vphi;
    }
    derive_params(p);
}

}      // namespace

extern "C" {

double hhd_gate_radius(const gr_config* c) { return gate_radius(c); }
double hhd_zeta(void) { return kPassCullZeta; }
double hhd_zeta_dip(void) { return kEntryCullZeta; }
double hhd_zeta_defer(void) { return kDeferCullZeta; }
// what memset + derive_params leave in Params::defer_cull (the older harnesses fill Params that way): must be 1
int hhd_default_defer_cull(void)
{
    Params p;
    std::memset(&p, 0, sizeof p);
    derive_params(p);
    return p.defer_cull;
}

// As hhe_render_tiles (host_harness_entry_cull.cpp), with the defer cull as a fifth switch (defer: 1 = as derive_params leaves it,
// 0 = off alone).  at_start: 0 = traced, 1 = decided at the start.  marked: 1 = Ray::init left the ray RAY_DEFER_DECIDED.
// defer_end: 1 = the step that cleared that bit also ended the ray at λ1.  entry_step: as there (the attempted step at which the
// entry cull ended the ray, else 0).  r_start, vr_start: r and v^r at the start.
int hhd_render_tiles(const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf, const int64_t* tiles, int64_t n_tiles,
                     int step_cull, int start_cull, double zeta, int entry, int defer, double* image, int32_t* status, int32_t* nacc,
                     int32_t* nrej, int32_t* at_start, int32_t* marked, int32_t* defer_end, int32_t* entry_step, double* r_start,
                     double* vr_start)
{
    const double gate = gate_radius(cfg);
    if (!(gate < HUGE_VAL) || pf->filter_id != GR_FILTER_INTERSECTED) return -1;
    Params p; Cold c;
    fill(p, c, cfg, plane, pf);
    const int64_t H = plane->height, n = plane->width * H;
    p.r_cull = step_cull ? gate : HUGE_VAL;
    p.r_cull_start = start_cull ? gate : HUGE_VAL;
    p.r_pass = pass_radius(p.r_cull_start, zeta);
    if (!entry) p.entry_cull = 0;
    if (!defer) p.defer_cull = 0;
    std::vector<double> img((size_t)n, 0.0);
    c.image = img.data();
    KerrMetric m;
    m.load(p.cfg);
    const int64_t tiles_per_col = H >> 3;
    const LdsView no_lds{ nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int64_t tx = tiles[t] / tiles_per_col, ty = tiles[t] - tx * tiles_per_col;
        for (int l = 0; l < 64; ++l) {
            const int64_t j = ((tx << 3) + (l >> 3)) * H + (ty << 3) + (l & 7);
            if (j >= n) return -2;
            const int64_t k = 64 * t + l;
            Ray<KerrMetric, GR_DISC_THIN> ray;
            const bool decided = ray.init(m, p, j);
            r_start[k] = ray.x[1];
            vr_start[k] = ray.v[1];
            marked[k] = (!decided && (ray.flags & RAY_DEFER_DECIDED)) ? 1 : 0;
            defer_end[k] = 0;
            entry_step[k] = 0;
            if (!decided) {
                bool done = false;
                while (!done) {
                    const bool armed = (ray.flags & RAY_ENTRY_ARMED) != 0, deferred = (ray.flags & RAY_DEFER_DECIDED) != 0;
                    done = ray.step(m, p);
                    if (done && armed && !(ray.flags & RAY_ENTRY_ARMED) && ray.v[1] < 0.0 && ray.t == p.cfg.lambda1)
                        entry_step[k] = ray.nacc + ray.nrej;
                    if (done && deferred && !(ray.flags & RAY_DEFER_DECIDED) && ray.t == p.cfg.lambda1) defer_end[k] = 1;
                }
            }
            ray.finalize(m, p, no_lds);
            image[k] = img[(size_t)j];
            status[k] = (ray.flags & GR_FLAG_MASK) ? -1 - (ray.flags & GR_FLAG_MASK) : ray.status;
            nacc[k] = ray.nacc;
            nrej[k] = ray.nrej;
            at_start[k] = decided ? 1 : 0;
        }
    }
    return 0;
}
}
