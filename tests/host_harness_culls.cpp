// host_harness_culls.cpp -- TEST INFRASTRUCTURE.  The device integrator (gr_device.hpp) compiled for the host with g++, for the miss
// culls of the fused fp64 Kerr kernels (Ray::start_decided, Ray::step): whole 8 x 8 tiles of an image plane traced,
// lanes as the one-ray-per-lane kernel lays them out, with the step loop's culls (escape and polar-rate), the decisions at the
// start, the pass cull (at any ζ), the entry cull and the defer cull switched one by one, as the launcher's environment switches
// do; per ray what the culls must not change (pixel, status), what they must (steps) and which of them ended it; and, ray by ray,
// the bounds the pass cull and the entry cull decide by.  Built with -DGR_DEFER_CULL_ZETA=... it is the census that chose
// kDeferCullZeta (scripts/cull_census.py --defer-cull).  Never linked into libgradus_mi355x.so.
#define GR_HOST_HARNESS 1
#ifndef GR_DEFER_CULL_ZETA
#define HHC_LIBRARY_CONSTANTS 1      // not a census build: the constants are the library's
#endif
#include <algorithm>
#include <cmath>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_device.hpp"
#include "host_harness_common.hpp"

using namespace GR_NS;

#ifdef HHC_LIBRARY_CONSTANTS
static_assert(kEntryCullZeta < kDeferCullZeta && kDeferCullZeta < kPassCullZeta, "ζ_dip < ζ_defer < ζ");
#endif
static_assert(RAY_DEFER_DECIDED < RAY_NO_CULL && RAY_DEFER_DECIDED != RAY_ENTRY_ARMED && RAY_DEFER_DECIDED != RAY_EVENT
                  && (RAY_DEFER_DECIDED & (GR_FLAG_MAXITERS | GR_FLAG_DTMIN | GR_FLAG_NAN)) == 0,
              "the defer cull's bit: below RAY_NO_CULL, apart from the other bits");

namespace {

typedef Ray<KerrMetric, GR_DISC_THIN> KerrRay;

// zeta < 0: the library's constant (pass_cull_radius); 0: the pass cull off; else R_pass = zeta R_cull
double pass_radius(double gate, double zeta)
{
    if (!(gate < HUGE_VAL) || zeta == 0.0) return HUGE_VAL;
    return zeta < 0.0 ? pass_cull_radius(gate) : zeta * gate;
}

void fill(Params& p, Cold& c, const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf)
{
    const int64_t n = plane->width * plane->height;
    hh::fill_plane(p, c, cfg, plane, gr_range{ 0, n, n, 1 }, 0, pf);
}

// Slots 0-15 of a row of hhc_pass_bounds / hhc_entry_bounds: the constants of motion of the state (r, θ, v), and what
// pass_cull_bounds forms for a turning point outside r_in.
void bounds_row(const KerrMetric& m, double r, double th, double s, double cth, const double* v, double gate, double r_in, double gtol,
                double* o)
{
    double g[5];
    metric_comps(m, r, th, s, cth, g);
    const double E = -(g[0] * v[0] + g[4] * v[3]), L = g[4] * v[0] + g[3] * v[3];
    const double Q = m.carter_constant(g[2] * v[2], s, cth, E, L);
    KerrMetric::PassBounds b;
    const bool dec = KerrMetric::pass_cull_bounds(m.M, m.a, E, L, Q, 1.0 / r, 1.0 / gate, 1.0 / r_in, cth, v[2] <= 0.0, gtol, b);
    o[0] = E; o[1] = L; o[2] = Q; o[3] = 1.0 / r; o[4] = 1.0 / gate; o[5] = cth; o[6] = v[2] <= 0.0 ? 1.0 : 0.0; o[7] = v[1];
    o[8] = b.u_lo; o[9] = b.u_hi; o[10] = b.Ta_lo; o[11] = b.Tb_hi; o[12] = b.Om_lo; o[13] = b.Om_hi; o[14] = b.psi0;
    o[15] = dec ? 1.0 : 0.0;
}

}      // namespace

extern "C" {

// The gating radius the launcher passes for a fused-Kerr scene: the library's own function (cull_gate_radius, gr_device.hpp), with
// the winding callback the launcher folds into cfg.upper_hemisphere (stage_disc_table) excluded here.  +inf where gated off.
double hhc_gate_radius(const gr_config* c)
{
    if (c->metric_id != GR_METRIC_KERR || c->count_windings != 0) return HUGE_VAL;
    return cull_gate_radius(*c, KerrMetric::kEscapeRadiusM);
}
double hhc_zeta(void) { return kPassCullZeta; }
double hhc_zeta_dip(void) { return kEntryCullZeta; }
double hhc_zeta_defer(void) { return kDeferCullZeta; }
// what memset + derive_params leave in Params::entry_cull and Params::defer_cull (hhc_render_tiles' entry = defer = 1): must be 1, 1
void hhc_default_culls(int32_t* entry, int32_t* defer)
{
    Params p;
    std::memset(&p, 0, sizeof p);
    derive_params(p);
    *entry = p.entry_cull;
    *defer = p.defer_cull;
}

// per ray, in tile-major lane order (64 per tile)
struct hhc_out {
    double* image;            // the pixel finalize() writes (out_mode 0)
    int32_t* status;          // hh::status_code
    int32_t* nacc;            // accepted steps
    int32_t* nrej;            // rejected steps
    int32_t* at_start;        // 1 = Ray::init decided it
    int32_t* by_pass;         // 1 = ... and would not have with the pass cull off (a second init with r_pass = +inf)
    int32_t* marked;          // 1 = Ray::init left it RAY_DEFER_DECIDED
    int32_t* defer_end;       // 1 = the step that cleared that bit also ended it at λ1
    int32_t* entry_step;      // the attempted step (accepted + rejected, from 1) at which the entry cull ended it, else 0
    double* r_start;          // r and v^r at the start
    double* vr_start;
    double* r_last;           // r and v^r after the last step (the start state of a ray that took none)
    double* vr_last;
};

// Tiles `tiles` (index = tile column * (H / 8) + tile row) of the plane, 64 rays each.  step_cull / start_cull: 0 = that mechanism
// off (radius +inf), else the gating radius.  zeta: pass_radius.  entry, defer: 1 = as derive_params leaves it, 0 = off alone.
// A ray counts as ended on entry when the step that cleared its RAY_ENTRY_ARMED bit also ended it at λ1 with v^r < 0: no other
// end of a ray moves λ to λ1 going in (the escape and polar-rate culls ask v^r > 0; λ1 itself is reached far outside R_cull).
// Returns -1 for a scene the launcher would gate off, or one that is not a fused Kerr with a thin disc.
int hhc_render_tiles(const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf, const int64_t* tiles, int64_t n_tiles,
                     int step_cull, int start_cull, double zeta, int entry, int defer, const hhc_out* o)
{
    const double gate = hhc_gate_radius(cfg);
    if (!(gate < HUGE_VAL) || pf->filter_id != GR_FILTER_INTERSECTED) return -1;
    Params p; Cold c;
    fill(p, c, cfg, plane, pf);
    const int64_t H = plane->height, n = plane->width * H;
    p.r_cull = step_cull ? gate : HUGE_VAL;
    p.r_cull_start = start_cull ? gate : HUGE_VAL;
    p.r_pass = pass_radius(p.r_cull_start, zeta);
    if (!entry) p.entry_cull = 0;
    if (!defer) p.defer_cull = 0;
    Params p_nopass = p;
    p_nopass.r_pass = HUGE_VAL;
    std::vector<double> img((size_t)n, 0.0);
    c.image = img.data();
    KerrMetric m;
    m.load(p.cfg);
    const LdsView no_lds = hh::no_lds();
    for (int64_t t = 0; t < n_tiles; ++t) {
        for (int l = 0; l < 64; ++l) {
            const int64_t j = hh::tile_lane_ray(tiles[t], l, H);
            if (j >= n) return -2;
            const int64_t k = 64 * t + l;
            KerrRay ray;
            const bool decided = ray.init(m, p, j);
            o->at_start[k] = decided ? 1 : 0;
            o->by_pass[k] = 0;
            o->r_start[k] = ray.x[1];
            o->vr_start[k] = ray.v[1];
            o->marked[k] = (!decided && (ray.flags & RAY_DEFER_DECIDED)) ? 1 : 0;
            o->defer_end[k] = 0;
            o->entry_step[k] = 0;
            if (decided) {
                KerrRay probe;
                o->by_pass[k] = probe.init(m, p_nopass, j) ? 0 : 1;
            } else {
                bool done = false;
                while (!done) {
                    const bool armed = (ray.flags & RAY_ENTRY_ARMED) != 0, deferred = (ray.flags & RAY_DEFER_DECIDED) != 0;
                    done = ray.step(m, p);
                    if (done && armed && !(ray.flags & RAY_ENTRY_ARMED) && ray.v[1] < 0.0 && ray.t == p.cfg.lambda1)
                        o->entry_step[k] = ray.nacc + ray.nrej;
                    if (done && deferred && !(ray.flags & RAY_DEFER_DECIDED) && ray.t == p.cfg.lambda1) o->defer_end[k] = 1;
                }
            }
            o->r_last[k] = ray.x[1];
            o->vr_last[k] = ray.v[1];
            ray.finalize(m, p, no_lds);
            o->image[k] = img[(size_t)j];
            o->status[k] = hh::status_code(ray);
            o->nacc[k] = ray.nacc;
            o->nrej[k] = ray.nrej;
        }
    }
    return 0;
}

// The pass cull's quantities for rays `rays` (plane indices) of a scene, 16 doubles per ray:
//   0 E  1 L  2 Q  3 u0  4 uc  5 μ0  6 dμ/dτ >= 0 (1 / 0)  7 v^r
//   8 u_lo  9 u_hi  10 T_a^lo  11 T_b^hi  12 Ω_lo  13 Ω_hi  14 ψ0  15 the decision of pass_cull_bounds (1 / 0)
// (8-14 hold what the function had formed when it returned; a condition that fails early leaves zeros behind it.)  The decision
// here is that of the closed forms alone: Ray::start_decided adds r0 > R_cull, v^r < 0, "the start cull's own test failed" and
// the bound on r_outer.
int hhc_pass_bounds(const gr_config* cfg, const gr_plane* plane, const int64_t* rays, int64_t n_rays, double zeta, double* out)
{
    const double gate = hhc_gate_radius(cfg);
    if (!(gate < HUGE_VAL)) return -1;
    Params p; Cold c;
    fill(p, c, cfg, plane, nullptr);
    const double r_pass = pass_radius(gate, zeta);
    KerrMetric m;
    m.load(p.cfg);
    for (int64_t i = 0; i < n_rays; ++i) {
        double x[4], v[4], s, cth;
        KerrRay::constrained_u0(m, p, rays[i], x, v);
        sincos_fast(x[2], s, cth);
        bounds_row(m, x[1], x[2], s, cth, v, gate, r_pass, cfg->gtol, out + 16 * i);
    }
    return 0;
}

// The entry cull's quantities for rays `rays` (plane indices) of a scene, at the state in which Ray::step asks: the end of the first
// accepted step with r <= R_cull of a ray that started outside R_cull going in and was not decided at the start (ζ as above),
// every cull of the step loop off.  18 doubles per ray: 0-15 as hhc_pass_bounds, at that state (3 u0 = 1/r there) and with the
// decision at R_dip,
//   16 asked (1: the ray reached such a state with v^r < 0 and the disc condition > 0; 0: the rest is zero)  17 steps taken by then
int hhc_entry_bounds(const gr_config* cfg, const gr_plane* plane, const int64_t* rays, int64_t n_rays, double zeta, double* out)
{
    const double gate = hhc_gate_radius(cfg);
    if (!(gate < HUGE_VAL)) return -1;
    Params p; Cold c;
    fill(p, c, cfg, plane, nullptr);
    p.r_cull_start = gate;
    p.r_pass = pass_radius(gate, zeta);
    KerrMetric m;
    m.load(p.cfg);
    for (int64_t i = 0; i < n_rays; ++i) {
        double* o = out + 18 * i;
        std::fill(o, o + 18, 0.0);
        KerrRay ray;
        if (ray.init(m, p, rays[i]) || !(ray.x[1] > gate) || !(ray.v[1] < 0.0)) continue;
        bool done = false;
        while (!done && ray.x[1] > gate) done = ray.step(m, p);
        if (done || !(ray.v[1] < 0.0) || !(ray.cprev > 0.0)) continue;
        bounds_row(m, ray.x[1], ray.x[2], ray.sth, ray.cth, ray.v, gate, kEntryCullZeta * gate, cfg->gtol, o);
        o[16] = 1.0; o[17] = (double)(ray.nacc + ray.nrej);
    }
    return 0;
}
}
