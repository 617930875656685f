// host_harness_entry_cull.cpp -- TEST INFRASTRUCTURE.  The device integrator (gr_device.hpp) compiled for the host with g++, for the
// entry cull (Ray::step, KerrFamily::pass_cull_bounds): whole 8 x 8 tiles traced with the step loop's culls, the
// decisions at the start (at any ζ, for the census that chose the library's) and the entry cull switched one by one, which rays
// the entry cull ended and at which step, and, ray by ray, the bounds it decides by at the state in which it is asked.  Never
// linked into libgradus_mi355x.so.
#define GR_HOST_HARNESS 1
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_device.hpp"

using namespace GR_NS;

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

double hhe_gate_radius(const gr_config* c) { return gate_radius(c); }
double hhe_zeta(void) { return kPassCullZeta; }
double hhe_zeta_dip(void) { return kEntryCullZeta; }
// what memset + derive_params leave in Params::entry_cull (the older harnesses fill Params that way): must be 1
int hhe_default_entry_cull(void)
{
    Params p;
    std::memset(&p, 0, sizeof p);
    derive_params(p);
    return p.entry_cull;
}

// As hhp_render_tiles (host_harness_pass_cull.cpp), with the entry cull as a fourth switch (entry: 1 = as derive_params leaves
// it, 0 = off alone).  at_start: 0 = traced, 1 = decided at the start.  entry_step: the number of the attempted step (accepted +
// rejected, from 1) at which the entry cull ended the ray, 0 for every other ray; r_last, vr_last: r and v^r of the ray's state
// after its last step (the start state of a ray that took none); r_start: its r at the start.
// A ray counts as ended on entry when the step that cleared its RAY_ENTRY_ARMED bit also ended it at λ1 with v^r < 0: no other
// end of a ray moves λ to λ1 going in (the escape and polar-rate culls ask v^r > 0; λ1 itself is reached far outside R_cull).
int hhe_render_tiles(const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf, const int64_t* tiles, int64_t n_tiles,
                     int step_cull, int start_cull, double zeta, int entry, double* image, int32_t* status, int32_t* nacc, int32_t* nrej,
                     int32_t* at_start, int32_t* entry_step, double* r_last, double* vr_last, double* r_start)
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
            entry_step[k] = 0;
            if (!decided) {
                bool done = false;
                while (!done) {
                    const bool armed = (ray.flags & RAY_ENTRY_ARMED) != 0;
                    done = ray.step(m, p);
                    if (done && armed && !(ray.flags & RAY_ENTRY_ARMED) && ray.v[1] < 0.0 && ray.t == p.cfg.lambda1)
                        entry_step[k] = ray.nacc + ray.nrej;
                }
            }
            r_last[k] = ray.x[1];
            vr_last[k] = ray.v[1];
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

// The entry cull's quantities for rays `rays` (plane indices) of a scene, at the state in which Ray::step asks: the end of the first
// accepted step with r <= R_cull of a ray that started outside R_cull going in and was not decided at the start (ζ as above),
// every cull of the step loop off.  18 doubles per ray:
//   0 E  1 L  2 Q  3 u0 = 1/r of that state  4 uc  5 μ0  6 dμ/dτ >= 0 (1 / 0)  7 v^r
//   8 u_lo  9 u_hi  10 T_a^lo  11 T_b^hi  12 Ω_lo  13 Ω_hi  14 ψ0  15 the decision of pass_cull_bounds at R_dip (1 / 0)
//   16 asked (1: the ray reached such a state with v^r < 0 and the disc condition > 0; 0: the rest is zero)  17 steps taken by then
// (8-14 hold what the function had formed when it returned; a condition that fails early leaves zeros behind it.)
int hhe_entry_bounds(const gr_config* cfg, const gr_plane* plane, const int64_t* rays, int64_t n_rays, double zeta, double* out)
{
    const double gate = gate_radius(cfg);
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
        Ray<KerrMetric, GR_DISC_THIN> ray;
        if (ray.init(m, p, rays[i]) || !(ray.x[1] > gate) || !(ray.v[1] < 0.0)) continue;
        bool done = false;
        while (!done && ray.x[1] > gate) done = ray.step(m, p);
        if (done || !(ray.v[1] < 0.0) || !(ray.cprev > 0.0)) continue;
        double g[5];
        metric_comps(m, ray.x[1], ray.x[2], ray.sth, ray.cth, g);
        const double E = -(g[0] * ray.v[0] + g[4] * ray.v[3]), L = g[4] * ray.v[0] + g[3] * ray.v[3];
        const double Q = m.carter_constant(g[2] * ray.v[2], ray.sth, ray.cth, E, L);
        KerrMetric::PassBounds b;
        const bool dec = KerrMetric::pass_cull_bounds(m.M, m.a, E, L, Q, 1.0 / ray.x[1], 1.0 / gate, 1.0 / (kEntryCullZeta * gate), ray.cth,
                                                      ray.v[2] <= 0.0, cfg->gtol, b);
        o[0] = E; o[1] = L; o[2] = Q; o[3] = 1.0 / ray.x[1]; o[4] = 1.0 / gate; o[5] = ray.cth; o[6] = ray.v[2] <= 0.0 ? 1.0 : 0.0;
        o[7] = ray.v[1];
        o[8] = b.u_lo; o[9] = b.u_hi; o[10] = b.Ta_lo; o[11] = b.Tb_hi; o[12] = b.Om_lo; o[13] = b.Om_hi; o[14] = b.psi0;
        o[15] = dec ? 1.0 : 0.0; o[16] = 1.0; o[17] = (double)(ray.nacc + ray.nrej);
    }
    return 0;
}
}
