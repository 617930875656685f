// host_harness_pass_cull.cpp -- TEST INFRASTRUCTURE.  The device integrator (gr_device.hpp) compiled for the host with g++, for the
// pass cull (Ray::start_decided, KerrFamily::pass_cull_bounds): whole 8 x 8 tiles traced with the step loop's
// culls, the start cull and the pass cull switched one by one (the pass cull at any ζ, for the census that chose the library's),
// and, ray by ray, the bounds the pass cull decides by.  Never linked into libgradus_mi355x.so.
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

double hhp_gate_radius(const gr_config* c) { return gate_radius(c); }
double hhp_zeta(void) { return kPassCullZeta; }

// As hhc_render_tiles (host_harness_cull.cpp), with the pass cull's ζ as a third switch.  at_start: 0 = traced, 1 = decided by
// the start cull's own test, 2 = decided by the pass cull (decided at ζ, not decided with the pass cull off).
int hhp_render_tiles(const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf, const int64_t* tiles, int64_t n_tiles,
                     int step_cull, int start_cull, double zeta, double* image, int32_t* status, int32_t* nacc, int32_t* nrej,
                     int32_t* at_start)
{
    const double gate = gate_radius(cfg);
    if (!(gate < HUGE_VAL) || pf->filter_id != GR_FILTER_INTERSECTED) return -1;
    Params p; Cold c;
    fill(p, c, cfg, plane, pf);
    const int64_t H = plane->height, n = plane->width * H;
    p.r_cull = step_cull ? gate : HUGE_VAL;
    p.r_cull_start = start_cull ? gate : HUGE_VAL;
    p.r_pass = pass_radius(p.r_cull_start, zeta);
    Params p_nopass = p;
    p_nopass.r_pass = HUGE_VAL;
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
            Ray<KerrMetric, GR_DISC_THIN> ray;
            const bool decided = ray.init(m, p, j);
            if (!decided)
                while (!ray.step(m, p)) {}
            ray.finalize(m, p, no_lds);
            const int64_t k = 64 * t + l;
            image[k] = img[(size_t)j];
            status[k] = (ray.flags & GR_FLAG_MASK) ? -1 - (ray.flags & GR_FLAG_MASK) : ray.status;
            nacc[k] = ray.nacc;
            nrej[k] = ray.nrej;
            at_start[k] = 0;
            if (decided) {
                Ray<KerrMetric, GR_DISC_THIN> probe;
                at_start[k] = probe.init(m, p_nopass, j) ? 1 : 2;
            }
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
int hhp_pass_bounds(const gr_config* cfg, const gr_plane* plane, const int64_t* rays, int64_t n_rays, double zeta, double* out)
{
    const double gate = gate_radius(cfg);
    if (!(gate < HUGE_VAL)) return -1;
    Params p; Cold c;
    fill(p, c, cfg, plane, nullptr);
    const double r_pass = pass_radius(gate, zeta);
    KerrMetric m;
    m.load(p.cfg);
    for (int64_t i = 0; i < n_rays; ++i) {
        double x[4], v[4], s, cth, g[5];
        Ray<KerrMetric, GR_DISC_THIN>::constrained_u0(m, p, rays[i], x, v);
        sincos_fast(x[2], s, cth);
        metric_comps(m, x[1], x[2], s, cth, g);
        const double E = -(g[0] * v[0] + g[4] * v[3]), L = g[4] * v[0] + g[3] * v[3];
        const double Q = m.carter_constant(g[2] * v[2], s, cth, E, L);
        KerrMetric::PassBounds b;
        const bool dec = KerrMetric::pass_cull_bounds(m.M, m.a, E, L, Q, 1.0 / x[1], 1.0 / gate, 1.0 / r_pass, cth, v[2] <= 0.0, cfg->gtol, b);
        double* o = out + 16 * i;
        o[0] = E; o[1] = L; o[2] = Q; o[3] = 1.0 / x[1]; o[4] = 1.0 / gate; o[5] = cth; o[6] = v[2] <= 0.0 ? 1.0 : 0.0; o[7] = v[1];
        o[8] = b.u_lo; o[9] = b.u_hi; o[10] = b.Ta_lo; o[11] = b.Tb_hi; o[12] = b.Om_lo; o[13] = b.Om_hi; o[14] = b.psi0;
        o[15] = dec ? 1.0 : 0.0;
    }
    return 0;
}
}
