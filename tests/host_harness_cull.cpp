// host_harness_cull.cpp -- TEST INFRASTRUCTURE.  The device integrator (gr_device.hpp) compiled for the host with g++, with the
// start cull (Ray::init) and the step loop's culls (Ray::step: escape and polar-rate) switched on or off one by one, as the
// launcher's two environment switches do.  Traces whole 8 x 8 tiles of an image plane, lanes as the
// one-ray-per-lane kernel lays them out, and hands back per ray what the culls must not change (pixel, status) and what they must
// (steps).  Never linked into libgradus_mi355x.so.
#define GR_HOST_HARNESS 1
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_device.hpp"

using namespace GR_NS;

extern "C" {

// The gating radius the launcher passes for a fused-Kerr scene: the library's own function (cull_gate_radius, gr_device.hpp), with
// the winding callback the launcher folds into cfg.upper_hemisphere (stage_disc_table) excluded here.  +inf where gated off.
double hhc_gate_radius(const gr_config* c)
{
    if (c->metric_id != GR_METRIC_KERR || c->count_windings != 0) return HUGE_VAL;
    return cull_gate_radius(*c, KerrMetric::kEscapeRadiusM);
}

// Tiles `tiles` (index = tile column * (H / 8) + tile row) of the plane, 64 rays each: lane l is column l / 8, row l % 8 of its
// tile.  Per ray, in tile-major lane order: the pixel finalize() writes (out_mode 0), the status, accepted and rejected steps and
// whether Ray::init decided it.  step_cull / start_cull: 0 = that mechanism off (radius +inf), else the gating radius.
// Returns -1 for a scene the launcher would gate off, or one that is not a fused Kerr with a thin disc.
int hhc_render_tiles(const gr_config* cfg, const gr_plane* plane, const gr_pointfunction* pf, const int64_t* tiles, int64_t n_tiles,
                     int step_cull, int start_cull, double* image, int32_t* status, int32_t* nacc, int32_t* nrej, int32_t* at_start)
{
    const double gate = hhc_gate_radius(cfg);
    if (!(gate < HUGE_VAL) || pf->filter_id != GR_FILTER_INTERSECTED) return -1;
    Params p; Cold c;
    std::memset(&p, 0, sizeof p); std::memset(&c, 0, sizeof c);
    const int64_t H = plane->height, n = plane->width * H;
    p.cfg = *cfg; p.n = n; p.cold = &c; c.winding_plane = cfg->winding_plane;
    c.src_mode = 0; c.out_mode = 0; c.plane = *plane; c.range = gr_range{ 0, n, n, 1 };
    c.pf.pf_id = pf->pf_id; c.pf.filter_id = pf->filter_id; c.pf.fill = pf->fill; c.pf.r_isco = pf->r_isco;
    c.pf.n_plunge = pf->n_plunge; c.pf.plunge_r = pf->plunge_r; c.pf.plunge_vt = pf->plunge_vt;
    c.pf.plunge_vr = pf->plunge_vr; c.pf.plunge_vphi = pf->plunge_vphi;
    derive_params(p);
    p.r_cull = step_cull ? gate : HUGE_VAL;
    p.r_cull_start = start_cull ? gate : HUGE_VAL;
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
            at_start[k] = decided ? 1 : 0;
        }
    }
    return 0;
}
}
