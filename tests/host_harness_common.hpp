// host_harness_common.hpp -- TEST INFRASTRUCTURE.  What every host harness of the device integrator does around Ray::init / step /
// finalize: the parameter block a launch gets, the status a ray is reported with, the lanes of a pixel tile, and no LDS.  Include
// after gr_device.hpp (it reads that header's namespace, GR_NS).  Never included by the library.
#pragma once
#include <cstring>

namespace hh {
using namespace GR_NS;

// Params and Cold zeroed, then what every launch has: the configuration, `n` rays, the point function (null: none) and the derived
// fields.  The rays' source, the output and its buffers are the caller's.
inline void fill(Params& p, Cold& c, const gr_config* cfg, int64_t n, const gr_pointfunction* pf)
{
    std::memset(&p, 0, sizeof p); std::memset(&c, 0, sizeof c);
    p.cfg = *cfg; p.n = n; p.cold = &c; c.winding_plane = cfg->winding_plane;
    if (pf) {
        c.pf.pf_id = pf->pf_id; c.pf.filter_id = pf->filter_id; c.pf.fill = pf->fill; c.pf.r_isco = pf->r_isco;
        c.pf.n_plunge = pf->n_plunge; c.pf.plunge_r = pf->plunge_r; c.pf.plunge_vt = pf->plunge_vt;
        c.pf.plunge_vr = pf->plunge_vr; c.pf.plunge_vphi = pf->plunge_vphi;
    }
    derive_params(p);
}

// ... for the rays `rg` of an image plane
inline void fill_plane(Params& p, Cold& c, const gr_config* cfg, const gr_plane* plane, const gr_range& rg, int out_mode,
                       const gr_pointfunction* pf)
{
    fill(p, c, cfg, rg.count, pf);
    c.src_mode = 0; c.out_mode = out_mode; c.plane = *plane; c.range = rg;
}

// a finished ray's status, or -1 - its flags where the integrator flagged it
template <class R>
inline int32_t status_code(const R& ray) { return (ray.flags & GR_FLAG_MASK) ? -1 - (ray.flags & GR_FLAG_MASK) : ray.status; }

// The plane index of lane l of the 8 x 8 tile `tile` (tile column * (H / 8) + tile row) of a plane H pixels high: column l / 8,
// row l % 8 of the tile, as the one-ray-per-lane kernel lays a wave out.
inline int64_t tile_lane_ray(int64_t tile, int l, int64_t H)
{
    const int64_t tiles_per_col = H >> 3;
    const int64_t tx = tile / tiles_per_col, ty = tile - tx * tiles_per_col;
    return ((tx << 3) + (l >> 3)) * H + (ty << 3) + (l & 7);
}

// no table staged in LDS, no record leaving through it: every pointer null
inline LdsView no_lds() { return LdsView{}; }

}      // namespace hh
