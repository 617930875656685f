// host_harness_transfer.cpp -- TEST INFRASTRUCTURE.  The TraceRadiativeTransfer flavour of the device integrator (gr_device.hpp
// with GR_RADTRANS, what kernels_tu.hip -DGR_TU_RT compiles for the GPU) compiled for the host with g++, so that the ray that goes
// THROUGH the disc -- the ninth state component, the surface crossings, the termination argument of Ray::rt_cross -- is proven ray
// by ray on a CPU before anything is launched.  Never linked into libgradus_mi355x.so.
// With -DHHR_MAIN the file is a stand-alone program (own main) for the sanitizer run: it traces a fan of rays through the torus of
// scene A (tests/transfer_scene.py) under each kind of medium and prints what it found.
#define GR_HOST_HARNESS 1
#define GR_RADTRANS 1
#define GR_NS grrt
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_device.hpp"
#include "host_harness_common.hpp"

using namespace GR_NS;

// one ray after the other, as k_trace_lane's lanes do: init, step until it says so, finalize.  iters[j]: passes through the step
// loop; crossings[j]: surface crossings; returns the largest pass count
template <class Metric, int DISC>
static int64_t run(const Params& p, int64_t* iters, int32_t* crossings)
{
    Metric m;
    m.load(p.cfg);
    int64_t worst = 0;
    for (int64_t j = 0; j < p.n; ++j) {
        Ray<Metric, DISC> ray;
        int64_t k = 0;
        if (!ray.init(m, p, j)) {
            for (;;) {
                ++k;
                if (ray.step(m, p)) break;
            }
        }
        ray.finalize(m, p, hh::no_lds());
        if (iters) iters[j] = k;
        if (crossings) crossings[j] = ray.ncross;
        worst = std::max(worst, k);
    }
    return worst;
}

template <class Metric>
static int64_t run_disc(const Params& p, int64_t* iters, int32_t* crossings)
{
    if (p.cfg.disc_id == GR_DISC_SHAKURA_SUNYAEV) return run<Metric, GR_DISC_SHAKURA_SUNYAEV>(p, iters, crossings);
    if (p.cfg.disc_id == GR_DISC_TABULATED) return run<Metric, GR_DISC_TABULATED>(p, iters, crossings);
    return -1;
}

// the seven catalogue metrics that have an ISCO (what kernelsrt_m<id>.o exists for)
static int64_t dispatch(Params& p, int64_t* iters, int32_t* crossings)
{
    p.disc_table = p.cfg.disc_table;      // host pointer is directly usable here
    p.cfg.upper_hemisphere = p.cfg.upper_hemisphere ? 1 : 0;
    switch (p.cfg.metric_id) {
    case GR_METRIC_KERR: return run_disc<KerrMetric>(p, iters, crossings);
    case GR_METRIC_JOHANNSEN: return run_disc<JohannsenMetric>(p, iters, crossings);
    case GR_METRIC_KERR_NEWMAN: return run_disc<KerrNewmanMetric>(p, iters, crossings);
    case GR_METRIC_BUMBLEBEE: return run_disc<GenericMetricT<GR_METRIC_BUMBLEBEE>>(p, iters, crossings);
    case GR_METRIC_JOHANNSEN_PSALTIS: return run_disc<GenericMetricT<GR_METRIC_JOHANNSEN_PSALTIS>>(p, iters, crossings);
    case GR_METRIC_DILATON_AXION: return run_disc<GenericMetricT<GR_METRIC_DILATON_AXION>>(p, iters, crossings);
    case GR_METRIC_KERR_REFRACTIVE: return run_disc<GenericMetricT<GR_METRIC_KERR_REFRACTIVE>>(p, iters, crossings);
    default: return -1;
    }
}

extern "C" {

// rays given by (x, v): the end-point records, the intensities beside them, passes through the step loop and crossings per ray
// (either may be null).  Returns the largest pass count, -1 for a metric or disc the flavour is not built for.
int64_t hhr_transfer_endpoints(const gr_config* cfg, const gr_transfer* transfer, const double* x, int64_t x_stride, const double* v,
                               int64_t n, gr_point* out, double* intensity, int64_t* iters, int32_t* crossings)
{
    Params p; Cold c;
    hh::fill(p, c, cfg, n, nullptr);
    c.src_mode = 1; c.out_mode = 1; c.x = x; c.x_stride = x_stride; c.v = v; c.points = out;
    c.range = gr_range{ 0, n, n > 0 ? n : 1, 1 };
    c.transfer = transfer; c.intensity = intensity;
    return dispatch(p, iters, crossings);
}

// the image of I over a plane (pf->pf_id = GR_PF_INTENSITY)
int64_t hhr_transfer_render(const gr_config* cfg, const gr_transfer* transfer, const gr_plane* plane, const gr_range* rg,
                            const gr_pointfunction* pf, double* image)
{
    Params p; Cold c;
    hh::fill_plane(p, c, cfg, plane, *rg, 0, pf);
    c.image = image;
    c.transfer = transfer; c.intensity = nullptr;
    return dispatch(p, nullptr, nullptr);
}

// the fluid's four-velocity as the kernel forms it (Kerr): (v^t, v^r, v^ϕ) at ρ
void hhr_fluid_velocity(const gr_config* cfg, double rho, double r_isco, double* out3)
{
    KerrMetric m;
    m.load(*cfg);
    real vt, vr, vp;
    Ray<KerrMetric, GR_DISC_TABULATED>::rt_fluid_velocity(m, rho, r_isco, vt, vr, vp);
    out3[0] = vt; out3[1] = vr; out3[2] = vp;
}

}      // extern "C"

#ifdef HHR_MAIN
// Scene A by hand (tests/transfer_scene.py holds the same numbers): Schwarzschild, observer at r = 100, θ = 85°, the torus
// sqrt(1 - (ρ - 10)²) on [9, 11] as a table, a fan of 24 x 9 rays over it from an image plane, every medium kind.
int main()
{
    const int64_t n_tab = 4097;
    std::vector<double> table((size_t)n_tab);
    for (int64_t k = 0; k < n_tab; ++k) {
        const double x = -1.0 + 2.0 * (double)k / (double)(n_tab - 1);
        table[(size_t)k] = std::sqrt(std::max(1.0 - x * x, 0.0));
    }
    gr_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.metric_id = GR_METRIC_KERR;
    cfg.params[0] = 1.0; cfg.params[1] = 0.0;
    cfg.disc_id = GR_DISC_TABULATED;
    cfg.r_inner = 2.02; cfg.r_outer = 12000.0;
    cfg.disc_r_in = 0.0; cfg.disc_r_out = HUGE_VAL;
    cfg.disc_params[0] = 9.0; cfg.disc_params[1] = 11.0; cfg.disc_params[2] = 1.0;
    cfg.disc_table = table.data(); cfg.disc_table_n = n_tab;
    cfg.gtol = 1e-2;
    cfg.lambda0 = 0.0; cfg.lambda1 = 200.0;
    cfg.abstol = cfg.reltol = 1e-9;
    cfg.maxiters = 100000;
    gr_plane pl;
    std::memset(&pl, 0, sizeof pl);
    const double r = 100.0, th = 85.0 * 3.14159265358979323846 / 180.0, f = 1.0 - 2.0 / r;
    pl.x_obs[0] = 0.0; pl.x_obs[1] = r; pl.x_obs[2] = th; pl.x_obs[3] = 0.0;
    // the static observer's tetrad of Schwarzschild: v = Mx p̄ with p̄ = (1, p_r, β p_r / r, α p_r / r)
    pl.Mx[0] = -1.0 / std::sqrt(f); pl.Mx[5] = std::sqrt(f); pl.Mx[10] = 1.0 / r; pl.Mx[15] = 1.0 / (r * std::sin(th));
    pl.alpha0 = -14.0; pl.alpha1 = 14.0; pl.beta0 = -5.0; pl.beta1 = 5.0;
    pl.width = 24; pl.height = 9;
    const int64_t n = pl.width * pl.height;
    const gr_range rg{ 0, n, n, 1 };
    gr_pointfunction pf;
    std::memset(&pf, 0, sizeof pf);
    pf.pf_id = GR_PF_INTENSITY; pf.filter_id = GR_FILTER_NONE; pf.fill = std::nan("");
    const gr_transfer media[4] = { { 1.0, 0.0, 0.0, 0.1, 0.0, 0.0, 0.0, 0.0, 6.0, 0.0 },      // emission only
                                   { 1.0, 1.0, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 6.0, 0.0 },      // absorption only
                                   { 1.0, 0.5, 0.3, 0.1, 1.0, 1.0, 0.0, 0.0, 6.0, 0.0 },      // both
                                   { 1.0, 1.0, 0.3, 0.1, 1.0, 1.0, 2.0, -1.0, 6.0, 0.0 } };   // equilibrium
    std::vector<double> img((size_t)n);
    int bad = 0;
    for (int k = 0; k < 4; ++k) {
        if (hhr_transfer_render(&cfg, &media[k], &pl, &rg, &pf, img.data()) < 0) return 2;
        int changed = 0;
        double lo = HUGE_VAL, hi = -HUGE_VAL;
        for (int64_t j = 0; j < n; ++j) {
            if (!(img[(size_t)j] == img[(size_t)j])) { ++bad; continue; }
            changed += img[(size_t)j] != media[k].I0;
            lo = std::min(lo, img[(size_t)j]); hi = std::max(hi, img[(size_t)j]);
        }
        std::printf("medium %d: %d of %lld rays changed I, range [%.6g, %.6g]\n", k, changed, (long long)n, lo, hi);
        if (changed == 0) ++bad;
    }
    return bad ? 1 : 0;
}
#endif
