// host_harness_offsetsolve.cpp -- TEST INFRASTRUCTURE.  gr_offsetsolve.hpp (the offset solve and the extremum search as state
// machines) driven by the host build of the tangent integrator: what k_offset_solve / k_offset_search do with a lane pair, a plain
// loop does here, one problem after the other.  hht_ray_tangent of host_harness_tangent.cpp is part of this library too (the same
// ray code, the same flags): the lock-step route of transfer_functions.py runs on it as the yardstick.
#include "host_harness_tangent.cpp"

#include <vector>

#include "../gradus.jl_amd/csrc/gr_offsetsolve.hpp"

static int64_t g_rays_traced = 0;      // every ray any hho_* call has traced

namespace {
struct Work {
    Params p;
    Cold c;
    std::vector<double> alpha, beta, rows;
};

void prepare(Work& w, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, int64_t n, const double* height)
{
    hh::fill(w.p, w.c, cfg, n, pf);
    w.alpha.assign((size_t)n, 0.0); w.beta.assign((size_t)n, 0.0); w.rows.assign((size_t)n * 8, 0.0);
    Cold& c = w.c;
    c.src_mode = 2; c.out_mode = 5;
    std::memcpy(c.plane.x_obs, rays->x_obs, sizeof c.plane.x_obs);
    std::memcpy(c.plane.Mx, rays->Mx, sizeof c.plane.Mx);
    c.plane.width = n; c.plane.height = 1;
    c.range = gr_range{ 0, n, n > 0 ? n : 1, 1 };
    c.alpha = w.alpha.data(); c.beta = w.beta.data(); c.area = nullptr;
    c.height = cfg->disc_id == GR_DISC_DATUM ? height : nullptr;
    c.lp_rmin = 0.0; c.lp_rmax = INFINITY; c.lp_pairs = w.rows.data();
    w.p.tangent_norm = g_tangent_norm;
    w.p.disc_table = w.p.cfg.disc_table;
    w.p.cfg.upper_hemisphere = (w.p.cfg.upper_hemisphere ? 1 : 0);
}

// problem j's ray at the offset r -> its row
template <class Metric, int DISC>
const double* trace(const Metric& m, Work& w, const gr_os::Solve& q, const gr_os::Setup& st, int64_t j, double r)
{
    gr_os::aim(q, st, r, w.alpha[(size_t)j], w.beta[(size_t)j]);
    const LdsView no_lds = hh::no_lds();
    Ray<Metric, DISC> ray;
    ray.init(m, w.p, j);
    while (!ray.step(m, w.p)) {}
    ray.finalize(m, w.p, no_lds);
    ++g_rays_traced;
    return w.rows.data() + 8 * j;
}

template <class Metric, int DISC>
void solve_all(Work& w, const gr_os::Setup& st, const double* r_target, const double* cos_t, const double* sin_t, double* out)
{
    Metric m;
    m.load(w.p.cfg);
    for (int64_t j = 0; j < w.p.n; ++j) {
        gr_os::Solve q;
        double r = gr_os::solve_start(q, r_target[j], cos_t[j], sin_t[j]);
        while (!gr_os::solve_feed(q, st, trace<Metric, DISC>(m, w, q, st, j, r))) r = q.cur;
        gr_os::solve_store(q, out + gr_os::kSolveOut * j);
    }
}

template <class Metric, int DISC>
void search_all(Work& w, const gr_os::Setup& st, const double* r_target, const double* lower, const double* upper, const double* sign,
                double* out)
{
    Metric m;
    m.load(w.p.cfg);
    const int64_t stride = gr_os::search_stride(st.iterations);
    for (int64_t j = 0; j < w.p.n; ++j) {
        gr_os::Solve q;
        gr_os::Search s;
        double* o = out + stride * j;
        double r = gr_os::search_start(s, q, r_target[j], lower[j], upper[j], sign[j]);
        for (;;) {
            if (!gr_os::solve_feed(q, st, trace<Metric, DISC>(m, w, q, st, j, r))) { r = q.cur; continue; }
            const int k = s.k;
            if (gr_os::search_feed(s, q, st, o + gr_os::kRecord * k, o + stride - 1)) break;
            r = q.cur;
        }
    }
}
}  // namespace

#define HHO_DISPATCH(CALL)                                                                        \
    do {                                                                                          \
        const int disc = w.p.cfg.disc_id, mid = w.p.cfg.metric_id;                                \
        if (disc != GR_DISC_THIN && disc != GR_DISC_DATUM) return -1;                             \
        if (disc == GR_DISC_THIN) {                                                               \
            if (mid == GR_METRIC_KERR) CALL(KerrMetric, GR_DISC_THIN);                            \
            else if (mid == GR_METRIC_KERR_NEWMAN) CALL(KerrNewmanMetric, GR_DISC_THIN);          \
            else if (mid == GR_METRIC_JOHANNSEN) CALL(JohannsenMetric, GR_DISC_THIN);             \
            else CALL(GenericMetric, GR_DISC_THIN);                                               \
        } else {                                                                                  \
            if (mid == GR_METRIC_KERR) CALL(KerrMetric, GR_DISC_DATUM);                           \
            else if (mid == GR_METRIC_KERR_NEWMAN) CALL(KerrNewmanMetric, GR_DISC_DATUM);         \
            else if (mid == GR_METRIC_JOHANNSEN) CALL(JohannsenMetric, GR_DISC_DATUM);            \
            else CALL(GenericMetric, GR_DISC_DATUM);                                              \
        }                                                                                         \
    } while (0)

extern "C" {

int64_t hho_rays_traced() { return g_rays_traced; }

// setup[5] = (alpha0, beta0, zero_atol, r_min, contrapoint_bias); out: n x 10 = (r, row[8], rays traced)
int hho_solve(const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, int64_t n, const double* r_target,
              const double* cos_t, const double* sin_t, const double* height, const double* setup, int32_t max_iter, double* out)
{
    Work w;
    prepare(w, cfg, rays, pf, n, height);
    const gr_os::Setup st{ setup[0], setup[1], setup[2], setup[3], setup[4], max_iter, 0 };
#define HHO_SOLVE(M, D) solve_all<M, D>(w, st, r_target, cos_t, sin_t, out)
    HHO_DISPATCH(HHO_SOLVE);
#undef HHO_SOLVE
    return 0;
}

// out: n x (12 (iterations + 1) + 1) = records (θ after the nudge, r, row[8], rays traced, failure flag), then the minimum found
int hho_search(const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf, int64_t n, const double* r_target,
               const double* lower, const double* upper, const double* sign, const double* height, const double* setup, int32_t max_iter,
               int32_t iterations, double* out)
{
    Work w;
    prepare(w, cfg, rays, pf, n, height);
    const gr_os::Setup st{ setup[0], setup[1], setup[2], setup[3], setup[4], max_iter, iterations };
#define HHO_SEARCH(M, D) search_all<M, D>(w, st, r_target, lower, upper, sign, out)
    HHO_DISPATCH(HHO_SEARCH);
#undef HHO_SEARCH
    return 0;
}
}
