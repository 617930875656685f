// host_harness_f32.cpp -- TEST INFRASTRUCTURE.  Compiles the SINGLE-PRECISION text of the device integrator (gr_device.hpp with
// GR_REAL_IS_FLOAT, as kernels_tu.hip does under -DGR_TU_F32) for the host, so that tests can run what the twelve kernels32_m*.o
// objects compute ray by ray on a CPU, next to the oracle, and log its steps.  Built with clang++ and the library's fp32 flags
// (-Xclang -cl-single-precision-constant -ffp-contract=on): g++ ignores ext_vector_type, which the packed stage sums need.
// Never linked into libgradus_mi355x.so.
//
// What differs from the device build is what GR_HOST_HARNESS replaces everywhere: exact 1/x and 1/sqrt(x) for the hardware's
// reciprocal seeds, libm's log2 / exp2 in the step controller, no inline assembly.  The metric functor per id is the one the
// kernel objects instantiate (MetricOf<ID>::type), not the run-time switch of host_harness.cpp.
#define GR_HOST_HARNESS 1
#define GR_REAL_IS_FLOAT 1
#define GR_NS gr32
#include <cmath>
#include <cstring>

#include "../gradus.jl_amd/csrc/gr_device.hpp"
#include "host_harness_common.hpp"

using namespace GR_NS;

// one row of the step log per attempted step: (λ, r, θ, h used, proposed dt, EEst², flags) after it
enum { HF_LOG_COLS = 7 };

template <class Metric, int DISC>
static void run(const Params& p, int64_t n, double* log, int64_t cap, int64_t* nlog)
{
    Metric m;
    m.load(p.cfg);
    for (int64_t j = 0; j < n; ++j) {
        Ray<Metric, DISC> ray;
        ray.init(m, p, j);
        int64_t k = 0;
#define HF_LOG(e2)                                                                                                \
        if (log && k < cap) {                                                                                      \
            double* row = log + HF_LOG_COLS * k++;                                                                 \
            row[0] = ray.t; row[1] = ray.x[1]; row[2] = ray.x[2]; row[3] = ray.h; row[4] = ray.dt; row[5] = (e2);  \
            row[6] = (double)(ray.flags & GR_FLAG_MASK);                                                           \
        }
        ray.h = 0.0;
        HF_LOG(0.0)
        for (;;) {
            const bool fin = ray.step(m, p);
            HF_LOG(ray.dbg_e2)
            if (fin) break;
        }
#undef HF_LOG
        ray.finalize(m, p, hh::no_lds());
        if (nlog) *nlog = k;
    }
}

template <int ID>
static void run_metric(const Params& p, double* log, int64_t cap, int64_t* nlog)
{
    typedef typename MetricOf<ID>::type M;
    if (p.cfg.disc_id == GR_DISC_THIN) run<M, GR_DISC_THIN>(p, p.n, log, cap, nlog);
    else run<M, GR_DISC_NONE>(p, p.n, log, cap, nlog);
}

// `p` as hh::fill leaves it (the derived fields included) with the rays' source and output set
static int dispatch(Params& p, double* log, int64_t cap, int64_t* nlog)
{
    if (p.cfg.disc_id != GR_DISC_THIN && p.cfg.disc_id != GR_DISC_NONE) return -1;
    p.cfg.upper_hemisphere = (p.cfg.upper_hemisphere ? 1 : 0) | (p.cfg.count_windings ? 4 : 0);   // as stage_disc_table does
    switch (p.cfg.metric_id) {
    case 0: run_metric<0>(p, log, cap, nlog); break;
    case 1: run_metric<1>(p, log, cap, nlog); break;
    case 2: run_metric<2>(p, log, cap, nlog); break;
    case 3: run_metric<3>(p, log, cap, nlog); break;
    case 4: run_metric<4>(p, log, cap, nlog); break;
    case 5: run_metric<5>(p, log, cap, nlog); break;
    case 6: run_metric<6>(p, log, cap, nlog); break;
    case 7: run_metric<7>(p, log, cap, nlog); break;
    case 8: run_metric<8>(p, log, cap, nlog); break;
    case 9: run_metric<9>(p, log, cap, nlog); break;
    case 10: run_metric<10>(p, log, cap, nlog); break;
    default: return -1;
    }
    return 0;
}

extern "C" {

int hf_render_endpoints(const gr_config* cfg, const gr_plane* plane, const gr_range* rg, gr_point* out)
{
    Params p; Cold c;
    hh::fill_plane(p, c, cfg, plane, *rg, 1, nullptr);
    c.points = out;
    return dispatch(p, nullptr, 0, nullptr);
}

int hf_render(const gr_config* cfg, const gr_plane* plane, const gr_range* rg, const gr_pointfunction* pf, double* image)
{
    Params p; Cold c;
    hh::fill_plane(p, c, cfg, plane, *rg, 0, pf);
    c.image = image;
    return dispatch(p, nullptr, 0, nullptr);
}

// one ray of a plane with a log of HF_LOG_COLS doubles per attempted step (row 0: the state after init); returns the rows written
int64_t hf_step_log(const gr_config* cfg, const gr_plane* plane, int64_t i, gr_point* out, double* log, int64_t cap)
{
    Params p; Cold c;
    hh::fill_plane(p, c, cfg, plane, gr_range{ i, 1, 1, 1 }, 1, nullptr);
    c.points = out;
    int64_t n = 0;
    if (dispatch(p, log, cap, &n) != 0) return -1;
    return n;
}
}
