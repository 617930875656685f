// host_harness_tfint.cpp -- TEST INFRASTRUCTURE.  The arithmetic that integrates transfer functions on the device (gr_tfint.hpp)
// compiled for the host with g++: the two passes of gr_tf_lineprofile / gr_tf_lagtransfer over (set, annulus, g bin) with the
// header's functions and the integer accumulators of k_tf, one deposit after the other.  Never linked into libgradus_mi355x.so.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_tfint.hpp"
#include "../include/gradus_mi355x.h"

namespace {

gr_tf::Set set_of(const gr_tfset& p)
{
    gr_tf::Set s;
    s.radii = p.radii; s.gmin = p.gmin; s.gmax = p.gmax; s.off = p.off;
    s.kg = p.knot_g; s.kf = p.knot_f; s.kt = p.knot_t;
    s.r_int = p.r_int; s.eps = p.eps_int; s.tsd = p.tsd_int ? p.tsd_int : p.eps_int;
    s.n_r = p.n_r; s.n_int = p.n_int; s.r_min = p.r_min; s.g_scale = p.g_scale;
    return s;
}

gr_tf::Quad quad_of(const gr_tfquad* p)
{
    gr_tf::Quad q{};
    q.h = p->h; q.n = (int)p->n_q;
    for (int i = 0; i < q.n; ++i) { q.x[i] = p->x[i]; q.w[i] = p->w[i]; }
    return q;
}

// every deposit of one set: f(cell, value)
template <class F>
void deposits(const gr_tf::Set& s, const gr_tf::Quad& q, const double* g_edges, int n_g, const double* t_edges, int n_t, bool lag, F&& f)
{
    for (int64_t ia = 0; ia < s.n_int; ++ia) {
        const gr_tf::Annulus an = gr_tf::annulus_of(s, ia);
        for (int j = 0; j < n_g - 1; ++j) {
            if (lag) {
                double v[2];
                int it[2];
                if (!gr_tf::lag_deposits(s, an, q, g_edges, j, t_edges, n_t, v, it)) continue;
                for (int k = 0; k < 2; ++k)
                    if (it[k] < n_t) f((size_t)j * (size_t)n_t + (size_t)it[k], v[k]);
            } else {
                double v;
                if (gr_tf::line_deposit(s, an, q, g_edges, j, v)) f((size_t)j, v);
            }
        }
    }
}

int64_t integrate(const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges, int64_t n_g, const double* t_edges,
                  int64_t n_t, bool lag, double* out)
{
    const gr_tf::Quad q = quad_of(quad);
    const size_t cells = (size_t)n_g * (size_t)(lag ? n_t : 1);
    int64_t count = 0;
    for (int64_t k = 0; k < n_sets; ++k) {
        const gr_tf::Set s = set_of(sets[k]);
        double vmax = 0.0;
        deposits(s, q, g_edges, (int)n_g, t_edges, (int)n_t, lag, [&](size_t, double v) { if (std::fabs(v) > vmax) vmax = std::fabs(v); });
        const gr_lag::CoronaGrid g = gr_lag::corona_grid(vmax, 2 * s.n_int);
        std::vector<unsigned long long> acc(2 * cells, 0ull);
        deposits(s, q, g_edges, (int)n_g, t_edges, (int)n_t, lag, [&](size_t cell, double v) {
            long long fh, fl;
            gr_lag::corona_split(v, g.sc, fh, fl);
            acc[cell] += (unsigned long long)fh;
            acc[cells + cell] += (unsigned long long)fl;
            ++count;
        });
        for (size_t c = 0; c < cells; ++c) out[(size_t)k * cells + c] = gr_lag::corona_sum((long long)acc[c], (long long)acc[cells + c], g);
    }
    return count;
}

}      // namespace

extern "C" {

// the argument lists of gr_tf_lineprofile / gr_tf_lagtransfer without the context; return the number of deposits
int64_t htf_lineprofile(const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges, int64_t n_g, double* out)
{
    return integrate(sets, n_sets, quad, g_edges, n_g, nullptr, 1, false, out);
}
int64_t htf_lagtransfer(const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges, int64_t n_g, const double* t_edges,
                        int64_t n_t, double* out)
{
    return integrate(sets, n_sets, quad, g_edges, n_g, t_edges, n_t, true, out);
}

// integrate_bin of annulus ia over [lo, hi] (mode 0: both branches, 1: lower, 2: upper); ann receives (gmin, gmax, weight)
double htf_bin(const gr_tfset* set, const gr_tfquad* quad, int64_t ia, int mode, double lo, double hi, double* ann)
{
    const gr_tf::Set s = set_of(*set);
    const gr_tf::Quad q = quad_of(quad);
    const gr_tf::Annulus an = gr_tf::annulus_of(s, ia);
    ann[0] = an.gmin; ann[1] = an.gmax; ann[2] = an.theta;
    const gr_tf::Integrand S{s, an, mode};
    return gr_tf::integrate_bin(S, q, lo, hi);
}

}      // extern "C"
