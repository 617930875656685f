// host_harness_tftd.cpp -- TEST INFRASTRUCTURE.  The arithmetic of gr_tf_lagtransfer_td (gr_tftd.hpp over gr_tfint.hpp) compiled
// for the host with g++: what k_tftd_em does per annulus and k_tftd per (annulus, g bin, fine bin, time sample), one after the
// other, with the header's functions and the integer accumulators of the kernels.  Never linked into libgradus_mi355x.so.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_tftd.hpp"
#include "../include/gradus_mi355x.h"

namespace {

// the table of k_tftd_em: per annulus t_lo, t_hi, em[k]
void em_table(const gr_tf::Set& s, const gr_tftd::Profile& p, int n_time, double* em)
{
    std::vector<double> raw_t(gr_tftd::kMaxCurves), raw_e(gr_tftd::kMaxCurves), knot_t(gr_tftd::kMaxCurves), knot_e(gr_tftd::kMaxCurves);
    std::vector<double> left(n_time);
    const int n_arms = 2 * (int)p.n_rings;
    for (int64_t ia = 0; ia < s.n_int; ++ia) {
        const double rho = s.r_int[ia];
        double* row = em + (size_t)ia * (size_t)(2 + n_time);
        double t_lo = 0.0, t_hi = 0.0;
        for (int arm = 0; arm < n_arms; ++arm) {
            const int64_t c0 = p.arm_off[arm], nc = p.arm_off[arm + 1] - c0;
            double lo = INFINITY, hi = -INFINITY;
            int64_t count = 0;
            for (int64_t j = 0; j < nc; ++j) {
                double t, e;
                gr_tftd::slice_at(p, c0 + j, rho, t, e);
                if (t == t) {
                    lo = std::fmin(lo, t);
                    hi = std::fmax(hi, t);
                    ++count;
                }
            }
            gr_tftd::fold_limits(lo, hi, count, p.dt[arm >> 1], arm == 0, t_lo, t_hi);
        }
        row[0] = t_lo;
        row[1] = t_hi;
        for (int k = 0; k < n_time; ++k) row[2 + k] = 0.0;
        for (int arm = 0; arm < n_arms; ++arm) {
            const int64_t c0 = p.arm_off[arm];
            const int nc = (int)(p.arm_off[arm + 1] - c0);
            for (int j = 0; j < nc; ++j) gr_tftd::slice_at(p, c0 + j, rho, raw_t[j], raw_e[j]);
            for (int j = 0; j < nc; ++j) {
                const int r = gr_tftd::rank_of(raw_t.data(), nc, j);
                knot_t[r] = raw_t[j];
                knot_e[r] = raw_e[j];
            }
            const double dt = p.dt[arm >> 1], w = p.w[arm >> 1];
            for (int k = 0; k < n_time; ++k) {
                const double v = gr_tftd::arm_at(knot_t.data(), knot_e.data(), nc, gr_tftd::time_sample(t_lo, t_hi, n_time, k) - dt);
                if (arm & 1) {
                    const double both = left[k] + v, term = both * w;
                    row[2 + k] += term;
                } else {
                    left[k] = v;
                }
            }
        }
    }
}

// every deposit: f(cell, value)
template <class F>
void deposits(const gr_tf::Set& s, const gr_tf::Quad& q, const double* g_edges, int n_g, const double* t_edges, int n_t, int upscale,
              int n_time, double t0, const double* em, F&& f)
{
    for (int64_t ia = 0; ia < s.n_int; ++ia) {
        const gr_tf::Annulus an = gr_tf::annulus_of(s, ia);
        const double* row = em + (size_t)ia * (size_t)(2 + n_time);
        const double t_lo = row[0], t_hi = row[1];
        const double dt_step = (t_hi - t_lo) / (double)n_time;
        for (int j = 0; j < n_g - 1; ++j) {
            const double glo = gr_tf::clampd(g_edges[j] / s.g_scale, an.gmin, an.gmax), ghi = gr_tf::clampd(g_edges[j + 1] / s.g_scale, an.gmin, an.gmax);
            if (glo == ghi) continue;
            for (int i = 0; i < upscale; ++i) {
                double lo, hi;
                gr_tftd::fine_bin(glo, ghi, upscale, i, lo, hi);
                const gr_tftd::FineBin fb = gr_tftd::fine_bin_of(s, an, q, lo, hi);
                for (int k = 0; k < n_time; ++k) {
                    const double time = gr_tftd::time_sample(t_lo, t_hi, n_time, k);
                    for (int b = 0; b < 2; ++b) {
                        double v;
                        int it;
                        if (gr_tftd::deposit(fb.k[b], fb.tb[b], time, row[2 + k], dt_step, t0, t_edges, n_t, v, it))
                            f((size_t)j * (size_t)n_t + (size_t)it, v);
                    }
                }
            }
        }
    }
}

}      // namespace

extern "C" {

// the argument list of gr_tf_lagtransfer_td without the context; returns the number of deposits
int64_t htftd_lagtransfer(const gr_tfset* set, const gr_tfprofile* prof, const gr_tfquad* quad, const double* g_edges, int64_t n_g,
                          const double* t_edges, int64_t n_t, int64_t g_upscale, int64_t n_time, double t0, double* out, double* em_out)
{
    const std::vector<double> ones((size_t)set->n_int, 1.0);
    gr_tf::Set s;
    s.radii = set->radii; s.gmin = set->gmin; s.gmax = set->gmax; s.off = set->off;
    s.kg = set->knot_g; s.kf = set->knot_f; s.kt = set->knot_t;
    s.r_int = set->r_int; s.eps = s.tsd = ones.data();
    s.n_r = set->n_r; s.n_int = set->n_int; s.r_min = set->r_min; s.g_scale = set->g_scale;
    gr_tftd::Profile p;
    p.n_rings = prof->n_rings; p.w = prof->ring_weight; p.dt = prof->ring_dt;
    p.arm_off = prof->arm_off; p.curve_off = prof->curve_off;
    p.kr = prof->knot_r; p.kt = prof->knot_t; p.ke = prof->knot_e;
    gr_tf::Quad q{};
    q.h = quad->h; q.n = (int)quad->n_q;
    for (int i = 0; i < q.n; ++i) { q.x[i] = quad->x[i]; q.w[i] = quad->w[i]; }
    std::vector<double> em((size_t)s.n_int * (size_t)(2 + n_time));
    em_table(s, p, (int)n_time, em.data());
    if (em_out) std::memcpy(em_out, em.data(), sizeof(double) * em.size());
    const size_t cells = (size_t)n_g * (size_t)n_t;
    double vmax = 0.0;
    deposits(s, q, g_edges, (int)n_g, t_edges, (int)n_t, (int)g_upscale, (int)n_time, t0, em.data(),
             [&](size_t, double v) { if (std::fabs(v) > vmax) vmax = std::fabs(v); });
    const gr_lag::CoronaGrid g = gr_lag::corona_grid(vmax, 2 * s.n_int * g_upscale * n_time);
    std::vector<unsigned long long> acc(2 * cells, 0ull);
    int64_t count = 0;
    deposits(s, q, g_edges, (int)n_g, t_edges, (int)n_t, (int)g_upscale, (int)n_time, t0, em.data(), [&](size_t cell, double v) {
        long long fh, fl;
        gr_lag::corona_split(v, g.sc, fh, fl);
        acc[cell] += (unsigned long long)fh;
        acc[cells + cell] += (unsigned long long)fl;
        ++count;
    });
    for (size_t c = 0; c < cells; ++c) out[c] = gr_lag::corona_sum((long long)acc[c], (long long)acc[cells + c], g);
    return count;
}

// the pieces, one by one: the rank of slice i among n keys, and time sample k
int htftd_rank(const double* t, int n, int i) { return gr_tftd::rank_of(t, n, i); }
double htftd_time_sample(double a, double b, int n, int k) { return gr_tftd::time_sample(a, b, n, k); }

}      // extern "C"
