// gr_tftd.hpp -- the arithmetic of integrate_lagtransfer for the time-dependent emissivity of an extended corona
// (RingCoronaProfile / DiscCoronaProfile: src/corona/radial.jl:164-324, src/corona/models/ring.jl:857-950) as
// transfer_functions._integrate_lagtransfer_td evaluates it on the host.  A profile is rings of two arms, an arm a run of
// curves (ρ, t, ε) on the disc, one per β slice of the source's sky.  At an annulus every curve that covers ρ gives a knot
// (t, ε); an arm's ε(t) is the NaNLinearInterpolator over its knots sorted by t, and it counts only between its first and
// last knot, so one slice that misses ρ (a NaN knot, sorted last) switches the arm off.  The annulus then smears the two
// branches' flux of every (g bin, fine bin) over n_time arrival times between the profile's limits.
// Plain functions for the host and the device: k_tftd_em / k_tftd (gradus_mi355x.hip) call them, and
// tests/host_harness_tftd.cpp compiles the same text with g++.  Nothing here may be contracted into an fma (gr_tfint.hpp).
#pragma once
#include "gr_tfint.hpp"

namespace gr_tftd {

constexpr int64_t kMaxRings = 1024, kMaxCurves = 1024, kMaxTime = 1024, kMaxUpscale = 64;

// gr_tfprofile with its arrays where the caller of these functions can read them
struct Profile {
    int64_t n_rings;
    const double *w, *dt;                   // per ring: weight and propagation delay
    const int64_t *arm_off, *curve_off;     // arm (i, left) = curves [arm_off[2i], arm_off[2i+1]), (i, right) the next run
    const double *kr, *kt, *ke;             // knots of the curves: ρ ascending within a curve, t and ε on them
};

GR_LAG_DEV double nan_value() { return __builtin_nan(""); }

// one slice at ρ: (t, ε) of curve c where it covers ρ, NaN where it does not
GR_LAG_DEV void slice_at(const Profile& p, int64_t c, double rho, double& t, double& e)
{
    const int64_t o = p.curve_off[c], n = p.curve_off[c + 1] - o;
    const double* r = p.kr + o;
    if (rho >= r[0] && rho <= r[n - 1]) {
        t = gr_tf::knots_at(r, p.kt + o, n, rho);
        e = gr_tf::knots_at(r, p.ke + o, n, rho);
    } else {
        t = e = nan_value();
    }
}

// sortperm as numpy's argsort(kind = "stable") has it: ascending, NaN last, equal keys in the order of their slices.
// The rank of slice i among the n keys t.
GR_LAG_DEV bool sorts_before(double a, int ia, double b, int ib)
{
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? ia < ib : bn;
    return a < b || (a == b && ia < ib);
}
GR_LAG_DEV int rank_of(const double* t, int n, int i)
{
    const double ti = t[i];
    int r = 0;
    for (int m = 0; m < n; ++m) r += sorts_before(t[m], m, ti, i) ? 1 : 0;
    return r;
}

// an arm at time x on its sorted knots: the interpolator between the first and the last knot, 0 outside -- and 0 everywhere
// if the last knot is NaN
GR_LAG_DEV double arm_at(const double* ts, const double* es, int n, double x)
{
    if (x >= ts[0] && x <= ts[n - 1]) return gr_tf::knots_at(ts, es, n, x);
    return 0.0;
}

// the limits of an arm from the extrema (lo, hi) of its `count` knots that are not NaN -- (0, 0) without any -- shifted by its
// ring's delay, folded into the profile's (t_lo, t_hi).  min / max and the monotone x + dt commute, so the arms fold in any order.
GR_LAG_DEV void fold_limits(double lo, double hi, int64_t count, double dt, bool first, double& t_lo, double& t_hi)
{
    GR_LAG_NO_CONTRACT
    if (count == 0) lo = hi = 0.0;
    const double a = lo + dt, b = hi + dt;
    t_lo = first ? a : fmin(t_lo, a);
    t_hi = first ? b : fmax(t_hi, b);
}

// time sample k of n as numpy.linspace(a, b, n) forms it
GR_LAG_DEV double time_sample(double a, double b, int n, int k)
{
    GR_LAG_NO_CONTRACT
    if (k == n - 1) return b;
    const double div = (double)(n - 1), delta = b - a, step = delta / div;
    if (step == 0.0) {
        const double f = (double)k / div, g = f * delta;
        return g + a;
    }
    const double ks = (double)k * step;
    return ks + a;
}

// fine bin i of `upscale` in the clamped g bin [glo, ghi]
GR_LAG_DEV void fine_bin(double glo, double ghi, int upscale, int i, double& lo, double& hi)
{
    GR_LAG_NO_CONTRACT
    const double dg = (ghi - glo) / (double)upscale;
    const double s = (double)i * dg;
    lo = glo + s;
    hi = lo + dg;
}

// what a fine bin of annulus `a` needs before its time loop: integrate_bin of the two branches times the annulus weight (formed
// with ε = 1) and the branches' times (_time_bins, integration.jl:95-102)
struct FineBin { double k[2], tb[2]; };
GR_LAG_DEV FineBin fine_bin_of(const gr_tf::Set& s, const gr_tf::Annulus& a, const gr_tf::Quad& q, double lo, double hi)
{
    GR_LAG_NO_CONTRACT
    FineBin f;
    const gr_tf::Integrand S1{s, a, 1}, S2{s, a, 2};
    f.k[0] = gr_tf::integrate_bin(S1, q, lo, hi) * a.theta;
    f.k[1] = gr_tf::integrate_bin(S2, q, lo, hi) * a.theta;
    const double s1 = gr_tf::clampd((lo - a.gmin) / a.span, 0.0, 1.0), s2 = gr_tf::clampd((hi - a.gmin) / a.span, 0.0, 1.0);
    double tl1, tu1, tl2, tu2;
    gr_tf::time_gs(s, a, q.h, s1, tl1, tu1);
    gr_tf::time_gs(s, a, q.h, s2, tl2, tu2);
    f.tb[0] = (tl1 + tl2) / 2.0;
    f.tb[1] = (tu1 + tu2) / 2.0;
    return f;
}

// one deposit: branch weight k θ at branch time tb, time sample `time` with emissivity em, step δt.  The t cell is the first
// edge >= the arrival time; false if the deposit is dropped (past the last edge) or adds nothing (0, or not finite).
GR_LAG_DEV bool deposit(double ktheta, double tb, double time, double em, double dt_step, double t0, const double* t_edges, int n_t,
                        double& v, int& cell)
{
    GR_LAG_NO_CONTRACT
    const double ke = ktheta * em;
    v = ke * dt_step;
    if (v == 0.0 || !(fabs(v) < INFINITY)) return false;
    const double sum = tb + time, arrival = sum - t0;
    cell = gr_tf::first_edge_not_below(t_edges, n_t, arrival);
    return cell < n_t;
}

}  // namespace gr_tftd
