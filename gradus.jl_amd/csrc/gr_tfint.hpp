// gr_tfint.hpp -- the arithmetic that integrates Cunningham transfer functions into a flux per energy bin (integrate_lineprofile,
// integrate_lagtransfer: src/transfer-functions/integration.jl:74-102,161-200,336-453) as transfer_functions.py evaluates it on the
// host: per annulus the radial blend of two neighbouring radii's branches and the weight of the annulus, per g bin integrate_bin
// with its closed-form edges, per lag deposit the arrival time and its t bin.  Plain functions for the host and the device:
// k_tf (gradus_mi355x.hip) calls them per (annulus, g bin), and tests/host_harness_tfint.cpp compiles the same text with g++.
//
// The host route forms every quantity with one rounding per operation, and a deposit's t cell is decided by comparing a time
// with the caller's edges, so nothing here may be contracted into an fma (GR_LAG_NO_CONTRACT, as in gr_lagbin.hpp).
#pragma once
#include "gr_lagbin.hpp"

namespace gr_tf {

constexpr int kMaxQuad = 32;
constexpr int64_t kMaxKnots = 1024;

// one parameter set (gr_tfset) with its arrays where the caller of these functions can read them
struct Set {
    const double *radii, *gmin, *gmax;      // n_r >= 2 emission radii, ascending
    const int64_t* off;                     // 2 n_r + 1: branch (radius k, lower) = [off[2k], off[2k+1]), (k, upper) = [off[2k+1], off[2k+2])
    const double *kg, *kf, *kt;             // knots g✶ (ascending per branch) and the values f, t on them
    const double *r_int, *eps, *tsd;        // n_int >= 2 integration radii, ε(rₑ) and coordtime(rₑ) - t0 there
    int64_t n_r, n_int;
    double r_min, g_scale;
};

struct Quad { double h; int n; double x[kMaxQuad], w[kMaxQuad]; };

GR_LAG_DEV double zero_if_nan(double v) { return (v != v) ? 0.0 : v; }

// NaNLinearInterpolator (src/interpolations.jl:1-30) on one branch: gr_lag::table_at without the clamp -- outside the knots the
// end intervals extrapolate
GR_LAG_DEV double knots_at(const double* g, const double* v, int64_t n, double x)
{
    GR_LAG_NO_CONTRACT
    int64_t a = 0, b = n;                   // number of knots <= x (a NaN sorts behind every knot, as numpy has it)
    if (x != x) a = n;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (g[mid] <= x) a = mid + 1; else b = mid;
    }
    const int64_t i0 = (a < 1 ? 1 : (a > n - 1 ? n - 1 : a)) - 1;
    const double x1 = g[i0], x2 = g[i0 + 1], y1 = v[i0], y2 = v[i0 + 1];
    const double w = (x - x1) / (x2 - x1);
    const double lo = (1.0 - w) * y1, hi = w * y2;
    double y = lo + hi;
    if (y != y) {
        const double pick = w < 0.5 ? y1 : y2;
        y = (pick != pick) ? 0.0 : pick;
    }
    return y;
}

// what an annulus needs of its set: (grid::InterpolatingTransferBranches)(rₑ) (transfer-functions-2d.jl:45-84) and the weight
// (rₑ - r_prev) rₑ ε π / (gmax - gmin) in the order transfer_functions.integrate_lineprofile multiplies
struct Annulus { int64_t i0; double w, gmin, gmax, span, theta, tsd; };
GR_LAG_DEV Annulus annulus_of(const Set& s, int64_t i)
{
    GR_LAG_NO_CONTRACT
    Annulus a;
    const double re = s.r_int[i];
    const double r_prev = i > 0 ? s.r_int[i - 1] : s.r_min - (s.r_int[1] - s.r_min);
    int64_t lo = 0, hi = s.n_r;
    if (re != re) lo = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (s.radii[mid] <= re) lo = mid + 1; else hi = mid;
    }
    a.i0 = (lo < 1 ? 1 : (lo > s.n_r - 1 ? s.n_r - 1 : lo)) - 1;
    const double r1 = s.radii[a.i0], r2 = s.radii[a.i0 + 1];
    a.w = (re - r1) / (r2 - r1);
    const double u = 1.0 - a.w;
    const double m1 = u * s.gmin[a.i0], m2 = a.w * s.gmin[a.i0 + 1];
    const double x1 = u * s.gmax[a.i0], x2 = a.w * s.gmax[a.i0 + 1];
    a.gmin = m1 + m2;
    a.gmax = x1 + x2;
    a.span = a.gmax - a.gmin;
    const double dr = re - r_prev;
    const double t1 = dr * re, t2 = t1 * s.eps[i], t3 = t2 * 3.141592653589793;
    a.theta = t3 / a.span;
    a.tsd = s.tsd[i];
    return a;
}

// one field (f or t) of one branch (0 lower, 1 upper) at g✶, blended between the two radii around the annulus
GR_LAG_DEV double blend(const Set& s, const Annulus& a, int which, const double* val, double gs)
{
    GR_LAG_NO_CONTRACT
    const int64_t o1 = s.off[2 * a.i0 + which], n1 = s.off[2 * a.i0 + which + 1] - o1;
    const int64_t o2 = s.off[2 * a.i0 + 2 + which], n2 = s.off[2 * a.i0 + 3 + which] - o2;
    const double y1 = knots_at(s.kg + o1, val + o1, n1, gs), y2 = knots_at(s.kg + o2, val + o2, n2, gs);
    const double lo = (1.0 - a.w) * y1, hi = a.w * y2;
    return lo + hi;
}

// the integrand g² f g / √(g✶ (1 - g✶)) with f = _zero_if_nan(lower) + _zero_if_nan(upper) (mode 0), the lower (1) or the
// upper branch alone (2)
struct Integrand {
    const Set& s;
    const Annulus& a;
    int mode;
    GR_LAG_DEV double operator()(double g) const
    {
        GR_LAG_NO_CONTRACT
        const double gs = (g - a.gmin) / a.span;
        double f;
        if (mode == 0) {
            const double fl = zero_if_nan(blend(s, a, 0, s.kf, gs)), fu = zero_if_nan(blend(s, a, 1, s.kf, gs));
            f = fl + fu;
        } else {
            f = zero_if_nan(blend(s, a, mode - 1, s.kf, gs));
        }
        const double g2 = g * g, n1 = g2 * f, n2 = n1 * g;
        const double c = 1.0 - gs, d = gs * c;
        return n2 / sqrt(d);
    }
};

GR_LAG_DEV double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }
GR_LAG_DEV double finite_or_zero(double v) { return fabs(v) < INFINITY ? v : 0.0; }

// integrate_edge (integration.jl:161-164)
GR_LAG_DEV double integrate_edge(const Integrand& S, double lim, double lim_gs, double h)
{
    GR_LAG_NO_CONTRACT
    const double p = S.a.span * lim_gs;
    const double gh = p + S.a.gmin;
    const double d = fabs(sqrt(gh) - sqrt(lim));
    const double v = S(gh) * d;
    return v * sqrt(h);
}

// integrate_bin (integration.jl:166-200) as transfer_functions._integrate_bins evaluates it: 0 for a bin outside [gmin, gmax];
// the closed-form edge term where g✶ < h or g✶ > 1 - h, returned alone for a bin wholly inside such an edge; Gauss-Legendre on
// what is left.  A non-finite result counts as 0.
GR_LAG_DEV double integrate_bin(const Integrand& S, const Quad& q, double lo, double hi)
{
    GR_LAG_NO_CONTRACT
    const double gmin = S.a.gmin, gmax = S.a.gmax, span = S.a.span, h = q.h;
    double glo = clampd(lo, gmin, gmax), ghi = clampd(hi, gmin, gmax);
    if (glo == ghi) return 0.0;
    const double slo = (lo - gmin) / span, shi = (hi - gmin) / span;
    const double one_h = 1.0 - h;
    double lum = 0.0;
    if (slo < h) {
        if (shi > h) {
            lum += integrate_edge(S, glo, h, h);
            const double p = span * h;
            glo = p + gmin;
        } else {
            return finite_or_zero(integrate_edge(S, glo, shi, h));
        }
    }
    if (shi > one_h) {
        if (slo < one_h) {
            lum += integrate_edge(S, ghi, one_h, h);
            const double p = span * one_h;
            ghi = p + gmin;
        } else {
            return finite_or_zero(integrate_edge(S, ghi, slo, h));
        }
    }
    const double half = 0.5 * (ghi - glo);
    double sum = 0.0;
    for (int k = 0; k < q.n; ++k) {
        const double xs = (q.x[k] + 1.0) * half;
        const double v = S(xs + glo) * q.w[k];
        sum += v;
    }
    const double quad = sum * half;
    lum += quad;
    return finite_or_zero(lum);
}

// _time_g✶ (integration.jl:74-93): the two branches' times at g✶, blended into each other within h of an extremum
GR_LAG_DEV void time_gs(const Set& s, const Annulus& a, double h, double gs, double& t1, double& t2)
{
    GR_LAG_NO_CONTRACT
    const bool lo_e = gs < h, hi_e = gs > 1.0 - h;
    if (!lo_e && !hi_e) {
        t1 = blend(s, a, 0, s.kt, gs);
        t2 = blend(s, a, 1, s.kt, gs);
        return;
    }
    const double r = 1.0 - gs, rh = r / h;
    const double om = lo_e ? gs / h : 1.0 - rh;
    const double at = lo_e ? h : 1.0 - h;
    const double tle = blend(s, a, 0, s.kt, at), tue = blend(s, a, 1, s.kt, at);
    const double c = 1.0 - om;
    const double a1 = tle * om, b1 = c * tue, a2 = tue * om, b2 = c * tle;
    t1 = a1 + b1;
    t2 = a2 + b2;
}

// searchsortedfirst: the first edge >= v; n (past the last edge: the deposit is dropped) for a NaN as well
GR_LAG_DEV int first_edge_not_below(const double* edges, int n, double v)
{
    if (v != v) return n;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Line profile: what annulus `a` adds to g bin j -- integrate_bin of both branches times the annulus weight.  false: nothing
// (the bin lies outside [gmin, gmax], or the product is not finite).
GR_LAG_DEV bool line_deposit(const Set& s, const Annulus& a, const Quad& q, const double* g_edges, int j, double& v)
{
    GR_LAG_NO_CONTRACT
    const double lo = g_edges[j] / s.g_scale, hi = g_edges[j + 1] / s.g_scale;
    if (clampd(lo, a.gmin, a.gmax) == clampd(hi, a.gmin, a.gmax)) return false;
    const Integrand S{s, a, 0};
    v = integrate_bin(S, q, lo, hi) * a.theta;
    return fabs(v) < INFINITY;
}

// Lag transfer: the lower and the upper branch's deposits of annulus `a` and g bin j, each with its t bin (_time_bins,
// integration.jl:95-102, then searchsortedfirst).  it[k] = n_t: dropped.  Returns false if the bin lies outside [gmin, gmax].
GR_LAG_DEV bool lag_deposits(const Set& s, const Annulus& a, const Quad& q, const double* g_edges, int j, const double* t_edges,
                             int n_t, double v[2], int it[2])
{
    GR_LAG_NO_CONTRACT
    const double glo = clampd(g_edges[j] / s.g_scale, a.gmin, a.gmax), ghi = clampd(g_edges[j + 1] / s.g_scale, a.gmin, a.gmax);
    if (glo == ghi) return false;
    const Integrand S1{s, a, 1}, S2{s, a, 2};
    v[0] = integrate_bin(S1, q, glo, ghi) * a.theta;
    v[1] = integrate_bin(S2, q, glo, ghi) * a.theta;
    const double s1 = clampd((glo - a.gmin) / a.span, 0.0, 1.0), s2 = clampd((ghi - a.gmin) / a.span, 0.0, 1.0);
    double tl1, tu1, tl2, tu2;
    time_gs(s, a, q.h, s1, tl1, tu1);
    time_gs(s, a, q.h, s2, tl2, tu2);
    const double ml = 0.5 * (tl1 + tl2), mu = 0.5 * (tu1 + tu2);
    it[0] = first_edge_not_below(t_edges, n_t, ml + a.tsd);
    it[1] = first_edge_not_below(t_edges, n_t, mu + a.tsd);
    if (!(fabs(v[0]) < INFINITY)) it[0] = n_t;
    if (!(fabs(v[1]) < INFINITY)) it[1] = n_t;
    return true;
}

}  // namespace gr_tf
