// host_harness_lagbin.cpp -- TEST INFRASTRUCTURE.  The per-hit arithmetic of the lag-energy bins (gr_lagbin.hpp) compiled for the
// host with g++: the two reductions of gr_lagtransfer_extrema / gr_lagtransfer_bin over rows (g, ρ, t, area) with the header's
// functions and the integer accumulators of the kernels, one row after the other.  Never linked into libgradus_mi355x.so.
#include <cstdint>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_lagbin.hpp"
#include "../include/gradus_mi355x.h"

namespace {

gr_lag::Profile profile_of(const gr_lagprofile* p)
{
    gr_lag::Profile q;
    q.E0 = p->E0; q.q = p->emissivity_index;
    q.eps_r = p->eps_r; q.eps_v = p->eps_v; q.eps_n = p->eps_n >= 2 ? p->eps_n : 0;
    q.time_r = p->time_r; q.time_v = p->time_v; q.time_n = p->time_n;
    return q;
}

// k_lag_extrema: min / max of E and t through the ordered bit patterns, the hit count and max |f|
void extrema(const gr_lag::Profile& q, const double* rows, int64_t n, double lims[4], int64_t* hits, double* fmax)
{
    unsigned long long v[4] = { ~0ull, 0ull, ~0ull, 0ull };
    *hits = 0;
    *fmax = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        gr_lag::Hit h;
        if (!gr_lag::hit_of(q, rows + 4 * i, h)) continue;
        const unsigned long long be = gr_lag::ordered_bits(h.E), bt = gr_lag::ordered_bits(h.t);
        v[0] = be < v[0] ? be : v[0];
        v[1] = be > v[1] ? be : v[1];
        v[2] = bt < v[2] ? bt : v[2];
        v[3] = bt > v[3] ? bt : v[3];
        const double af = std::fabs(h.f);
        if (af < INFINITY && af > *fmax) *fmax = af;
        ++*hits;
    }
    for (int k = 0; k < 4; ++k) lims[k] = gr_lag::ordered_value(v[k]);
}

// k_lag_bin: Σ f per cell as two integers on the grid of (max |f|, hits)
void bin(const gr_lag::Profile& q, const double* rows, int64_t n, const double* e_edges, int n_e, const double* t_edges, int n_t,
         const gr_lag::CoronaGrid& g, double* out)
{
    const size_t cells = (size_t)n_e * (size_t)n_t;
    std::vector<unsigned long long> acc(2 * cells, 0ull);
    for (int64_t i = 0; i < n; ++i) {
        gr_lag::Hit h;
        if (!gr_lag::hit_of(q, rows + 4 * i, h) || !(std::fabs(h.f) < INFINITY)) continue;
        const size_t cell = (size_t)gr_lag::bucket(e_edges, n_e, h.E) * (size_t)n_t + (size_t)gr_lag::bucket(t_edges, n_t, h.t);
        long long fh, fl;
        gr_lag::corona_split(h.f, g.sc, fh, fl);
        acc[cell] += (unsigned long long)fh;
        acc[cells + cell] += (unsigned long long)fl;
    }
    for (size_t c = 0; c < cells; ++c) out[c] = gr_lag::corona_sum((long long)acc[c], (long long)acc[cells + c], g);
}

}      // namespace

extern "C" {

int hlb_extrema(const gr_lagprofile* p, const double* rows, int64_t n, double* lims, double* flux_sum, int64_t* hits)
{
    const gr_lag::Profile q = profile_of(p);
    double fmax;
    extrema(q, rows, n, lims, hits, &fmax);
    const double edge = 0.0;
    bin(q, rows, n, &edge, 1, &edge, 1, gr_lag::corona_grid(fmax, *hits), flux_sum);
    return 0;
}

int hlb_bin(const gr_lagprofile* p, const double* rows, int64_t n, const double* e_edges, int64_t n_e, const double* t_edges,
            int64_t n_t, double* out)
{
    const gr_lag::Profile q = profile_of(p);
    double lims[4], fmax;
    int64_t hits;
    extrema(q, rows, n, lims, &hits, &fmax);
    bin(q, rows, n, e_edges, (int)n_e, t_edges, (int)n_t, gr_lag::corona_grid(fmax, hits), out);
    return 0;
}

// one hit's (E, t, f) and its cell, for the tests of the interpolation rule and of the clamped bucket
int hlb_hit(const gr_lagprofile* p, const double* row, double* etf)
{
    gr_lag::Hit h;
    if (!gr_lag::hit_of(profile_of(p), row, h)) return 0;
    etf[0] = h.E; etf[1] = h.t; etf[2] = h.f;
    return 1;
}
// radius index of every local ray 0 .. n-1 of a separable set laid out as rays_params (gradus_mi355x.hip) lays it out
void hlb_sep_rows(int64_t nr, int64_t nt, int tiled, int64_t first, int64_t block, int64_t stride, int64_t n, int64_t* out)
{
    gr_lag::LagSep p{};
    const bool t = tiled && nr >= 8 && nt >= 8;
    p.nr = nr; p.core_rows = t ? (nr / 8) * 8 : 0; p.core_cols = t ? (nt / 8) * 8 : 0;
    p.first = first; p.block = block; p.stride = stride;
    for (int64_t j = 0; j < n; ++j) out[j] = gr_lag::sep_row(p, j);
}
int hlb_bucket(const double* edges, int64_t n, double v) { return gr_lag::bucket(edges, (int)n, v); }

}      // extern "C"
