// Host build of what gr_sky_bin_grid, gr_sky_fill and gr_disc_area_factor run per leaf, per column and per radius -- the map and
// fill arithmetic of gr_skygrid.hpp, the fixed-point sums of gr_lagbin.hpp and disc_area_factor of gr_device.hpp -- for
// tests/test_skymaps_host.py: the loops the kernels run, serially, on numpy's arrays.  TEST INFRASTRUCTURE, never linked into the
// library.
#define GR_HOST_HARNESS 1
#include <cmath>
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_device.hpp"
#include "../gradus.jl_amd/csrc/gr_lagbin.hpp"
#include "../gradus.jl_amd/csrc/gr_skygrid.hpp"
#include "host_harness_common.hpp"

using namespace gr_skygrid;

extern "C" {

struct hsm_grid {
    double* pos;
    int32_t* level;
    int64_t* children;
    int64_t* neighbours;
    int64_t* parent;
    int8_t* location;
    int64_t n;
    double limits[4];
};

static Grid grid_of(const hsm_grid* h)
{
    Grid g;
    g.pos = h->pos;
    g.level = h->level;
    g.children = h->children;
    g.neighbours = h->neighbours;
    g.parent = h->parent;
    g.location = h->location;
    g.n = h->n;
    g.x1 = h->limits[0];
    g.x2 = h->limits[1];
    g.y1 = h->limits[2];
    g.y2 = h->limits[3];
    return g;
}

// gr_sky_bin_grid: the reduction of k_sky_map_extrema, the grid of the sums, map_accumulate per leaf as k_sky_map_bin calls it and
// the driver's own last pass (map_finish).  `order`: the cells in the order they are visited (the device's order is whatever the
// launch makes it).  0, or -2 where a bin's terms vanish.
int hsm_bin_grid(const hsm_grid* h, const double* rows, const int64_t* order, int64_t n_order, int what, const double* r_bins, int64_t nr,
                 const double* phi_bins, int64_t nphi, int has_gamma, double gamma, const double* area, double* out, double* solid_angle)
{
    const Grid g = grid_of(h);
    MapBins b;
    b.r_bins = r_bins;
    b.nr = nr;
    b.phi_bins = phi_bins;
    b.nphi = nphi;
    b.r_max = r_bins[0];
    for (int64_t k = 1; k < nr; ++k) b.r_max = r_bins[k] > b.r_max ? r_bins[k] : b.r_max;
    const int64_t cells = nr * nphi;
    double max_term = 0.0, max_solid = 0.0;
    for (int64_t q = 0; q < n_order; ++q) {
        const int64_t c = order[q];
        if (c < 1 || c > g.n || !is_leaf(g, c)) continue;
        int64_t bin;
        double solid, term;
        if (!map_term(g, rows, c, b, what, has_gamma != 0, gamma, area, bin, solid, term)) continue;
        const double at = std::fabs(term), as = std::fabs(solid);
        if (at < INFINITY && at > max_term) max_term = at;
        if (as < INFINITY && as > max_solid) max_solid = as;
    }
    const gr_lag::CoronaGrid gt = gr_lag::corona_grid(max_term, g.n), gs = gr_lag::corona_grid(max_solid, g.n);
    std::vector<long long> acc((size_t)(4 * cells), 0);
    std::vector<unsigned int> cnt((size_t)cells, 0);
    std::vector<uint8_t> flag((size_t)(4 * cells), 0);
    for (int64_t q = 0; q < n_order; ++q) {
        const int64_t c = order[q];
        if (c < 1 || c > g.n || !is_leaf(g, c)) continue;
        int64_t bin;
        double solid, term;
        if (!map_term(g, rows, c, b, what, has_gamma != 0, gamma, area, bin, solid, term)) continue;
        map_accumulate(bin, solid, term, cells, gt.sc, gs.sc, flag.data(), [&](int64_t at, long long v) { acc[(size_t)at] += v; },
                       [&](int64_t at) { ++cnt[(size_t)at]; });
    }
    const int rc = map_finish(acc.data(), cnt.data(), flag.data(), cells, gt, gs, out, solid_angle) ? -2 : 0;
    return rc;
}

// gr_sky_fill: the θ grid walked in theta_order, then k_sky_fill one column after the other: the cells of the points, the first
// point of every run compacted in chunks of `chunk` points with the carries of the two scans, the check that the column's θ
// ascend, then every point, stored at the caller's index.  out: n_theta x n_phi x 6, cells: n_theta x n_phi x 2, counts: the
// compacted cells per column.  Returns the number of columns whose θ do not ascend strictly.
int64_t hsm_fill(const hsm_grid* h, const double* rows, const double* phi, int64_t n_phi, const double* theta, const double* cos_theta,
                 int64_t n_theta, int64_t chunk, double* out, int64_t* cells, int64_t* counts, int64_t* compacted)
{
    const Grid g = grid_of(h);
    std::vector<int64_t> idx((size_t)n_theta), comp((size_t)n_theta), perm((size_t)n_theta);
    std::vector<double> col((size_t)n_theta), sorted((size_t)n_theta), sorted_cos((size_t)n_theta);
    theta_order(theta, n_theta, perm.data());
    for (int64_t j = 0; j < n_theta; ++j) {
        sorted[(size_t)j] = theta[perm[(size_t)j]];
        sorted_cos[(size_t)j] = cos_theta[perm[(size_t)j]];
    }
    theta = sorted.data();
    cos_theta = sorted_cos.data();
    int64_t bad = 0;
    for (int64_t k = 0; k < n_phi; ++k) {
        for (int64_t j = 0; j < n_theta; ++j) idx[(size_t)j] = parent_index(g, cos_theta[j], phi[k]);
        int64_t carry_cell = 0, carry_count = 0;
        for (int64_t t = 0; t < n_theta; t += chunk) {
            int64_t last = 0, count = 0;      // the inclusive scans inside the chunk
            for (int64_t j = t; j < t + chunk && j < n_theta; ++j) {
                const int64_t c = idx[(size_t)j];
                const int64_t before = last_nonzero(carry_cell, last);
                if (first_of_run(c, before)) {
                    comp[(size_t)(carry_count + count)] = c;
                    col[(size_t)(carry_count + count)] = std::acos(g.pos[2 * c]);
                    ++count;
                }
                last = last_nonzero(last, c);
            }
            carry_cell = last_nonzero(carry_cell, last);
            carry_count += count;
        }
        const int64_t m = carry_count;
        counts[k] = m;
        for (int64_t q = 0; q < m; ++q) compacted[k * n_theta + q] = comp[(size_t)q];
        bool ascending = true;
        for (int64_t q = 0; q + 1 < m; ++q)
            if (!(col[(size_t)q] < col[(size_t)q + 1])) ascending = false;
        if (!ascending) ++bad;
        for (int64_t j = 0; j < n_theta; ++j) {
            const int64_t at = perm[(size_t)j] * n_phi + k;
            double* o = out + 6 * at;
            int64_t lower = 0, upper = 0;
            if (m < 2) {
                for (int q = 0; q < 6; ++q) o[q] = NAN;
            } else {
                fill_point(col.data(), comp.data(), m, rows, theta[j], o, lower, upper);
            }
            cells[2 * at] = lower;
            cells[2 * at + 1] = upper;
        }
    }
    return bad;
}

// k_disc_area_factor: disc_area_factor of gr_device.hpp at n radii, the plunging table read through its host pointers.  0, or -1
// for a metric the harness does not instantiate.
int hsm_area_factor(const gr_config* cfg, const gr_pointfunction* pf, const double* r, int64_t n, double* out)
{
    using namespace GR_NS;
    Params p;
    Cold c;
    hh::fill(p, c, cfg, n, pf);      // (disc_area_factor reads the configuration and the point function's ISCO and plunging table)
    if (cfg->metric_id == GR_METRIC_TABULATED) return -1;
#define HSM_RUN(M)                                                              \
    do {                                                                        \
        M m;                                                                    \
        m.load(p.cfg);                                                          \
        for (int64_t i = 0; i < n; ++i) out[i] = disc_area_factor(m, p, c, r[i]); \
    } while (0)
    if (cfg->metric_id == GR_METRIC_KERR) HSM_RUN(KerrMetric);
    else if (cfg->metric_id == GR_METRIC_KERR_NEWMAN) HSM_RUN(KerrNewmanMetric);
    else if (cfg->metric_id == GR_METRIC_JOHANNSEN) HSM_RUN(JohannsenMetric);
    else HSM_RUN(GenericMetric);
#undef HSM_RUN
    return 0;
}

}  // extern "C"
