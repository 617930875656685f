// Host build of gr_skygrid.hpp -- the tree logic of a resident adaptive sky (the k_sky_* kernels of gradus_mi355x.hip call the
// same functions per cell) -- for tests/test_skygrid_host.py: the loops the kernels run, serially, on numpy's arrays.
#include <cstring>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_skygrid.hpp"

using namespace gr_skygrid;

extern "C" {

struct hsg_grid {
    double* pos;
    int32_t* level;
    int64_t* children;
    int64_t* neighbours;
    int64_t* parent;
    int8_t* location;
    int64_t n;
    double limits[4];
};

static Grid grid_of(const hsg_grid* h)
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

int hsg_max_level(void) { return GR_SKY_MAX_LEVEL; }

// gr_sky_create: row 0 and the nine top cells
int64_t hsg_top(hsg_grid* h, int x_periodic)
{
    Grid g = grid_of(h);
    top_cells(g, x_periodic != 0);
    h->n = g.n;
    return g.n;
}

// k_sky_pair_count + scan + k_sky_pair_fill; i1 / i2 may be null (count only).  -1: a walk ran out of stack
int64_t hsg_pairs(const hsg_grid* h, int64_t* i1, int64_t* i2, int64_t cap)
{
    const Grid g = grid_of(h);
    int64_t total = 0;
    for (int64_t c = 1; c <= g.n; ++c) {
        if (!is_leaf(g, c)) continue;
        const int k = walk_bordering(g, c, [&](int64_t other) {
            if (i1 && i2 && total < cap) {
                i1[total] = c;
                i2[total] = other;
            }
            ++total;
        });
        if (k < 0) return -1;
    }
    return total;
}

// k_sky_mark_need + k_sky_compact: the marked cells, ascending
int64_t hsg_find_need_refine(const hsg_grid* h, const double* rows, const gr_sky_criterion* cr, int64_t* list)
{
    const Grid g = grid_of(h);
    std::vector<uint8_t> mark((size_t)g.n + 1, 0);
    for (int64_t c = 1; c <= g.n; ++c) {
        if (!is_leaf(g, c)) continue;
        const int k = walk_bordering(g, c, [&](int64_t other) {
            if (need_refine(*cr, g, rows, c, other)) mark[(size_t)other] = 1;
        });
        if (k < 0) return -1;
    }
    int64_t m = 0;
    for (int64_t c = 0; c <= g.n; ++c)
        if (mark[(size_t)c]) list[m++] = c;
    return m;
}

// k_sky_refusals + k_sky_children (the grid's arrays hold n + 1 + 9 m rows): 0, or the refusal (1 range, 2 refined already,
// 3 deepest level, 4 named twice) with the grid as it was.  rows (may be null): the middle child takes its parent's row.
int hsg_refine(hsg_grid* h, const int64_t* list, int64_t m, double* rows)
{
    const Grid g = grid_of(h);
    std::vector<uint32_t> seen((size_t)g.n + 1, 0);
    int why = 0;
    for (int64_t k = 0; k < m; ++k) {
        int w = refine_refusal(g, list[k]);
        if (w == 0 && seen[(size_t)list[k]]++ != 0) w = 4;
        if (w > why) why = w;
    }
    if (why) return why;
    for (int64_t w = 0; w < 9 * m; ++w) {
        const int64_t k = w / 9;
        const int c = (int)(w - 9 * k);
        const int64_t first = g.n + 1 + 9 * k;
        write_child(g, list[k], first, c);
        if (rows && c == 4) std::memcpy(rows + 6 * (first + c), rows + 6 * list[k], 6 * sizeof(double));
    }
    h->n = g.n + 9 * m;
    return 0;
}

void hsg_parent_index(const hsg_grid* h, const double* x, const double* y, int64_t k, int64_t* out)
{
    const Grid g = grid_of(h);
    for (int64_t j = 0; j < k; ++j) out[j] = parent_index(g, x[j], y[j]);
}

// the leaves that land in a bin, ascending: (leaf, r index, ϕ index); and k_sky_occupancy's counts (may be null)
int64_t hsg_bins(const hsg_grid* h, const double* rows, const double* r_bins, int64_t nr, const double* phi_bins, int64_t nphi, int has_gamma,
                 double gamma, int64_t* leaf, int64_t* ri, int64_t* pi, int64_t* counts)
{
    const Grid g = grid_of(h);
    double r_max = r_bins[0];
    for (int64_t k = 1; k < nr; ++k) r_max = r_bins[k] > r_max ? r_bins[k] : r_max;
    int64_t m = 0;
    for (int64_t c = 1; c <= g.n; ++c) {
        if (!is_leaf(g, c)) continue;
        int64_t a, b;
        if (!bin_of(rows + 6 * c, r_bins, nr, r_max, phi_bins, nphi, a, b)) continue;
        leaf[m] = c;
        ri[m] = a;
        pi[m] = b;
        ++m;
        if (counts && lights(rows + 6 * c, has_gamma != 0, gamma)) ++counts[a * nphi + b];
    }
    return m;
}

int hsg_need_refine(const hsg_grid* h, const double* rows, const gr_sky_criterion* cr, int64_t i1, int64_t i2)
{
    return need_refine(*cr, grid_of(h), rows, i1, i2) ? 1 : 0;
}

}  // extern "C"
