// Host build of what the k_plane_* kernels run per pair, per column and per point -- the criterion and the fill arithmetic of
// gr_planegrid.hpp over the tree logic of gr_skygrid.hpp -- for tests/test_planegrid_host.py: the loops the kernels run, serially,
// on numpy's arrays.  TEST INFRASTRUCTURE, never linked into the library.
#include <cmath>
#include <vector>

#include "../gradus.jl_amd/csrc/gr_planegrid.hpp"

using namespace gr_skygrid;

extern "C" {

struct hpg_grid {
    double* pos;
    int32_t* level;
    int64_t* children;
    int64_t* neighbours;
    int64_t* parent;
    int8_t* location;
    int64_t n;
    double limits[4];
};

static Grid grid_of(const hpg_grid* h)
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

// gr_planegrid::need_refine per pair, as k_plane_mark_need calls it: kind GR_SKY_CRIT_PLANE or GR_SKY_CRIT_LEVEL
void hpg_need_refine(const hpg_grid* h, const gr_point* pts, int kind, int level, double rtol, const int64_t* i1, const int64_t* i2, int64_t n,
                     uint8_t* out)
{
    const Grid g = grid_of(h);
    gr_sky_criterion cr = {};
    cr.kind = kind;
    cr.level = level;
    cr.rtol = rtol;
    for (int64_t k = 0; k < n; ++k) out[k] = gr_planegrid::need_refine(cr, g, pts, i1[k], i2[k]) ? 1 : 0;
}

// gr_sky_fill_plane: the y grid walked in theta_order, then the three passes of the kernels one column after the other.
// out: n_y x n_x, cells: n_y x n_x x 2, counts: the cells recorded per column.
void hpg_fill(const hpg_grid* h, const gr_point* pts, const double* val, const double* x, int64_t n_x, const double* y, int64_t n_y, double* out,
              int64_t* cells, int64_t* counts)
{
    const Grid g = grid_of(h);
    std::vector<int64_t> perm((size_t)n_y), idx((size_t)n_y), comp((size_t)n_y);
    std::vector<double> sorted((size_t)n_y), col((size_t)n_y), colval((size_t)n_y);
    theta_order(y, n_y, perm.data());
    for (int64_t j = 0; j < n_y; ++j) sorted[(size_t)j] = y[perm[(size_t)j]];
    for (int64_t k = 0; k < n_x; ++k) {
        for (int64_t j = 0; j < n_y; ++j) idx[(size_t)j] = parent_index(g, x[k], sorted[(size_t)j]);
        const int64_t m = gr_planegrid::build_column(g, pts, val, x[k], idx.data(), n_y, comp.data(), col.data(), colval.data());
        counts[k] = m;
        for (int64_t j = 0; j < n_y; ++j) {
            const int64_t at = perm[(size_t)j] * n_x + k;
            int64_t lower = 0, upper = 0;
            out[at] = m < 2 ? NAN : gr_planegrid::fill_point(col.data(), colval.data(), comp.data(), m, sorted[(size_t)j], lower, upper);
            cells[2 * at] = lower;
            cells[2 * at + 1] = upper;
        }
    }
}

// gr_skygrid::top_cells: the neighbours of the nine top cells (10 x 4)
void hpg_top_neighbours(const double* limits, int x_periodic, int64_t* neighbours)
{
    double pos[20];
    int32_t level[10];
    int64_t children[90], parent[10];
    int8_t location[10];
    Grid g;
    g.pos = pos;
    g.level = level;
    g.children = children;
    g.neighbours = neighbours;
    g.parent = parent;
    g.location = location;
    g.n = 0;
    g.x1 = limits[0];
    g.x2 = limits[1];
    g.y1 = limits[2];
    g.y2 = limits[3];
    top_cells(g, x_periodic != 0);
}

}  // extern "C"
