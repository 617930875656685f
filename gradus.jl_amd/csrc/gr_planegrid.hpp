// gr_planegrid.hpp -- what an adaptive image PLANE (AdaptivePlane, src/image-planes/adaptive-plane.jl) adds to the tree logic of
// gr_skygrid.hpp: the same 3 x 3 refinement tree laid over an observer's impact parameters (α, β), one GeodesicPoint (gr_point,
// 152 bytes) per cell.  The pair criterion of adaptive-plane.jl:24-50 and the filled image of adaptive-plane.jl:100-181, as plain
// functions for the host and the device: the k_plane_* kernels (gradus_mi355x.hip) call them, tests/host_harness_planegrid.cpp
// compiles the same text with g++ against adaptive.py.  The discipline is that of gr_skygrid.hpp: every decision has to be the
// one numpy makes from the same numbers, so one rounding per operation and nothing contracted into an fma.
//
// Where the reference is wrong or cannot run, this header decides:
//  * adaptive-plane.jl:130 takes the neighbour's x from `pos[2]`, its y position -- a typo.  The neighbour's x position is used.
//  * a column with fewer than two cells is NaN, as gr_sky_fill makes it; the reference indexes out of bounds there.
//  * the image is out[β index, α index]; the reference's `reshape` to (length(x_grid), length(y_grid)) of values pushed column by
//    column is only meaningful for square grids.
//  * the values are doubles (one per cell, val[cell]); the reference pushes them into a Vector{Union{Nothing,GeodesicPoint}},
//    which cannot convert.
//  * the β grid may come in any order: it is walked as gr_skygrid::theta_order sorts it, the results land at the caller's indices.
//  * a neighbour that lies across the periodic wrap of an x_periodic grid (to the left of a cell and not left of it) is no
//    neighbour to interpolate with: the cell's own value is taken, as where there is no neighbour at all (neighbour 0, where the
//    reference reads row 0 of its arrays).
#pragma once
#include "gr_skygrid.hpp"

namespace gr_planegrid {

using gr_skygrid::Grid;

GR_SKY_DEV bool hit(const gr_point& p) { return p.status == GR_STATUS_INTERSECTED_WITH_GEOMETRY; }

// check_refine of adaptive-plane.jl:24-50 on two rows: both miss -> false; exactly one hits -> true; both hit -> log10 of the
// coordinate radius x[1] (not the equatorial projection) or θ = x[2] folded into [0, 2π) are not isapprox at rtol (atol = 0,
// false on NaN).  The reference also computes a ϕ term (`ph_too_coarse`) and never uses it: it is left out here.
GR_SKY_DEV bool pair_differs(const gr_point& a, const gr_point& b, double rtol)
{
    GR_SKY_NO_CONTRACT
    const bool h1 = hit(a), h2 = hit(b);
    if (!h1 && !h2) return false;
    if (!h1 || !h2) return true;
    const bool r_too_coarse = !gr_skygrid::isapprox(log10(a.x[1]), log10(b.x[1]), rtol);
    const bool th_too_coarse = !gr_skygrid::isapprox(gr_skygrid::fold_2pi(a.x[2]), gr_skygrid::fold_2pi(b.x[2]), rtol);
    return r_too_coarse || th_too_coarse;
}

// check_refine(sky, i1, i2) of a criterion on a plane sky: GR_SKY_CRIT_PLANE, or GR_SKY_CRIT_LEVEL (refine_to_level; a pair of
// cells that both miss is left alone, as on a corona sky -- "miss" is a status other than IntersectedWithGeometry here)
GR_SKY_DEV bool need_refine(const gr_sky_criterion& cr, const Grid& g, const gr_point* pts, int64_t i1, int64_t i2)
{
    const gr_point &a = pts[i1], &b = pts[i2];
    if (!hit(a) && !hit(b)) return false;
    if (cr.kind == GR_SKY_CRIT_LEVEL) return g.level[i2] < cr.level;
    return pair_differs(a, b, cr.rtol);
}

// ---- the filled image: adaptive-plane.jl:100-181, one column (an α of the x grid) at a time ----

// The value a column takes at cell c for the abscissa x: interpolated across α between c and its left (x < pos_x(c)) or right
// neighbour, with w as the reference writes it for each direction; the cell's own value if there is no neighbour, if the
// neighbour lies across the periodic wrap or if the neighbour's ray did not meet the geometry.
GR_SKY_DEV double column_value(const Grid& g, const gr_point* pts, const double* val, int64_t c, double x)
{
    GR_SKY_NO_CONTRACT
    const double cx = g.pos[2 * c];
    const bool left = x < cx;
    const int64_t nb = g.neighbours[4 * c + (left ? 3 : 1)];
    if (nb == 0) return val[c];
    const double nx = g.pos[2 * nb];
    if (left ? !(nx < cx) : !(nx > cx)) return val[c];
    if (!hit(pts[nb])) return val[c];
    if (left) {
        const double num = x - nx, den = cx - nx;
        const double w = num / den, u = 1.0 - w;
        const double p = u * val[nb], q = w * val[c];
        return p + q;
    }
    const double num = x - cx, den = nx - cx;
    const double w = num / den, u = 1.0 - w;
    const double p = u * val[c], q = w * val[nb];
    return p + q;
}

// One column: idx[j] is the cell that holds (x, y_j), y ascending along j (gr_skygrid::parent_index; 0 outside the domain or
// on a boundary of top-level cells).  Every run of points held by one cell is recorded in the order met -- `index > 0 &&
// index != curr_index` of the reference -- as (cell, pos_y(cell), column_value).  Returns the number of cells recorded (<= n).
GR_SKY_DEV int64_t build_column(const Grid& g, const gr_point* pts, const double* val, double x, const int64_t* idx, int64_t n,
                                int64_t* cells, double* column, double* values)
{
    int64_t current = 0, m = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t c = idx[j];
        if (!gr_skygrid::first_of_run(c, current)) continue;
        current = c;
        cells[m] = c;
        column[m] = g.pos[2 * c + 1];
        values[m] = column_value(g, pts, val, c, x);
        ++m;
    }
    return m;
}

// point y of a column of m >= 2 cells: clamp(searchsortedlast(column, y), 1, m - 1), linear in y; the two cells it lies between
GR_SKY_DEV double fill_point(const double* column, const double* values, const int64_t* cells, int64_t m, double y, int64_t& lower,
                             int64_t& upper)
{
    GR_SKY_NO_CONTRACT
    int64_t k = gr_skygrid::count_le(column, m, y);
    k = (k < 1 ? 1 : (k > m - 1 ? m - 1 : k)) - 1;
    lower = cells[k];
    upper = cells[k + 1];
    const double num = y - column[k], den = column[k + 1] - column[k];
    const double w = num / den, u = 1.0 - w;
    const double a = u * values[k], b = w * values[k + 1];
    return a + b;
}

}  // namespace gr_planegrid
