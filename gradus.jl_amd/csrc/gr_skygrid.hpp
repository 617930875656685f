// gr_skygrid.hpp -- the tree logic of an adaptive sky (Grids.AdaptiveGrid, src/image-planes/adaptive-grid.jl; find_need_refine,
// src/image-planes/adaptive-sky.jl:130-152; the criteria and the (r, ϕ) bins of src/corona/adaptive-sample.jl) on the arrays of
// grids.AdaptiveGrid as they are: pos (2 doubles), level, children (9), neighbours (4), parent, location per cell and one row of
// 6 doubles (t, r, ϕ, g, J, status).  Cells count from 1 and row 0 is the null cell.
// Plain functions for the host and the device: the k_sky_* kernels (gradus_mi355x.hip) call them per cell, and
// tests/host_harness_skygrid.cpp compiles the same text with g++ against grids.py / adaptive.py.
//
// Every decision here -- which cell holds a point, which bin a leaf lands in, whether two rows differ by more than a tolerance --
// has to be the one numpy makes from the same numbers, so nothing may be contracted into an fma (the library is built with
// -ffp-contract=on): positions, widths and tolerances are formed with one rounding per operation, as numpy forms them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/gradus_mi355x.h"
#include "gr_lagbin.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GR_SKY_DEV __host__ __device__ __forceinline__
#else
#define GR_SKY_DEV inline
#endif
#if defined(__clang__)
#define GR_SKY_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GR_SKY_NO_CONTRACT      // (g++ fuses only with -mfma / -march; the harness is built with -ffp-contract=off all the same)
#endif

#define GR_SKY_MAX_LEVEL 20     // the deepest level a cell may have: refining a cell of this level is refused
#define GR_SKY_STACK 64         // the bordering walk's stack: at most 1 + 2 GR_SKY_MAX_LEVEL entries are ever on it

namespace gr_skygrid {

struct Grid {
    double* pos;            // (n + 1) x 2
    int32_t* level;
    int64_t* children;      // (n + 1) x 9; 0 in column 0 = not refined
    int64_t* neighbours;    // (n + 1) x 4: top, right, bottom, left
    int64_t* parent;
    int8_t* location;       // the child index (1 ... 9) a cell holds in its parent
    int64_t n;              // cells
    double x1, x2, y1, y2;  // limits, x1 <= x2, y1 <= y2
};

// 3.0 ** level: exact (3^33 < 2^53)
GR_SKY_DEV double pow3(int level)
{
    double f = 1.0;
    for (int k = 0; k < level; ++k) f *= 3.0;
    return f;
}

GR_SKY_DEV bool is_leaf(const Grid& g, int64_t cell) { return g.children[9 * cell] == 0; }

// get_cell_width
GR_SKY_DEV void cell_width(const Grid& g, int64_t cell, double& wx, double& wy)
{
    const double f = pow3(g.level[cell]);
    wx = fabs(g.x2 - g.x1) / f;
    wy = fabs(g.y2 - g.y1) / f;
}

// AdaptiveGrid.__init__: row 0 and the nine top cells (arrays of at least 10 rows)
inline void top_cells(Grid& g, bool x_periodic)
{
    GR_SKY_NO_CONTRACT
    const double dx = g.x2 - g.x1, dy = g.y2 - g.y1;
    const double mx = dx / 2 + g.x1, my = dy / 2 + g.y1;
    for (int i = 0; i < 10; ++i) {
        for (int c = 0; c < 9; ++c) g.children[9 * i + c] = 0;
        for (int d = 0; d < 4; ++d) g.neighbours[4 * i + d] = 0;
        g.parent[i] = 0;
        g.level[i] = i == 0 ? 0 : 1;
        g.location[i] = (int8_t)i;
    }
    g.pos[0] = g.pos[1] = NAN;
    for (int i = 1; i < 10; ++i) {
        const double ox = (double)((i - 1) / 3 - 1), oy = (double)((i - 1) % 3 - 1);
        const double sx = (dx / 3) * ox, sy = (dy / 3) * oy;
        g.pos[2 * i] = mx + sx;
        g.pos[2 * i + 1] = my + sy;
    }
    const int64_t p = x_periodic ? 1 : 0;
    const int64_t nb[9][4] = { { 0, 4, 2, 7 * p }, { 1, 5, 3, 8 * p }, { 2, 6, 0, 9 * p }, { 0, 7, 5, 1 }, { 4, 8, 6, 2 },
                               { 5, 9, 0, 3 },     { 0, 1 * p, 8, 4 }, { 7, 2 * p, 9, 5 }, { 8, 3 * p, 0, 6 } };
    for (int i = 1; i < 10; ++i)
        for (int d = 0; d < 4; ++d) g.neighbours[4 * i + d] = nb[i - 1][d];
    g.n = 9;
}

// refine_many, one child: child c (0 ... 8, column order) of `cell`, whose nine children take the rows first ... first + 8.
// Positions from _DIRECTIONS, neighbours from _CHILD_NEIGHBOURS: a sibling inside the parent, the PARENT's neighbour outside it.
GR_SKY_DEV void write_child(const Grid& g, int64_t cell, int64_t first, int c)
{
    GR_SKY_NO_CONTRACT
    const int64_t row = first + c;
    const int lev = g.level[cell] + 1;
    const double f = pow3(lev);
    const double wx = fabs(g.x2 - g.x1) / f, wy = fabs(g.y2 - g.y1) / f;
    const int cx = c / 3, cy = c % 3;
    const double sx = wx * (double)(cx - 1), sy = wy * (double)(cy - 1);
    g.pos[2 * row] = g.pos[2 * cell] + sx;
    g.pos[2 * row + 1] = g.pos[2 * cell + 1] + sy;
    g.level[row] = lev;
    g.parent[row] = cell;
    g.location[row] = (int8_t)(c + 1);
    for (int k = 0; k < 9; ++k) g.children[9 * row + k] = 0;
    const int64_t* out = g.neighbours + 4 * cell;
    g.neighbours[4 * row + 0] = cy > 0 ? first + c - 1 : out[0];
    g.neighbours[4 * row + 1] = cx < 2 ? first + c + 3 : out[1];
    g.neighbours[4 * row + 2] = cy < 2 ? first + c + 1 : out[2];
    g.neighbours[4 * row + 3] = cx > 0 ? first + c - 3 : out[3];
    g.children[9 * cell + c] = row;
}

// what refine_many raises on, and the level cap: 0 = the cell may be refined
GR_SKY_DEV int refine_refusal(const Grid& g, int64_t cell)
{
    if (cell < 1 || cell > g.n) return 1;                      // out of range
    if (!is_leaf(g, cell)) return 2;                           // already refined
    if (g.level[cell] >= GR_SKY_MAX_LEVEL) return 3;           // its children would lie below the deepest level
    return 0;
}

// _FACINGS[direction][k]: the child indices (0-based) on the top / right / bottom / left side of a cell
GR_SKY_DEV int facing(int direction, int k)
{
    return direction == 0 ? 3 * k : direction == 1 ? 6 + k : direction == 2 ? 2 + 3 * k : k;
}

// get_bordering / _get_facing without recursion: the leaves that touch the four sides of `cell`, in the reference's order
// (directions top, right, bottom, left; children in _FACINGS order), each given to visit(other).  A neighbour coarser than the
// asking cell is followed along the asking cell's own place (its `locations`, read by walking parent / location).
// Returns the number of leaves visited, or -1 if the stack would overflow (no tree within GR_SKY_MAX_LEVEL can do that).
template <class F>
GR_SKY_DEV int walk_bordering(const Grid& g, int64_t cell, F&& visit)
{
    const int level = g.level[cell];
    int8_t loc[GR_SKY_MAX_LEVEL + 1];
    for (int l = 0; l <= GR_SKY_MAX_LEVEL; ++l) loc[l] = 1;
    {
        int64_t i = cell;
        for (int l = level; l >= 1 && l <= GR_SKY_MAX_LEVEL && i != 0; --l) {
            loc[l - 1] = g.location[i];
            i = g.parent[i];
        }
    }
    int64_t stack[GR_SKY_STACK];
    int count = 0;
    for (int d = 0; d < 4; ++d) {
        const int64_t nb = g.neighbours[4 * cell + d];
        if (nb == 0) continue;
        const int direction = (d + 2) & 3;      // _FACING_LOOKUP: the side of the neighbour that faces the cell
        int sp = 0;
        stack[sp++] = nb;
        while (sp > 0) {
            const int64_t c = stack[--sp];
            const int64_t* kids = g.children + 9 * c;
            if (kids[0] == 0) {
                visit(c);
                ++count;
                continue;
            }
            const int own = g.level[c];
            if (own < level) {
                const int l = loc[own < GR_SKY_MAX_LEVEL ? own : GR_SKY_MAX_LEVEL];
                const int position = (direction & 1) ? (l - 1) % 3 : (l - 1) / 3;
                stack[sp++] = kids[facing(direction, position)];
            } else {
                if (sp + 3 > GR_SKY_STACK) return -1;
                for (int k = 2; k >= 0; --k) stack[sp++] = kids[facing(direction, k)];
            }
        }
    }
    return count;
}

// contains / _relative_location / get_parent_index exactly as grids.py writes them: the most refined cell that contains
// (x, y); 0 outside the domain or on a boundary between top-level cells
GR_SKY_DEV bool contains(const Grid& g, int64_t cell, double x, double y)
{
    GR_SKY_NO_CONTRACT
    double wx, wy;
    cell_width(g, cell, wx, wy);
    const double px = g.pos[2 * cell], py = g.pos[2 * cell + 1];
    const double hx = wx / 2, hy = wy / 2;
    return (px - hx < x) && (px + hx > x) && (py - hy < y) && (py + hy > y);
}
GR_SKY_DEV int relative_location(const Grid& g, int64_t cell, double x, double y)
{
    GR_SKY_NO_CONTRACT
    double wx, wy;
    cell_width(g, cell, wx, wy);
    const double sx = wx / 6, sy = wy / 6;
    const double px = g.pos[2 * cell], py = g.pos[2 * cell + 1];
    const int xo = px - sx > x ? -1 : (px + sx < x ? 1 : 0);
    const int yo = py - sy > y ? -1 : (py + sy < y ? 1 : 0);
    return (1 + xo) * 3 + yo + 2;
}
GR_SKY_DEV int64_t parent_index(const Grid& g, double x, double y)
{
    int64_t current = 0;
    for (int64_t i = 1; i < 10; ++i)
        if (contains(g, i, x, y)) {
            current = i;
            break;
        }
    if (current == 0) return 0;
    while (!is_leaf(g, current)) current = g.children[9 * current + relative_location(g, current, x, y) - 1];
    return current;
}

// ---- the pair criteria (adaptive-sample.jl:123-140, 682-719) on rows (t, r, ϕ, g, J, status) ----

// adaptive._isapprox: Base.isapprox(a, b; rtol) with atol = 0, false wherever either is NaN
GR_SKY_DEV bool isapprox(double a, double b, double rtol)
{
    GR_SKY_NO_CONTRACT
    if (a == b) return true;
    const double diff = fabs(a - b), big = fmax(fabs(a), fabs(b));
    const double bound = rtol * big;
    return diff <= bound;        // (NaN on either side: false)
}

// np.mod(ϕ, 2π) spelled out: fmod, then + 2π if the result is negative
GR_SKY_DEV double fold_2pi(double phi)
{
    const double two_pi = 6.283185307179586;
    double m = fmod(phi, two_pi);
    if (m < 0.0) m += two_pi;
    return m;
}

GR_SKY_DEV bool in_interval(double v, double lo, double hi, int open_lo, int open_hi)
{
    return (open_lo ? v > lo : v >= lo) && (open_hi ? v < hi : v <= hi);
}

// a box: an r interval and zero, one or two intervals of mod(ϕ, 2π)
GR_SKY_DEV bool in_box(const gr_sky_box& b, const double* row)
{
    if (!in_interval(row[1], b.r_lo, b.r_hi, b.r_open_lo, b.r_open_hi)) return false;
    if (b.n_phi <= 0) return true;
    const double p = fold_2pi(row[2]);
    for (int k = 0; k < b.n_phi && k < 2; ++k)
        if (in_interval(p, b.phi_lo[k], b.phi_hi[k], b.phi_open_lo, b.phi_open_hi)) return true;
    return false;
}
GR_SKY_DEV bool in_any_box(const gr_sky_criterion& cr, const double* row)
{
    for (int k = 0; k < cr.n_boxes && k < GR_SKY_MAX_BOXES; ++k)
        if (in_box(cr.boxes[k], row)) return true;
    return false;
}

// check_refine(sky, i1, i2) of the criterion: i1 the leaf, i2 its bordering leaf (the one that is refined)
GR_SKY_DEV bool need_refine(const gr_sky_criterion& cr, const Grid& g, const double* rows, int64_t i1, int64_t i2)
{
    const double *v1 = rows + 6 * i1, *v2 = rows + 6 * i2;
    if (v1[1] != v1[1] && v2[1] != v2[1]) return false;        // both miss
    if (cr.kind == GR_SKY_CRIT_LEVEL) return g.level[i2] < cr.level;
    if (cr.kind == GR_SKY_CRIT_FUNCTION) return in_any_box(cr, v1) || in_any_box(cr, v2);
    const bool coarse = !isapprox(v1[3], v2[3], cr.rtol) || !isapprox(v1[4], v2[4], cr.rtol);
    if (cr.kind == GR_SKY_CRIT_FINE) return coarse && (in_any_box(cr, v1) || in_any_box(cr, v2));
    return coarse;
}

// ---- the (r, ϕ) bin of a leaf, as adaptive._binned_cells finds it ----

// np.searchsorted(edges, v, side = "right"): the number of edges <= v; a NaN sorts behind every edge
GR_SKY_DEV int64_t count_le(const double* edges, int64_t n, double v)
{
    if (v != v) return n;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// false: the leaf is dropped (NaN r, r above r_max = the largest edge, r or ϕ mod 2π below the first edge)
GR_SKY_DEV bool bin_of(const double* row, const double* r_bins, int64_t nr, double r_max, const double* phi_bins, int64_t nphi,
                       int64_t& ri, int64_t& pi)
{
    const double r = row[1];
    if (r != r || r > r_max) return false;
    ri = count_le(r_bins, nr, r);
    pi = count_le(phi_bins, nphi, fold_2pi(row[2]));
    if (ri == 0 || pi == 0) return false;
    --ri;
    --pi;
    return true;
}
// does the leaf light its bin -- is J g^Γ anything but ±0 (a NaN counts)?  has_gamma = false leaves the redshift out.
GR_SKY_DEV bool lights(const double* row, bool has_gamma, double gamma)
{
    const double w = has_gamma ? row[4] * pow(row[3], gamma) : row[4];
    return !(w == 0.0);
}

// ---- the (r, ϕ) maps: adaptive._binned_cells / _bin_grid (adaptive-sample.jl:266-450) ----

// ΔΩ of a leaf: wx wy / sin(acos(cos θ))
GR_SKY_DEV double leaf_solid_angle(const Grid& g, int64_t cell)
{
    GR_SKY_NO_CONTRACT
    double wx, wy;
    cell_width(g, cell, wx, wy);
    const double theta = acos(g.pos[2 * cell]);
    const double a = wx * wy;
    return a / sin(theta);
}
// what a leaf's ΔΩ is multiplied by: J (g^Γ γA) for the emissivity (`area` = γ(r) A(r) of the leaf's r), g, or t
GR_SKY_DEV double map_weight(int what, const double* row, bool has_gamma, double gamma, double area)
{
    GR_SKY_NO_CONTRACT
    if (what == GR_SKY_MAP_REDSHIFT) return row[3];
    if (what == GR_SKY_MAP_TIME) return row[0];
    const double redshift = has_gamma ? pow(row[3], gamma) : 1.0;
    const double ra = redshift * area;
    return row[4] * ra;
}
struct MapBins { const double* r_bins; int64_t nr; double r_max; const double* phi_bins; int64_t nphi; };
// the bin of leaf c, its ΔΩ and its term ΔΩ w; false: the leaf is dropped.  area: γA per cell (emissivity only)
GR_SKY_DEV bool map_term(const Grid& g, const double* rows, int64_t c, const MapBins& b, int what, bool has_gamma, double gamma,
                         const double* area, int64_t& bin, double& solid, double& term)
{
    GR_SKY_NO_CONTRACT
    int64_t ri, pi;
    if (!bin_of(rows + 6 * c, b.r_bins, b.nr, b.r_max, b.phi_bins, b.nphi, ri, pi)) return false;
    bin = ri * b.nphi + pi;
    solid = leaf_solid_angle(g, c);
    term = solid * map_weight(what, rows + 6 * c, has_gamma, gamma, what == GR_SKY_MAP_EMISSIVITY ? area[c] : 0.0);
    return true;
}

// One leaf's share of its bin, for the kernel (k_sky_map_bin: `add` an integer atomic) and the host harness (a plain +=) alike.
// acc: 4 x cells integers (Σ ΔΩ w hi / lo, Σ ΔΩ hi / lo) on the grids `st` / `ss`; `count(bin)`: one more non-zero finite term;
// flag: 4 x cells bytes -- a NaN term, a +∞ term, a -∞ term, a ΔΩ that is not finite -- set by a plain store of 1 (idempotent)
template <class Add, class Count>
GR_SKY_DEV void map_accumulate(int64_t bin, double solid, double term, int64_t cells, const gr_lag::CoronaScale& st,
                               const gr_lag::CoronaScale& ss, uint8_t* flag, Add&& add, Count&& count)
{
    if (!(fabs(solid) < INFINITY)) {
        flag[bin] = 1;
        flag[3 * cells + bin] = 1;
        return;
    }
    long long hi, lo;
    gr_lag::corona_split(solid, ss, hi, lo);
    add(2 * cells + bin, hi);
    add(3 * cells + bin, lo);
    if (term != term) flag[bin] = 1;
    else if (term == INFINITY) flag[cells + bin] = 1;
    else if (term == -INFINITY) flag[2 * cells + bin] = 1;
    else if (term != 0.0) {
        gr_lag::corona_split(term, st, hi, lo);
        add(bin, hi);
        add(cells + bin, lo);
        count(bin);
    }
}

// what the sums and the flags of a bin stand for: Σ ΔΩ w / Σ ΔΩ where Σ ΔΩ > 0 -- `output[lit] /= solid_angle[lit]`, a bin
// without leaves keeps its 0 -- with the NaN and ±∞ np.add.at would have summed to.  Host only (long double, gr_lag::corona_sum).
inline void map_bin_value(double num, double den, const uint8_t flags[4], double& value, double& solid)
{
    if (flags[3]) den = NAN;
    if (flags[0] || (flags[1] && flags[2])) num = NAN;
    else if (flags[1]) num = INFINITY;
    else if (flags[2]) num = -INFINITY;
    value = den > 0.0 ? num / den : num;
    solid = den;
}
// The last pass of gr_sky_bin_grid over what map_accumulate left: out (and solid_angle, may be null) per bin.  Returns the number
// of bins that hold non-zero terms, no NaN, and sum to 0: terms below the resolution gt.step * gt.lo_unit of the sums.
inline int64_t map_finish(const long long* acc, const unsigned int* cnt, const uint8_t* flag, int64_t cells, const gr_lag::CoronaGrid& gt,
                          const gr_lag::CoronaGrid& gs, double* out, double* solid_angle)
{
    int64_t vanished = 0;
    for (int64_t k = 0; k < cells; ++k) {
        const uint8_t f[4] = { flag[k], flag[cells + k], flag[2 * cells + k], flag[3 * cells + k] };
        double v, den;
        map_bin_value(gr_lag::corona_sum(acc[k], acc[cells + k], gt), gr_lag::corona_sum(acc[2 * cells + k], acc[3 * cells + k], gs), f, v, den);
        if (cnt[k] > 0 && v == 0.0) ++vanished;
        out[k] = v;
        if (solid_angle) solid_angle[k] = den;
    }
    return vanished;
}

// ---- the filled image: adaptive.fill_sky_values (adaptive-sample.jl:196-250), one column ϕ at a time ----

// the scan operator that carries the last non-zero cell along a column
GR_SKY_DEV int64_t last_nonzero(int64_t a, int64_t b) { return b != 0 ? b : a; }
// is point j the first of its cell's run -- a cell, and not the one the last non-zero point before it holds?
GR_SKY_DEV bool first_of_run(int64_t cell, int64_t previous_nonzero) { return cell != 0 && cell != previous_nonzero; }

// The order gr_sky_fill walks a θ grid in: ascending, NaN last, equal values in the caller's order -- a column then meets its cells
// in ascending θ whatever order the caller's grid has.  perm[k]: the caller's index of the k-th point.  Host only.
inline void theta_order(const double* theta, int64_t n, int64_t* perm)
{
    for (int64_t j = 0; j < n; ++j) perm[j] = j;
    std::stable_sort(perm, perm + n, [&](int64_t a, int64_t b) {
        const double x = theta[a], y = theta[b];
        return (x == x) && (!(y == y) || x < y);
    });
}

// point θ of a column of m >= 2 cells (`cells`, their θ ascending in `column`): the interval of np.searchsorted(column, θ,
// side = "right") clipped to [1, m - 1], the two cells, and the six fields (1 - w) v1 + w v2 as numpy rounds them
GR_SKY_DEV void fill_point(const double* column, const int64_t* cells, int64_t m, const double* rows, double theta, double* out,
                           int64_t& lower, int64_t& upper)
{
    GR_SKY_NO_CONTRACT
    int64_t k = count_le(column, m, theta);
    k = (k < 1 ? 1 : (k > m - 1 ? m - 1 : k)) - 1;
    lower = cells[k];
    upper = cells[k + 1];
    const double num = theta - column[k], den = column[k + 1] - column[k];
    const double w = num / den, u = 1.0 - w;
    const double *v1 = rows + 6 * lower, *v2 = rows + 6 * upper;
    for (int q = 0; q < 6; ++q) {
        const double a = u * v1[q], b = w * v2[q];
        out[q] = a + b;
    }
}

}  // namespace gr_skygrid
