"""Adaptive tracing of a source's sky (src/image-planes/adaptive-sky.jl, src/corona/adaptive-sample.jl): `AdaptiveSky`,
`trace_initial`, `trace_step`, `unpack_sky`, `fill_sky_values` and the (r, ϕ) illumination maps `bin_emissivity_grid`,
`bin_redshift_grid`, `bin_time_grid`.

A sky is an `AdaptiveGrid` over (cos θ, ϕ) of the source's local sky with one `CoronaGridValues` row per cell -- t, r, ϕ,
g, J = |∂(r, ϕ_disc)/∂(θ, ϕ_sky)| / sin θ and the status as a float -- in a structured array (`SKY_DTYPE`): `sky.values[i]` is
cell i's row, cells count from 1 as in the reference, and row 0 is a null row.  Every refinement step traces ALL its new
cells in one call of `calc_values(cos θ[], ϕ[])`: for a corona that is one launch of the tangent kernels (`gr_sky_cells`),
dual numbers in the sky angles through the integrator.  The middle child of a refined cell sits where its parent does and
inherits the parent's row.

`check_refine(sky, i1, i2)` receives index ARRAYS and returns a bool array, so the reference's criteria read the same
with `np.isnan(sky.values["r"][i1])`.
"""
from __future__ import annotations

import math

import numpy as np

from .grids import AdaptiveGrid

SKY_FIELDS = ("t", "r", "ϕ", "g", "J", "status")
SKY_DTYPE = np.dtype([(f, np.float64) for f in SKY_FIELDS])
TWO_PI = 2.0 * math.pi


def make_null(n=1):
    """make_null(CoronaGridValues): n rows of NaN"""
    out = np.empty(n, dtype=SKY_DTYPE)
    for f in SKY_FIELDS:
        out[f] = np.nan
    return out


def _isapprox(a, b, rtol):
    """Base.isapprox(a, b; rtol) with atol = 0 on arrays: false wherever either is NaN"""
    with np.errstate(invalid="ignore"):
        return (a == b) | (np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b)))


def check_refine(sky, i1, i2, percentage=2):
    """The default criterion (adaptive-sample.jl:123-140): g or J differ by more than `percentage` per cent between the two
    cells; a pair of cells that both miss the disc is left alone."""
    v1, v2 = sky.values[np.asarray(i1)], sky.values[np.asarray(i2)]
    both_miss = np.isnan(v1["r"]) & np.isnan(v2["r"])
    g_too_coarse = ~_isapprox(v1["g"], v2["g"], percentage / 100)
    J_too_coarse = ~_isapprox(v1["J"], v2["J"], percentage / 100)
    return ~both_miss & (g_too_coarse | J_too_coarse)


def refine_function(f):
    """refine_function(f) (adaptive-sample.jl:682-691): `f(values)` is given the rows of an index array's cells and returns a
    bool array; a pair is refined where f holds for either cell, unless both miss."""

    def _refine(sky, i1, i2):
        v1, v2 = sky.values[np.asarray(i1)], sky.values[np.asarray(i2)]
        both_miss = np.isnan(v1["r"]) & np.isnan(v2["r"])
        return ~both_miss & (np.asarray(f(v1), dtype=bool) | np.asarray(f(v2), dtype=bool))

    return _refine


def fine_refine_function(f, **kwargs):
    """fine_refine_function(f; kwargs...) (adaptive-sample.jl:700-710): the default criterion AND f on either cell"""

    def _refine(sky, i1, i2):
        v1, v2 = sky.values[np.asarray(i1)], sky.values[np.asarray(i2)]
        return check_refine(sky, i1, i2, **kwargs) & (np.asarray(f(v1), dtype=bool) | np.asarray(f(v2), dtype=bool))

    return _refine


def refine_to_level(n):
    """refine_to_level(n) (adaptive-sample.jl:712-719): refine the second cell of a pair while its level is below n"""

    def refiner(sky, i1, i2):
        i1, i2 = np.asarray(i1), np.asarray(i2)
        both_miss = np.isnan(sky.values["r"][i1]) & np.isnan(sky.values["r"][i2])
        return ~both_miss & (sky.grid.level[i2] < n)

    return refiner


class AdaptiveSky:
    """AdaptiveSky(calc_values, check_refine; pole_offset = 1e-6) -- the generic form, adaptive-sky.jl:26-46: `calc_values(cos θ[],
    ϕ[])` returns a structured array of SKY_DTYPE -- or AdaptiveSky(m, corona, d; ensemble, t_max, solver_opts...)
    (adaptive-sample.jl:156-178), whose `calc_values` is one `gr_sky_cells` launch per call."""

    def __init__(self, *args, check_refine=None, pole_offset=1e-6, **kwargs):
        if len(args) == 3 and not callable(args[0]):
            if check_refine is not None:
                raise TypeError("AdaptiveSky(m, corona, d) brings the default criterion; pass another to trace_step")
            calc_values, self.tracer = _make_emissivity_tracer(*args, **kwargs)
            criterion = globals()["check_refine"]
        else:
            if kwargs:
                raise TypeError(f"unexpected keyword arguments {sorted(kwargs)}")
            if len(args) == 2 and check_refine is None:
                calc_values, criterion = args
            elif len(args) == 1:
                calc_values, criterion = args[0], (globals()["check_refine"] if check_refine is None else check_refine)
            else:
                raise TypeError("AdaptiveSky(calc_values, check_refine) or AdaptiveSky(m, corona, d)")
            self.tracer = None
        self.grid = AdaptiveGrid(math.cos(pole_offset), math.cos(math.pi - pole_offset), -math.pi, math.pi)
        self.calculate_value = calc_values
        self.check_refine = criterion
        self._values = make_null(1)
        self.n_values = 0

    def __repr__(self):
        return f"AdaptiveSky[N={self.n_values}]"

    @property
    def values(self):
        """the cells' rows, a view: row i for cell i -- cells count from 1, row 0 is a null row (NaN)"""
        return self._values[:self.n_values + 1]

    def _append(self, rows):
        need = self.n_values + rows.size
        if need + 1 > self._values.size:
            grown = np.empty(max(need + 1, 2 * self._values.size, 1024), dtype=SKY_DTYPE)
            grown[:self.n_values + 1] = self._values[:self.n_values + 1]
            self._values = grown
        self._values[self.n_values + 1:need + 1] = rows
        self.n_values = need

    def _trace(self, cells):
        """the rows of the cells `cells` (indices from 1), all in one call of calc_values"""
        cells = np.asarray(cells, dtype=np.int64)
        pos = self.grid.pos[cells]
        rows = np.asarray(self.calculate_value(np.ascontiguousarray(pos[:, 0]), np.ascontiguousarray(pos[:, 1])))
        if rows.dtype != SKY_DTYPE or rows.shape != (cells.size,):
            raise ValueError("calc_values must return one SKY_DTYPE row per cell")
        return rows


def trace_initial(sky, level=3):
    """trace_initial!(sky; level = 3) (adaptive-sky.jl:106-122): the nine top cells, then every cell refined `level - 1` times;
    one call of calc_values per level."""
    if sky.n_values != 0:
        raise ValueError("the sky has been traced already")
    sky._append(sky._trace(np.arange(1, len(sky.grid) + 1)))
    for _ in range(1, level):
        refine_and_trace(sky, sky.grid.leaves())
    return sky


def find_need_refine(sky, check_refine=None):
    """find_need_refine(sky, check_refine) (adaptive-sky.jl:130-152): the sorted cells that `check_refine(sky, leaf, bordering
    leaf)` names -- it is the BORDERING cell of a pair that is refined."""
    check_refine = sky.check_refine if check_refine is None else check_refine
    i1, i2 = sky.grid.bordering_pairs()
    if i1.size == 0:
        return np.empty(0, dtype=np.int64)
    need = np.asarray(check_refine(sky, i1, i2), dtype=bool)
    return np.unique(i2[need])


def refine_and_trace(sky, cell_ids):
    """refine_and_trace!(sky, cell_ids) (adaptive-sky.jl:166-196): refine the cells, give every middle child its parent's row
    and trace all the other children in one call."""
    cell_ids = np.asarray(cell_ids, dtype=np.int64).reshape(-1)
    if cell_ids.size == 0:
        return sky
    kids = sky.grid.refine_many(cell_ids)
    rows = make_null(kids.size).reshape(kids.shape)
    rows[:, 4] = sky.values[cell_ids]
    outer = np.ones(9, dtype=bool)
    outer[4] = False
    rows[:, outer] = sky._trace(kids[:, outer].reshape(-1)).reshape(-1, 8)
    sky._append(rows.reshape(-1))
    return sky


def trace_step(sky, check_refine=None):
    """trace_step!(sky; check_refine = sky.check_refine) (adaptive-sky.jl:210-213)"""
    return refine_and_trace(sky, find_need_refine(sky, check_refine))


def unpack_sky(sky):
    """unpack_sky(sky) (adaptive-sky.jl:295-309): (ϕ, cos θ, rows) of the leaves"""
    leaves = sky.grid.leaves()
    pos = sky.grid.pos[leaves]
    return pos[:, 1].copy(), pos[:, 0].copy(), sky.values[leaves].copy()


def fill_sky_values(sky, grid):
    """fill_sky_values(sky, N) -> (ϕ grid, θ grid, rows[θ, ϕ]); fill_sky_values(sky, (ϕ grid, θ grid)) -> rows[θ, ϕ]
    (adaptive-sample.jl:196-250): per column of ϕ, the cells that hold the grid's points, sorted by θ and linearly interpolated.
    All six fields are averaged: the reference's _to_vector packs five of the six into a six-vector and so drops the status
    (adaptive-sample.jl:28); a column with fewer than two cells (the reference indexes out of bounds there) is NaN."""
    if np.isscalar(grid):
        ϕ_grid = np.linspace(-math.pi, math.pi, int(grid))
        θ_grid = np.linspace(0.0, math.pi, int(grid))
        return ϕ_grid, θ_grid, fill_sky_values(sky, (ϕ_grid, θ_grid))
    ϕ_grid, θ_grid = (np.asarray(a, dtype=np.float64) for a in grid)
    out = make_null(θ_grid.size * ϕ_grid.size).reshape(θ_grid.size, ϕ_grid.size)
    cosθ = np.cos(θ_grid)
    for k, ph in enumerate(ϕ_grid):
        cells = {sky.grid.get_parent_index(c, ph) for c in cosθ}
        cells.discard(0)
        if len(cells) < 2:
            continue
        cells = np.fromiter(cells, dtype=np.int64)
        column = np.arccos(sky.grid.pos[cells, 0])
        order = np.argsort(column, kind="stable")
        column, vals = column[order], sky.values[cells[order]]
        idx = np.clip(np.searchsorted(column, θ_grid, side="right"), 1, column.size - 1) - 1
        w = (θ_grid - column[idx]) / (column[idx + 1] - column[idx])
        for f in SKY_FIELDS:
            out[f][:, k] = (1.0 - w) * vals[f][idx] + w * vals[f][idx + 1]
    return out


def _binned_cells(sky, r_bins, ϕ_bins):
    """the leaves that land in a bin: (rows, ΔΩ, r index, ϕ index) -- adaptive-sample.jl:337-348"""
    r_bins, ϕ_bins = np.asarray(r_bins, dtype=np.float64), np.asarray(ϕ_bins, dtype=np.float64)
    leaves = sky.grid.leaves()
    v = sky.values[leaves]
    with np.errstate(invalid="ignore"):
        keep = ~np.isnan(v["r"]) & ~(v["r"] > np.max(r_bins))
    leaves, v = leaves[keep], v[keep]
    θ = np.arccos(sky.grid.pos[leaves, 0])
    wx, wy = sky.grid.get_cell_width(leaves)
    ΔΩ = wx * wy / np.sin(θ)
    # searchsortedlast: the last edge <= the value, counted from 1; 0 = below the first edge, dropped
    r_i = np.searchsorted(r_bins, v["r"], side="right")
    ϕ_i = np.searchsorted(ϕ_bins, np.mod(v["ϕ"], TWO_PI), side="right")
    ok = (r_i != 0) & (ϕ_i != 0)
    return v[ok], ΔΩ[ok], r_i[ok] - 1, ϕ_i[ok] - 1


def _bin_grid(sky, r_bins, ϕ_bins, weight):
    v, ΔΩ, r_i, ϕ_i = _binned_cells(sky, r_bins, ϕ_bins)
    output = np.zeros((len(r_bins), len(ϕ_bins)))
    solid_angle = np.zeros_like(output)
    np.add.at(output, (r_i, ϕ_i), ΔΩ * weight(v))
    np.add.at(solid_angle, (r_i, ϕ_i), ΔΩ)
    lit = solid_angle > 0
    output[lit] /= solid_angle[lit]
    return output


def bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky, Γ=2, ensemble=None):
    """bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky; Γ = 2) (adaptive-sample.jl:266-362): per (r, ϕ) bin the solid-angle
    weighted mean of J g^Γ γ(r) A(r) over the leaves that land in it; Γ = None leaves the redshift out."""
    from .corona import _plunging_table, _proper_area, keplerian_velocity_projector, lorentz_factor

    tracer = getattr(sky, "tracer", None)
    if tracer is not None and ensemble is None:
        ensemble = tracer["ensemble"]
    plunging = None
    disc_velocity = [None]

    def area(r):
        if disc_velocity[0] is None:
            table = plunging
            if np.any(r < m.isco()):
                from .tracing import EnsembleMI355X

                table = _plunging_table(m, EnsembleMI355X() if ensemble is None else ensemble)
            disc_velocity[0] = keplerian_velocity_projector(m, plunging=table, ensemble=ensemble)
        x = np.zeros((r.size, 4))
        x[:, 1], x[:, 2] = r, math.pi / 2
        return lorentz_factor(m, x, disc_velocity[0](x)) * _proper_area(m, r, np.full(r.size, math.pi / 2))

    def weight(v):
        if v.size == 0:
            return np.zeros(0)
        redshift = np.ones(v.size) if Γ is None else v["g"] ** Γ
        return v["J"] * (redshift * area(v["r"]))

    return _bin_grid(sky, r_bins, ϕ_bins, weight)


def bin_redshift_grid(r_bins, ϕ_bins, sky):
    """bin_redshift_grid(r_bins, ϕ_bins, sky) (adaptive-sample.jl:364-406): the solid-angle weighted mean of g per bin"""
    return _bin_grid(sky, r_bins, ϕ_bins, lambda v: v["g"])


def bin_time_grid(r_bins, ϕ_bins, sky):
    """bin_time_grid(r_bins, ϕ_bins, sky) (adaptive-sample.jl:408-450): the solid-angle weighted mean of t per bin"""
    return _bin_grid(sky, r_bins, ϕ_bins, lambda v: v["t"])


def interpolate_emissivity_grid(output, r_bins, ϕ_bins):
    """interpolate_emissivity_grid!(output, r_bins, ϕ_bins) (adaptive-sample.jl:458-484), in place: per radius, the empty ϕ bins
    are filled by linear interpolation over the bins that are lit (extrapolating from the end intervals)."""
    from .corona import _nan_linear_interp

    ϕ_bins = np.asarray(ϕ_bins, dtype=np.float64)
    if output.shape != (len(r_bins), ϕ_bins.size):
        raise ValueError("output must be (len(r_bins), len(ϕ_bins))")
    for i in range(output.shape[0]):
        lit = output[i] != 0
        if np.count_nonzero(lit) < 2:
            continue
        output[i] = np.abs(_nan_linear_interp(ϕ_bins[lit], output[i][lit], ϕ_bins, default=np.nan))
    return output


def _make_emissivity_tracer(m, corona, d, *, ensemble=None, t_max=1_000_000.0, **solver_opts):
    """_make_emissivity_tracer (adaptive-sample.jl:83-121): the source from sample_position_velocity, the upper-hemisphere
    callback, chart_for_metric(m, 2 t_max), the Keplerian / plunging disc velocity as device_radial_profile sets it up.
    Returns (calc_values, what it keeps alive)."""
    import ctypes as C

    from . import _lib
    from .corona import _cart_to_spher_jacobian, _plunging_table, tetradframe_matrix
    from .pointfunctions import GR_PF_REDSHIFT, PointFunction
    from .rendering import abi_pointfunction
    from .tracing import chart_for_metric, domain_upper_hemisphere, tracing_configuration

    x_src, v_src = corona.sample_position_velocity(m)
    x_src, v_src = np.array(x_src, dtype=np.float64), np.asarray(v_src, dtype=np.float64)
    B = np.eye(4)
    B[1:, 1:] = _cart_to_spher_jacobian(x_src[2], x_src[3])
    Mx = np.ascontiguousarray(tetradframe_matrix(m, x_src, v_src) @ B)
    solver_opts.setdefault("chart", chart_for_metric(m, 2 * t_max))
    solver_opts.setdefault("callback", domain_upper_hemisphere())
    config = tracing_configuration(m, x_src, np.zeros((1, 4)), d, (0.0, t_max), ensemble=ensemble, **solver_opts)
    ens = config.ensemble
    plunging = _plunging_table(m, ens)
    rpf = PointFunction(None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": m.isco(), "plunge": plunging})
    pf, keep_pf = abi_pointfunction(rpf)
    pf.has_u_src = 1
    for q in range(4):
        pf.u_src[q] = v_src[q]
    cfg = config.abi_config()
    L = _lib.load()
    keep = {"config": config, "cfg": cfg, "pf": pf, "keep_pf": keep_pf, "ensemble": ens, "x_src": x_src, "v_src": v_src,
            "Mx": Mx, "launches": []}

    def calc_values(cosθ, ϕ):
        cosθ = np.ascontiguousarray(cosθ, dtype=np.float64)
        ϕ = np.ascontiguousarray(ϕ, dtype=np.float64)
        cells = _lib.gr_skycells()
        for q in range(4):
            cells.x_src[q] = x_src[q]
        for q, val in enumerate(Mx.ravel()):
            cells.Mx[q] = val
        cells.cos_theta, cells.phi, cells.n = cosθ.ctypes.data, ϕ.ctypes.data, cosθ.size
        out = np.empty(cosθ.size, dtype=SKY_DTYPE)
        if ens.multi:
            ctx_arr, ctx_stats = _lib.ctx_array(ens.contexts)
            _lib.check(L.gr_sky_cells_multi(ctx_arr, len(ens.contexts), C.byref(cfg), C.byref(cells), C.byref(pf), out.ctypes.data, ctx_stats))
            st = _lib.merge_stats(ctx_stats)
        else:
            st = _lib.gr_stats()
            _lib.check(L.gr_sky_cells(ens.ctx.handle, C.byref(cfg), C.byref(cells), C.byref(pf), out.ctypes.data, C.byref(st)))
        keep["launches"].append((int(cosθ.size), float(st.call_ms)))
        return out

    return calc_values, keep
