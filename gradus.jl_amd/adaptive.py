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

`AdaptiveSky(m, corona, d, resident=True)` keeps the tree and the rows on the device (`gr_sky_*`): the pair search, the
refinement and the census of the (r, ϕ) bins run there, `sky.grid` and `sky.values` are host mirrors brought up to date on
first read after a change.  The criteria of this module carry a `gr_sky_criterion` where they can be written as one (the
default criterion, `refine_to_level`, `refine_function` / `fine_refine_function` over `RadialBox`es); any other callable is
evaluated on the mirror against the pair list the device returns.  The maps and `fill_sky_values` read the mirror unless asked
for `route="device"`, which forms them from the device's rows (`gr_sky_bin_grid`, `gr_sky_fill`) without a download.

`AdaptivePlane(m, x, d)` (src/image-planes/adaptive-plane.jl) is the same tree laid over an observer's image plane (α, β): its rows
are GeodesicPoints (`POINT_DTYPE`), its criterion `check_refine_plane` (hit against miss, or end points on the disc too far
apart), every step's new cells one `gr_plane_cells` launch, `resident=True` as above (`gr_sky_create_plane`), and
`fill_sky_values` interpolates one value per cell first across α, then along β (`gr_sky_fill_plane` for `route="device"`).  The
maps and the drivers below read a corona's rows and refuse a plane.

The drivers of adaptive-sample.jl:486-842 -- `empty_fraction`, `evaluate_refinement_metric`, `step_block`,
`adaptive_solve` -- work on both kinds of sky.
"""
from __future__ import annotations

import enum
import math
import sys
import time

import numpy as np

from .grids import AdaptiveGrid

SKY_FIELDS = ("t", "r", "ϕ", "g", "J", "status")
SKY_DTYPE = np.dtype([(f, np.float64) for f in SKY_FIELDS])
TWO_PI = 2.0 * math.pi


def make_null(n=1, dtype=SKY_DTYPE):
    """make_null(CoronaGridValues): n rows of NaN -- or, for another row type, n rows with NaN in every float field, 0 in every
    integer field and, for a GeodesicPoint (POINT_DTYPE), the status NoStatus"""
    out = np.zeros(n, dtype=dtype)
    for f in out.dtype.names:
        if out.dtype[f].base.kind == "f":
            out[f] = np.nan
    if "status" in out.dtype.names and out.dtype["status"].kind == "i":
        out["status"] = _NO_STATUS
    return out


_HIT, _NO_STATUS = 2, 3          # StatusCodes.IntersectedWithGeometry, StatusCodes.NoStatus


def _is_plane(sky):
    return bool(getattr(sky, "is_plane", False))


def _both_miss(sky, i1, i2):
    """a pair of cells whose rays both miss the geometry: NaN r on a corona sky, a status other than IntersectedWithGeometry on a
    plane"""
    if _is_plane(sky):
        status = sky.values["status"]
        return (status[i1] != _HIT) & (status[i2] != _HIT)
    r = sky.values["r"]
    return np.isnan(r[i1]) & np.isnan(r[i2])


def _corona_only(sky, name):
    if _is_plane(sky):
        raise TypeError(f"{name} reads the (t, r, ϕ, g, J) rows of a corona's sky: an AdaptivePlane holds GeodesicPoints")


def _isapprox(a, b, rtol):
    """Base.isapprox(a, b; rtol) with atol = 0 on arrays: false wherever either is NaN"""
    with np.errstate(invalid="ignore"):
        return (a == b) | (np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b)))


class RadialBox:
    """RadialBox(r_min, r_max, ϕ=None, open=True, ϕ_open=False): a region of the disc as a predicate over rows, the `f` of
    `refine_function` / `fine_refine_function` -- r in an interval and, if ϕ is given, mod(ϕ, 2π) in one interval `(lo, hi)` or
    in either of two `((lo, hi), (lo, hi))` (a block that wraps around ϕ = 0).  `open` / `ϕ_open`: a bool or a pair (lower,
    upper) -- is the bound itself outside?  `v.r > 800` is RadialBox(800, inf, open=(True, False)); the block test of
    step_block! (`_is_in`) is closed.  A NaN r lies in no box."""

    def __init__(self, r_min, r_max, ϕ=None, open=True, ϕ_open=False):
        self.r = (float(r_min), float(r_max))
        self.open = (bool(open),) * 2 if isinstance(open, (bool, np.bool_)) else tuple(bool(o) for o in open)
        self.ϕ_open = (bool(ϕ_open),) * 2 if isinstance(ϕ_open, (bool, np.bool_)) else tuple(bool(o) for o in ϕ_open)
        if ϕ is None:
            self.ϕ = ()
        elif np.ndim(ϕ) == 1:
            self.ϕ = ((float(ϕ[0]), float(ϕ[1])),)
        else:
            self.ϕ = tuple((float(lo), float(hi)) for lo, hi in ϕ)
        if len(self.open) != 2 or len(self.ϕ_open) != 2 or len(self.ϕ) > 2:
            raise ValueError("RadialBox: open / ϕ_open are a bool or a pair, ϕ is one or two intervals")

    def __repr__(self):
        return f"RadialBox(r={self.r}, ϕ={self.ϕ}, open={self.open}, ϕ_open={self.ϕ_open})"

    @staticmethod
    def _inside(x, lo, hi, open_):
        return (x > lo if open_[0] else x >= lo) & (x < hi if open_[1] else x <= hi)

    def __call__(self, v):
        with np.errstate(invalid="ignore"):
            inside = self._inside(v["r"], self.r[0], self.r[1], self.open)
            if self.ϕ:
                folded = np.mod(v["ϕ"], TWO_PI)
                in_ϕ = np.zeros(np.shape(folded), dtype=bool)
                for lo, hi in self.ϕ:
                    in_ϕ |= self._inside(folded, lo, hi, self.ϕ_open)
                inside = inside & in_ϕ
        return inside


def _boxes_of(f):
    """the RadialBoxes `f` stands for (one, or a list of up to 8), or None for any other callable"""
    if isinstance(f, RadialBox):
        return [f]
    if isinstance(f, (list, tuple)) and f and all(isinstance(b, RadialBox) for b in f):
        return list(f)
    return None


def _any_box(boxes):
    def f(v):
        out = np.zeros(np.shape(v["r"]), dtype=bool)
        for b in boxes:
            out |= b(v)
        return out

    return f


def _criterion(kind, percentage=2, level=0, boxes=()):
    """what a resident sky marshals into a gr_sky_criterion; None if the boxes do not fit"""
    if len(boxes) > 8:
        return None
    return {"kind": kind, "rtol": percentage / 100, "level": int(level), "boxes": list(boxes)}


def check_refine(sky, i1, i2, percentage=2):
    """The default criterion (adaptive-sample.jl:123-140): g or J differ by more than `percentage` per cent between the two
    cells; a pair of cells that both miss the disc is left alone."""
    v1, v2 = sky.values[np.asarray(i1)], sky.values[np.asarray(i2)]
    both_miss = np.isnan(v1["r"]) & np.isnan(v2["r"])
    g_too_coarse = ~_isapprox(v1["g"], v2["g"], percentage / 100)
    J_too_coarse = ~_isapprox(v1["J"], v2["J"], percentage / 100)
    return ~both_miss & (g_too_coarse | J_too_coarse)


check_refine.gr_criterion = _criterion(0)


def refine_function(f):
    """refine_function(f) (adaptive-sample.jl:682-691): `f(values)` is given the rows of an index array's cells and returns a
    bool array; a pair is refined where f holds for either cell, unless both miss.  `f` may be a RadialBox or a list of them."""
    boxes = _boxes_of(f)
    if boxes is not None:
        f = _any_box(boxes)

    def _refine(sky, i1, i2):
        v1, v2 = sky.values[np.asarray(i1)], sky.values[np.asarray(i2)]
        both_miss = np.isnan(v1["r"]) & np.isnan(v2["r"])
        return ~both_miss & (np.asarray(f(v1), dtype=bool) | np.asarray(f(v2), dtype=bool))

    if boxes is not None:
        _refine.gr_criterion = _criterion(1, boxes=boxes)
    return _refine


def fine_refine_function(f, **kwargs):
    """fine_refine_function(f; kwargs...) (adaptive-sample.jl:700-710): the default criterion AND f on either cell.  `f` may be
    a RadialBox or a list of them."""
    boxes = _boxes_of(f)
    if boxes is not None:
        f = _any_box(boxes)

    def _refine(sky, i1, i2):
        v1, v2 = sky.values[np.asarray(i1)], sky.values[np.asarray(i2)]
        return check_refine(sky, i1, i2, **kwargs) & (np.asarray(f(v1), dtype=bool) | np.asarray(f(v2), dtype=bool))

    if boxes is not None and set(kwargs) <= {"percentage"}:
        _refine.gr_criterion = _criterion(2, boxes=boxes, **kwargs)
    return _refine


def refine_to_level(n):
    """refine_to_level(n) (adaptive-sample.jl:712-719): refine the second cell of a pair while its level is below n"""

    def refiner(sky, i1, i2):
        i1, i2 = np.asarray(i1), np.asarray(i2)
        return ~_both_miss(sky, i1, i2) & (sky.grid.level[i2] < n)

    refiner.gr_criterion = _criterion(3, level=n)
    return refiner


def check_refine_plane(sky, i1, i2, percentage=20):
    """The criterion of an AdaptivePlane (adaptive-plane.jl:24-50) over index arrays: a pair whose rays both miss the geometry is
    left alone, a pair of which one hits is refined, a pair that both hit is refined where log10 of the coordinate radius x[1] or
    θ = x[2] mod 2π differ by more than `percentage` per cent.  (The reference also computes a ϕ term and never uses it.)"""
    v1, v2 = sky.values[np.asarray(i1)], sky.values[np.asarray(i2)]
    hit1, hit2 = v1["status"] == _HIT, v2["status"] == _HIT
    x1, x2 = v1["x"], v2["x"]
    with np.errstate(invalid="ignore", divide="ignore"):
        r_too_coarse = ~_isapprox(np.log10(x1[..., 1]), np.log10(x2[..., 1]), percentage / 100)
        θ_too_coarse = ~_isapprox(np.mod(x1[..., 2], TWO_PI), np.mod(x2[..., 2], TWO_PI), percentage / 100)
    return (hit1 | hit2) & (~(hit1 & hit2) | r_too_coarse | θ_too_coarse)


check_refine_plane.gr_criterion = _criterion(4, percentage=20)


def refine_plane(percentage=20):
    """check_refine_plane at another percentage, as a criterion a resident plane evaluates on the device"""

    def _refine(sky, i1, i2):
        return check_refine_plane(sky, i1, i2, percentage=percentage)

    _refine.gr_criterion = _criterion(4, percentage=percentage)
    return _refine


def gr_criterion_of(check_refine):
    """the gr_sky_criterion a criterion of this module carries (what a resident sky hands to the device), or None for a plain
    callable"""
    from . import _lib

    spec = getattr(check_refine, "gr_criterion", None)
    if spec is None:
        return None
    cr = _lib.gr_sky_criterion()
    cr.kind, cr.level, cr.rtol, cr.n_boxes = spec["kind"], spec["level"], spec["rtol"], len(spec["boxes"])
    for k, box in enumerate(spec["boxes"]):
        b = cr.boxes[k]
        b.r_lo, b.r_hi = box.r
        b.r_open_lo, b.r_open_hi = (int(o) for o in box.open)
        b.phi_open_lo, b.phi_open_hi = (int(o) for o in box.ϕ_open)
        b.n_phi = len(box.ϕ)
        for q, (lo, hi) in enumerate(box.ϕ):
            b.phi_lo[q], b.phi_hi[q] = lo, hi
    return cr


class AdaptiveSky:
    """AdaptiveSky(calc_values, check_refine; pole_offset = 1e-6) -- the generic form, adaptive-sky.jl:26-46: `calc_values(cos θ[],
    ϕ[])` returns a structured array of SKY_DTYPE -- or AdaptiveSky(m, corona, d; ensemble, t_max, solver_opts...)
    (adaptive-sample.jl:156-178), whose `calc_values` is one `gr_sky_cells` launch per call.  With `resident=True` the tree and
    the rows of the latter live on the device (one context), and `grid` / `values` are mirrors of them.
    The generic form takes `limits=(x1, x2, y1, y2)`, `x_periodic=` and `null=` (one null row of another structured dtype: the
    row type of `calc_values`) for a grid over something else than a source's sky -- AdaptivePlane builds on it."""

    def __init__(self, *args, check_refine=None, pole_offset=1e-6, limits=None, x_periodic=True, null=None, **kwargs):
        self._dev = None
        self._null = make_null(1) if null is None else np.array(null).reshape(1)
        self._dtype = self._null.dtype
        resident = bool(kwargs.pop("resident", False))
        if len(args) == 3 and not callable(args[0]) and (limits is not None or null is not None):
            raise TypeError("limits / null belong to the generic form AdaptiveSky(calc_values, check_refine)")
        if len(args) == 3 and not callable(args[0]):
            if check_refine is not None:
                raise TypeError("AdaptiveSky(m, corona, d) brings the default criterion; pass another to trace_step")
            ensemble = kwargs.get("ensemble")
            if resident and ensemble is not None and ensemble.multi:
                raise ValueError("AdaptiveSky(resident=True) keeps the sky on ONE context: pass an ensemble of one device, "
                                 "or resident=False to share every step's cells among the contexts")
            calc_values, self.tracer = _make_emissivity_tracer(*args, **kwargs)
            criterion = globals()["check_refine"]
        elif resident:
            raise TypeError("resident=True needs AdaptiveSky(m, corona, d): the device traces the cells")
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
        if limits is None:
            self._grid = AdaptiveGrid(math.cos(pole_offset), math.cos(math.pi - pole_offset), -math.pi, math.pi)
        else:
            self._grid = AdaptiveGrid(*limits, x_periodic=x_periodic)
        self.calculate_value = calc_values
        self.check_refine = criterion
        self._values = self._null.copy()
        self._n_values = 0
        if resident:
            self._make_resident()

    def __repr__(self):
        return f"AdaptiveSky[N={self.n_values}]"

    @property
    def resident(self):
        return self._dev is not None

    @property
    def is_plane(self):
        """are the rows GeodesicPoints (an AdaptivePlane) rather than a corona's (t, r, ϕ, g, J, status)?"""
        from ._lib import POINT_DTYPE

        return self._dtype == POINT_DTYPE

    def make_null(self, n=1):
        """n null rows of this sky's row type"""
        return np.repeat(self._null, n)

    @property
    def n_cells(self):
        """the number of cells (on a resident sky: asked of the device, the mirrors stay as they are)"""
        return self._device_size() if self._dev is not None else self._grid.n

    @property
    def grid(self):
        self._sync()
        return self._grid

    @grid.setter
    def grid(self, value):
        self._grid = value

    @property
    def n_values(self):
        self._sync()
        return self._n_values

    @n_values.setter
    def n_values(self, value):
        self._n_values = value

    @property
    def values(self):
        """the cells' rows, a view: row i for cell i -- cells count from 1, row 0 is a null row (NaN)"""
        self._sync()
        return self._values[:self._n_values + 1]

    # ---- the resident sky: the tree and the rows on the device, grid / values as mirrors ----
    def _make_resident(self):
        import ctypes as C

        from . import _lib

        tr = self.tracer
        if tr["ensemble"].multi:
            raise ValueError("AdaptiveSky(resident=True) keeps the sky on ONE context")
        if self.is_plane:
            (x1, x2), (y1, y2) = self._grid.limits
            limits = (C.c_double * 4)(x1, x2, y1, y2)
            handle = C.c_void_p()
            self._L = _lib.load()
            _lib.check(self._L.gr_sky_create_plane(tr["ensemble"].ctx.handle, C.byref(tr["cfg"]), C.byref(tr["plane"]), limits,
                                                   int(self._grid.x_periodic), C.byref(handle)))
            self._dev = handle
            self._stale = False
            return
        source = _lib.gr_skycells()
        for q in range(4):
            source.x_src[q] = tr["x_src"][q]
        for q, val in enumerate(tr["Mx"].ravel()):
            source.Mx[q] = val
        (x1, x2), (y1, y2) = self._grid.limits
        limits = (C.c_double * 4)(x1, x2, y1, y2)
        handle = C.c_void_p()
        self._L = _lib.load()
        _lib.check(self._L.gr_sky_create(tr["ensemble"].ctx.handle, C.byref(tr["cfg"]), C.byref(source), C.byref(tr["pf"]), limits,
                                         int(self._grid.x_periodic), C.byref(handle)))
        self._dev = handle
        self._stale = False

    def __del__(self):
        try:
            if getattr(self, "_dev", None):
                self._L.gr_sky_destroy(self._dev)
                self._dev = None
        except Exception:
            pass

    def _device_size(self):
        import ctypes as C

        from . import _lib

        n = C.c_int64(0)
        _lib.check(self._L.gr_sky_size(self._dev, C.byref(n)))
        return int(n.value)

    def _sync(self):
        """bring the mirrors up to date: the cells made since the last read, and the `children` rows of their parents"""
        if self._dev is None or not self._stale:
            return
        import ctypes as C

        from . import _lib

        self._stale = False
        g, n = self._grid, self._device_size()
        first = 0 if self._n_values == 0 else self._n_values + 1
        count = n + 1 - first
        if count <= 0:
            return
        g._reserve(n - g.n)
        if n + 1 > self._values.size:
            grown = np.empty(max(n + 1, 2 * self._values.size, 1024), dtype=self._dtype)
            grown[:self._n_values + 1] = self._values[:self._n_values + 1]
            self._values = grown
        groups = count // 9 if first >= 10 else 0
        refined = np.empty(groups, dtype=np.int64)
        kids = np.empty((groups, 9), dtype=np.int64)
        ptr = lambda a: C.c_void_p(a[first:].ctypes.data)
        _lib.check(self._L.gr_sky_download(self._dev, first, count, ptr(g.pos), ptr(g.level), ptr(g.children), ptr(g.neighbours), ptr(g.parent),
                                           ptr(g.location), None if self.is_plane else ptr(self._values),
                                           C.c_void_p(refined.ctypes.data) if groups else None, C.c_void_p(kids.ctypes.data) if groups else None))
        if self.is_plane:
            _lib.check(self._L.gr_sky_download_points(self._dev, first, count, ptr(self._values)))
        if groups:
            g.children[refined] = kids
        g.n = n
        self._n_values = n

    def _device_find(self, check_refine):
        """gr_sky_find_need_refine: the number of cells it names (they stay in a device list), or None if the criterion is a
        plain callable"""
        import ctypes as C

        from . import _lib

        cr = gr_criterion_of(check_refine)
        if cr is None:
            return None
        if self.is_plane != (cr.kind == _lib.GR_SKY_CRIT_PLANE) and cr.kind != _lib.GR_SKY_CRIT_LEVEL:
            raise TypeError("a plane's criteria are check_refine_plane / refine_plane and refine_to_level; check_refine, refine_function "
                            "and fine_refine_function read the rows of a corona's sky (and check_refine_plane those of a plane)")
        count = C.c_int64(0)
        _lib.check(self._L.gr_sky_find_need_refine(self._dev, C.byref(cr), C.byref(count)))
        return int(count.value)

    def _device_list(self, count):
        import ctypes as C

        from . import _lib

        cells = np.empty(count, dtype=np.int64)
        _lib.check(self._L.gr_sky_need_refine_list(self._dev, C.c_void_p(cells.ctypes.data)))
        return cells

    def _device_refine(self, cells=None):
        """gr_sky_refine_and_trace of a host list, or (None) of the device list of the last _device_find"""
        import ctypes as C

        from . import _lib

        traced, st = C.c_int64(0), _lib.gr_stats()
        if cells is None:
            rc = self._L.gr_sky_refine_and_trace(self._dev, None, 0, C.byref(traced), C.byref(st))
        else:
            cells = np.ascontiguousarray(cells, dtype=np.int64)
            rc = self._L.gr_sky_refine_and_trace(self._dev, C.c_void_p(cells.ctypes.data), cells.size, C.byref(traced), C.byref(st))
        if rc == -1:      # GR_ERR_INVALID_ARGUMENT: a cell out of range, refined already or named twice
            raise ValueError(self._L.gr_last_error().decode("utf-8", "replace"))      # (refine_many raises the same)
        _lib.check(rc)
        if traced.value:
            self._stale = True
            self.tracer["launches"].append((int(traced.value), float(st.kernel_ms)))

    def device_pairs(self):
        """gr_sky_pairs: every (leaf, bordering leaf) pair, as grid.bordering_pairs() lists them"""
        import ctypes as C

        from . import _lib

        n = C.c_int64(0)
        _lib.check(self._L.gr_sky_pairs(self._dev, None, None, 0, C.byref(n)))
        i1, i2 = np.empty(n.value, dtype=np.int64), np.empty(n.value, dtype=np.int64)
        _lib.check(self._L.gr_sky_pairs(self._dev, C.c_void_p(i1.ctypes.data), C.c_void_p(i2.ctypes.data), n.value, C.byref(n)))
        return i1, i2

    def device_occupancy(self, r_bins, ϕ_bins, Γ=2):
        """gr_sky_occupancy: per (r, ϕ) bin the leaves that land in it with J g^Γ != 0 -- where bin_emissivity_grid is non-zero"""
        import ctypes as C

        from . import _lib

        r_bins, ϕ_bins = np.ascontiguousarray(r_bins, dtype=np.float64), np.ascontiguousarray(ϕ_bins, dtype=np.float64)
        counts = np.zeros((r_bins.size, ϕ_bins.size), dtype=np.int64)
        gamma = None if Γ is None else C.byref(C.c_double(float(Γ)))
        _lib.check(self._L.gr_sky_occupancy(self._dev, C.c_void_p(r_bins.ctypes.data), r_bins.size, C.c_void_p(ϕ_bins.ctypes.data), ϕ_bins.size,
                                            gamma, C.c_void_p(counts.ctypes.data)))
        return counts

    def device_bin_grid(self, what, r_bins, ϕ_bins, Γ=2, solid_angle=False):
        """gr_sky_bin_grid: the (r, ϕ) map `what` ("emissivity", "redshift" or "time") of the resident sky, formed on the device
        from its rows: Σ ΔΩ w / Σ ΔΩ per bin in order-independent integer sums -- the same bits on every call.  With
        `solid_angle` also Σ ΔΩ.  Raises if the terms of a bin vanish below the resolution of the sums."""
        import ctypes as C

        from . import _lib

        kinds = {"emissivity": _lib.GR_SKY_MAP_EMISSIVITY, "redshift": _lib.GR_SKY_MAP_REDSHIFT, "time": _lib.GR_SKY_MAP_TIME}
        r_bins, ϕ_bins = np.ascontiguousarray(r_bins, dtype=np.float64), np.ascontiguousarray(ϕ_bins, dtype=np.float64)
        out = np.zeros((r_bins.size, ϕ_bins.size))
        ΔΩ = np.zeros_like(out) if solid_angle else None
        gamma = None if Γ is None else C.byref(C.c_double(float(Γ)))
        _lib.check(self._L.gr_sky_bin_grid(self._dev, kinds.get(what, what), C.c_void_p(r_bins.ctypes.data), r_bins.size,
                                           C.c_void_p(ϕ_bins.ctypes.data), ϕ_bins.size, gamma, C.c_void_p(out.ctypes.data),
                                           None if ΔΩ is None else C.c_void_p(ΔΩ.ctypes.data)))
        return (out, ΔΩ) if solid_angle else out

    def device_fill(self, ϕ_grid, θ_grid):
        """gr_sky_fill: (rows[θ, ϕ], lower cell[θ, ϕ], upper cell[θ, ϕ]) of fill_sky_values, one workgroup per column"""
        import ctypes as C

        from . import _lib

        ϕ_grid, θ_grid = np.ascontiguousarray(ϕ_grid, dtype=np.float64), np.ascontiguousarray(θ_grid, dtype=np.float64)
        out = np.empty((θ_grid.size, ϕ_grid.size), dtype=SKY_DTYPE)
        cells = np.empty((θ_grid.size, ϕ_grid.size, 2), dtype=np.int64)
        _lib.check(self._L.gr_sky_fill(self._dev, C.c_void_p(ϕ_grid.ctypes.data), ϕ_grid.size, C.c_void_p(θ_grid.ctypes.data), θ_grid.size,
                                       C.c_void_p(out.ctypes.data), C.c_void_p(cells.ctypes.data)))
        return out, cells[..., 0].copy(), cells[..., 1].copy()

    def _append(self, rows):
        need = self.n_values + rows.size
        if need + 1 > self._values.size:
            grown = np.empty(max(need + 1, 2 * self._values.size, 1024), dtype=self._dtype)
            grown[:self.n_values + 1] = self._values[:self.n_values + 1]
            self._values = grown
        self._values[self.n_values + 1:need + 1] = rows
        self.n_values = need

    def _trace(self, cells):
        """the rows of the cells `cells` (indices from 1), all in one call of calc_values"""
        cells = np.asarray(cells, dtype=np.int64)
        pos = self.grid.pos[cells]
        rows = np.asarray(self.calculate_value(np.ascontiguousarray(pos[:, 0]), np.ascontiguousarray(pos[:, 1])))
        if rows.dtype != self._dtype or rows.shape != (cells.size,):
            raise ValueError(f"calc_values must return one row of {'SKY_DTYPE' if self._dtype == SKY_DTYPE else self._dtype} per cell")
        return rows


def trace_initial(sky, level=3):
    """trace_initial!(sky; level = 3) (adaptive-sky.jl:106-122): the nine top cells, then every cell refined `level - 1` times;
    one call of calc_values per level."""
    if sky.n_values != 0:
        raise ValueError("the sky has been traced already")
    if sky.resident:
        import ctypes as C

        from . import _lib

        sizes = (C.c_int64 * int(level))()
        _lib.check(sky._L.gr_sky_trace_initial(sky._dev, int(level), sizes))
        sky._stale = True
        sky.tracer["launches"].extend((int(n), float("nan")) for n in sizes)
        return sky
    sky._append(sky._trace(np.arange(1, len(sky.grid) + 1)))
    for _ in range(1, level):
        refine_and_trace(sky, sky.grid.leaves())
    return sky


def find_need_refine(sky, check_refine=None):
    """find_need_refine(sky, check_refine) (adaptive-sky.jl:130-152): the sorted cells that `check_refine(sky, leaf, bordering
    leaf)` names -- it is the BORDERING cell of a pair that is refined."""
    check_refine = sky.check_refine if check_refine is None else check_refine
    if sky.resident:
        count = sky._device_find(check_refine)
        if count is not None:
            return sky._device_list(count)
        i1, i2 = sky.device_pairs()
    else:
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
    if sky.resident:
        sky._device_refine(cell_ids)
        return sky
    kids = sky.grid.refine_many(cell_ids)
    rows = sky.make_null(kids.size).reshape(kids.shape)
    rows[:, 4] = sky.values[cell_ids]
    outer = np.ones(9, dtype=bool)
    outer[4] = False
    rows[:, outer] = sky._trace(kids[:, outer].reshape(-1)).reshape(-1, 8)
    sky._append(rows.reshape(-1))
    return sky


def trace_step(sky, check_refine=None):
    """trace_step!(sky; check_refine = sky.check_refine) (adaptive-sky.jl:210-213).  On a resident sky with a criterion of this
    module the list of cells never leaves the device."""
    _refine_found(sky, _find(sky, check_refine))
    return sky


def _find(sky, check_refine=None):
    """find_need_refine as (number of cells, their indices -- or None where they stay in the resident sky's device list)"""
    if sky.resident:
        count = sky._device_find(sky.check_refine if check_refine is None else check_refine)
        if count is not None:
            return count, None
    cells = find_need_refine(sky, check_refine)
    return cells.size, cells


def _refine_found(sky, found):
    count, cells = found
    if count == 0:
        return
    if cells is None:
        sky._device_refine(None)
    else:
        refine_and_trace(sky, cells)


def unpack_sky(sky):
    """unpack_sky(sky) (adaptive-sky.jl:295-309): (ϕ, cos θ, rows) of the leaves"""
    leaves = sky.grid.leaves()
    pos = sky.grid.pos[leaves]
    return pos[:, 1].copy(), pos[:, 0].copy(), sky.values[leaves].copy()


def _device_route(sky, route):
    """route = None / "host": the numpy code on sky.grid / sky.values; "device": the kernels, on a resident sky only"""
    if route is None or route == "host":
        return False
    if route != "device":
        raise ValueError(f'route must be None, "host" or "device", not {route!r}')
    if not getattr(sky, "resident", False):
        raise ValueError('route="device" needs a resident sky: AdaptiveSky(m, corona, d, resident=True)')
    return True


def _plane_cell_values(sky, pf, metric):
    """one double per cell (row 0 included) for fill_sky_values of a plane: x[0] of every point (the reference's default pf), an
    array of the caller's, a built-in point function evaluated by the device on the mirror's points (gr_apply_pointfunction, as
    the resident route evaluates it on the device's), any other PointFunction point by point, or a callable given the points"""
    from .pointfunctions import AbstractPointFunction

    points = sky.values
    if pf is None:
        return np.ascontiguousarray(points["x"][:, 0])
    if isinstance(pf, AbstractPointFunction):
        tracer = getattr(sky, "tracer", None)
        val = np.full(points.size, np.nan)
        if pf.fusable:
            if tracer is None:
                raise TypeError("a built-in point function is evaluated on the device: this sky has no tracer (pass a callable over the points)")
            from .rendering import apply_pointfunction

            val[1:] = apply_pointfunction(tracer["ensemble"], tracer["config"], pf, points[1:], tracer["cfg"].lambda1)
        else:
            max_time = tracer["cfg"].lambda1 if tracer is not None else math.inf
            val[1:] = [pf(metric, gp, max_time) for gp in points[1:]]
        return val
    val = np.ascontiguousarray(pf(points) if callable(pf) else pf, dtype=np.float64)
    if val.shape != (points.size,):
        raise ValueError("pf must give one value per cell, row 0 included")
    return val


def _fill_plane_values(sky, x_grid, y_grid, metric=None, pf=None, route=None, cells=False):
    """fill_sky_values of an AdaptivePlane (adaptive-plane.jl:100-181) -> out[β, α].  Per column (an α of the x grid) the β grid is
    walked ascending and every run of points held by one cell c is recorded; c's value is interpolated across α with its left
    (x < pos_x(c)) or right neighbour -- unless there is none, it lies across the periodic wrap, or its ray did not hit -- and
    the column is interpolated linearly in β between pos_y of its cells.  Where the reference is wrong or cannot run: the
    neighbour's x is its x position (the reference reads pos[2], a typo); a column with fewer than two cells is NaN (the
    reference indexes out of bounds); the image is out[β index, α index] (the reference's reshape is meaningful for square grids
    only); the values are doubles; the β grid may come in any order."""
    from .pointfunctions import AbstractPointFunction

    if _device_route(sky, route):
        import ctypes as C

        from . import _lib

        x_grid, y_grid = np.ascontiguousarray(x_grid), np.ascontiguousarray(y_grid)
        out = np.empty((y_grid.size, x_grid.size))
        held = np.empty((y_grid.size, x_grid.size, 2), dtype=np.int64) if cells else None
        s, keep, val = None, None, None
        if isinstance(pf, AbstractPointFunction) and pf.fusable:
            from .rendering import abi_pointfunction

            s, keep = abi_pointfunction(pf)
        elif pf is not None:
            val = _plane_cell_values(sky, pf, metric)
        _lib.check(sky._L.gr_sky_fill_plane(sky._dev, None if s is None else C.byref(s), None if val is None else C.c_void_p(val.ctypes.data),
                                            C.c_void_p(x_grid.ctypes.data), x_grid.size, C.c_void_p(y_grid.ctypes.data), y_grid.size,
                                            C.c_void_p(out.ctypes.data), None if held is None else C.c_void_p(held.ctypes.data)))
        del keep
        return (out, (held[..., 0].copy(), held[..., 1].copy())) if cells else out
    g, val, status = sky.grid, _plane_cell_values(sky, pf, metric), sky.values["status"]
    out = np.full((y_grid.size, x_grid.size), np.nan)
    lower, upper = (np.zeros(out.shape, dtype=np.int64) for _ in range(2))
    order = np.argsort(y_grid, kind="stable")          # ascending, NaN last, equal values in the caller's order (theta_order)
    ys = y_grid[order]
    for k, x in enumerate(x_grid):
        idx = np.fromiter((g.get_parent_index(x, y) for y in ys), dtype=np.int64, count=ys.size)
        idx = idx[idx != 0]
        if idx.size == 0:
            continue
        first = np.ones(idx.size, dtype=bool)
        first[1:] = idx[1:] != idx[:-1]
        held = idx[first]
        if held.size < 2:
            continue
        cx = g.pos[held, 0]
        left = x < cx
        nb = np.where(left, g.neighbours[held, 3], g.neighbours[held, 1])
        nx = g.pos[nb, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            usable = (nb != 0) & np.where(left, nx < cx, nx > cx) & (status[nb] == _HIT)
            w = (x - nx) / (cx - nx)
            from_left = (1.0 - w) * val[nb] + w * val[held]
            w = (x - cx) / (nx - cx)
            from_right = (1.0 - w) * val[held] + w * val[nb]
            values = np.where(usable, np.where(left, from_left, from_right), val[held])
            column = g.pos[held, 1]
            i = np.clip(np.searchsorted(column, ys, side="right"), 1, column.size - 1) - 1
            w = (ys - column[i]) / (column[i + 1] - column[i])
            out[order, k] = (1.0 - w) * values[i] + w * values[i + 1]
        lower[order, k], upper[order, k] = held[i], held[i + 1]
    return (out, (lower, upper)) if cells else out


def fill_sky_values(sky, grid, route=None, cells=False, metric=None, pf=None):
    """fill_sky_values(sky, N) -> (ϕ grid, θ grid, rows[θ, ϕ]); fill_sky_values(sky, (ϕ grid, θ grid)) -> rows[θ, ϕ]
    (adaptive-sample.jl:196-250): per column of ϕ, the cells that hold the grid's points, sorted by θ and linearly interpolated.
    All six fields are averaged: the reference's _to_vector packs five of the six into a six-vector and so drops the status
    (adaptive-sample.jl:28); a column with fewer than two cells (the reference indexes out of bounds there) is NaN.
    `cells=True` appends (lower cell[θ, ϕ], upper cell[θ, ϕ]) -- the two cells every point is interpolated between, 0 in a NaN
    column -- to what is returned.  `route="device"` forms the image on a resident sky's device (gr_sky_fill) instead of
    reading the mirror.  The θ grid may be in any order on both routes.
    On an AdaptivePlane: fill_sky_values(sky, N, metric=m) -> (α grid, β grid, out[β, α]) and fill_sky_values(sky, (α grid, β grid),
    metric=m) -> out[β, α] of adaptive-plane.jl:93-181, one double per point: `pf` is a point function (None: the coordinate time
    x[0] of the end point, the reference's default; a built-in of ConstPointFunctions is evaluated on the device; any other
    callable is given the mirror's points, row 0 included, and returns one value per row; an array is taken as those values).
    `route="device"`: gr_sky_fill_plane.  See _fill_plane_values for what is decided where the reference cannot run."""
    if _is_plane(sky):
        if np.isscalar(grid):
            (x1, x2), (y1, y2) = sky.grid.limits
            x_grid, y_grid = np.linspace(x1, x2, int(grid)), np.linspace(y1, y2, int(grid))
            filled = _fill_plane_values(sky, x_grid, y_grid, metric=metric, pf=pf, route=route, cells=cells)
            return (x_grid, y_grid) + (filled if cells else (filled,))
        x_grid, y_grid = (np.asarray(a, dtype=np.float64) for a in grid)
        return _fill_plane_values(sky, x_grid, y_grid, metric=metric, pf=pf, route=route, cells=cells)
    if pf is not None:
        raise TypeError("pf belongs to an AdaptivePlane: a corona's sky is filled with its six row fields")
    if np.isscalar(grid):
        ϕ_grid = np.linspace(-math.pi, math.pi, int(grid))
        θ_grid = np.linspace(0.0, math.pi, int(grid))
        filled = fill_sky_values(sky, (ϕ_grid, θ_grid), route=route, cells=cells)
        return (ϕ_grid, θ_grid) + (filled if cells else (filled,))
    ϕ_grid, θ_grid = (np.asarray(a, dtype=np.float64) for a in grid)
    if _device_route(sky, route):
        out, lower, upper = sky.device_fill(ϕ_grid, θ_grid)
        return (out, (lower, upper)) if cells else out
    out = make_null(θ_grid.size * ϕ_grid.size).reshape(θ_grid.size, ϕ_grid.size)
    lower, upper = (np.zeros(out.shape, dtype=np.int64) for _ in range(2))
    cosθ = np.cos(θ_grid)
    for k, ph in enumerate(ϕ_grid):
        held = {sky.grid.get_parent_index(c, ph) for c in cosθ}
        held.discard(0)
        if len(held) < 2:
            continue
        held = np.fromiter(held, dtype=np.int64)
        column = np.arccos(sky.grid.pos[held, 0])
        order = np.argsort(column, kind="stable")
        column, held = column[order], held[order]
        vals = sky.values[held]
        idx = np.clip(np.searchsorted(column, θ_grid, side="right"), 1, column.size - 1) - 1
        w = (θ_grid - column[idx]) / (column[idx + 1] - column[idx])
        for f in SKY_FIELDS:
            out[f][:, k] = (1.0 - w) * vals[f][idx] + w * vals[f][idx + 1]
        lower[:, k], upper[:, k] = held[idx], held[idx + 1]
    return (out, (lower, upper)) if cells else out


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


def bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky, Γ=2, ensemble=None, route=None):
    """bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky; Γ = 2) (adaptive-sample.jl:266-362): per (r, ϕ) bin the solid-angle
    weighted mean of J g^Γ γ(r) A(r) over the leaves that land in it; Γ = None leaves the redshift out.  `route="device"`: formed
    on a resident sky's device (gr_sky_bin_grid; γ A by k_disc_area_factor with the sky's own ISCO and plunging table).  The two
    routes agree to rounding (DESIGN_measurements.md §M33) with one exception: for KerrRefractive, at radii within 1.25 of its
    corona_radius, the device's γ A carries ∂n/∂r of the refractive index and numpy's (metrics.KerrRefractive._components)
    does not, so the maps differ by up to 1.6 % in the bins of those radii."""
    _corona_only(sky, "bin_emissivity_grid")
    if _device_route(sky, route):
        return sky.device_bin_grid("emissivity", r_bins, ϕ_bins, Γ=Γ)
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


def bin_redshift_grid(r_bins, ϕ_bins, sky, route=None):
    """bin_redshift_grid(r_bins, ϕ_bins, sky) (adaptive-sample.jl:364-406): the solid-angle weighted mean of g per bin;
    `route="device"`: on a resident sky's device"""
    _corona_only(sky, "bin_redshift_grid")
    if _device_route(sky, route):
        return sky.device_bin_grid("redshift", r_bins, ϕ_bins, Γ=None)
    return _bin_grid(sky, r_bins, ϕ_bins, lambda v: v["g"])


def bin_time_grid(r_bins, ϕ_bins, sky, route=None):
    """bin_time_grid(r_bins, ϕ_bins, sky) (adaptive-sample.jl:408-450): the solid-angle weighted mean of t per bin;
    `route="device"`: on a resident sky's device"""
    _corona_only(sky, "bin_time_grid")
    if _device_route(sky, route):
        return sky.device_bin_grid("time", r_bins, ϕ_bins, Γ=None)
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
        st = ens.call("gr_sky_cells", C.byref(cfg), C.byref(cells), C.byref(pf), out.ctypes.data)
        keep["launches"].append((int(cosθ.size), float(st.call_ms)))
        return out

    return calc_values, keep


def _make_plane_tracer(m, x, d, *, ensemble=None, t_max=None, **solver_opts):
    """_init_adaptive_tracer (adaptive-plane.jl:1-22): chart_for_metric(m, 2 * 2 x[1]), no callback, λ in (0, t_max = 2 x[1]).
    Returns (calc_values(α[], β[]) -> POINT_DTYPE rows, what it keeps alive)."""
    import ctypes as C

    from . import _lib
    from .tracing import chart_for_metric, lnr_momentum_to_global_velocity_matrix, tracing_configuration

    x = np.array(x, dtype=np.float64)
    t_max = 2 * x[1] if t_max is None else float(t_max)
    solver_opts.setdefault("chart", chart_for_metric(m, 2 * 2 * x[1]))
    config = tracing_configuration(m, x, np.zeros((1, 4)), d, (0.0, t_max), ensemble=ensemble, **solver_opts)
    ens = config.ensemble
    cfg = config.abi_config()
    plane = _lib.gr_plane()
    for q in range(4):
        plane.x_obs[q] = x[q]
    for q, val in enumerate(np.ascontiguousarray(lnr_momentum_to_global_velocity_matrix(m, x)).ravel()):
        plane.Mx[q] = val
    keep = {"config": config, "cfg": cfg, "plane": plane, "ensemble": ens, "x_obs": x, "launches": []}

    def calc_values(α, β):
        α, β = np.ascontiguousarray(α, dtype=np.float64), np.ascontiguousarray(β, dtype=np.float64)
        out = np.zeros(α.size, dtype=_lib.POINT_DTYPE)
        st = ens.call("gr_plane_cells", C.byref(cfg), C.byref(plane), α.ctypes.data, β.ctypes.data, α.size, out.ctypes.data)
        keep["launches"].append((int(α.size), float(st.call_ms)))
        return out

    return calc_values, keep


def AdaptivePlane(m, x, d, *, check_refine=None, α_lims=(-10, 10), β_lims=(-10, 10), ensemble=None, t_max=None, x_periodic=False,
                  resident=False, **solver_opts):
    """AdaptivePlane(m, x, d; check_refine = check_refine_plane, α_lims, β_lims, t_max = 2 x[1], solver_opts...)
    (adaptive-plane.jl:60-91): an AdaptiveSky over an observer's impact parameters (α, β) whose rows are GeodesicPoints
    (`sky.values` is a POINT_DTYPE array; row 0 a null point, NaN fields and NoStatus).  Cell (α, β) is the ray
    map_impact_parameters(m, x, -α, β); every step's new cells are ONE gr_plane_cells launch (shared among the contexts of a
    multi-device ensemble).  `resident=True` keeps the tree and the points on the device (gr_sky_create_plane; one context).
    `x_periodic=False` is a deliberate deviation: the reference's AdaptiveGrid(α_lims..., β_lims...) inherits x_periodic = true
    by accident and so pairs the left edge of an image with its right edge; `x_periodic=True` reproduces the reference's grid."""
    from . import _lib

    if resident and ensemble is not None and ensemble.multi:
        raise ValueError("AdaptivePlane(resident=True) keeps the plane on ONE context: pass an ensemble of one device, "
                         "or resident=False to share every step's cells among the contexts")
    calc_values, tracer = _make_plane_tracer(m, x, d, ensemble=ensemble, t_max=t_max, **solver_opts)
    sky = AdaptiveSky(calc_values, check_refine_plane if check_refine is None else check_refine,
                      limits=(α_lims[0], α_lims[1], β_lims[0], β_lims[1]), x_periodic=x_periodic, null=make_null(1, _lib.POINT_DTYPE))
    sky.tracer = tracer
    if resident:
        sky._make_resident()
    return sky


# ---- the drivers: adaptive-sample.jl:486-842 ----

class AxisLimits:
    """AxisLimits(l1[, l2]) (adaptive-sample.jl:486-503): one or two ranges of bin indices, 1-based and inclusive as the
    reference's UnitRanges are"""

    def __init__(self, l1, l2=None):
        self.l1 = (int(l1[0]), int(l1[1]))
        self.l2 = None if l2 is None else (int(l2[0]), int(l2[1]))

    def __repr__(self):
        return f"AxisLimits({self.l1[0]}:{self.l1[1]}" + ("" if self.l2 is None else f", {self.l2[0]}:{self.l2[1]}") + ")"

    def as_index(self):
        """_as_index, 0-based for numpy"""
        idx = np.arange(self.l1[0] - 1, self.l1[1])
        return idx if self.l2 is None else np.concatenate([idx, np.arange(self.l2[0] - 1, self.l2[1])])

    def intervals(self, domain):
        """the closed intervals of `domain` the ranges span (_is_in)"""
        spans = [(float(domain[self.l1[0] - 1]), float(domain[self.l1[1] - 1]))]
        if self.l2 is not None and self.l2[1] >= self.l2[0]:
            spans.append((float(domain[self.l2[0] - 1]), float(domain[self.l2[1] - 1])))
        return spans


def empty_fraction(r, ϕ, block):
    """empty_fraction(r, ϕ, block) (adaptive-sample.jl:505-511): count(!=(0), block) / length(block) -- the FILLED fraction,
    as the reference computes it despite its name"""
    block = np.asarray(block)
    return np.count_nonzero(block) / block.size


def evaluate_refinement_metric(m, d, sky, r_bins, ϕ_bins, split=6, metric=empty_fraction):
    """evaluate_refinement_metric(m, d, sky, r_bins, phi_bins; split, metric) (adaptive-sample.jl:532-562): the (r, ϕ) map of the
    sky in blocks of N ÷ split + 1 bins, every (N ÷ split) ÷ 4 bins, and `metric(r, ϕ, block)` of each.  A list of
    (r limits, ϕ limits, score) in the reference's order: the blocks that wrap around ϕ = 0 first, then ϕ by ϕ, r fastest.
    On a resident sky the default metric reads the device's census of the bins (gr_sky_occupancy), which is non-zero exactly
    where the map is; any other metric is given the map of the mirror."""
    _corona_only(sky, "evaluate_refinement_metric")
    N = len(r_bins)
    if len(ϕ_bins) != N:
        raise ValueError("r_bins and ϕ_bins must have the same length")
    if sky.resident and metric is empty_fraction:
        output = sky.device_occupancy(r_bins, ϕ_bins)
    else:
        output = bin_emissivity_grid(m, d, r_bins, ϕ_bins, sky)
    stencil = N // split
    half = stencil // 2

    def eval_metric(i, j):
        r = AxisLimits((i, i + stencil))
        ϕ = AxisLimits((1, half), (N - half, N)) if j == 0 else AxisLimits((j, j + stencil))
        block = output[np.ix_(r.as_index(), ϕ.as_index())]
        return r, ϕ, metric(r, ϕ, block)

    axis = range(1, N - stencil + 1, stencil // 4)
    return [eval_metric(i, 0) for i in axis] + [eval_metric(i, j) for j in axis for i in axis]


class StepBlockCodes(enum.Enum):
    converged = 0
    not_converged = 1
    limit_exceeded = 2


def step_block(m, d, sky, check_threshold=True, threshold=0.2, N=500, top=3, split=6, percentage=10, limit=200_000,
               metric=empty_fraction):
    """step_block!(m, d, sky; ...) (adaptive-sample.jl:603-665): bin the sky into N x N bins of logrange(isco, 1000) x
    range(0, 2π), score the blocks, and refine -- to `percentage` per cent -- the pairs with a cell in one of the `top`
    lowest-scoring blocks (those below `threshold` if check_threshold).  StepBlockCodes.converged if no block is left,
    limit_exceeded (and nothing refined) if more than `limit` cells would be refined, else not_converged."""
    _corona_only(sky, "step_block")
    r_bins = np.geomspace(m.isco(), 1000.0, N)
    ϕ_bins = np.linspace(0.0, TWO_PI, N)
    counts = evaluate_refinement_metric(m, d, sky, r_bins, ϕ_bins, split=split, metric=metric)
    counts = [c for c in counts if c[2] != 0]
    counts.sort(key=lambda c: c[2])          # (stable, as the reference's sort! of a vector of tuples is)
    if check_threshold:
        counts = [c for c in counts if c[2] < threshold]
        if not counts:
            return StepBlockCodes.converged
    boxes = []
    for r, ϕ, _ in counts[:top]:
        (r_lo, r_hi), = r.intervals(r_bins)
        boxes.append(RadialBox(r_lo, r_hi, ϕ=ϕ.intervals(ϕ_bins), open=False, ϕ_open=False))
    found = _find(sky, fine_refine_function(boxes, percentage=percentage))
    if found[0] > limit:
        print(f"Convergence failed. Limit {limit} exceeded: too many cells to refine (N = {found[0]}).", file=sys.stderr)
        return StepBlockCodes.limit_exceeded
    _refine_found(sky, found)
    return StepBlockCodes.not_converged


def adaptive_solve(m, d, sky, verbose=True, limit=50, trace_calls=2, **step_block_kwargs):
    """adaptive_solve!(m, d, sky; verbose, limit, trace_calls, kwargs...) (adaptive-sample.jl:745-842): trace_initial, 1 +
    trace_calls plain steps, a pass over the far radii (r > 800 at 10 %) and one over the innermost (r_isco < r < 2 at 20 %), then
    step_block (split = 5, top = 4 unless given) until every block is covered or `limit` iterations are spent, then levels 4
    and 5.  Returns the number of refinement iterations."""
    _corona_only(sky, "adaptive_solve")
    i = 0
    t0 = time.perf_counter()

    def report(what):
        if verbose:
            print(f"adaptive_solve: iteration {i:3d} {what:<14} cells {sky.n_cells:>9}  {time.perf_counter() - t0:8.2f} s", file=sys.stderr)

    trace_initial(sky)
    trace_step(sky)
    i += 1
    report("trace_step")
    for _ in range(trace_calls):
        trace_step(sky)
        i += 1
        report("trace_step")
    trace_step(sky, fine_refine_function(RadialBox(800.0, math.inf, open=(True, False)), percentage=10))
    i += 1
    report("far")
    trace_step(sky, fine_refine_function(RadialBox(m.isco(), 2.0, open=True), percentage=20))
    i += 1
    report("inner")
    kwargs = {"split": 5, "top": 4}
    kwargs.update(step_block_kwargs)
    status = StepBlockCodes.not_converged
    while status is StepBlockCodes.not_converged:
        status = step_block(m, d, sky, **kwargs)
        i += 1
        report(status.name)
        if i >= limit:
            break
    for level in (4, 5):
        trace_step(sky, refine_to_level(level))
        i += 1
        report(f"level {level}")
    return i
