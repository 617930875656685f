"""lineprofile(bins, ε, m, u, d, BinningMethod(); ...) -- src/line-profiles.jl:152-198.

The image plane (PolarPlane / CartesianPlane) is traced on the device from its impact parameters;
for a power-law emissivity the weighting ε(r) g³ area and the binning over g are fused into the
trace kernel (fp64 atomics into the flux array), otherwise the device returns (g, ρ) per ray and
the emissivity and `bucket` run on the host.  `bucket(Simple(), g, f, bins)` is Buckets.jl
(third party, not vendored by the reference): restated as "last bin edge <= g, clamped to the
first / last bin".  The line-profile tests constrain it only through the profile's edges and unit
sum (test/line-profiles/test-binning.jl:5-32); the convention itself is pinned by the golden
emissivity vector of test/unit/emissivity.jl:27-48, which goes through the same `Simple()` bucket
(corona.py) and is reproduced to 1e-10 with this rule and not at all with the other.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .planes import GeometricGrid, PolarPlane, impact_parameters, unnormalized_areas
from .pointfunctions import ConstPointFunctions
from .rendering import abi_pointfunction
from .tracing import (domain_upper_hemisphere, lnr_momentum_to_global_velocity_matrix, separable_rayset,
                      tracing_configuration)


class BinningMethod:
    pass


class TransferFunctionMethod:
    """line-profiles.jl:126-152: Cunningham transfer functions integrated over the disc (the
    reference's default method); the transfer functions of all radii are solved in one batch on the device."""


class PowerLawEmissivity:
    """ε(r) = r^-q ; recognised by `lineprofile` and evaluated on the device."""

    def __init__(self, q=3.0):
        self.q = float(q)

    def __call__(self, r):
        return r ** (-self.q)


def bucket_simple(g, f, bins):
    """bucket(Simple(), g, f, bins)"""
    bins = np.asarray(bins, dtype=np.float64)
    idx = np.clip(np.searchsorted(bins, g, side="right") - 1, 0, bins.size - 1)
    return np.bincount(idx, weights=f, minlength=bins.size)


def _tile_order(n_rows, n_cols, tr=8, tc=8):
    """Permutation of the column-major ray index of an n_rows x n_cols plane that walks it in tr x tc
    tiles: the 64 rays a wave traces together are then neighbours in BOTH plane coordinates (similar
    length, same fate), like the 8 x 8 pixel tiles of the render kernels.  A histogram does not care in
    which order its rays arrive."""
    if os.environ.get("GRADUS_MI355X_TILE_RAYS", "1") == "0" or n_rows < tr or n_cols < tc:
        return None
    R, Cc = (n_rows // tr) * tr, (n_cols // tc) * tc
    i = np.arange(R, dtype=np.int64).reshape(R // tr, 1, tr, 1)           # [tile row, tile col, row in tile, col in tile]
    j = np.arange(Cc, dtype=np.int64).reshape(1, Cc // tc, 1, tc)
    core = np.transpose(i + n_rows * j, (1, 0, 3, 2)).reshape(-1)         # tiles down a column strip, lanes column-major in the tile
    rest = np.ones(n_rows * n_cols, dtype=bool)
    rest[core] = False
    return np.concatenate([core, np.nonzero(rest)[0]])


def _sep_index(k, nr, nt, tiled):
    """Ray k of a separable set -> (radius index i, angle index j): the map `Ray::sep_index` (gr_device.hpp) applies on the
    device, vectorised (only the (g, ρ)-pairs route needs it on the host, to weight each ray with its area)."""
    k = np.asarray(k, dtype=np.int64)
    if not tiled:
        return k % nr, k // nr
    R, Cc = (nr // 8) * 8, (nt // 8) * 8
    core = R * Cc
    i, j = np.empty_like(k), np.empty_like(k)
    a = k < core
    ka = k[a]
    t = ka >> 6
    tiles_down = R >> 3
    i[a] = ((t % tiles_down) << 3) + (ka & 7)
    j[a] = ((t // tiles_down) << 3) + ((ka >> 3) & 7)
    kb = k[~a] - core
    tail = nr - R
    first = kb < Cc * tail
    jb = np.where(first, kb // max(tail, 1), Cc + (kb - Cc * tail) // nr)
    ib = np.where(first, R + kb % max(tail, 1), (kb - Cc * tail) % nr)
    i[~a], j[~a] = ib, jb
    return i, j


class _LazyAreas:
    """unnormalized_areas of a separable ray set in the device's ray order, built on first use."""

    def __init__(self, r, nr, nt, tiled):
        self.r, self.nr, self.nt, self.tiled, self._a = r, nr, nt, tiled, None

    def __getitem__(self, I):
        I = np.asarray(I)
        if I.dtype == bool:
            I = np.flatnonzero(I)
        i, _ = _sep_index(I.astype(np.int64, copy=False), self.nr, self.nt, self.tiled)      # only the rays asked for (the hits)
        r = self.r[i]
        return r * r


def _rayset(config, plane, keep):
    from .planes import PolarPlane

    if isinstance(plane, PolarPlane) and os.environ.get("GRADUS_MI355X_SEPARABLE_RAYS", "1") != "0":
        # α = r_i cos θ_j, β = r_i sin θ_j, area = r_i² (planes.jl:96-131): three small tables cross the boundary and the
        # device forms the rays (for C5, 4096² rays: 100 KB instead of 403 MB, and no 5 s of host-side fancy indexing)
        tiled = os.environ.get("GRADUS_MI355X_TILE_RAYS", "1") != "0" and plane.Nr >= 8 and plane.Nθ >= 8
        rs, (r, cs, sn) = separable_rayset(config.metric, config.position, plane, tiled)
        keep += [r, cs, sn]
        rs._tiled = tiled
        return rs, _LazyAreas(r, plane.Nr, plane.Nθ, tiled)
    αs, βs = impact_parameters(plane, config.position)
    areas = np.ascontiguousarray(unnormalized_areas(plane).ravel(order="F"), dtype=np.float64)
    shape = unnormalized_areas(plane).shape
    perm = _tile_order(shape[0], shape[1]) if αs.size == shape[0] * shape[1] else None
    if perm is not None:
        αs, βs, areas = αs[perm], βs[perm], areas[perm]
    αs = np.ascontiguousarray(αs, dtype=np.float64)
    βs = np.ascontiguousarray(βs, dtype=np.float64)
    keep += [αs, βs, areas]
    rs = _lib.gr_rayset()
    for i in range(4):
        rs.x_obs[i] = float(config.position[i])
    Mx = lnr_momentum_to_global_velocity_matrix(config.metric, config.position)
    for i in range(4):
        for k in range(4):
            rs.Mx[4 * i + k] = float(Mx[i, k])
    rs.alpha, rs.beta, rs.area, rs.n = αs.ctypes.data, βs.ctypes.data, areas.ctypes.data, αs.size
    rs._tiled = perm is not None
    return rs, areas


def lineprofile(bins, ε, m, u, d, method=None, *, λ_max=None, redshift_pf=None, minrₑ=None, maxrₑ=50.0,
                plane=None, callback="default", ensemble=None, stats=False, integrate_on_device=False, **solver_args):
    """lineprofile(bins, ε, m, u, d, [method]; ...) -> (bins, normalised flux).  As in the reference
    (line-profiles.jl:100-119) the default method is TransferFunctionMethod(); BinningMethod() bins the
    image plane `plane` (fused on the device for a power-law ε).  `integrate_on_device=True` (TransferFunctionMethod
    only) also integrates the transfer functions on the device (gr_tf_lineprofile) instead of in numpy."""
    if method is None:
        method = TransferFunctionMethod()
    if isinstance(method, TransferFunctionMethod):
        from .transfer_functions import integrate_lineprofile, transferfunctions

        kw = dict(solver_args)
        numrₑ = kw.pop("numre", 100)      # identifiers are NFKC-normalised: the keyword numrₑ arrives as "numre"
        h = kw.pop("h", 2e-8)
        n_radii = kw.pop("n_radii", 1000)
        tfs = transferfunctions(m, u, d, minrₑ=(m.isco() + 1e-2 if minrₑ is None else minrₑ), maxrₑ=maxrₑ, numrₑ=numrₑ,
                                ensemble=ensemble, **kw)
        bins = np.ascontiguousarray(bins, dtype=np.float64)
        if integrate_on_device:
            from .tracing import EnsembleMI355X

            return bins, integrate_lineprofile(ε, tfs, bins, h=h, n_radii=n_radii,
                                               ensemble=EnsembleMI355X() if ensemble is None else ensemble)
        return bins, integrate_lineprofile(ε, tfs, bins, h=h, n_radii=n_radii)
    if method is not None and not isinstance(method, BinningMethod):
        raise NotImplementedError("method must be BinningMethod() or TransferFunctionMethod()")
    u = np.asarray(u, dtype=np.float64)
    bins = np.ascontiguousarray(bins, dtype=np.float64)
    λ_max = 2.0 * u[1] if λ_max is None else λ_max
    minrₑ = m.isco() if minrₑ is None else minrₑ
    if plane is None:
        plane = PolarPlane(GeometricGrid(), Nr=450, Nθ=1300, r_max=5 * maxrₑ)
    if callback == "default":
        callback = domain_upper_hemisphere()
    if redshift_pf is None:
        redshift_pf = ConstPointFunctions.redshift(m, u, **({"ensemble": ensemble} if m.metric_id != 0 else {}))
    config = tracing_configuration(m, u, np.zeros((1, 4)), d, (0.0, λ_max), callback=callback, ensemble=ensemble,
                                   **solver_args)
    cfg = config.abi_config()
    keep = []
    rs, areas = _rayset(config, plane, keep)
    pf, keep_pf = abi_pointfunction(redshift_pf)
    # The library takes caller-ordered ray sets to the persistent kernel (neighbours may differ wildly).  Rays handed
    # over in tiles are as coherent as an image plane, and then one ray per lane wins while a ray is long: measured
    # on C5 (4096² rays) -4 % at tolerance 1e-9, -6 % at 1e-7, even at 1e-5, +18 % at 1e-3 (21 vs 18 ms: with 14
    # steps per ray the per-workgroup histogram flush decides).
    ens = config.ensemble
    lane = getattr(rs, "_tiled", False) and ens.knobs.get("kernel", 2) == 2 and max(config.abstol, config.reltol) <= 1e-6
    fused = isinstance(ε, PowerLawEmissivity) or _emissivity_table(ε) is not None
    ctxs = ens.contexts if (ens.multi and fused) else [ens.ctx]       # the contexts _lineprofile_call runs on
    if lane:
        for c in ctxs:
            c.set("kernel", 0)
    try:
        return _lineprofile_call(ens, cfg, rs, pf, ε, bins, minrₑ, maxrₑ, areas, stats)
    finally:
        if lane:
            for c in ctxs:
                c.set("kernel", 2)


def _emissivity_table(ε):
    """(radii, values) of an emissivity given as a RadialDiscProfile (anything with `radii` and `ε` arrays and the
    reference's `emissivity_at` semantics, src/corona/radial.jl:15-18), else None."""
    r, v = getattr(ε, "radii", None), getattr(ε, "ε", None)
    if r is None or v is None or not hasattr(ε, "emissivity_at"):
        return None
    r, v = np.ascontiguousarray(r, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    if r.ndim != 1 or r.size < 2 or r.shape != v.shape or np.any(np.diff(r) <= 0):
        return None
    return r, v


def _lineprofile_call(ens, cfg, rs, pf, ε, bins, minrₑ, maxrₑ, areas, stats):
    table = None if isinstance(ε, PowerLawEmissivity) else _emissivity_table(ε)
    if isinstance(ε, PowerLawEmissivity) or table is not None:
        b = _lib.gr_binning(float(minrₑ), float(maxrₑ), ε.q if table is None else 0.0, bins.size, bins.ctypes.data)
        if table is not None:
            # an emissivity profile is a table: interpolated on the device like the power law is evaluated there
            b.eps_r, b.eps_v, b.eps_n = table[0].ctypes.data, table[1].ctypes.data, table[0].size
        flux = np.zeros(bins.size)
        # several devices: the plane's rays dealt over them, one histogram each, added by the host (gr_lineprofile_multi)
        st = ens.call("gr_lineprofile", C.byref(cfg), C.byref(rs), C.byref(pf), C.byref(b), flux.ctypes.data)
    else:
        # the (g, ρ) route for callable emissivities: one device
        pairs = np.zeros((rs.n, 2))
        st = _lib.gr_stats()
        _lib.check(_lib.load().gr_redshift_radius(ens.ctx.handle, C.byref(cfg), C.byref(rs), C.byref(pf), float(minrₑ), float(maxrₑ),
                                                  pairs.ctypes.data, C.byref(st)))
        I = np.flatnonzero(~np.isnan(pairs[:, 0]))
        g, r = pairs[I, 0], pairs[I, 1]
        f = (ε(r) if callable(ε) else ε.emissivity_at(r)) * (g * g * g) * areas[I]
        flux = bucket_simple(g, f, bins)
    total = flux.sum()
    out = flux / total if total != 0 else flux
    return (bins, out, st.asdict()) if stats else (bins, out)
