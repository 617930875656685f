"""Corona -> disc tracing and emissivity profiles (first half).

Host-side mirror of src/corona/{corona-models,samplers,emissivity,flux-calculations,radial,spectra}.jl
and src/corona/models/lamp-post.jl.  Every geodesic is traced by the device integrator through
`tracegeodesics(m, xs, vs, d, λmax; callback = domain_upper_hemisphere())` -- the same
`gr_trace_endpoints` entry point as any other array input; what is here is the source-frame set-up
(sky angles -> tetrad -> global velocity) and the reduction of the end points to a radial
emissivity profile.  No tracing happens on the host.

`bucket!(IndexBucket, Simple(), radii, bins)` is Buckets.jl (third party): restated, as in
lineprofiles.py, as "last bin edge <= value, clamped to the first / last bin".  The reference's
golden emissivity vector (test/unit/emissivity.jl:27-48, N = 10 bins, asserted at rtol 1e-2) pins
that choice: it is reproduced to 1e-10 with this rule.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from .orthonormalization import tetradframe, tetradframe_batch
from .planes import GeometricGrid
from .status import StatusCodes
from .tracing import domain_upper_hemisphere, tracegeodesics as _tracegeodesics

TWO_PI = 2.0 * math.pi


# ------------------------------------------------------------------------------------------
# samplers (src/corona/samplers.jl)
# ------------------------------------------------------------------------------------------
class LowerHemisphere:
    pass


class BothHemispheres:
    pass


class RandomGenerator:
    """geti = rand()·N (samplers.jl:32-33); `seed` makes a run repeatable (the reference draws from
    Julia's global RNG)."""

    def __init__(self, seed=None):
        self.rng = np.random.default_rng(seed)


class GoldenSpiralGenerator:
    pass


class EvenGenerator:
    pass


class EvenSampler:
    def __init__(self, domain=None, generator=None):
        self.domain = LowerHemisphere() if domain is None else domain
        self.generator = GoldenSpiralGenerator() if generator is None else generator


class WeierstrassSampler:
    def __init__(self, res=100.0, domain=None, generator=None):
        self.resolution = float(res)
        self.domain = LowerHemisphere() if domain is None else domain
        self.generator = GoldenSpiralGenerator() if generator is None else generator


def geti(sampler, index, N):
    """samplers.jl:30-33; `index` is the 1-based sample number (array or scalar)."""
    index = np.asarray(index, dtype=np.float64)
    g = sampler.generator
    if isinstance(g, EvenGenerator):
        return index / N
    if isinstance(g, GoldenSpiralGenerator):
        return index
    if isinstance(g, RandomGenerator):
        return g.rng.random(index.shape) * N
    raise NotImplementedError(type(g).__name__)


def sample_radial(sampler, i):
    if isinstance(sampler.generator, GoldenSpiralGenerator):
        return math.pi * (1.0 + math.sqrt(5.0)) * i
    return TWO_PI * i


def sample_elevation(sampler, i):
    both = isinstance(sampler.domain, BothHemispheres)
    if isinstance(sampler, EvenSampler):
        return np.arccos(1.0 - 2.0 * i) if both else np.arccos(1.0 - i)
    if isinstance(sampler, WeierstrassSampler):
        ph = 2.0 * np.arctan(np.sqrt(sampler.resolution / i))
        if not both:
            return ph
        even = (np.floor(i) == i) & (np.mod(i, 2.0) == 0.0)      # iseven on a Float64
        return np.where(even, ph, math.pi - ph)
    raise NotImplementedError(f"Not implemented for {type(sampler).__name__}.")


def sample_angles(sampler, i, N):
    """(θ, ϕ) on the emitter's sky (samplers.jl:41-44)."""
    i = np.asarray(i, dtype=np.float64)
    el = sample_elevation(sampler, i) if isinstance(sampler, WeierstrassSampler) else sample_elevation(sampler, i / N)
    return el, np.mod(sample_radial(sampler, i), TWO_PI)


def _cart_to_spher_jacobian(θ, ϕ):
    s, c, sp, cp = float(np.sin(θ)), float(np.cos(θ)), float(np.sin(ϕ)), float(np.cos(ϕ))      # (numpy's: as _sky_rows_batch)
    return np.array([[s * cp, s * sp, c], [c * cp, c * sp, -s], [-sp, cp, 0.0]])


def _cart_local_direction(θ, ϕ):
    θ, ϕ = np.asarray(θ, dtype=np.float64), np.asarray(ϕ, dtype=np.float64)
    return np.stack([np.sin(θ) * np.cos(ϕ), np.sin(θ) * np.sin(ϕ), np.cos(θ) + 0.0 * ϕ], axis=-1)


def _components_at(m, x):
    """the five metric components at x with numpy's sin / cos (what the array routes below use: the same bits either way)"""
    return tuple(float(q) for q in m._components(x[1], float(np.sin(x[2])), float(np.cos(x[2]))))


def _metric_matrix(g):
    G4 = np.zeros((4, 4))
    G4[0, 0], G4[1, 1], G4[2, 2], G4[3, 3] = g[0], g[1], g[2], g[3]
    G4[0, 3] = G4[3, 0] = g[4]
    return G4


def tetradframe_matrix(m, x, v):
    return np.column_stack(tetradframe(_metric_matrix(_components_at(m, x)), v))


def sky_angles_to_velocity(m, x, v_source, θ, ϕ, E0=1.0):
    """samplers.jl:81-99.  θ, ϕ may be arrays: returns (n, 4) unconstrained velocities."""
    hat = -_cart_local_direction(θ, ϕ)
    k = hat @ _cart_to_spher_jacobian(x[2], x[3]).T
    p = np.concatenate([np.full(k.shape[:-1] + (1,), E0), E0 * k], axis=-1)
    return p @ tetradframe_matrix(m, x, v_source).T


# ------------------------------------------------------------------------------------------
# corona models (src/corona/models/lamp-post.jl)
# ------------------------------------------------------------------------------------------
class AbstractCoronaModel:
    point_source = False      # on-axis point source: the angular emissivity method applies
    fixed_position = False    # sample_position_velocity is deterministic: one tetrad serves every sample

    def sample_position_velocity(self, m):
        raise NotImplementedError(
            f"This functions needs to be implemented for {type(self).__name__}. See the documentation for this "
            "function for instructions.")


@dataclass(frozen=True)
class LampPostModel(AbstractCoronaModel):
    h: float = 5.0
    θ: float = 0.01
    ϕ: float = 0.0
    point_source = True

    def sample_position_velocity(self, m):
        x = np.array([0.0, self.h, self.θ, self.ϕ])
        g = m.metric_components(x[1], x[2])
        return x, np.array([1.0 / math.sqrt(-g[0]), 0.0, 0.0, 0.0])


def constrain_time(g, v, μ=0.0):
    """constrain_time (auto-diff.jl:161-179) on the host, for source velocities."""
    disc = -g[0] * g[1] * v[1] ** 2 - g[0] * g[2] * v[2] ** 2 - g[0] * μ * μ - (g[0] * g[3] - g[4] ** 2) * v[3] ** 2
    return -(g[4] * v[3] + math.sqrt(disc)) / g[0]


def _dot(g, a, b):
    """g_{μν} a^μ b^ν from the five components; works on (..., 4) arrays."""
    return (g[0] * a[..., 0] * b[..., 0] + g[1] * a[..., 1] * b[..., 1] + g[2] * a[..., 2] * b[..., 2]
            + g[3] * a[..., 3] * b[..., 3] + g[4] * (a[..., 0] * b[..., 3] + a[..., 3] * b[..., 0]))


def constrain_normalize(m, x, v, μ=0.0):
    """constraints.jl:27-30"""
    g = m.metric_components(x[1], x[2])
    v = np.asarray(v, dtype=np.float64)
    vn = v / math.sqrt(abs(_dot(g, v, v)))
    return np.array([constrain_time(g, vn, μ), vn[1], vn[2], vn[3]])


@dataclass(frozen=True)
class BeamedPointSource(AbstractCoronaModel):
    """Point source on the axis moving radially with speed β (lamp-post.jl:26-48)."""

    r: float
    β: float
    point_source = True

    def sample_position_velocity(self, m):
        x = np.array([0.0, self.r, 1e-4, 0.0])
        g = m.metric_components(x[1], x[2])
        vbar = np.array([1.0, self.β * math.sqrt(-g[0] / g[1]), 0.0, 0.0])
        return x, constrain_normalize(m, x, vbar, μ=1.0)


class SourceVelocities:
    """src/corona/models/extended.jl:1-46"""

    @staticmethod
    def co_rotating(m, x):
        """the source co-rotates with the (Keplerian) disc below it"""
        s = float(np.sin(x[2]))
        v = circular_fourvelocity(m, np.array([max(m.isco(), x[1] * s)]))[0] * s
        g = _components_at(m, x)
        v = v / math.sqrt(abs(_dot(g, v, v)))
        return np.array([constrain_time(g, v, 1.0), v[1], v[2], v[3]])

    @staticmethod
    def stationary(m, x):
        g = _components_at(m, x)
        return np.array([1.0 / math.sqrt(-g[0]), 0.0, 0.0, 0.0])

    @staticmethod
    def batch(vf, m, x):
        """vf(m, x[k]) for every row of x (n, 4), or None for a velocity function this module does not know (a user's callable: the
        caller then asks sample by sample)."""
        x = np.asarray(x, dtype=np.float64)
        s, c = np.sin(x[:, 2]), np.cos(x[:, 2])
        g = [np.asarray(q, dtype=np.float64) + 0.0 * x[:, 1] for q in m._components(x[:, 1], s, c)]
        out = np.zeros_like(x)
        if vf is SourceVelocities.stationary:
            out[:, 0] = 1.0 / np.sqrt(-g[0])
            return out
        if vf is SourceVelocities.co_rotating:
            v = circular_fourvelocity(m, np.maximum(m.isco(), x[:, 1] * s)) * s[:, None]
            v = v / np.sqrt(np.abs(_dot(g, v, v)))[:, None]
            disc = -g[0] * g[1] * v[:, 1] ** 2 - g[0] * g[2] * v[:, 2] ** 2 - g[0] - (g[0] * g[3] - g[4] ** 2) * v[:, 3] ** 2      # constrain_time, μ = 1
            out[:, 0] = -(g[4] * v[:, 3] + np.sqrt(disc)) / g[0]
            out[:, 1:] = v[:, 1:]
            return out
        return None


class RingCorona(AbstractCoronaModel):
    """RingCorona(vf, r, h): an infinitely thin ring of radius r at height h (extended.jl:55-82).  A
    representative point of the ring is returned; axis symmetry does the rest.  Its emissivity goes
    through the generic Monte-Carlo route (`emissivity_profile(..., sampler=...)`).  Its time-dependent emissivity is a
    `RingCoronaProfile` (two arms of per-slice curves), which `integrate_lagtransfer` integrates on the host and, with
    `ensemble=`, on the device (ring.jl:857-950); `ring_corona_profile` (or `emissivity_profile(..., time_dependent=True)`)
    builds it from the model: the arms of every slice of the ring's sky are traced and searched on the device (`corona_arms`,
    ring.jl:1-485)."""

    fixed_position = True

    def __init__(self, *args, r=5.0, h=5.0, vf=SourceVelocities.co_rotating):
        # RingCorona(vf, r, h) | RingCorona(r, h) | RingCorona(; r, h, vf)   (extended.jl:67-71)
        if len(args) == 3:
            vf, r, h = args
        elif len(args) == 2:
            r, h = args
        elif args:
            raise TypeError("RingCorona(vf, r, h) | RingCorona(r, h) | RingCorona(r=, h=, vf=)")
        self.vf, self.r, self.h = vf, float(r), float(h)

    def sample_position_velocity(self, m):
        x = np.array([0.0, math.hypot(self.r, self.h), math.atan2(self.r, self.h), 0.0])
        return x, np.asarray(self.vf(m, x), dtype=np.float64)


class DiscCorona(AbstractCoronaModel):
    """DiscCorona(vf, r, h): a disc of radius r at height h above the accretion disc (extended.jl:165-181); every sample leaves
    from a point of its own, x = rand() r along the disc (sample_position_velocity, extended.jl:176-183).  Its emissivity goes
    through the Monte-Carlo route (`emissivity_profile(..., sampler=...)`: tracecorona + RadialDiscProfile); the reference's
    concentric-ring profile is `DiscCoronaProfile` (rings of `RingCoronaProfile`), which `integrate_lagtransfer` integrates on
    the host and, with `ensemble=`, on the device; `disc_corona_profile` (or `emissivity_profile(..., time_dependent=True)`) builds
    it from the model, the arms of all its rings traced in one device call (extended.jl:185-200).
    `seed`: the generator behind rand()."""

    def __init__(self, *args, r=5.0, h=5.0, vf=SourceVelocities.co_rotating, seed=None):
        if len(args) == 3:
            vf, r, h = args
        elif len(args) == 2:
            r, h = args
        elif args:
            raise TypeError("DiscCorona(vf, r, h) | DiscCorona(r, h) | DiscCorona(r=, h=, vf=)")
        self.vf, self.r, self.h = vf, float(r), float(h)
        self.rng = np.random.default_rng(seed)

    def sample_position_velocity(self, m):
        ρ = self.rng.random() * self.r
        # (numpy's hypot / arctan2, as sample_positions: the two routes give the same bits)
        x = np.array([0.0, float(np.hypot(ρ, self.h)), float(np.arctan2(ρ, self.h)), 0.0])      # (x, y) flipped: off the z axis
        return x, np.asarray(self.vf(m, x), dtype=np.float64)

    def sample_positions(self, m, n, r_reject=0.0):
        """The positions of the next n calls of sample_position_velocity -- the same draws in the same order, a draw inside `r_reject`
        redrawn as corona-models.jl:1-33 does -- as an (n, 4) array."""
        xs = np.zeros((0, 4))
        if math.hypot(self.r, self.h) < r_reject:
            raise ValueError("every position of the source lies inside 1.9 inner radii")
        while xs.shape[0] < n:
            ρ = self.rng.random(n - xs.shape[0]) * self.r
            x = np.stack([np.zeros_like(ρ), np.hypot(ρ, self.h), np.arctan2(ρ, self.h), np.zeros_like(ρ)], axis=1)
            xs = np.concatenate([xs, x[x[:, 1] >= r_reject]])
        return xs


def oblate_spheroid_to_spherical(x, h, a):
    """utils.jl:186-200: (x along the equatorial axis, height h) -> Boyer-Lindquist (r, θ)"""
    if abs(a) < 1e-8:
        return math.hypot(x, h), math.atan2(x, h)
    cosθ = math.sqrt((math.sqrt(4 * a * a * h * h + (h * h + x * x - a * a) ** 2) + a * a - h * h - x * x) / (2 * a * a))
    return h / cosθ, math.acos(cosθ)


def sample_position_direction_velocity(m, model, sampler, N):
    """corona-models.jl:1-33 -> (xs, vs, vs_source), each (N, 4)."""
    idx = np.arange(1, N + 1)
    i = geti(sampler, idx, N)
    θ, ϕ = sample_angles(sampler, i, N)
    rmin = m.inner_radius() * 1.9
    if model.point_source or model.fixed_position:
        x, v = model.sample_position_velocity(m)
        if x[1] < rmin:
            raise ValueError("source position lies inside 1.9 inner radii")
        x = x.copy()
        x[2] = min(max(x[2], 1e-3), math.pi - 1e-3)             # avoid coordinate singularities :18-24
        vs = sky_angles_to_velocity(m, x, v, θ, ϕ)
        return np.tile(x, (N, 1)), vs, np.tile(v, (N, 1))
    batch = _sky_rows_batch(m, model, int(N), rmin) if hasattr(model, "sample_positions") else None
    if batch is not None:
        # every sample's position and matrix at once (the rows the device route hands over): v = M (1, -k̂)
        rows, vsrc = batch
        hat = -_cart_local_direction(θ, ϕ)
        pb = np.concatenate([np.ones((int(N), 1)), hat], axis=1)
        return rows[:, 0:4].copy(), np.einsum("nij,nj->ni", rows[:, 4:20].reshape(int(N), 4, 4), pb), vsrc
    xs, vs, vsrc = np.zeros((N, 4)), np.zeros((N, 4)), np.zeros((N, 4))
    for k in range(N):
        x, v = model.sample_position_velocity(m)
        redraws = 0
        while x[1] < rmin:
            x, v = model.sample_position_velocity(m)
            redraws += 1
            if redraws > 100_000:
                raise ValueError("source positions lie inside 1.9 inner radii")
        x = np.array(x, dtype=np.float64)
        x[2] = min(max(x[2], 1e-3), math.pi - 1e-3)
        xs[k], vsrc[k] = x, v
        vs[k] = sky_angles_to_velocity(m, x, v, θ[k], ϕ[k])
    return xs, vs, vsrc


def _device_corona_enabled(m, sampler):
    """GRADUS_MI355X_DEVICE_CORONA=0 keeps the record route (tracecorona + build_radial_profile on the host's numpy)."""
    import os

    return (os.environ.get("GRADUS_MI355X_DEVICE_CORONA", "1") != "0" and isinstance(sampler, (EvenSampler, WeierstrassSampler))
            and getattr(m, "metric_id", None) is not None)


def _sky_route(m, model, sampler):
    """Sky rays formed on the device: a source at one position crosses the boundary as one matrix, any other as 28 doubles per
    sample (gr_rayset.sky_rows, ABI 8)."""
    return _device_corona_enabled(m, sampler)


def _sky_endpoints(m, model, sampler, n_samples, geometry, λs, stats=False, **kwargs):
    """End-point records of a sky ray set (gr_rayset_endpoints): the directions are formed per lane on the device, nothing
    per ray crosses PCIe on the way in (a caller's generator: its 8 bytes per ray)."""
    import ctypes as C

    from . import _lib
    from .tracing import tracing_configuration

    rs, keep, x, v_src = sky_rayset(m, model, sampler, n_samples)
    config = tracing_configuration(m, x, np.zeros((1, 4)), geometry, λs, **kwargs)
    cfg = config.abi_config()
    out = np.zeros(rs.n, dtype=_lib.POINT_DTYPE)
    st = _lib.gr_stats() if stats else None
    _lib.check(_lib.load().gr_rayset_endpoints(config.ensemble.ctx.handle, C.byref(cfg), C.byref(rs), out.ctypes.data,
                                               C.byref(st) if stats else None))
    return (out, st, v_src) if stats else (out, v_src)


def tracegeodesics(m, model, *args, n_samples=1024, sampler=None, **kwargs):
    """tracegeodesics(m, model::AbstractCoronaModel, [d], λ; n_samples, sampler) corona-models.jl:143-153"""
    sampler = EvenSampler(BothHemispheres(), GoldenSpiralGenerator()) if sampler is None else sampler
    if _sky_route(m, model, sampler) and len(args) in (1, 2) and not kwargs.get("stats"):
        geometry, λs = args if len(args) == 2 else (None, args[0])
        return _sky_endpoints(m, model, sampler, n_samples, geometry, λs, **kwargs)[0]
    xs, vs, _ = sample_position_direction_velocity(m, model, sampler, n_samples)
    return _tracegeodesics(m, xs, vs, *args, **kwargs)


@dataclass
class CoronaGeodesics:
    metric: object
    geometry: object
    model: object
    geodesic_points: np.ndarray
    source_velocity: np.ndarray


def tracecorona(m, g, model, *, λmax=10_000.0, n_samples=1024, sampler=None, callback="default", **kwargs):
    """corona-models.jl:164-190"""
    sampler = EvenSampler(BothHemispheres(), RandomGenerator()) if sampler is None else sampler
    if callback == "default":
        callback = domain_upper_hemisphere()
    if _sky_route(m, model, sampler):
        gps, v_src = _sky_endpoints(m, model, sampler, n_samples, g, λmax, callback=callback, **kwargs)
        mask = gps["status"] == StatusCodes.IntersectedWithGeometry
        # (a source of many positions: v_src holds one source velocity per sample)
        return CoronaGeodesics(m, g, model, gps[mask], v_src[mask] if np.ndim(v_src) == 2 else np.tile(v_src, (int(mask.sum()), 1)))
    xs, vs, vsrc = sample_position_direction_velocity(m, model, sampler, n_samples)
    gps = _tracegeodesics(m, xs, vs, g, λmax, callback=callback, **kwargs)
    mask = gps["status"] == StatusCodes.IntersectedWithGeometry
    return CoronaGeodesics(m, g, model, gps[mask], vsrc[mask])


# ------------------------------------------------------------------------------------------
# disc kinematics on arrays of points
# ------------------------------------------------------------------------------------------
def _components(m, r, θ):
    return m._components(r, np.sin(θ), np.cos(θ))


def _equatorial_project(x):
    return x[..., 1] * np.abs(np.sin(x[..., 2]))


def circular_fourvelocity(m, r):
    """CircularOrbits.fourvelocity(m, r) at θ = π/2 for an array of radii (circular-orbits.jl:11-37,114-123)."""
    from .special_radii import Jet

    r = np.asarray(r, dtype=np.float64)
    g = [Jet.lift(c) for c in m._components(Jet(r, np.ones_like(r), np.zeros_like(r)), 1.0, 0.0)]
    gv = [c.v + 0.0 * r for c in g]
    dg = [c.d + 0.0 * r for c in g]
    Om = -(dg[4] - np.sqrt(dg[4] * dg[4] - dg[0] * dg[3])) / dg[3]
    D = gv[0] * gv[3] - gv[4] * gv[4]
    itt, ipp, itp = gv[3] / D, gv[0] / D, -gv[4] / D
    A = -(Om * itt - itp)
    B = Om * itp - ipp
    den = B * B * itt + 2.0 * A * B * itp + A * A * ipp
    d = -np.sign(den) * np.sqrt(1.0 / np.abs(den))
    ut, up = B * d, A * d
    out = np.zeros(r.shape + (4,))
    out[..., 0] = itt * ut + itp * up
    out[..., 3] = itp * ut + ipp * up
    return out


def _nan_linear_interp(t, u, x, default=0.0):
    """NaNLinearInterpolator (interpolations.jl:1-30): linear, extrapolating from the end intervals."""
    t, u, x = np.asarray(t), np.asarray(u), np.asarray(x, dtype=np.float64)
    idx = np.clip(np.searchsorted(t, x, side="right"), 1, t.size - 1) - 1
    x1, x2, y1, y2 = t[idx], t[idx + 1], u[idx], u[idx + 1]
    w = (x - x1) / (x2 - x1)
    y = (1.0 - w) * y1 + w * y2
    bad = np.isnan(y)
    if np.any(bad):
        pick = np.where(w < 0.5, y1, y2)
        y = np.where(bad, np.where(np.isnan(pick), default, pick), y)
    return y


def keplerian_velocity_projector(m, plunging=None, ensemble=None):
    """_keplerian_velocity_projector(m) (circular-orbits.jl:155-170): x (n, 4) -> disc four-velocity,
    Keplerian outside the ISCO, the tabulated plunge (v^r sign flipped) inside.  `plunging` is the
    (r, v^t, v^r, v^ϕ) table; by default it is traced on the device (interpolate_plunging_velocities)."""
    r_isco = m.isco()
    table = [plunging]

    def project(x):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            return project(x[None, :])[0]
        r = _equatorial_project(x)
        out = circular_fourvelocity(m, np.where(r < r_isco, r_isco, r))
        inside = r < r_isco
        if np.any(inside):
            if table[0] is None:
                from .special_radii import interpolate_plunging_velocities

                table[0] = interpolate_plunging_velocities(m, ensemble=ensemble)
            tr, tvt, tvr, tvp = table[0]
            ri = r[inside]
            out[inside, 0] = _nan_linear_interp(tr, tvt, ri)
            out[inside, 1] = -_nan_linear_interp(tr, tvr, ri)
            out[inside, 2] = 0.0
            out[inside, 3] = _nan_linear_interp(tr, tvp, ri)
        return out

    return project


def energy_ratio(m, gps, v_src, v_disc):
    """flux-calculations.jl:96-110: e_src / e_disc for arrays of GeodesicPoint records."""
    gs = _components(m, gps["x_init"][:, 1], gps["x_init"][:, 2])
    gd = _components(m, gps["x"][:, 1], gps["x"][:, 2])
    return _dot(gs, gps["v_init"], v_src) / _dot(gd, gps["v"], v_disc)


def lorentz_factor(m, x, v):
    """lorentz_factor(m, x, v; component = 4) (flux-calculations.jl:20-40): 𝒱^ϕ measured in the
    LNRF, whose ϕ and t legs are √g_ϕϕ (dϕ - ω dt) and √(-1/g^tt) dt for every static axis-symmetric
    metric (the closed form of `lnrbasis`; checked against the Gram-Schmidt basis in the tests)."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    g = _components(m, x[..., 1], x[..., 2])
    om = -g[4] / g[3]
    alpha = np.sqrt(-g[0] + g[4] * g[4] / g[3])
    V = np.sqrt(g[3]) * (v[..., 3] - om * v[..., 0]) / (alpha * v[..., 0])
    return 1.0 / np.sqrt(1.0 - V * V)


def _proper_area(m, r, θ):
    g = _components(m, np.asarray(r, dtype=np.float64), np.asarray(θ, dtype=np.float64))
    return TWO_PI * np.sqrt(g[1] * g[3])


@dataclass(frozen=True)
class PowerLawSpectrum:
    Γ: float = 2.0


def coronal_spectrum(spectrum, g):
    return g ** (-spectrum.Γ)


def point_source_equatorial_disc_emissivity(spec, θ, g, A, γ):
    return np.abs(np.sin(θ)) * coronal_spectrum(spec, g) / (A * γ)


def source_to_disc_emissivity(m, spec, N, A, x, g, v_disc):
    return N * coronal_spectrum(spec, g) / (A * lorentz_factor(m, x, v_disc))


# ------------------------------------------------------------------------------------------
# radial profiles (src/corona/radial.jl)
# ------------------------------------------------------------------------------------------
@dataclass
class RadialDiscProfile:
    radii: np.ndarray
    ε: np.ndarray
    t: np.ndarray
    _warned: list = field(default_factory=list, repr=False)

    def _bounded(self, r):
        return np.clip(r, self.radii[0], self.radii[-1])

    def emissivity_at(self, r):
        return _nan_linear_interp(self.radii, self.ε, self._bounded(np.asarray(r, dtype=np.float64)))

    def coordtime_at(self, r):
        return _nan_linear_interp(self.radii, self.t, self._bounded(np.asarray(r, dtype=np.float64)))


def emissivity_at(prof, r):
    return prof.emissivity_at(r)


def coordtime_at(prof, r):
    return prof.coordtime_at(r)


# ------------------------------------------------------------------------------------------
# time-dependent profiles of the extended coronae (src/corona/radial.jl:164-324)
# ------------------------------------------------------------------------------------------
class _TimeInterpolation:
    """NaNLinearInterpolator over an arm's knots (t, ε) sorted by t, default 0: `.t`, `.u` and a call"""

    def __init__(self, t, u):
        self.t, self.u = t, u

    def __call__(self, x):
        with np.errstate(all="ignore"):
            return _nan_linear_interp(self.t, self.u, x, 0.0)


def _in_range(interp, x):
    """an arm's ε(t) where its first knot <= x <= its last knot, 0 elsewhere: everywhere, if its last knot is NaN"""
    x = np.asarray(x, dtype=np.float64)
    inside = (x >= interp.t[0]) & (x <= interp.t[-1])
    if not np.any(inside):
        return np.zeros(x.shape)
    return np.where(inside, interp(np.where(inside, x, interp.t[0])), 0.0)


class TimeDependentRadialDiscProfile:
    """radial.jl:171-227: one arm of a ring corona.  Slice i of the source's sky met the disc along the curve
    (radii[i], t[i], ε[i]), radii[i] ascending.  At a radius ρ every slice whose curve covers ρ gives a knot (t, ε); the
    emissivity as a function of time interpolates the knots sorted by t (a stable sort, NaN last)."""

    def __init__(self, weights, radii, t, ε):
        as_list = lambda v: [np.ascontiguousarray(a, dtype=np.float64) for a in v]
        self.weights = np.asarray(weights, dtype=np.float64)
        self.radii, self.t, self.ε = as_list(radii), as_list(t), as_list(ε)
        self._last = None
        if not (len(self.radii) == len(self.t) == len(self.ε) == self.weights.size):
            raise ValueError("one weight, one radii, one t and one ε array per slice")
        for r, t_, e in zip(self.radii, self.t, self.ε):
            if not (r.ndim == 1 and r.shape == t_.shape == e.shape and r.size >= 2):
                raise ValueError("a slice is three arrays of one length, at least 2")

    def _knots(self, ρ):
        """(t, ε) of every slice at ρ, NaN where the slice does not cover it (kept for the last ρ: the limits and the
        interpolation of one annulus ask for the same knots)"""
        ρ = float(ρ)
        if self._last is not None and self._last[0] == ρ:
            return self._last[1], self._last[2]
        ts, εs = np.full(len(self.radii), np.nan), np.full(len(self.radii), np.nan)
        for i, radii in enumerate(self.radii):
            if radii[0] <= ρ <= radii[-1]:
                ts[i] = _nan_linear_interp(radii, self.t[i], ρ)
                εs[i] = _nan_linear_interp(radii, self.ε[i], ρ)
        self._last = (ρ, ts, εs)
        return ts, εs

    def emissivity_at(self, ρ):
        """the time-averaged value: Σ over the slices that cover ρ"""
        ρ = float(ρ)
        total = 0.0
        for radii, ε in zip(self.radii, self.ε):
            total = total + (float(_nan_linear_interp(radii, ε, ρ)) if radii[0] <= ρ <= radii[-1] else 0.0)
        return total

    def emissivity_interp(self, ρ):
        ts, εs = self._knots(ρ)
        J = np.argsort(ts, kind="stable")          # sortperm: stable, NaN last
        return _TimeInterpolation(ts[J], εs[J])

    def emissivity_interp_limits(self, ρ):
        ts, _ = self._knots(ρ)
        ts = ts[~np.isnan(ts)]
        return (float(ts.min()), float(ts.max())) if ts.size else (0.0, 0.0)


class RingCoronaProfile:
    """radial.jl:235-267: the two arms of a ring.  An arm counts at time x only between its first and its last knot -- so
    not at all at a radius that one of its slices misses (its last knot is then NaN)."""

    def __init__(self, left_arm, right_arm):
        self.left_arm, self.right_arm = left_arm, right_arm

    def emissivity_at(self, ρ):
        return self.left_arm.emissivity_at(ρ) + self.right_arm.emissivity_at(ρ)

    def emissivity_interp(self, ρ):
        left, right = self.left_arm.emissivity_interp(ρ), self.right_arm.emissivity_interp(ρ)
        return lambda x: _in_range(left, x) + _in_range(right, x)

    def emissivity_interp_limits(self, ρ):
        l_min, l_max = self.left_arm.emissivity_interp_limits(ρ)
        r_min, r_max = self.right_arm.emissivity_interp_limits(ρ)
        return min(l_min, r_min), max(l_max, r_max)


def _no_delay(radius):
    return 0.0


class DiscCoronaProfile:
    """radial.jl:269-324: concentric rings at `radii` (equally spaced: ring i weighs radii[i] (radii[1] - radii[0])), ring i
    delayed by propagation_velocity(radii[i])."""

    def __init__(self, radii, rings, propagation_velocity=_no_delay):
        self.radii = np.asarray(radii, dtype=np.float64)
        self.rings = list(rings)
        self.propagation_velocity = propagation_velocity
        if self.radii.size != len(self.rings) or len(self.rings) < 2:
            raise ValueError("a DiscCoronaProfile needs one radius per ring and at least 2 rings")

    def with_propagation_velocity(self, func):
        return DiscCoronaProfile(self.radii, self.rings, func)

    def _ring_weighting(self, i):
        return float(self.radii[i] * (self.radii[1] - self.radii[0]))

    def _delays(self):
        return [float(self.propagation_velocity(float(r))) for r in self.radii]

    def emissivity_at(self, ρ):
        total = 0.0
        for i, ring in enumerate(self.rings):
            total = total + ring.emissivity_at(ρ) * self._ring_weighting(i)
        return total

    def emissivity_interp(self, ρ):
        funcs = [ring.emissivity_interp(ρ) for ring in self.rings]
        dts = self._delays()

        def sum_ring_contributions(x):
            x = np.asarray(x, dtype=np.float64)
            total = np.zeros(x.shape)
            for i, f in enumerate(funcs):
                total = total + f(x - dts[i]) * self._ring_weighting(i)
            return total

        return sum_ring_contributions

    def emissivity_interp_limits(self, ρ):
        lo = hi = None
        for dt, ring in zip(self._delays(), self.rings):
            a, b = ring.emissivity_interp_limits(ρ)
            a, b = a + dt, b + dt
            lo, hi = (a, b) if lo is None else (min(lo, a), max(hi, b))
        return lo, hi


def emissivity_interp(prof, ρ):
    return prof.emissivity_interp(ρ)


def emissivity_interp_limits(prof, ρ):
    return prof.emissivity_interp_limits(ρ)


def _bucket_index(values, bins):
    """Buckets.Simple(): the bin of a value is the last edge <= value (clamped to the ends).  This is
    what the reference's golden emissivity vector implies: with "first edge >= value" the first bin
    would hold one photon and a 14x larger emissivity than recorded."""
    return np.clip(np.searchsorted(bins, values, side="right") - 1, 0, bins.size - 1)


def _profile_from_bins(m, spec, bins, count, gsum, tsum, grouped, disc_velocity):
    """the second half of _build_radial_profile (radial.jl:70-100): per-bin means -> emissivity."""
    with np.errstate(invalid="ignore", divide="ignore"):
        gs = gsum / count          # mean per bin; NaN when empty
        ts = tsum / count
    g_at = _nan_linear_interp(bins, gs, bins)
    dr = np.diff(np.concatenate([[0.0], bins]))
    xb = np.zeros((bins.size, 4))
    xb[:, 1], xb[:, 2] = bins, math.pi / 2
    vb = disc_velocity(xb)
    A = dr * _proper_area(m, bins, math.pi / 2)
    with np.errstate(all="ignore"):          # empty bins: 0 photons x (0 redshift)^-Γ = NaN, as in the reference
        ε = source_to_disc_emissivity(m, spec, grouped, A, xb, g_at, vb)
    return RadialDiscProfile(bins, ε, ts)


def build_radial_profile(m, spec, points, source_velocities, *, grid=None, N=100, intensity=None, disc_velocity=None,
                         ensemble=None):
    """_build_radial_profile + the sorting wrapper (radial.jl:38-100,132-141,155-165)."""
    grid = GeometricGrid() if grid is None else grid
    disc_velocity = keplerian_velocity_projector(m, ensemble=ensemble) if disc_velocity is None else disc_velocity
    radii = _equatorial_project(points["x"])
    J = np.argsort(radii, kind="stable")
    points, source_velocities, radii = points[J], np.asarray(source_velocities)[J], radii[J]
    times = points["x"][:, 0]
    bins = np.asarray(grid(radii.min(), radii.max(), N), dtype=np.float64)
    idx = _bucket_index(radii, bins)
    count = np.bincount(idx, minlength=bins.size).astype(np.float64)
    g_all = energy_ratio(m, points, source_velocities, disc_velocity(points["x"]))
    gsum = np.bincount(idx, weights=g_all, minlength=bins.size)
    tsum = np.bincount(idx, weights=times, minlength=bins.size)
    grouped = count if intensity is None else np.bincount(idx, weights=np.asarray(intensity)[J], minlength=bins.size)
    return _profile_from_bins(m, spec, bins, count, gsum, tsum, grouped, disc_velocity)


# ------------------------------------------------------------------------------------------
# corona -> disc on the device (gr_corona_trace / gr_corona_bin)
# ------------------------------------------------------------------------------------------
def _sky_rows_batch(m, model, n, rmin):
    """The 28-double rows of n samples of a source without one position, all at once (a Python loop over the samples costs 0.3 ms
    each: five minutes for 10⁶): positions from the model's own generator in the order its sample_position_velocity would draw them,
    velocities from SourceVelocities.batch, tetrads from tetradframe_batch.  None when the model's velocity function is not one this
    module can evaluate on arrays (the caller then loops)."""
    state = model.rng.bit_generator.state
    xs = model.sample_positions(m, n, rmin)
    with np.errstate(invalid="ignore"):
        vs = SourceVelocities.batch(model.vf, m, xs)          # (the velocity belongs to the position as drawn, the clamp comes after)
    xs[:, 2] = np.clip(xs[:, 2], 1e-3, math.pi - 1e-3)
    if vs is None or not np.all(np.isfinite(vs)):
        model.rng.bit_generator.state = state      # nothing drawn
        return None
    s, c = np.sin(xs[:, 2]), np.cos(xs[:, 2])
    g = [np.asarray(q, dtype=np.float64) + 0.0 * s for q in m._components(xs[:, 1], s, c)]
    G4 = np.zeros((n, 4, 4))
    G4[:, 0, 0], G4[:, 1, 1], G4[:, 2, 2], G4[:, 3, 3] = g[0], g[1], g[2], g[3]
    G4[:, 0, 3] = G4[:, 3, 0] = g[4]
    T = np.stack(tetradframe_batch(G4, vs), axis=2)            # columns: the four vectors (tetradframe_matrix)
    sp, cp = np.sin(xs[:, 3]), np.cos(xs[:, 3])
    B = np.zeros((n, 4, 4))
    B[:, 0, 0] = 1.0
    B[:, 1, 1], B[:, 1, 2], B[:, 1, 3] = s * cp, s * sp, c                    # _cart_to_spher_jacobian
    B[:, 2, 1], B[:, 2, 2], B[:, 2, 3] = c * cp, c * sp, -s
    B[:, 3, 1], B[:, 3, 2] = -sp, cp
    rows = np.zeros((n, 28))
    rows[:, 0:4] = xs
    rows[:, 4:20] = np.einsum("nij,njk->nik", T, B).reshape(n, 16)
    rows[:, 20] = g[0] * vs[:, 0] + g[4] * vs[:, 3]
    rows[:, 21], rows[:, 22] = g[1] * vs[:, 1], g[2] * vs[:, 2]
    rows[:, 23] = g[3] * vs[:, 3] + g[4] * vs[:, 0]
    rows[:, 24], rows[:, 27] = g[0], g[4]
    return rows, vs


def sky_rayset(m, model, sampler, n_samples):
    """The gr_rayset of `tracegeodesics(m, model, ...)` for a source at one position: the tetrad and the
    Cartesian -> spherical Jacobian go in as one matrix (v = T (1, J k̂), samplers.jl:81-99) and sample number ->
    sky angles -> k̂ happens per lane on the device (samplers.jl:30-44).  Returns (rayset, keepalive, x, v_source)."""
    from . import _lib

    rmin = m.inner_radius() * 1.9

    def matrix_at(x, v):
        B = np.eye(4)
        B[1:, 1:] = _cart_to_spher_jacobian(x[2], x[3])
        return tetradframe_matrix(m, x, v) @ B

    rs = _lib.gr_rayset()
    rows = None
    if model.point_source or model.fixed_position:
        x, v = model.sample_position_velocity(m)
        if x[1] < rmin:
            raise ValueError("source position lies inside 1.9 inner radii")
        x = np.array(x, dtype=np.float64)
        x[2] = min(max(x[2], 1e-3), math.pi - 1e-3)             # avoid coordinate singularities, corona-models.jl:18-24
        v = np.asarray(v, dtype=np.float64)
        Mx = matrix_at(x, v)
    else:
        # A source without one position (DiscCorona; any model whose sample_position_velocity draws): every sample brings its own
        # position, matrix and -- for the energy ratio -- its source velocity with the index lowered, and g_tμ there: 28 doubles
        # (gr_rayset.sky_rows), in the order corona-models.jl:1-33 draws them (rejecting positions inside 1.9 inner radii).
        rows = np.zeros((int(n_samples), 28))
        vsrc = np.zeros((int(n_samples), 4))
        batch = _sky_rows_batch(m, model, int(n_samples), rmin) if hasattr(model, "sample_positions") else None
        if batch is not None:
            rows, vsrc = batch
        for k in range(int(n_samples) if batch is None else 0):
            xk, vk = model.sample_position_velocity(m)
            redraws = 0
            while xk[1] < rmin:
                xk, vk = model.sample_position_velocity(m)
                redraws += 1
                if redraws > 100_000:
                    raise ValueError("source positions lie inside 1.9 inner radii")
            xk = np.array(xk, dtype=np.float64)
            xk[2] = min(max(xk[2], 1e-3), math.pi - 1e-3)
            vk = np.asarray(vk, dtype=np.float64)
            g = _components_at(m, xk)
            rows[k, 0:4] = xk
            rows[k, 4:20] = matrix_at(xk, vk).ravel()
            rows[k, 20:24] = (g[0] * vk[0] + g[4] * vk[3], g[1] * vk[1], g[2] * vk[2], g[3] * vk[3] + g[4] * vk[0])
            rows[k, 24:28] = (g[0], 0.0, 0.0, g[4])
            vsrc[k] = vk
        x, v, Mx = rows[int(np.argmax(rows[:, 1])), 0:4].copy(), vsrc, np.eye(4)      # (x: the outermost sample, for the chart's range checks)
        rs.sky_rows = rows.ctypes.data
    for q in range(4):
        rs.x_obs[q] = x[q]
    for q, val in enumerate(np.ascontiguousarray(Mx).ravel()):
        rs.Mx[q] = val
    rs.n = int(n_samples)
    if isinstance(sampler, EvenSampler):
        rs.sky_sampler = 1
    elif isinstance(sampler, WeierstrassSampler):
        rs.sky_sampler, rs.sky_resolution = 2, sampler.resolution
    else:
        raise NotImplementedError(f"Not implemented for {type(sampler).__name__}.")
    rs.sky_both = 1 if isinstance(sampler.domain, BothHemispheres) else 0
    keep = None
    g = sampler.generator
    if isinstance(g, GoldenSpiralGenerator):
        rs.sky_generator = 0
    elif isinstance(g, EvenGenerator):
        rs.sky_generator = 1
    else:
        # any other generator (RandomGenerator: rand() N): its numbers cross, 8 bytes per ray
        keep = np.ascontiguousarray(geti(sampler, np.arange(1, n_samples + 1), n_samples), dtype=np.float64)
        rs.sky_generator, rs.sky_i = 2, keep.ctypes.data
    return rs, (None if keep is None and rows is None else (keep, rows)), x, v


_PLUNGING_TABLES = {}


def _plunging_table(m, ensemble):
    """interpolate_plunging_velocities(m) once per metric value: one saved geodesic, a few ms, reused by every profile."""
    from .special_radii import interpolate_plunging_velocities

    try:
        if hasattr(m, "cache_key"):
            # a compiled metric: its module's build id, not its metric id -- a module slot is reused after an unload
            key = (type(m).__name__,) + tuple(m.cache_key())
        else:
            key = (type(m).__name__, int(m.metric_id)) + tuple(float(p) for p in m.abi_params())
        if not hasattr(m, "cache_key") and m.metric_id == 11:
            key += (float(m.table[8]),)          # the table's build id (unique per fit; an id() is reused once its object is gone)
    except Exception:          # a metric without flat parameters: no reuse
        return tuple(interpolate_plunging_velocities(m, ensemble=ensemble))
    if key not in _PLUNGING_TABLES:
        if len(_PLUNGING_TABLES) >= 16:
            _PLUNGING_TABLES.pop(next(iter(_PLUNGING_TABLES)))
        _PLUNGING_TABLES[key] = tuple(interpolate_plunging_velocities(m, ensemble=ensemble))
    return _PLUNGING_TABLES[key]


def disc_area_factor(m, r, *, ensemble=None, plunging="traced", r_isco=None):
    """γ(r) A(r) of the disc in the equatorial plane on the device (gr_disc_area_factor): `lorentz_factor` of the Keplerian /
    plunging disc velocity times `_proper_area`, what bin_emissivity_grid weights a leaf by.  `plunging`: the (r, v^t, v^r, v^ϕ)
    table read inside `r_isco` (default: the traced table of `_plunging_table`, as every corona profile uses it; None: Kerr's
    analytic plunge); radii inside the table's first row take that row."""
    import ctypes as C

    from . import _lib
    from .pointfunctions import GR_PF_REDSHIFT, PointFunction
    from .rendering import abi_pointfunction
    from .tracing import tracing_configuration

    r = np.ascontiguousarray(r, dtype=np.float64)
    config = tracing_configuration(m, np.array([0.0, 1000.0, math.pi / 2, 0.0]), np.zeros((1, 4)), None, (0.0, 1.0), ensemble=ensemble)
    ens = config.ensemble
    if isinstance(plunging, str):
        plunging = _plunging_table(m, ens)
    rpf = PointFunction(None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": m.isco() if r_isco is None else float(r_isco), "plunge": plunging})
    pf, keep_pf = abi_pointfunction(rpf)
    cfg = config.abi_config()
    out = np.empty(r.shape)
    ctx = ens.contexts[0] if ens.multi else ens.ctx
    _lib.check(_lib.load().gr_disc_area_factor(ctx.handle, C.byref(cfg), C.byref(pf), C.c_void_p(r.ctypes.data), r.size,
                                               C.c_void_p(out.ctypes.data)))
    del keep_pf
    return out


def device_radial_profile(m, d, model, spectrum=None, *, λmax=10_000.0, sampler=None, n_samples=1000, grid=None, N=100,
                          callback="default", ensemble=None, stats=False, **solver_args):
    """emissivity_profile(m, d, model, spectrum; n_samples, sampler, N, grid) (emissivity.jl:118-168) with the whole
    per-ray half on the device: sky sampling, tracing, energy_ratio against the Keplerian / plunging disc velocity
    (gr_corona_trace) and the radial bucketing with the per-bin sums of g and t (gr_corona_bin).  What comes back
    over PCIe is (ρ_min, ρ_max, hits) and 3 N doubles; the N-bin tail of radial.jl:86-100 runs on the host."""
    import ctypes as C

    from . import _lib
    from .rendering import abi_pointfunction
    from .tracing import tracing_configuration

    spectrum = PowerLawSpectrum(2.0) if spectrum is None else spectrum
    sampler = EvenSampler(BothHemispheres(), GoldenSpiralGenerator()) if sampler is None else sampler
    grid = GeometricGrid() if grid is None else grid
    if callback == "default":
        callback = domain_upper_hemisphere()
    rs, keep, x, v_src = sky_rayset(m, model, sampler, n_samples)
    config = tracing_configuration(m, x, np.zeros((1, 4)), d, (0.0, λmax), callback=callback, ensemble=ensemble, **solver_args)
    ens = config.ensemble
    # the disc velocity of _keplerian_velocity_projector (circular-orbits.jl:155-170): ALWAYS the traced plunging
    # table inside the ISCO (the analytic Kerr plunge of the image-plane redshift is a different, if close, function)
    plunging = _plunging_table(m, ens)
    disc_velocity = keplerian_velocity_projector(m, plunging=plunging, ensemble=ens)
    from .pointfunctions import GR_PF_REDSHIFT, PointFunction

    rpf = PointFunction(None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": m.isco(), "plunge": plunging})
    pf, keep_pf = abi_pointfunction(rpf)
    if np.ndim(v_src) == 1:
        pf.has_u_src = 1
        for q in range(4):
            pf.u_src[q] = v_src[q]
    # (a source of many positions: the rows of the ray set carry each sample's source velocity, pf.has_u_src stays 0)
    cfg = config.abi_config()
    lim = np.zeros(2)
    hits = C.c_int64(0)
    # several devices: the samples shard like any ray set (gr_rayset.sky_first / sky_total, ABI 8); every context keeps and bins
    # its own rows, the integer accumulators add up to the bits one context would give
    st = ens.call("gr_corona_trace", C.byref(cfg), C.byref(rs), C.byref(pf), lim.ctypes.data, C.byref(hits), stats=bool(stats))
    if hits.value == 0:
        raise ValueError("no ray of the corona reached the disc")
    bins = np.ascontiguousarray(grid(lim[0], lim[1], N), dtype=np.float64)
    out = np.zeros((3, bins.size))
    ens.call("gr_corona_bin", bins.ctypes.data, bins.size, out.ctypes.data, stats=None)
    prof = _profile_from_bins(m, spectrum, bins, out[0], out[1], out[2], out[0], disc_velocity)
    return (prof, st) if stats else prof


def _point_source_emissivity(m, spec, source_velocity, r, δs, points, disc_velocity, gs=None):
    """lamp-post.jl:118-156 on sorted arrays.  `gs`: the energy ratios, where the caller has them already (rows traced on the
    device carry g; `points` then needs its "x" field only)."""
    v_disc = disc_velocity(points["x"])
    n = r.size
    if gs is None:
        vsrc = np.tile(np.asarray(source_velocity, dtype=np.float64), (n, 1))
        gs = energy_ratio(m, points, vsrc, v_disc)
    γ = lorentz_factor(m, points["x"], v_disc)
    k = np.arange(n)
    i2 = np.where(k == 0, 1, np.where(k != n - 1, k + 1, k - 1))
    i4 = np.where(k == 0, 1, k - 1)
    Δr = (np.abs(r[k] - r[i2]) + np.abs(r[k] - r[i4])) / 2
    weight = (np.abs(δs[k] - δs[i2]) + np.abs(δs[k] - δs[i4])) / 4
    A = _proper_area(m, points["x"][:, 1], points["x"][:, 2]) * Δr
    return weight * point_source_equatorial_disc_emissivity(spec, δs, gs, A, γ), gs


def point_source_profile_from_points(m, spec, source_velocity, δs, gps, disc_velocity):
    """the reduction half of _point_source_symmetric_emissivity_profile (lamp-post.jl:97-115)"""
    I = gps["status"] == StatusCodes.IntersectedWithGeometry
    points, δs = gps[I], np.asarray(δs)[I]
    rs = _equatorial_project(points["x"])
    J = np.argsort(rs, kind="stable")
    rs, points, δs = rs[J], points[J], δs[J]
    ε, _ = _point_source_emissivity(m, spec, source_velocity, rs, δs, points, disc_velocity)
    return RadialDiscProfile(rs, ε, points["x"][:, 0].copy())


def polar_angle_velocities(m, x, v, δs, ϕ=0.0):
    """polar_angle_to_velfunc (emissivity.jl:175-179) evaluated for every δ."""
    return sky_angles_to_velocity(m, x, v, np.asarray(δs, dtype=np.float64), np.full(len(δs), ϕ))


def emissivity_profile(m, d, model, spectrum=None, *, λmax=10_000.0, δmin=0.01, δmax=179.99, sampler=None,
                       n_samples=1000, grid=None, N=100, callback="default", ensemble=None, time_dependent=False, **kwargs):
    """emissivity_profile(m, d, model, [spectrum]; n_samples, sampler, N, grid) emissivity.jl:118-168;
    point sources without an explicit sampler take the angular method of lamp-post.jl:68-115,158-166.
    `time_dependent=True` is the reference's EmissivityProfileSetup{true}: a RingCorona gives a RingCoronaProfile
    (`ring_corona_profile`), a DiscCorona a DiscCoronaProfile (`disc_corona_profile`); their keywords (βs, extrema_iter, h, n_rings,
    chart, route, tracer) pass through and λmax is theirs (10⁶, ring.jl:266), not this function's."""
    if time_dependent:
        if isinstance(model, RingCorona):
            return ring_corona_profile(m, d, model, spectrum=spectrum, n_samples=n_samples, ensemble=ensemble, **kwargs)
        if isinstance(model, DiscCorona):
            return disc_corona_profile(m, d, model, spectrum=spectrum, n_samples=n_samples, ensemble=ensemble, **kwargs)
        raise NotImplementedError(f"no time-dependent emissivity profile for {type(model).__name__}")
    spectrum = PowerLawSpectrum(2.0) if spectrum is None else spectrum
    if callback == "default":
        callback = domain_upper_hemisphere()
    disc_velocity = keplerian_velocity_projector(m, ensemble=ensemble)
    if sampler is None and model.point_source:
        δs = np.radians(np.linspace(δmin, δmax, n_samples))
        x, v = model.sample_position_velocity(m)
        vs = polar_angle_velocities(m, x, v, δs)
        gps = _tracegeodesics(m, x, vs, d, λmax, callback=callback, ensemble=ensemble, **kwargs)
        return point_source_profile_from_points(m, spectrum, v, δs, gps, disc_velocity)
    sampler = EvenSampler(BothHemispheres(), GoldenSpiralGenerator()) if sampler is None else sampler
    if _sky_route(m, model, sampler):
        return device_radial_profile(m, d, model, spectrum, λmax=λmax, sampler=sampler, n_samples=n_samples, grid=grid, N=N,
                                     callback=callback, ensemble=ensemble, **kwargs)
    cg = tracecorona(m, d, model, sampler=sampler, λmax=λmax, n_samples=n_samples, ensemble=ensemble)
    return build_radial_profile(m, spectrum, cg.geodesic_points, cg.source_velocity, grid=grid, N=N,
                                disc_velocity=disc_velocity)


# ------------------------------------------------------------------------------------------
# the longitudinal arms of ring coronae (src/corona/models/ring.jl:1-485, src/corona/models/extended.jl:89-200)
# ------------------------------------------------------------------------------------------
INVPHI = (math.sqrt(5.0) - 1.0) / 2.0          # ring.jl:1
_HIT = int(StatusCodes.IntersectedWithGeometry)


def DEFAULT_β_ANGLES(n=100):
    """extended.jl:53"""
    return np.sort(np.linspace(0.0, math.pi - math.pi / n, n))


@dataclass
class LongitudalArms:
    """extended.jl:89-97: what one β slice of a ring's sky lights on the disc, as two arms (r ascending, t, ε on them)"""

    β: float
    left_r: np.ndarray
    left_t: np.ndarray
    left_ε: np.ndarray
    right_r: np.ndarray
    right_t: np.ndarray
    right_ε: np.ndarray


def ring_base_angles(n_samples=1000, extrema_iter=80, h=1e-7):
    """The local angles of a slice's base rays (_RingCoronaCache, ring.jl:74-96): N = n_samples - 2 extrema_iter of them, ascending --
    range(h, π - h, N / 2) and the same shifted by π.  The reference's two errors for too few samples and an odd N."""
    N = int(n_samples) - 2 * int(extrema_iter)
    if N <= 0:
        raise ValueError(f"Too few samples for selected method. Pass `n_samples` of more than {2 * int(extrema_iter)}")
    if N % 2 != 0:
        raise ValueError(f"`n_samples` must be an even number for this method (given {N})")
    left = np.linspace(h, math.pi - h, N // 2)
    return np.sort(np.concatenate([left, np.mod(left + math.pi, TWO_PI)]))


def rodrigues_rotate(k, v, θ):
    """emissivity.jl:220"""
    return v * np.cos(θ) + np.cross(k, v) * np.sin(θ) + k * np.dot(k, v) * (1.0 - np.cos(θ))


def ring_sky_angles(x, β, θ):
    """rotatorfunctor (ring.jl:105-118) up to the sky angles: (th, ph) of the ray at local angle θ in the slice β of the sky of x"""
    axis = x[2]
    k = _cart_local_direction(axis, 0.0)
    θ = np.atleast_1d(np.asarray(θ, dtype=np.float64))
    th, ph = np.zeros(θ.size), np.zeros(θ.size)
    for i, t in enumerate(θ):
        b = rodrigues_rotate(k, _cart_local_direction(t + axis, 0.0), β)
        ph[i] = np.arctan2(b[1], b[0])
        th[i] = np.arctan2(np.sqrt(b[1] ** 2 + b[0] ** 2), b[2])
    return th, ph


def ring_velocities(m, x, v_source, β, θ):
    """rotatorfunctor (ring.jl:105-118) on the host: the unconstrained velocities (n, 4) of the rays at local angles θ"""
    th, ph = ring_sky_angles(x, β, θ)
    return sky_angles_to_velocity(m, x, v_source, th, ph)


def ring_frames(m, models):
    """Per ring the 28 doubles gr_ring_rays / gr_ring_arms form its rays from -- the layout of a row of gr_rayset.sky_rows: position,
    tetrad times Jacobian, the source velocity with its index lowered, (g_tt, 0, 0, g_tϕ).  The tetrad is host work: a ring has one
    position.  Returns (frames (n, 28), positions (n, 4), source velocities (n, 4))."""
    frames, xs, vs = np.zeros((len(models), 28)), np.zeros((len(models), 4)), np.zeros((len(models), 4))
    for k, model in enumerate(models):
        x, v = model.sample_position_velocity(m)
        x, v = np.array(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
        B = np.eye(4)
        B[1:, 1:] = _cart_to_spher_jacobian(x[2], x[3])
        g = _components_at(m, x)
        frames[k, 0:4] = x
        frames[k, 4:20] = (tetradframe_matrix(m, x, v) @ B).ravel()
        frames[k, 20:24] = (g[0] * v[0] + g[4] * v[3], g[1] * v[1], g[2] * v[2], g[3] * v[3] + g[4] * v[0])
        frames[k, 24:28] = (g[0], 0.0, 0.0, g[4])
        xs[k], vs[k] = x, v
    return frames, xs, vs


# ---- bracket and golden-section update: gr_ringarm.hpp in numpy, bit for bit (sums, differences, one product) ----
def _better(target, a, b):
    return a < b if target == 0 else a > b


def determine_bracket(rows, angles, target):
    """_determine_bracket (ring.jl:131-166) on a slice's base rows (g, ρ, t, status): (a - 2δ, b + 2δ, best_estimate), or None when
    no row met the geometry.  The strict comparison keeps the FIRST extreme row, whose two neighbour-is-a-miss widenings count."""
    N = rows.shape[0]
    hit = rows[:, 3].astype(np.int64) == _HIT
    if not hit.any():
        return None
    ρ = np.where(hit, rows[:, 1], np.inf if target == 0 else -np.inf)
    i = int(np.argmin(ρ) if target == 0 else np.argmax(ρ))
    a = b = float(angles[i])
    if i < N - 1 and not hit[i + 1]:
        b = float(angles[i + 1])
    if i > 0 and not hit[i - 1]:
        a = float(angles[i - 1])
    δ = math.pi / min(N, 32)
    return a - 2.0 * δ, b + 2.0 * δ, float(rows[i, 1])


class GoldenSearch:
    """The state of one _golden_bracket! (ring.jl:172-237)"""

    __slots__ = ("a", "b", "best", "n", "iters", "too_many", "done", "target")

    def __init__(self, a, b, best, target):
        self.a, self.b, self.best, self.target = a, b, best, target
        self.n = self.iters = 0
        self.too_many = self.done = False

    def probes(self):
        return self.b - (self.b - self.a) * INVPHI, self.a + (self.b - self.a) * INVPHI

    def update(self, extrema_iter, c_status, c_ρ, d_status, d_ρ):
        """one iteration given the probes' outcomes: 0 nothing kept, 1 the probe at c, 2 the probe at d.  best is never updated;
        n also counts every iteration once iters has passed extrema_iter"""
        c, d = self.probes()
        c_value = c_ρ if c_status == _HIT else self.best
        d_value = d_ρ if d_status == _HIT else self.best
        append = 0
        if _better(self.target, c_value, d_value):
            if _better(self.target, c_value, self.best):
                self.n += 1
                append = 1
            elif self.too_many:
                self.n += 1
            self.b = d
        else:
            if _better(self.target, d_value, self.best):
                self.n += 1
                append = 2
            elif self.too_many:
                self.n += 1
            self.a = c
        self.iters += 1
        if not self.too_many and self.iters > extrema_iter:
            self.too_many = True
        self.done = not (self.n < extrema_iter)
        return append


class NoHitError(ValueError):
    pass


def _no_hit_error(missing, n_slices):
    names = ", ".join(f"(ring {s // n_slices}, slice {s % n_slices})" for s in missing[:8])
    return NoHitError(f"no base ray met the disc in {names}{' ...' if len(missing) > 8 else ''}: no extremum to search for "
                      "(the reference fails in _determine_bracket, ring.jl:163)")


def lockstep_arm_traces(tracer, n_rings, n_slices, base_angles, extrema_iter, searches_out=None):
    """_ring_arm_traces! (ring.jl:250-288) for every slice of every ring, the searches advancing together: every row comes from
    `tracer(ring, slice, angles) -> rows (n, 4) = (g, ρ, t, status)`, called once for the base rays and once per iteration with
    the two probes of every live search.  Returns what gr_ring_arms returns: rows (n_rings, n_slices, N + 2 extrema_iter, 5) =
    (θ as probed, g, ρ, t, status) and counts (n_rings, n_slices, 3) = (N, kept by the minima search, kept by the maxima search),
    (N, -1, -1) for a slice without a hit.  `searches_out`: a dict that receives the final GoldenSearch of search 2 (ring n_slices +
    slice) + target."""
    base = np.ascontiguousarray(base_angles, dtype=np.float64)
    S, NB, E = n_rings * n_slices, base.size, int(extrema_iter)
    ring_of, slice_of = np.arange(S) // n_slices, np.arange(S) % n_slices
    rows0 = np.asarray(tracer(np.repeat(ring_of, NB), np.repeat(slice_of, NB), np.tile(base, S))).reshape(S, NB, 4)
    rows = np.zeros((S, NB + 2 * E, 5))
    rows[:, :NB, 0], rows[:, :NB, 1:] = base, rows0
    counts = np.zeros((S, 3), dtype=np.int64)
    counts[:, 0] = NB
    searches, kept = {}, {}
    for s in range(S):
        for target in (0, 1):
            br = determine_bracket(rows0[s], base, target)
            if br is None:
                counts[s, 1:] = -1
            else:
                searches[2 * s + target], kept[2 * s + target] = GoldenSearch(*br, target), []
    for _ in range(2 * E + 1):
        live = [q for q, sr in searches.items() if not sr.done]
        if not live:
            break
        angles = np.array([θ for q in live for θ in searches[q].probes()])
        sl = np.repeat(np.array(live) // 2, 2)
        pr = np.asarray(tracer(ring_of[sl], slice_of[sl], angles)).reshape(len(live), 2, 4)
        for k, q in enumerate(live):
            append = searches[q].update(E, int(pr[k, 0, 3]), float(pr[k, 0, 1]), int(pr[k, 1, 3]), float(pr[k, 1, 1]))
            if append and len(kept[q]) < E:
                kept[q].append(np.concatenate([[angles[2 * k + append - 1]], pr[k, append - 1]]))
    if searches_out is not None:
        searches_out.update(searches)
    for q, run in kept.items():
        s, target = q // 2, q % 2
        at = NB + (counts[s, 1] if target else 0)
        counts[s, 1 + target] = len(run)
        if run:
            rows[s, at:at + len(run)] = np.array(run)
    return rows.reshape(n_rings, n_slices, NB + 2 * E, 5), counts.reshape(n_rings, n_slices, 3)


class RingTracer:
    """`tracer(ring, slice, angles) -> rows` on the device (gr_ring_rays): the rays of (ring, slice, local angle) triples formed and
    traced by the kernels gr_ring_arms uses.  `launches` and `rays` count what went through it."""

    def __init__(self, m, d, models, βs, *, λmax=1_000_000.0, chart=None, ensemble=None, **solver_args):
        from . import _lib
        from .pointfunctions import GR_PF_REDSHIFT, PointFunction
        from .rendering import abi_pointfunction
        from .tracing import chart_for_metric, tracing_configuration

        self.m = m
        self.frames, self.xs, self.v_src = ring_frames(m, models)
        self.βs = np.ascontiguousarray(βs, dtype=np.float64)
        chart = chart_for_metric(m, 1_000_000.0) if chart is None else chart
        x_far = self.xs[int(np.argmax(self.xs[:, 1]))]          # (the outermost ring: the chart's range checks)
        self.config = tracing_configuration(m, x_far, np.zeros((1, 4)), d, (0.0, λmax), callback=domain_upper_hemisphere(), chart=chart,
                                            ensemble=ensemble, **solver_args)
        self.ensemble = self.config.ensemble
        if getattr(m, "M", None) == 0.0:
            # flat space: no orbit, no ISCO, no plunge -- the rows' ρ and t are straight lines' (their g is not defined)
            r_isco, self.plunging, self.disc_velocity = float(np.finfo(np.float64).tiny), None, None
        else:
            r_isco, self.plunging = m.isco(), _plunging_table(m, self.ensemble)
            self.disc_velocity = keplerian_velocity_projector(m, plunging=self.plunging, ensemble=self.ensemble)
        self.pf, self._keep_pf = abi_pointfunction(PointFunction(None, device_pf=GR_PF_REDSHIFT, extra={"r_isco": r_isco, "plunge": self.plunging}))
        self.cfg = self.config.abi_config()
        self.launches = self.rays = 0
        self._lib = _lib

    def ringset(self, base_angles=None, extrema_iter=0):
        rs = self._lib.gr_ringset()
        rs.n_rings, rs.n_slices = self.frames.shape[0], self.βs.size
        rs.frames, rs.betas = self.frames.ctypes.data, self.βs.ctypes.data
        if base_angles is not None:
            rs.n_base, rs.extrema_iter, rs.base_angles = base_angles.size, int(extrema_iter), base_angles.ctypes.data
        return rs

    def __call__(self, ring, slice_, angles, velocities=False, stats=None):
        import ctypes as C

        angles = np.ascontiguousarray(angles, dtype=np.float64)
        pairs = np.ascontiguousarray(np.stack([np.asarray(ring), np.asarray(slice_)], axis=1), dtype=np.int64)
        rows, v = np.zeros((angles.size, 4)), (np.zeros((angles.size, 4)) if velocities else None)
        rs = self.ringset()
        self._lib.check(self._lib.load().gr_ring_rays(self.ensemble.ctx.handle, C.byref(self.cfg), C.byref(rs), C.byref(self.pf), angles.size,
                                                     pairs.ctypes.data, angles.ctypes.data, rows.ctypes.data, None if v is None else v.ctypes.data,
                                                     None if stats is None else C.byref(stats)))
        self.launches += 1
        self.rays += angles.size
        return (rows, v) if velocities else rows

    def arms(self, base_angles, extrema_iter, stats=None):
        """gr_ring_arms: the whole producer in one call -> (rows, counts)"""
        import ctypes as C

        base = np.ascontiguousarray(base_angles, dtype=np.float64)
        R, S, W = self.frames.shape[0], self.βs.size, base.size + 2 * int(extrema_iter)
        rows, counts = np.zeros((R, S, W, 5)), np.zeros((R, S, 3), dtype=np.int64)
        rs = self.ringset(base, extrema_iter)
        self._lib.check(self._lib.load().gr_ring_arms(self.ensemble.ctx.handle, C.byref(self.cfg), C.byref(rs), C.byref(self.pf), rows.ctypes.data,
                                                     counts.ctypes.data, None if stats is None else C.byref(stats)))
        return rows, counts


def _arm_traces(m, d, models, βs, *, n_samples=1000, extrema_iter=80, h=1e-7, λmax=1_000_000.0, chart=None, ensemble=None,
                route="device", tracer=None, stats=None):
    βs = DEFAULT_β_ANGLES() if βs is None else np.ascontiguousarray(βs, dtype=np.float64)
    base = ring_base_angles(n_samples, extrema_iter, h)
    if route not in ("device", "lockstep"):
        raise ValueError(f"route {route!r}: \"device\" or \"lockstep\"")
    if tracer is None:
        from .geometry import ThinDisc

        if type(d) is not ThinDisc:
            raise NotImplementedError("the arms of a ring corona are traced onto a ThinDisc (gr_ring_arms: GR_ERR_UNSUPPORTED otherwise)")
        tracer = RingTracer(m, d, models, βs, λmax=λmax, chart=chart, ensemble=ensemble)
    elif route == "device":
        raise ValueError("a tracer drives the lock-step route: pass route=\"lockstep\"")
    if route == "device":
        rows, counts = tracer.arms(base, extrema_iter, stats=stats)
    else:
        rows, counts = lockstep_arm_traces(tracer, len(models), βs.size, base, extrema_iter)
    missing = np.flatnonzero(counts.reshape(-1, 3)[:, 1] < 0)
    if missing.size:
        raise _no_hit_error(missing.tolist(), βs.size)
    return rows, counts, base, tracer


def corona_arm_traces(m, d, models, βs=None, **kwargs):
    """The traced cache of every β slice of every ring of `models` (RingCorona each): (rows, counts, base angles) as gr_ring_arms lays
    them out.  route "device": one gr_ring_arms call; "lockstep": the same bracket / golden-section logic in numpy, every row through
    `tracer(ring, slice, angles) -> rows` -- gr_ring_rays unless given.  A slice none of whose base rays met the disc: ValueError.
    Keywords: n_samples, extrema_iter, h, λmax, chart, ensemble, route, tracer, stats (a gr_stats to fill, device route)."""
    return _arm_traces(m, d, models, βs, **kwargs)[:3]


# ---- a slice's cache -> its two arms (ring.jl:290-438), on the host ----
def _split_branches_further(inds, rs, cutoff_r=1e3, delta=0.01, min_length=3):
    """ring.jl:304-351.  `inds`: 1-based indices into rs, as in the reference (so that the index arithmetic reads the same)."""
    N = len(inds)
    if N == 0:
        raise ValueError("an arm without a point (findmin of an empty collection, ring.jl:306)")
    vals = [rs[i - 1] for i in inds]
    first_i = int(np.argmin(vals)) + 1                 # findmin: the first minimum
    prev = vals[first_i - 1]
    splits = [1, first_i]
    increasing = True
    for j in range(N):
        k = (j + first_i) % N + 1
        r = rs[inds[k - 1] - 1]
        if r > cutoff_r:
            increasing = False
            prev = r
            continue
        if increasing and r < prev - delta:
            increasing = False
            splits.append(k - 1 if k > 1 else N)
        elif not increasing and r > prev + delta:
            increasing = True
            splits.append(k - 1 if k > 1 else N)
        prev = r
    splits.sort()
    if len(splits) > 2:
        # merge slices that are smaller than the minimum length together
        slices = []
        i1 = splits[0]
        for i2 in splits[1:]:
            if i2 - i1 >= min_length:
                if N - i2 <= min_length:
                    i2 = N
                slices.append(list(inds[i1 - 1:i2]))
                i1 = i2
        if i1 < N:
            slices.append(list(inds[i1 - 1:]))
        return slices
    return [list(inds)]


def _split_arms_indices(angles, ρs):
    """ring.jl:353-386: 1-based index lists, each in ascending ρ (canonical_orders!: a stable sort by ρ); vcat(l1, l2)."""
    ρs = np.asarray(ρs, dtype=np.float64)
    n = ρs.size
    start = int(np.flatnonzero(~np.isnan(ρs))[0]) + 1
    i_min = i_max = start
    r_min = r_max = ρs[start - 1]
    for i in range(1, n + 1):
        r = ρs[i - 1]
        if r < r_min:
            i_min, r_min = i, r
        if r > r_max:
            i_max, r_max = i, r
    lo, hi = min(i_min, i_max), max(i_min, i_max)
    r1 = list(range(hi + 1, n + 1)) + list(range(1, lo))
    r2 = list(range(lo + 1, hi + 1))
    canonical = lambda lists: [sorted(I, key=lambda i: ρs[i - 1]) for I in lists]
    return canonical(_split_branches_further(r1, ρs)) + canonical(_split_branches_further(r2, ρs))


def _process_ring_traces(m, spectrum, v_source, disc_velocity, g, ρ, t, δs, where=""):
    """extended.jl:145-154 through _point_source_emissivity: (r, t, ε) of one arm, r ascending, ε = abs.(ε) (:153).
    Rows of bit-equal ρ (ring_arm has dropped the re-probed angles; what is left would be two angles with one ρ) keep the first:
    every Δr of _point_source_emissivity (lamp-post.jl:146-149) stays positive."""
    J = np.argsort(ρ, kind="stable")
    g, ρ, t, δs = g[J], ρ[J], t[J], δs[J]
    first = np.concatenate([[True], np.diff(ρ) != 0.0])
    g, ρ, t, δs = g[first], ρ[first], t[first], δs[first]
    if ρ.size < 2:
        raise ValueError(f"{where}an arm of the slice has fewer than 2 points")
    points = np.zeros(ρ.size, dtype=[("x", np.float64, (4,))])
    points["x"][:, 0], points["x"][:, 1], points["x"][:, 2] = t, ρ, math.pi / 2
    ε, _ = _point_source_emissivity(m, spectrum, v_source, ρ, δs, points, disc_velocity, gs=g)
    return ρ, t, np.abs(ε)


def ring_arm(m, spectrum, v_source, disc_velocity, β, rows, where=""):
    """_ring_arm! behind its traces (ring.jl:397-437): the filled prefix of a slice's cache (θ, g, ρ, t, status) -> LongitudalArms.
    The rows carry ρ = r |sin θ| of the hit, not its (r, θ): proper area, disc velocity and Lorentz factor are evaluated at
    (ρ, π/2) -- the hit itself up to the ThinDisc's gtol cone."""
    rows = rows[rows[:, 4].astype(np.int64) == _HIT]
    angles = np.mod(rows[:, 0], TWO_PI)
    I = np.argsort(angles, kind="stable")
    rows, angles = rows[I], angles[I]
    # One departure from the reference.  A golden-section iteration probes again, to rounding, the angle the iteration before it
    # kept (its c is the earlier d, ring.jl:207-208); both beat best_estimate and both join the cache, so the sorted cache holds
    # runs of rows at one angle with ρ equal to the last bit or nearly.  The reference splits and weighs them as they are: a run
    # next to the minimum becomes an "arm" of one radius that displaces a real one (the first-two rule below), and three equal ρ
    # in a row give Δr = 0 and ε = 0 / 0 (lamp-post.jl:146-149).  Here a row within 1e-12 of the angle before it is the same sample.
    fresh = np.concatenate([[True], np.diff(angles) > 1e-12])
    rows, angles = rows[fresh], angles[fresh]
    ρs = rows[:, 2]
    if ρs.size < 2:
        raise ValueError(f"{where}fewer than 2 rays of the slice met the disc")
    lists = _split_arms_indices(angles, ρs)
    if len(lists) < 2:
        raise ValueError(f"{where}the slice has one arm only")
    arms = []
    for I1 in lists[:2]:          # `r1, r2 = _split_arms_indices(...)` (ring.jl:415): the first two lists, however many there are
        if len(I1) < 2:
            raise ValueError(f"{where}an arm of the slice has fewer than 2 points")
        sel = np.array(I1) - 1
        arms.append(_process_ring_traces(m, spectrum, v_source, disc_velocity, rows[sel, 1], ρs[sel], rows[sel, 3], angles[sel], where))
    (lr, lt, le), (rr, rt, re_) = arms
    return LongitudalArms(float(β), lr, lt, le, rr, rt, re_)


def _arms_of_models(m, d, models, βs, *, spectrum=None, disc_velocity=None, ensemble=None, **kw):
    """the LongitudalArms of every slice of every ring: [ring][slice]"""
    βs = DEFAULT_β_ANGLES() if βs is None else np.ascontiguousarray(βs, dtype=np.float64)
    spectrum = PowerLawSpectrum(2.0) if spectrum is None else spectrum
    rows, counts, _, tracer = _arm_traces(m, d, models, βs, ensemble=ensemble, **kw)
    if isinstance(tracer, RingTracer):
        v_srcs = tracer.v_src
        disc_velocity = tracer.disc_velocity if disc_velocity is None else disc_velocity
    else:
        v_srcs = ring_frames(m, models)[2]
        disc_velocity = keplerian_velocity_projector(m, ensemble=ensemble) if disc_velocity is None else disc_velocity
    out = []
    for i in range(len(models)):
        arms = []
        for j, β in enumerate(βs):
            filled = int(counts[i, j].sum())
            arms.append(ring_arm(m, spectrum, v_srcs[i], disc_velocity, β, rows[i, j, :filled], where=f"ring {i}, slice {j}: "))
        out.append(arms)
    return out


def corona_arms(m, d, model, βs=None, *, n_samples=1000, extrema_iter=80, h=1e-7, λmax=1_000_000.0, chart=None, spectrum=None,
                ensemble=None, route="device", tracer=None, disc_velocity=None):
    """corona_arms(setup, m, d, model::RingCorona, βs) (ring.jl:456-484): the LongitudalArms of every β slice of the ring's sky
    (βs: DEFAULT_β_ANGLES(100); callback domain_upper_hemisphere(); chart: chart_for_metric(m, 1e6)).  Per slice N = n_samples -
    2 extrema_iter evenly spaced rays and two golden-section searches for the extrema of ρ.  route "device": gr_ring_arms, all
    slices' searches in lock-step on the device; "lockstep": the same logic in numpy over `tracer(ring, slice, angles) -> rows
    (g, ρ, t, status)` -- gr_ring_rays unless given.  `disc_velocity`: the disc's velocity projector (default: Keplerian with the
    traced plunging table)."""
    return _arms_of_models(m, d, [model], βs, spectrum=spectrum, disc_velocity=disc_velocity, tracer=tracer, ensemble=ensemble,
                           n_samples=n_samples, extrema_iter=extrema_iter, h=h, λmax=λmax, chart=chart, route=route)[0]


def _make_time_dependent_radial_emissivity(arms):
    """extended.jl:99-130 (weights of zeros, as there)"""
    w = np.zeros(len(arms))
    left = TimeDependentRadialDiscProfile(w, [a.left_r for a in arms], [a.left_t for a in arms], [a.left_ε for a in arms])
    right = TimeDependentRadialDiscProfile(w, [a.right_r for a in arms], [a.right_t for a in arms], [a.right_ε for a in arms])
    return RingCoronaProfile(left, right)


def ring_corona_profile(m, d, model, βs=None, **kwargs):
    """emissivity_profile(setup{true}, m, d, model::RingCorona; βs) (extended.jl:133-143) -> RingCoronaProfile; keywords: corona_arms'"""
    if not isinstance(model, RingCorona):
        raise TypeError("ring_corona_profile takes a RingCorona")
    return _make_time_dependent_radial_emissivity(corona_arms(m, d, model, βs, **kwargs))


def disc_corona_profile(m, d, model, βs=None, *, n_rings=10, n_samples=1000, extrema_iter=80, h=1e-7, λmax=1_000_000.0, chart=None,
                        spectrum=None, ensemble=None, route="device", tracer=None, disc_velocity=None):
    """emissivity_profile(setup{true}, m, d, model::DiscCorona; n_rings) (extended.jl:187-200) -> DiscCoronaProfile over the rings
    RingCorona(model.vf, r, model.h), r in linspace(1e-2, model.r, n_rings) -- all of them in ONE gr_ring_arms call."""
    if not isinstance(model, DiscCorona):
        raise TypeError("disc_corona_profile takes a DiscCorona")
    radii = np.linspace(1e-2, model.r, int(n_rings))
    models = [RingCorona(model.vf, float(r), model.h) for r in radii]
    per_ring = _arms_of_models(m, d, models, βs, spectrum=spectrum, disc_velocity=disc_velocity, tracer=tracer, ensemble=ensemble,
                               n_samples=n_samples, extrema_iter=extrema_iter, h=h, λmax=λmax, chart=chart, route=route)
    return DiscCoronaProfile(radii, [_make_time_dependent_radial_emissivity(arms) for arms in per_ring])
