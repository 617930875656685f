"""gradus.jl_amd -- MI355X-native backend for Gradus.jl's image-plane render path.

Host-side mirror of the reference API (rendergeodesics / tracegeodesics / PointFunction /
AbstractMetric) over the C ABI of libgradus_mi355x.so (include/gradus_mi355x.h).  All per-ray
work runs in hand-written HIP kernels for gfx950; there is no CPU fallback.
"""
from . import _lib
from ._lib import Context, GradusMI355XError, POINT_DTYPE
from . import device, distributed
from . import corona, reverberation, transfer_functions
from .corona import (BeamedPointSource, BothHemispheres, CoronaGeodesics, DiscCorona, EvenGenerator, EvenSampler,
                     GoldenSpiralGenerator, LampPostModel, LowerHemisphere, PowerLawSpectrum, RadialDiscProfile, RingCorona,
                     SourceVelocities, DiscCoronaProfile, RingCoronaProfile, TimeDependentRadialDiscProfile,
                     emissivity_interp, emissivity_interp_limits,
                     RandomGenerator, WeierstrassSampler, coordtime_at, emissivity_at, emissivity_profile,
                     energy_ratio, lorentz_factor, sky_angles_to_velocity, tetradframe_matrix, tracecorona,
                     DEFAULT_β_ANGLES, LongitudalArms, corona_arm_traces, corona_arms, disc_corona_profile, ring_corona_profile)
from . import adaptive, grids
from .adaptive import (AdaptivePlane, AdaptiveSky, AxisLimits, RadialBox, StepBlockCodes, adaptive_solve, bin_emissivity_grid, bin_redshift_grid,
                       bin_time_grid, check_refine, check_refine_plane, empty_fraction, evaluate_refinement_metric, fill_sky_values, find_need_refine,
                       fine_refine_function, interpolate_emissivity_grid, refine_and_trace, refine_function, refine_plane,
                       refine_to_level,
                       step_block, trace_initial, trace_step, unpack_sky)
from .grids import AdaptiveGrid
from .distributed import gather_buffers, gather_image, gather_image_async, gather_points, shard_plan
from .geometry import (CompositeGeometry, DatumPlane, EllipticalDisc, MeshAccretionGeometry, PrecessingDisc, ShakuraSunyaev, ThickDisc,
                       ThinDisc, WarpedThinDisc, bounding_box)
from .polish_doughnut import PolishDoughnut
from .lineprofiles import BinningMethod, PowerLawEmissivity, TransferFunctionMethod, bucket_simple, lineprofile
from .metrics import (BumblebeeMetric, DilatonAxion, JohannsenMetric, JohannsenPsaltisMetric, KerrDarkMatter, KerrMetric,
                      KerrNewmanMetric, KerrRefractive, MorrisThorneWormhole, NoZMetric, SphericalMetric, TabulatedMetric, inner_radius, isco)
from .compiled_metric import CompiledMetric, UntraceableMetric
from .orthonormalization import lnrbasis, lnrbasis_matrix, lnrframe, lnrframe_matrix
from .planes import (CartesianPlane, GeometricGrid, InverseGrid, LinearGrid, PolarPlane, image_plane,
                     impact_parameters, trajectory_count, unnormalized_areas)
from .pointfunctions import ConstPointFunctions, FilterPointFunction, FilterStatusCode, PointFunction
from .rendering import (EndpointRenderCache, apply, impact_axes, prerendergeodesics, render_configuration,
                        render_into_image, rendergeodesics)
from .status import StatusCodes
from .tracing import (EnsembleMI355X, TraceGeodesic, TraceWindings, TraceRadiativeTransfer, PowerLawMedium, winding_number, PolarChart, PoloidalShapeChart, TracingConfiguration, chart_for_metric,
                      domain_upper_hemisphere, event_horizon, event_horizon_chart, is_naked_singularity,
                      ensemble_solve_tracing_problem, local_momentum, lnr_momentum_to_global_velocity_transform,
                      map_impact_parameters, tracegeodesic_path, tracegeodesic_paths, tracegeodesics, tracing_configuration)
from .transfer_functions import (CunninghamTransferData, CunninghamTransferGrid, CunninghamTransferTable,
                                make_transfer_function_table, transfer_function_grid, InterpolatingTransferBranches, TransferBranches,
                                cunningham_transfer_function, cunningham_transfer_functions, integrate_lagtransfer,
                                integrate_lineprofile, integrate_lineprofiles,
                                interpolate_branches, splitbranches, time_dependent_emissivity_table, transferfunctions)
from .reverberation import (AnalyticRadialDiscProfile, DeviceLagTransfer, LagTransferFunction, bin_transfer_function, binflux,
                            continuum_time, lag_frequency,
                            lagtransfer, lagtransfer_device, observer_to_disc)
from .orbit_solving import (measure_stability, solve_equatorial_circular_orbit, trace_equatorial_circular_orbit,
                            trace_single_orbit)
from .precision_solvers import (find_offset_for_radius, impact_parameters_for_radius, impact_parameters_for_radius_obscured,
                                impact_parameters_for_target, jacobian_αβ_gr, optimize_for_target)
from .special_radii import (CircularOrbits, PlungingInterpolation, generic_isco, interpolate_plunging_velocities,
                            plunging_fourvelocity)

__all__ = [n for n in dir() if not n.startswith("_")]

interpolate_redshift = ConstPointFunctions.interpolate_redshift


# ---- small pieces of the reference's exported surface (src/Gradus.jl exports) ----
def metric_components(m, rθ):
    """metric_components(m, rθ): (g_tt, g_rr, g_θθ, g_ϕϕ, g_tϕ)"""
    return m.metric_components(rθ[0], rθ[1])


def cross_section(d, ρ):
    """cross_section(d::AbstractThickAccretionDisc, ρ) (geometry/discs.jl:27-53)"""
    return d.cross_section(ρ)


def g_to_g_star(g, gmin, gmax):
    """g_to_g✶ (transfer-functions/utils.jl): (g - gmin) / (gmax - gmin)"""
    return (g - gmin) / (gmax - gmin)


def g_star_to_g(g_star, gmin, gmax):
    """g✶_to_g: (gmax - gmin) g✶ + gmin"""
    return (gmax - gmin) * g_star + gmin


def minkowski_matrix():
    """minkowski_matrix() (metrics/minkowski.jl:36-41)"""
    import numpy as _np

    return _np.diag([-1.0, 1.0, 1.0, 1.0])


def spherical_to_cartesian(v):
    """spherical_to_cartesian((r, θ, ϕ)) -> (x, y, z)"""
    import numpy as _np

    r, θ, ϕ = v[-3], v[-2], v[-1]
    return _np.array([r * _np.sin(θ) * _np.cos(ϕ), r * _np.sin(θ) * _np.sin(ϕ), r * _np.cos(θ)])


def cartesian_squared_distance(m, x1, x2):
    """cartesian_squared_distance(m, x1, x2) (geometry/geometry.jl): squared Euclidean distance of two four-positions
    in the coordinates' own (r, θ, ϕ)"""
    import numpy as _np

    return float(_np.sum((spherical_to_cartesian(x1) - spherical_to_cartesian(x2)) ** 2))


def cartesian_distance(m, x1, x2):
    return cartesian_squared_distance(m, x1, x2) ** 0.5


def unpack_solution(points):
    """unpack_solution(sol): the device entry points already return GeodesicPoint records."""
    return points


__all__ = [n for n in dir() if not n.startswith("_")]
