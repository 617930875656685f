"""ctypes binding of libgradus_mi355x.so (the C ABI declared in include/gradus_mi355x.h).

There is deliberately no fallback: if the shared library is missing, or no gfx950 device is
present when a context is created, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GRADUS_MI355X_LIB selects another build of the same library (A/B timing of compiler flags)
LIB_PATH = os.environ.get("GRADUS_MI355X_LIB") or os.path.join(_HERE, "csrc", "libgradus_mi355x.so")



def kernel_source_sha16() -> str:
    """sha256[:16] over the kernel sources of the library in this tree with comments and white space removed (a
    comment edit is not a different kernel).  rocprofv3 summaries under profiles/ record it, and bench.py refuses to
    price a launch with counters taken from a different build of the kernels."""
    import hashlib
    import re

    h = hashlib.sha256()
    root = os.path.dirname(_HERE)
    for rel in ("gradus.jl_amd/csrc/gr_device.hpp", "gradus.jl_amd/csrc/gr_kernels.hpp", "gradus.jl_amd/csrc/gr_tangent.hpp",
                "gradus.jl_amd/csrc/gr_tabmetric.hpp", "gradus.jl_amd/csrc/gr_lagbin.hpp", "gradus.jl_amd/csrc/gr_tfint.hpp", "gradus.jl_amd/csrc/gr_tftd.hpp", "gradus.jl_amd/csrc/gr_stats_fold.hpp", "gradus.jl_amd/csrc/gr_tile_order.hpp", "gradus.jl_amd/csrc/metric_table.hip",
                "gradus.jl_amd/csrc/kernels_tu.hip",
                "gradus.jl_amd/csrc/gradus_mi355x.hip",
                "include/gradus_mi355x.h"):
        with open(os.path.join(root, rel), "r", encoding="utf-8") as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)      # block comments
        text = re.sub(r"//[^\n]*", " ", text)                    # line comments (no string literal here holds "//")
        h.update(" ".join(text.split()).encode("utf-8"))
    return h.hexdigest()[:16]


GR_OK = 0
ABI_VERSION = 8      # GR_ABI_VERSION of include/gradus_mi355x.h this module mirrors (checked in load() and tests/test_host_api.py)
ERROR_NAMES = {
    -1: "GR_ERR_INVALID_ARGUMENT",
    -2: "GR_ERR_UNSUPPORTED",
    -3: "GR_ERR_NO_DEVICE",
    -4: "GR_ERR_HIP",
    -5: "GR_ERR_OUT_OF_MEMORY",
}


class GradusMI355XError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


class gr_user_module_info_t(C.Structure):
    """What a compiled metric's kernel module says about itself (its `gr_user_module_info`)."""

    _fields_ = [("abi_version", C.c_int32), ("metric_id", C.c_int32), ("build_id", C.c_int64), ("header_hash", C.c_int64 * 4)]


class gr_metric_resources(C.Structure):
    _fields_ = [("vgprs", C.c_int32), ("scratch_bytes", C.c_int32), ("lds_bytes", C.c_int32), ("max_threads", C.c_int32)]


GR_METRIC_COMPILED = 12
GR_METRIC_MODULE_SLOTS = 16
MODULE_KERNELS = ("trace_lane", "trace_persistent", "tangent", "tangent_pairs")      # GR_MODULE_KERNEL_*


class gr_disc_component(C.Structure):
    _fields_ = [("disc_id", C.c_int32), ("_pad", C.c_int32), ("disc_r_in", C.c_double), ("disc_r_out", C.c_double),
                ("disc_params", C.c_double * 4)]


GR_COMP_MAX = 4


class gr_config(C.Structure):
    _fields_ = [
        ("metric_id", C.c_int32),
        ("disc_id", C.c_int32),
        ("params", C.c_double * 8),
        ("r_inner", C.c_double),
        ("r_outer", C.c_double),
        ("disc_r_in", C.c_double),
        ("disc_r_out", C.c_double),
        ("gtol", C.c_double),
        ("lambda0", C.c_double),
        ("lambda1", C.c_double),
        ("abstol", C.c_double),
        ("reltol", C.c_double),
        ("mu", C.c_double),
        ("maxiters", C.c_int64),
        ("upper_hemisphere", C.c_int32),
        ("_pad", C.c_int32),
        ("hemi_delta", C.c_double),
        ("disc_params", C.c_double * 4),
        ("disc_table", C.c_void_p),
        ("disc_table_n", C.c_int64),
        ("chart_table", C.c_void_p),
        ("chart_table_n", C.c_int64),
        ("chart_theta0", C.c_double),
        ("chart_theta1", C.c_double),
        ("q", C.c_double),
        ("count_windings", C.c_int32),
        ("_pad2", C.c_int32),
        ("winding_plane", C.c_double),
        ("comp_n", C.c_int32),
        ("_pad3", C.c_int32),
        ("comp", gr_disc_component * GR_COMP_MAX),
        ("metric_table", C.c_void_p),      # GR_METRIC_TABULATED (ABI 7): the table gr_metric_table_fit wrote, host pointer
        ("metric_table_n", C.c_int64),
    ]


GR_METRIC_MAX_SEG = 12


class gr_metric_break(C.Structure):
    """A radius where metric_components changes form (scale 0), or the centre of a feature that narrow (scale > 0)."""

    _fields_ = [("radius", C.c_double), ("scale", C.c_double)]


class gr_metric_segment(C.Structure):
    _fields_ = [
        ("r_lo", C.c_double),
        ("r_hi", C.c_double),
        ("anchor", C.c_double),
        ("xmin", C.c_double),
        ("fit_lo", C.c_double),
        ("fit_hi", C.c_double),
        ("e_lo", C.c_int32),
        ("e_hi", C.c_int32),
        ("first_row", C.c_int32),
        ("n_rows", C.c_int32),
        ("dir", C.c_int32),
        ("core", C.c_int32),
    ]


class gr_metric_grid(C.Structure):
    """Patch grid of a tabulated metric (include/gradus_mi355x.h, "tabulated metrics")."""

    _fields_ = [
        ("r0", C.c_double),
        ("r_min", C.c_double),
        ("r_max", C.c_double),
        ("e_min", C.c_int32),
        ("n_oct", C.c_int32),
        ("m_r", C.c_int32),
        ("n_theta", C.c_int32),
        ("degree", C.c_int32),
        ("fit_nodes", C.c_int32),
        ("pole_factor", C.c_int32),
        ("n_seg", C.c_int32),
        ("n_r_nodes", C.c_int64),
        ("n_theta_nodes", C.c_int64),
        ("table_doubles", C.c_int64),
        ("n_rows", C.c_int32),
        ("reserved", C.c_int32),
        ("seg", gr_metric_segment * GR_METRIC_MAX_SEG),
    ]


class gr_plane(C.Structure):
    _fields_ = [
        ("x_obs", C.c_double * 4),
        ("Mx", C.c_double * 16),
        ("alpha0", C.c_double),
        ("alpha1", C.c_double),
        ("beta0", C.c_double),
        ("beta1", C.c_double),
        ("width", C.c_int64),
        ("height", C.c_int64),
        ("offset", C.c_double),
    ]


class gr_range(C.Structure):
    _fields_ = [("first", C.c_int64), ("count", C.c_int64), ("block", C.c_int64), ("stride_blocks", C.c_int64)]


class gr_pointfunction(C.Structure):
    _fields_ = [
        ("pf_id", C.c_int32),
        ("filter_id", C.c_int32),
        ("fill", C.c_double),
        ("r_isco", C.c_double),
        ("n_plunge", C.c_int64),
        ("plunge_r", C.POINTER(C.c_double)),
        ("plunge_vt", C.POINTER(C.c_double)),
        ("plunge_vr", C.POINTER(C.c_double)),
        ("plunge_vphi", C.POINTER(C.c_double)),
        ("has_u_src", C.c_int32),
        ("_pad_u", C.c_int32),
        ("u_src", C.c_double * 4),
    ]


class gr_transfer(C.Structure):
    """TraceRadiativeTransfer's launch-uniform block: ν₀, I₀, the power-law medium and the ISCO (include/gradus_mi355x.h)"""

    _fields_ = [(k, C.c_double) for k in ("nu0", "I0", "a0", "j0", "pa", "pj", "sa", "sj", "r_isco", "reserved")]


class gr_rayset(C.Structure):
    _fields_ = [
        ("x_obs", C.c_double * 4),
        ("Mx", C.c_double * 16),
        ("alpha", C.c_void_p),
        ("beta", C.c_void_p),
        ("area", C.c_void_p),
        ("n", C.c_int64),
        ("height", C.c_void_p),
        ("sep_r", C.c_void_p),
        ("sep_cos", C.c_void_p),
        ("sep_sin", C.c_void_p),
        ("sep_nr", C.c_int64),
        ("sep_nt", C.c_int64),
        ("sep_tiled", C.c_int32),
        ("sep_reserved", C.c_int32),
        ("sep_first", C.c_int64),
        ("sep_block", C.c_int64),
        ("sep_stride", C.c_int64),
        ("sky_sampler", C.c_int32),
        ("sky_both", C.c_int32),
        ("sky_generator", C.c_int32),
        ("sky_reserved", C.c_int32),
        ("sky_resolution", C.c_double),
        ("sky_i", C.c_void_p),
        ("sky_first", C.c_int64),          # ABI 8: a share of a source's samples (the *_multi entry points set them per context)
        ("sky_total", C.c_int64),
        ("sky_rows", C.c_void_p),          # ABI 8: a source without one position: 28 doubles per ray (x, Mx, lowered source velocity, g_tμ)
    ]


class gr_offset_problems(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("r_target", C.c_void_p),
        ("cos_theta", C.c_void_p),
        ("sin_theta", C.c_void_p),
        ("height", C.c_void_p),
        ("alpha0", C.c_double),
        ("beta0", C.c_double),
        ("zero_atol", C.c_double),
        ("r_min", C.c_double),
        ("max_iter", C.c_int64),
        ("contrapoint_bias", C.c_double),
        ("per_wave", C.c_int64),
    ]


class gr_offset_searches(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("r_target", C.c_void_p),
        ("lower", C.c_void_p),
        ("upper", C.c_void_p),
        ("sign", C.c_void_p),
        ("height", C.c_void_p),
        ("alpha0", C.c_double),
        ("beta0", C.c_double),
        ("zero_atol", C.c_double),
        ("r_min", C.c_double),
        ("max_iter", C.c_int64),
        ("contrapoint_bias", C.c_double),
        ("per_wave", C.c_int64),
        ("iterations", C.c_int64),
    ]


class gr_binning(C.Structure):
    _fields_ = [
        ("r_min", C.c_double),
        ("r_max", C.c_double),
        ("emissivity_index", C.c_double),
        ("n_bins", C.c_int64),
        ("bin_edges", C.c_void_p),
        ("eps_r", C.c_void_p),
        ("eps_v", C.c_void_p),
        ("eps_n", C.c_int64),
    ]


class gr_lagprofile(C.Structure):
    """What turns a row (g, ρ, t, area) of gr_lagtransfer_trace into (E, t, f): the line's energy, ε(ρ) as gr_binning has it and
    the coordtime_at table."""

    _fields_ = [
        ("E0", C.c_double),
        ("emissivity_index", C.c_double),
        ("eps_r", C.c_void_p),
        ("eps_v", C.c_void_p),
        ("eps_n", C.c_int64),
        ("time_r", C.c_void_p),
        ("time_v", C.c_void_p),
        ("time_n", C.c_int64),
    ]


class gr_tfset(C.Structure):
    """One parameter set of gr_tf_lineprofile / gr_tf_lagtransfer: the branches of n_r emission radii (ragged knots behind
    `off`) and the annuli of the integration with ε and the source -> disc time evaluated at each."""

    _fields_ = [
        ("n_r", C.c_int64),
        ("radii", C.c_void_p),
        ("gmin", C.c_void_p),
        ("gmax", C.c_void_p),
        ("off", C.c_void_p),
        ("knot_g", C.c_void_p),
        ("knot_f", C.c_void_p),
        ("knot_t", C.c_void_p),
        ("n_int", C.c_int64),
        ("r_int", C.c_void_p),
        ("eps_int", C.c_void_p),
        ("tsd_int", C.c_void_p),
        ("r_min", C.c_double),
        ("g_scale", C.c_double),
    ]


class gr_tfquad(C.Structure):
    """integrate_bin's edge width and the quadrature rule on [-1, 1]"""

    _fields_ = [("h", C.c_double), ("n_q", C.c_int64), ("x", C.c_void_p), ("w", C.c_void_p)]


class gr_tfprofile(C.Structure):
    """The time-dependent emissivity of gr_tf_lagtransfer_td: rings of two arms, an arm a run of curves (ρ, t, ε)"""

    _fields_ = [
        ("n_rings", C.c_int64),
        ("ring_weight", C.c_void_p),
        ("ring_dt", C.c_void_p),
        ("arm_off", C.c_void_p),
        ("curve_off", C.c_void_p),
        ("knot_r", C.c_void_p),
        ("knot_t", C.c_void_p),
        ("knot_e", C.c_void_p),
    ]


class gr_ringset(C.Structure):
    """The rings of gr_ring_rays / gr_ring_arms: per ring a frame of 28 doubles, the slices' angles β, a slice's base angles"""

    _fields_ = [
        ("n_rings", C.c_int64),
        ("n_slices", C.c_int64),
        ("n_base", C.c_int64),
        ("extrema_iter", C.c_int64),
        ("frames", C.c_void_p),
        ("betas", C.c_void_p),
        ("base_angles", C.c_void_p),
    ]


class gr_skycells(C.Structure):
    """The cells of a source's adaptive sky (gr_sky_cells): the source's position and sky frame, per cell cos θ and ϕ"""

    _fields_ = [
        ("x_src", C.c_double * 4),
        ("Mx", C.c_double * 16),
        ("cos_theta", C.c_void_p),
        ("phi", C.c_void_p),
        ("n", C.c_int64),
    ]


GR_SKY_MAX_BOXES = 8
GR_SKY_CRIT_DEFAULT, GR_SKY_CRIT_FUNCTION, GR_SKY_CRIT_FINE, GR_SKY_CRIT_LEVEL, GR_SKY_CRIT_PLANE = 0, 1, 2, 3, 4
GR_SKY_MAP_EMISSIVITY, GR_SKY_MAP_REDSHIFT, GR_SKY_MAP_TIME = 0, 1, 2


class gr_sky_box(C.Structure):
    """An r interval and zero, one or two intervals of mod(ϕ, 2π), every bound open or closed (gr_sky_criterion)"""

    _fields_ = [
        ("r_lo", C.c_double),
        ("r_hi", C.c_double),
        ("phi_lo", C.c_double * 2),
        ("phi_hi", C.c_double * 2),
        ("r_open_lo", C.c_int32),
        ("r_open_hi", C.c_int32),
        ("phi_open_lo", C.c_int32),
        ("phi_open_hi", C.c_int32),
        ("n_phi", C.c_int32),
        ("reserved", C.c_int32),
    ]


class gr_sky_criterion(C.Structure):
    """A pair criterion of a resident adaptive sky (gr_sky_find_need_refine)"""

    _fields_ = [
        ("kind", C.c_int32),
        ("level", C.c_int32),
        ("rtol", C.c_double),
        ("n_boxes", C.c_int32),
        ("reserved", C.c_int32),
        ("boxes", gr_sky_box * GR_SKY_MAX_BOXES),
    ]


class gr_stats(C.Structure):
    _fields_ = [
        ("rays", C.c_int64),
        ("accepted_steps", C.c_int64),
        ("rejected_steps", C.c_int64),
        ("rhs_evals", C.c_int64),
        ("flagged_rays", C.c_int64),
        ("status_count", C.c_int64 * 4),
        ("kernel_ms", C.c_double),     # host variants: start of the call's device work -> end of its last trace kernel
        ("call_ms", C.c_double),       # ... -> end of the last copy into the caller's buffer (ABI 5)
        ("enqueue_ms", C.c_double),    # *_multi: host time spent enqueueing this context's share (ABI 6); 0 elsewhere
    ]

    def asdict(self):
        return {
            "rays": self.rays,
            "accepted_steps": self.accepted_steps,
            "rejected_steps": self.rejected_steps,
            "rhs_evals": self.rhs_evals,
            "flagged_rays": self.flagged_rays,
            "status_count": list(self.status_count),
            "kernel_ms": self.kernel_ms,
            "call_ms": self.call_ms,
            "enqueue_ms": self.enqueue_ms,
        }


# GeodesicPoint{Float64,Nothing}: 152 bytes (src/solution-processing.jl:15-32)
POINT_DTYPE = np.dtype(
    [
        ("status", np.int32),
        ("flags", np.int32),
        ("lambda_min", np.float64),
        ("lambda_max", np.float64),
        ("x_init", np.float64, (4,)),
        ("x", np.float64, (4,)),
        ("v_init", np.float64, (4,)),
        ("v", np.float64, (4,)),
    ],
    align=True,
)
assert POINT_DTYPE.itemsize == 152

# every symbol include/gradus_mi355x.h declares
EXPORTS = [
    "gr_metric_module_load",
    "gr_metric_module_unload",
    "gr_metric_module_build_id",
    "gr_metric_module_resources",
    "gr_abi_version",
    "gr_last_error",
    "gr_ctx_create",
    "gr_ctx_destroy",
    "gr_ctx_set",
    "gr_host_alloc",
    "gr_host_free",
    "gr_render_device",
    "gr_render",
    "gr_render_multi",
    "gr_render_endpoints_device",
    "gr_render_endpoints",
    "gr_trace_endpoints_device",
    "gr_trace_endpoints",
    "gr_trace_path",
    "gr_trace_paths",
    "gr_lineprofile_device",
    "gr_lineprofile",
    "gr_redshift_radius_device",
    "gr_redshift_radius",
    "gr_ray_summary_device",
    "gr_ray_summary",
    "gr_ray_tangent_device",
    "gr_ray_tangent",
    "gr_offset_solve_device",
    "gr_offset_solve",
    "gr_offset_search_device",
    "gr_offset_search",
    "gr_rayset_endpoints_device",
    "gr_rayset_endpoints",
    "gr_apply_pointfunction_device",
    "gr_apply_pointfunction",
    "gr_corona_trace",
    "gr_corona_bin",
    "gr_corona_trace_multi",
    "gr_corona_bin_multi",
    "gr_lagtransfer_trace",
    "gr_lagtransfer_extrema",
    "gr_lagtransfer_bin",
    "gr_lagtransfer_rows",
    "gr_tf_lineprofile",
    "gr_tf_lagtransfer",
    "gr_tf_lagtransfer_td",
    "gr_ring_rays",
    "gr_ring_arms",
    "gr_sky_cells",
    "gr_sky_cells_device",
    "gr_sky_cells_multi",
    "gr_sky_create",
    "gr_sky_destroy",
    "gr_sky_size",
    "gr_sky_trace_initial",
    "gr_sky_find_need_refine",
    "gr_sky_need_refine_list",
    "gr_sky_pairs",
    "gr_sky_refine_and_trace",
    "gr_sky_occupancy",
    "gr_sky_download",
    "gr_disc_area_factor_device",
    "gr_disc_area_factor",
    "gr_sky_bin_grid",
    "gr_sky_fill",
    "gr_plane_cells",
    "gr_plane_cells_device",
    "gr_plane_cells_multi",
    "gr_sky_create_plane",
    "gr_sky_download_points",
    "gr_sky_fill_plane",
    "gr_render_endpoints_multi",
    "gr_trace_endpoints_multi",
    "gr_rayset_endpoints_multi",
    "gr_ray_summary_multi",
    "gr_ray_tangent_multi",
    "gr_offset_solve_multi",
    "gr_offset_search_multi",
    "gr_redshift_radius_multi",
    "gr_lineprofile_multi",
    "gr_metric_grid_plan",
    "gr_metric_grid_plan_breaks",
    "gr_metric_grid_nodes",
    "gr_metric_table_fit",
    "gr_metric_table_eval",
    "gr_transfer_render_device",
    "gr_transfer_render",
    "gr_transfer_endpoints",
]

_lib = None


def load():
    """Load the shared library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GradusMI355XError(
            -3, f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.gr_abi_version.restype = i32
    # the structs below are laid out for ONE version of include/gradus_mi355x.h: a library of another version (an older
    # build named by GRADUS_MI355X_LIB, a variant of scripts/build_variant.sh) would read them wrongly without any error
    if L.gr_abi_version() != ABI_VERSION:
        raise GradusMI355XError(-1, f"{LIB_PATH} has ABI version {L.gr_abi_version()}, this binding is written for {ABI_VERSION}")
    L.gr_last_error.restype = C.c_char_p
    L.gr_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.gr_ctx_destroy.argtypes = [vp]
    L.gr_ctx_set.argtypes = [vp, C.c_char_p, i64]
    L.gr_host_alloc.argtypes = [vp, i64, C.POINTER(vp)]
    L.gr_host_free.argtypes = [vp, vp]
    cfgp, plp, pfp, rgp, stp = (C.POINTER(t) for t in (gr_config, gr_plane, gr_pointfunction, gr_range, gr_stats))
    L.gr_render_device.argtypes = [vp, cfgp, plp, pfp, rgp, vp, vp, vp]
    L.gr_render.argtypes = [vp, cfgp, plp, pfp, rgp, vp, stp]
    L.gr_render_multi.argtypes = [C.POINTER(vp), i32, cfgp, plp, pfp, i64, vp, vp]
    L.gr_render_endpoints_device.argtypes = [vp, cfgp, plp, rgp, vp, vp, vp]
    L.gr_render_endpoints.argtypes = [vp, cfgp, plp, rgp, vp, stp]
    L.gr_trace_endpoints_device.argtypes = [vp, cfgp, vp, i64, vp, i64, vp, vp, vp]
    L.gr_trace_endpoints.argtypes = [vp, cfgp, vp, i64, vp, i64, vp, stp]
    trp = C.POINTER(gr_transfer)
    L.gr_transfer_render_device.argtypes = [vp, cfgp, trp, plp, pfp, rgp, vp, vp, vp]
    L.gr_transfer_render.argtypes = [vp, cfgp, trp, plp, pfp, rgp, vp, stp]
    L.gr_transfer_endpoints.argtypes = [vp, cfgp, trp, vp, i64, vp, i64, vp, vp, stp]
    L.gr_trace_path.argtypes = [vp, cfgp, vp, vp, i64, vp, C.POINTER(i64), vp]
    L.gr_trace_paths.argtypes = [vp, cfgp, vp, i64, vp, i64, i64, vp, vp, vp]
    rsp, bnp = C.POINTER(gr_rayset), C.POINTER(gr_binning)
    L.gr_lineprofile_device.argtypes = [vp, cfgp, rsp, pfp, bnp, vp, vp, vp]
    L.gr_lineprofile.argtypes = [vp, cfgp, rsp, pfp, bnp, vp, stp]
    L.gr_redshift_radius_device.argtypes = [vp, cfgp, rsp, pfp, C.c_double, C.c_double, vp, vp, vp]
    L.gr_redshift_radius.argtypes = [vp, cfgp, rsp, pfp, C.c_double, C.c_double, vp, stp]
    L.gr_ray_summary_device.argtypes = [vp, cfgp, rsp, pfp, vp, vp, vp]
    L.gr_ray_summary.argtypes = [vp, cfgp, rsp, pfp, vp, stp]
    L.gr_ray_tangent_device.argtypes = [vp, cfgp, rsp, pfp, vp, vp, vp]
    L.gr_ray_tangent.argtypes = [vp, cfgp, rsp, pfp, vp, stp]
    opp, osp = C.POINTER(gr_offset_problems), C.POINTER(gr_offset_searches)
    L.gr_offset_solve_device.argtypes = [vp, cfgp, rsp, pfp, opp, vp, vp, vp]
    L.gr_offset_solve.argtypes = [vp, cfgp, rsp, pfp, opp, vp, stp]
    L.gr_offset_search_device.argtypes = [vp, cfgp, rsp, pfp, osp, vp, vp, vp]
    L.gr_offset_search.argtypes = [vp, cfgp, rsp, pfp, osp, vp, stp]
    L.gr_offset_solve_multi.argtypes = [C.POINTER(vp), i32, cfgp, rsp, pfp, opp, vp, vp]
    L.gr_offset_search_multi.argtypes = [C.POINTER(vp), i32, cfgp, rsp, pfp, osp, vp, vp]
    L.gr_rayset_endpoints_device.argtypes = [vp, cfgp, rsp, vp, vp, vp]
    L.gr_rayset_endpoints.argtypes = [vp, cfgp, rsp, vp, stp]
    L.gr_apply_pointfunction_device.argtypes = [vp, cfgp, pfp, vp, i64, C.c_double, vp, vp]
    L.gr_apply_pointfunction.argtypes = [vp, cfgp, pfp, vp, i64, C.c_double, vp]
    L.gr_corona_trace.argtypes = [vp, cfgp, rsp, pfp, vp, C.POINTER(C.c_int64), stp]
    L.gr_corona_bin.argtypes = [vp, vp, i64, vp]
    L.gr_corona_trace_multi.argtypes = [vp, i32, cfgp, rsp, pfp, vp, C.POINTER(C.c_int64), stp]
    L.gr_corona_bin_multi.argtypes = [vp, i32, vp, i64, vp]
    lpp = C.POINTER(gr_lagprofile)
    L.gr_lagtransfer_trace.argtypes = [vp, cfgp, rsp, pfp, C.POINTER(C.c_int64), stp]
    L.gr_lagtransfer_extrema.argtypes = [vp, lpp, vp, vp]
    L.gr_lagtransfer_bin.argtypes = [vp, lpp, vp, i64, vp, i64, vp]
    L.gr_lagtransfer_rows.argtypes = [vp, vp]
    tsp, tqp = C.POINTER(gr_tfset), C.POINTER(gr_tfquad)
    L.gr_tf_lineprofile.argtypes = [vp, tsp, i64, tqp, vp, i64, vp]
    L.gr_tf_lagtransfer.argtypes = [vp, tsp, i64, tqp, vp, i64, vp, i64, vp]
    L.gr_tf_lagtransfer_td.argtypes = [vp, tsp, C.POINTER(gr_tfprofile), tqp, vp, i64, vp, i64, i64, i64, C.c_double, vp, vp]
    L.gr_ring_rays.argtypes = [vp, cfgp, C.POINTER(gr_ringset), pfp, i64, vp, vp, vp, vp, stp]
    L.gr_ring_arms.argtypes = [vp, cfgp, C.POINTER(gr_ringset), pfp, vp, vp, stp]
    scp = C.POINTER(gr_skycells)
    L.gr_sky_cells.argtypes = [vp, cfgp, scp, pfp, vp, stp]
    L.gr_sky_cells_device.argtypes = [vp, cfgp, scp, pfp, vp, vp, vp]
    ctxa = C.POINTER(vp)
    L.gr_sky_cells_multi.argtypes = [ctxa, i32, cfgp, scp, pfp, vp, vp]
    i64p = C.POINTER(i64)
    L.gr_sky_create.argtypes = [vp, cfgp, scp, pfp, vp, i32, C.POINTER(vp)]
    L.gr_sky_destroy.argtypes = [vp]
    L.gr_sky_size.argtypes = [vp, i64p]
    L.gr_sky_trace_initial.argtypes = [vp, i32, vp]
    L.gr_sky_find_need_refine.argtypes = [vp, C.POINTER(gr_sky_criterion), i64p]
    L.gr_sky_need_refine_list.argtypes = [vp, vp]
    L.gr_sky_pairs.argtypes = [vp, vp, vp, i64, i64p]
    L.gr_sky_refine_and_trace.argtypes = [vp, vp, i64, i64p, stp]
    L.gr_sky_occupancy.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    L.gr_sky_download.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gr_disc_area_factor_device.argtypes = [vp, cfgp, pfp, vp, i64, vp, vp]
    L.gr_disc_area_factor.argtypes = [vp, cfgp, pfp, vp, i64, vp]
    L.gr_sky_bin_grid.argtypes = [vp, i32, vp, i64, vp, i64, vp, vp, vp]
    L.gr_sky_fill.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    L.gr_plane_cells.argtypes = [vp, cfgp, plp, vp, vp, i64, vp, stp]
    L.gr_plane_cells_device.argtypes = [vp, cfgp, plp, vp, vp, i64, vp, vp, vp]
    L.gr_plane_cells_multi.argtypes = [ctxa, i32, cfgp, plp, vp, vp, i64, vp, vp]
    L.gr_sky_create_plane.argtypes = [vp, cfgp, plp, vp, i32, C.POINTER(vp)]
    L.gr_sky_download_points.argtypes = [vp, i64, i64, vp]
    L.gr_sky_fill_plane.argtypes = [vp, pfp, vp, vp, i64, vp, i64, vp, vp]
    L.gr_render_endpoints_multi.argtypes = [ctxa, i32, cfgp, plp, i64, vp, vp]
    L.gr_trace_endpoints_multi.argtypes = [ctxa, i32, cfgp, vp, i64, vp, i64, vp, vp]
    L.gr_rayset_endpoints_multi.argtypes = [ctxa, i32, cfgp, rsp, vp, vp]
    L.gr_ray_summary_multi.argtypes = [ctxa, i32, cfgp, rsp, pfp, vp, vp]
    L.gr_ray_tangent_multi.argtypes = [ctxa, i32, cfgp, rsp, pfp, vp, vp]
    L.gr_redshift_radius_multi.argtypes = [ctxa, i32, cfgp, rsp, pfp, C.c_double, C.c_double, vp, vp]
    L.gr_lineprofile_multi.argtypes = [ctxa, i32, cfgp, rsp, pfp, bnp, vp, vp]
    gdp, dp = C.POINTER(gr_metric_grid), C.POINTER(C.c_double)
    L.gr_metric_grid_plan.argtypes = [C.c_double, C.c_double, C.c_double, i32, i32, gdp]
    L.gr_metric_grid_plan_breaks.argtypes = [C.c_double, C.c_double, C.c_double, i32, i32, i32, C.POINTER(gr_metric_break), gdp]
    L.gr_metric_grid_nodes.argtypes = [gdp, vp, vp]
    L.gr_metric_table_fit.argtypes = [gdp, vp, vp, dp]
    L.gr_metric_table_eval.argtypes = [vp, i64, C.c_double, C.c_double, dp, dp, dp]
    L.gr_metric_module_load.argtypes = [C.c_char_p, C.POINTER(i64)]
    L.gr_metric_module_unload.argtypes = [i32]
    L.gr_metric_module_build_id.argtypes = [i32, C.POINTER(i64)]
    L.gr_metric_module_resources.argtypes = [i32, cfgp, C.POINTER(gr_metric_resources)]
    for name in EXPORTS:
        if name not in ("gr_last_error",):
            getattr(L, name).restype = i32
    L.gr_last_error.restype = C.c_char_p
    _lib = L
    return L


def check(code):
    if code != GR_OK:
        raise GradusMI355XError(code, load().gr_last_error().decode("utf-8", "replace"))


def ctx_array(ctxs):
    """(ctypes array of the contexts' handles, array of gr_stats, one per context) for a *_multi call."""
    arr = (C.c_void_p * len(ctxs))(*[c.handle for c in ctxs])
    return arr, (gr_stats * len(ctxs))()


def merge_stats(sts) -> gr_stats:
    """One gr_stats for a *_multi call: counters summed over the contexts, times = the slowest context
    (they run side by side), enqueue_ms = the sum (the host enqueues them one after another)."""
    st = gr_stats()
    for f in ("rays", "accepted_steps", "rejected_steps", "rhs_evals", "flagged_rays"):
        setattr(st, f, sum(getattr(x, f) for x in sts))
    for q in range(4):
        st.status_count[q] = sum(x.status_count[q] for x in sts)
    st.kernel_ms = max(x.kernel_ms for x in sts)
    st.call_ms = max(x.call_ms for x in sts)
    st.enqueue_ms = sum(x.enqueue_ms for x in sts)
    return st


class PinnedBlock:
    """A result buffer the LIBRARY page-locked (gr_host_alloc, ABI 5): what the Julia shim wraps as its
    Vector{GeodesicPoint} so that 152 B per ray come back by DMA under the trace instead of through the pageable path.
    `array(dtype, count)` views it as a numpy array that keeps the block alive; the block is returned when the last view
    is gone (gr_host_free needs no context)."""

    def __init__(self, ctx, nbytes: int):
        p = C.c_void_p()
        check(load().gr_host_alloc(ctx.handle, int(nbytes), C.byref(p)))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def array(self, dtype, count: int):
        buf = (C.c_char * self.nbytes).from_address(self.ptr)
        buf._pinned_block = self                      # the view keeps the block alive
        return np.frombuffer(buf, dtype=dtype, count=count)

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                load().gr_host_free(None, C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


PINNED_RESULT_MIN_BYTES = 64 << 20


def result_points(ctx, n: int):
    """The array an end-point call fills: pinned by the library from 64 MiB up (GRADUS_MI355X_PINNED_RESULTS=0: never),
    an ordinary numpy array below that or when page-locking is refused."""
    nbytes = int(n) * POINT_DTYPE.itemsize
    if nbytes >= PINNED_RESULT_MIN_BYTES and os.environ.get("GRADUS_MI355X_PINNED_RESULTS", "1") != "0":
        try:
            return PinnedBlock(ctx, nbytes).array(POINT_DTYPE, int(n))
        except GradusMI355XError:
            pass
    return np.zeros(int(n), dtype=POINT_DTYPE)


PINNED_IMAGE_MIN_BYTES = 8 << 20


def result_image(ctx, n: int):
    """The image a fused render fills: from 8 MiB up a block the library page-locked (registered huge pages, taken from the
    pool of freed blocks when one fits), which the kernel writes across the link itself -- no staging image in HBM, no copy;
    below that, or when page-locking is refused (or GRADUS_MI355X_PINNED_RESULTS=0), an ordinary numpy array."""
    nbytes = int(n) * 8
    if nbytes >= PINNED_IMAGE_MIN_BYTES and os.environ.get("GRADUS_MI355X_PINNED_RESULTS", "1") != "0":
        try:
            return PinnedBlock(ctx, nbytes).array(np.float64, int(n))
        except GradusMI355XError:
            pass
    return np.zeros(int(n))


class Context:
    """Owns one gr_ctx (one HIP device)."""

    def __init__(self, device: int = 0):
        self._lib = load()
        h = C.c_void_p()
        check(self._lib.gr_ctx_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)

    def set(self, key: str, value: int):
        check(self._lib.gr_ctx_set(self.handle, key.encode(), int(value)))
        return self

    def close(self):
        if getattr(self, "handle", None):
            self._lib.gr_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
