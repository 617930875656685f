/*
 * gradus_mi355x.h -- C ABI of libgradus_mi355x.so, the MI355X (gfx950) backend for the
 * image-plane render path of Gradus.jl.
 *
 * Drop-in boundary: Gradus.ensemble_solve_tracing_problem(ensemble, problem, config)
 * (reference: src/tracing/tracing.jl:113-196; the DiffEqGPU extension overloads the same
 * method at ext/GradusDiffEqGPUExt/GradusDiffEqGPUExt.jl:10-31).  A Julia method for a new
 * ensemble type `EnsembleMI355X` ccall's the entry points below (binding shown in
 * INTEGRATION.md); everything under the boundary -- constrain_all, the Tsit5 integration
 * of the second-order geodesic ODE with chart / disc callbacks, unpack_solution and the
 * built-in PointFunctions -- runs in hand-written HIP kernels.
 *
 * Conventions
 *   - every function returns 0 on success or a negative gr_status; nothing throws;
 *     gr_last_error() returns a thread-local message for the last failure.
 *   - "_device" entry points take DEVICE pointers and a hipStream_t (as void*) and are
 *     asynchronous on that stream; the host variants take HOST pointers, stage through
 *     the context and block until the result is in the caller's buffer.
 *   - the caller owns every buffer passed in; pointers are only used during the call
 *     (host variants) or until the stream work completes (device variants).
 *   - one gr_ctx is bound to one HIP device; a ctx is not thread-safe, distinct ctxs are
 *     independent.  There is NO CPU fallback: without a gfx950 device gr_ctx_create fails.
 */
#ifndef GRADUS_MI355X_H
#define GRADUS_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_ABI_VERSION 8

typedef enum {
    GR_OK = 0,
    GR_ERR_INVALID_ARGUMENT = -1, /* null pointer, bad size, unsorted limits ...           */
    GR_ERR_UNSUPPORTED = -2,      /* unknown metric / disc / point-function id             */
    GR_ERR_NO_DEVICE = -3,        /* no usable HIP device (this library has no CPU path)   */
    GR_ERR_HIP = -4,              /* a HIP runtime call failed; see gr_last_error()        */
    GR_ERR_OUT_OF_MEMORY = -5
} gr_status;

/* StatusCodes -- src/Gradus.jl:59-64 (EnumX, declaration order) */
enum {
    GR_STATUS_OUT_OF_DOMAIN = 0,
    GR_STATUS_WITHIN_INNER_BOUNDARY = 1,
    GR_STATUS_INTERSECTED_WITH_GEOMETRY = 2,
    GR_STATUS_NO_STATUS = 3
};

/* AbstractStaticAxisSymmetric metrics available on the device.
 *   KERR               src/metrics/kerr-metric.jl:11-28,62-72          params = {M, a}
 *   JOHANNSEN          src/metrics/johannsen-ad.jl:12-34,49-67         params = {M, a, α13, α22, α52, ϵ3}
 *   MORRIS_THORNE      src/metrics/morris-thorne-ad.jl:4-39            params = {b}
 *   BUMBLEBEE          src/metrics/bumblebee-ad.jl:6-52                params = {M, a, l}
 *   KERR_NEWMAN        src/metrics/kerr-newman-ad.jl:6-64 (null rays / q = 0 only)   params = {M, a, Q}
 *   JOHANNSEN_PSALTIS  src/metrics/johannsen-psaltis-ad.jl:4-46        params = {M, a, ϵ3} */
enum {
    GR_METRIC_KERR = 0,
    GR_METRIC_JOHANNSEN = 1,
    GR_METRIC_MORRIS_THORNE = 2,
    GR_METRIC_BUMBLEBEE = 3,
    GR_METRIC_KERR_NEWMAN = 4,
    GR_METRIC_JOHANNSEN_PSALTIS = 5,
    GR_METRIC_DILATON_AXION = 6,       /* DilatonAxion(M, a, β, b) src/metrics/dilaton-axion-ad.jl:49-70 */
    GR_METRIC_SPHERICAL = 7,           /* SphericalMetric() (flat space) src/metrics/minkowski.jl:1-15; no params */
    GR_METRIC_KERR_DARK_MATTER = 8,    /* KerrDarkMatter(M, a, M_dark_matter, Δr, rₛ) src/metrics/kerr-dark-matter.jl:6-70 */
    GR_METRIC_KERR_REFRACTIVE = 9,     /* KerrRefractive(M, a, n, corona_radius) src/metrics/kerr-refractive-ad.jl:8-58 */
    GR_METRIC_NOZ = 10,                /* NoZMetric(M, a, ϵ) src/metrics/noz-metric.jl:7-66 */
    /* ABI 7 -- ANY AbstractStaticAxisSymmetric metric: the reference's plugin contract is a struct and ONE method,
     * metric_components(m, (r, θ)) -> (g_tt, g_rr, g_θθ, g_ϕϕ, g_tϕ) (src/Gradus.jl:78-86, src/metrics/kerr-metric.jl:62-70);
     * ForwardDiff supplies the Jacobian (src/tracing/method-implementations/auto-diff.jl:206-211).  A closure cannot cross this
     * ABI, so the caller samples its metric_components on the nodes gr_metric_grid_nodes() names, gr_metric_table_fit() turns
     * the samples into piecewise polynomials (total degree 5 on patches geometric in r - r0 and uniform in θ), and the kernels
     * evaluate the five components and their (∂r, ∂θ) derivatives from that table (gr_config.metric_table; params unused).
     * See "tabulated metrics" below.  Every flavour of the kernels ("precision" 32: the table stays fp64 and is evaluated in double, the step is fp32). */
    GR_METRIC_TABULATED = 11,
    /* A metric whose component function was compiled into a kernel module of its own and loaded at run time
     * (gr_metric_module_load, "compiled metrics" below): ids GR_METRIC_COMPILED ... GR_METRIC_COMPILED + GR_METRIC_MODULE_SLOTS - 1,
     * one per loaded module.  params = the P[0..5] the module's component function reads.  fp64 and tangent kernels only:
     * GR_ERR_UNSUPPORTED with "precision" 32. */
    GR_METRIC_COMPILED = 12
};
#define GR_METRIC_MODULE_SLOTS 16

/* accretion geometry
 *   THIN             ThinDisc        src/geometry/discs/thin-disc.jl:9-26       disc_r_in, disc_r_out, gtol
 *   SHAKURA_SUNYAEV  ShakuraSunyaev  src/geometry/discs/shakura-sunyaev.jl:22-33 disc_r_in = inner_radius,
 *                    disc_params = {Ṁ/Ṁ_Edd, 1/η}; height 3 (1/η)(Ṁ/Ṁ_Edd)(1 - sqrt(r_in/ρ)); thick-disc
 *                    distance_to_disc of src/geometry/discs/thick-disc.jl:60-66 (no gtol)
 *   TABULATED        ThickDisc(f)    src/geometry/discs/thick-disc.jl:30-66: the user's cross_section
 *                    closure cannot run on the device, so the host samples it on a uniform ρ grid:
 *                    disc_params = {ρ_first, ρ_last, max height}, disc_table[disc_table_n] = f(ρ_k);
 *                    linear interpolation, height <= 0 (or ρ outside the grid) = no disc there.
 *                    disc_params[3] != 0: WarpedThinDisc (thin-disc.jl:42-66) -- the table is the SIGNED height
 *                    h(ρ) of a thin sheet, |h(ρ) - r cosθ| < gtol |r| within disc_r_in <= ρ <= disc_r_out
 *                    (disc_params[2] = max |h|)
 *   DATUM            DatumPlane      src/geometry/discs/datum-plane.jl:1-10: the plane z = r cosθ = height
 *                    (disc_params[0]), signed (no underside), no radial extent; what the transfer-function
 *                    solvers trace against for a thin disc (cunningham-transfer-functions.jl:1-5)
 *   ELLIPTICAL       EllipticalDisc  src/geometry/discs.jl:57-72: disc_r_in = inner_radius, disc_params = {semi_major,
 *                    semi_minor}; |z| < sqrt((1 - (r/a)²) b²) + gtol |r| for inner_radius <= r <= semi_major
 *   PRECESSING_THIN  PrecessingDisc(ThinDisc(r_in, r_out), β, γ)  src/geometry/discs.jl:74-96: the thin disc tilted by β
 *                    about the x axis and turned by γ about the spin axis; disc_params = {β, γ, cos β, sin β}
 *   COMPOSITE        CompositeGeometry(d1, d2, ...) = d1 ∘ d2  src/geometry/composite.jl:1-26, the VectorContinuousCallback of
 *                    src/geometry/bootstrap.jl:76-110: comp_n (2..GR_COMP_MAX) components in gr_config.comp[], each a THIN,
 *                    SHAKURA_SUNYAEV, ELLIPTICAL or DATUM geometry with its own radii and parameters (gtol is shared, as in the
 *                    reference); the ray ends at the EARLIEST intersection with any of them
 *   MESH             MeshAccretionGeometry(mesh)  src/geometry/meshes.jl:1-80: a triangle mesh in Cartesian coordinates
 *                    (x, y, z) = (r sinθ cosϕ, r sinθ sinϕ, r cosθ), tested with a DiscreteCallback: after every accepted step the
 *                    segment from the previous to the new position is tested (jsf_algorithm, src/geometry/intersections.jl:58-101,
 *                    ϵ = 1e-8, front faces only) against the triangles whose first vertex lies within 3 of the new position, when
 *                    the new position is strictly inside the bounding box; the ray ends AT the step's end (no root finding) with
 *                    IntersectedWithGeometry.  disc_table = x_min, x_max, y_min, y_max, z_min, z_max (the x/y/z_extent fields of
 *                    the reference's struct), then 9 doubles V1 V2 V3 per triangle; disc_table_n = number of triangles (>= 1);
 *                    gtol and the other disc fields are not read.  fp64 only: GR_ERR_UNSUPPORTED with "precision" 32 and in
 *                    the tangent entry points (gr_ray_tangent*).  Cost per accepted step inside the box: one pass over the
 *                    triangle list per wave (the reference's "naive implementation" loop, meshes.jl:53-64) */
enum { GR_DISC_NONE = 0, GR_DISC_THIN = 1, GR_DISC_SHAKURA_SUNYAEV = 2, GR_DISC_TABULATED = 3, GR_DISC_DATUM = 4,
       GR_DISC_ELLIPTICAL = 5, GR_DISC_PRECESSING_THIN = 6, GR_DISC_COMPOSITE = 7, GR_DISC_MESH = 8 };
#define GR_COMP_MAX 4

/* one component of a GR_DISC_COMPOSITE geometry: the fields of gr_config with the same names, per component */
typedef struct gr_disc_component {
    int32_t disc_id;          /* GR_DISC_THIN | SHAKURA_SUNYAEV | ELLIPTICAL | DATUM               */
    int32_t _pad;
    double disc_r_in, disc_r_out;
    double disc_params[4];
} gr_disc_component;

/* per-ray anomaly bits written next to the status (SciML retcodes MaxIters /
 * DtLessThanMin / Unstable, which EnsembleEndpointThreads discards, tracing.jl:250) */
enum { GR_FLAG_MAXITERS = 1, GR_FLAG_DTMIN = 2, GR_FLAG_NAN = 4, GR_FLAG_MASK = 0xFFFF /* bits 16..31: winding count */ };

/* TracingConfiguration (src/tracing/configuration.jl:3-29) + TraceGeodesic.μ
 * (src/tracing/tracing.jl:1-7) + the geometry callback's gtol (src/geometry/bootstrap.jl:8)
 * flattened to plain data. */
typedef struct gr_config {
    int32_t metric_id;        /* GR_METRIC_*                                             */
    int32_t disc_id;          /* GR_DISC_*                                               */
    double params[8];         /* metric parameters, see GR_METRIC_*                      */
    double r_inner;           /* PolarChart.inner_radius (charts.jl:3-6), already scaled */
    double r_outer;           /* PolarChart.outer_radius                                 */
    double disc_r_in;         /* ThinDisc.inner_radius                                   */
    double disc_r_out;        /* ThinDisc.outer_radius                                   */
    double gtol;              /* geometry tolerance, default 1e-2                        */
    double lambda0, lambda1;  /* λ_domain                                                */
    double abstol, reltol;    /* default 1e-9 (configuration.jl:1)                       */
    double mu;                /* geodesic mass μ (0 = null)                              */
    int64_t maxiters;         /* OrdinaryDiffEq default 1_000_000                        */
    int32_t upper_hemisphere; /* 1 = domain_upper_hemisphere callback (callbacks.jl:31)  */
    int32_t _pad;
    double hemi_delta;        /* its δ, default 1e-4                                     */
    double disc_params[4];    /* extra geometry parameters, see GR_DISC_*                */
    const double* disc_table; /* GR_DISC_TABULATED (disc_table_n samples) / GR_DISC_MESH (6 + 9 disc_table_n doubles): HOST */
    int64_t disc_table_n;     /*   pointer in every entry point (copied into the context); NULL / 0 otherwise            */
    /* PoloidalShapeChart (charts.jl:26-48, event_horizon_chart :61-70): inner boundary r_min(θ),
     * chart_table[k] = r_min(θ_k) on the uniform grid θ_k = chart_theta0 + k (chart_theta1 -
     * chart_theta0)/(n-1), already scaled by closest_approach; linear interpolation (end intervals
     * extended).  HOST pointer, copied into the context.  n = 0: PolarChart with r_inner.       */
    const double* chart_table;
    int64_t chart_table_n;
    double chart_theta0, chart_theta1;
    double q;                 /* test-particle charge, TraceGeodesic.q (tracing.jl:1-7): adds the
                                 Lorentz force q F^μ_ν v^ν (q/μ for μ != 0) for GR_METRIC_KERR_NEWMAN,
                                 kerr-newman-ad.jl:66-100; ignored by metrics without a field     */
    int32_t count_windings;   /* 1 = TraceWindings (src/tracing/photon-rings.jl:1-71): count the crossings of the
                                 cone θ = winding_plane at step ends; the count is returned in bits 16..31 of
                                 gr_point.flags and by GR_PF_WINDING                                  */
    int32_t _pad2;
    double winding_plane;     /* TraceWindings.plane_inc, default π/2                                */
    int32_t comp_n;           /* GR_DISC_COMPOSITE: number of components (2..GR_COMP_MAX), else 0    */
    int32_t _pad3;
    gr_disc_component comp[GR_COMP_MAX];
    /* ABI 7, GR_METRIC_TABULATED: the table gr_metric_table_fit() wrote (HOST pointer in every entry point; the library keeps a
     * device copy per context, keyed by the table's build id, so a table is uploaded once) and its length in doubles.
     * NULL / 0 for every other metric. */
    const double* metric_table;
    int64_t metric_table_n;
} gr_config;

/* GeodesicPoint{Float64,Nothing} -- src/solution-processing.jl:15-32.  152 bytes, same
 * field order and padding as the Julia isbits struct (status::Int32 enum + 4 pad bytes,
 * which carry the anomaly flags here). */
typedef struct gr_point {
    int32_t status;
    int32_t flags;
    double lambda_min, lambda_max;
    double x_init[4], x[4], v_init[4], v[4];
} gr_point;

/* The pixel -> initial-velocity closure of _render_velocity_function
 * (src/rendering/rendering.jl:140-163) as data. */
typedef struct gr_plane {
    double x_obs[4];          /* observer four-position                                   */
    double Mx[16];            /* row-major 4x4: ginv * hcat(lnrbasis(g)...) of
                                 lnr_momentum_to_global_velocity_transform
                                 (src/tracing/utility.jl:32-40), computed by the caller   */
    double alpha0, alpha1;    /* αlims                                                    */
    double beta0, beta1;      /* βlims                                                    */
    int64_t width, height;    /* image_width, image_height                                */
    double offset;            /* the +1e-6 of rendering.jl:158-159                        */
} gr_plane;

/* Which rays of the W*H image (0-based linear index i = x*H + y, Julia's column-major
 * H x W matrix) a call processes: local ray j in [0, count) is image ray
 *     i = first + ((j / block) * stride_blocks + 0) * block + (j % block)
 * i.e. blocks of `block` consecutive rays, every `stride_blocks`-th block.  A contiguous
 * range is {first, count, count, 1}.  Used to shard an image over GPUs. */
typedef struct gr_range {
    int64_t first;
    int64_t count;
    int64_t block;
    int64_t stride_blocks;
} gr_range;

/* Built-in point functions -- src/const-point-functions.jl:26-79, src/redshift.jl:192-276 */
enum {
    GR_PF_AFFINE_TIME = 0,    /* gp.λ_max                                                */
    GR_PF_REDSHIFT = 1,       /* ConstPointFunctions.redshift(m, x)                      */
    GR_PF_STATUS = 2,         /* Float64(gp.status)                                      */
    GR_PF_RADIUS = 3,         /* _equatorial_project(gp.x)                               */
    GR_PF_WINDING = 4,        /* gp.aux.winding of a TraceWindings trace (photon-ring order) */
    GR_PF_INTENSITY = 5       /* gp.aux[1] of a TraceRadiativeTransfer trace: the gr_transfer_* entry points only */
};
enum {
    GR_FILTER_NONE = 0,
    GR_FILTER_EARLY_TERM = 1, /* filter_early_term: gp.λ_max < max_time                  */
    GR_FILTER_INTERSECTED = 2 /* filter_intersected: status == IntersectedWithGeometry   */
};
typedef struct gr_pointfunction {
    int32_t pf_id;
    int32_t filter_id;
    double fill;              /* FilterPointFunction.default (NaN)                       */
    double r_isco;            /* isco(m), host-computed                                  */
    /* PlungingInterpolation table for non-Kerr redshift (src/orbits/orbit-solving.jl:99-131,
     * src/interpolations.jl:1-45); n_plunge = 0 selects the analytic Kerr branch.  HOST
     * pointers in every entry point (the table is copied into the context). */
    int64_t n_plunge;
    const double* plunge_r;
    const double* plunge_vt;
    const double* plunge_vr;
    const double* plunge_vphi;
    /* ABI 7: the four-velocity the photon's energy is measured against at its START, for GR_PF_REDSHIFT:
     * has_u_src = 0 [every image-plane caller]: the static observer (1, 0, 0, 0) of _redshift_dotproduct (redshift.jl:192-220);
     * has_u_src = 1: u_src -- energy_ratio(m, gp, v_src, v_disc) = (g v_init u_src) / (g v v_disc) of
     * src/corona/flux-calculations.jl:96-110, the redshift between a moving coronal source and the disc.                    */
    int32_t has_u_src;
    int32_t _pad_u;
    double u_src[4];
} gr_pointfunction;

/* aggregate counters of one call (device-side reductions) */
typedef struct gr_stats {
    int64_t rays;
    int64_t accepted_steps;
    int64_t rejected_steps;
    int64_t rhs_evals;
    int64_t flagged_rays;     /* rays with a GR_FLAG_* bit set                           */
    int64_t status_count[4];  /* histogram over StatusCodes                              */
    /* host variants only (ABI 5 tells the two apart): device time from the start of the call's work on the context's
     * stream to the end of its LAST TRACE KERNEL (staging of inputs and tables included) ...                            */
    double kernel_ms;
    /* ... and to the end of the last copy back into the caller's buffer: kernel_ms plus the D2H part.  The wall time
     * of the blocking call is this plus the launch / synchronisation latency of the host side.                        */
    double call_ms;
    /* *_multi entry points only (ABI 6; 0 from every other call): host wall-clock time the calling thread spent ENQUEUEING
     * this context's share -- staging its inputs and launching its kernel, before it moved on to the next context.  Small
     * against kernel_ms means the devices ran side by side; comparable to kernel_ms would mean the call had waited for
     * device k before it started device k+1 (tests/test_gpu_multi.py asserts the former, for pageable and pinned results). */
    double enqueue_ms;
} gr_stats;

typedef struct gr_ctx gr_ctx;

int32_t gr_abi_version(void);
const char* gr_last_error(void);

/* Create / destroy a context on HIP device `device`. */
int32_t gr_ctx_create(int32_t device, gr_ctx** out);
int32_t gr_ctx_destroy(gr_ctx* ctx);
/* Tuning knobs: key/value.  ("kernel", 0 = one ray per lane, 1 = persistent with wave-ballot
 * refill, 2 = chosen per launch [default]: image planes -> one ray per lane in one-wave workgroups,
 * line profiles and caller-ordered ray arrays -> persistent); ("block", threads per workgroup,
 * 0 = auto [default]: 64 for kernel 0, 256 for kernel 1); ("refill_threshold", idle lanes that
 * trigger a refill, 0 = auto [default]: 16 for the fp64 kernels, 32 for the fp32 ones); ("waves_per_simd"), ("swizzle"), ("lpt"), ("lpt_lane"), ("lds"),
 * ("precision", 64 | 32); ("pipeline", bands of the end-point return); ("hugepages", 1 [default] = large caller-owned
 * result buffers are madvise(MADV_HUGEPAGE)d before they are pre-faulted, 0 = the caller's mapping is left alone);
 * ("tangent_norm", 1 [default] = gr_ray_tangent's step-size controller sees values AND tangents -- DiffEqBase's norm on
 * Dual state, what the reference's solves under ForwardDiff use (src/tracing/precision-solvers.jl:73-131,401-451); two
 * independent integrators then agree on the Jacobians to 1e-6 (tests/test_oracle_tangent.py) --, 0 = values only: the
 * tangents ride on the very steps of the plain trace and are good to ~1e-5, 4e-3 on rays through the polar axis);
 * ("tangent_pairs", gr_ray_tangent's kernel shape: 0 = one lane carries a ray with both directions of the Jacobian (least work:
 * 1024² rays in 20.9 ms), 1 = a PAIR of lanes per ray, one direction each (shortest step: the reference's default line profile,
 * 909 launches of ~126 rays, in 1.16 s against 1.55 s), 2 [default] = pairs for launches that cannot fill the SIMDs anyway
 * (2 n lanes <= one wave per SIMD), one lane per ray beyond; same results to rounding either way);
 * ("xcd_spread", 1 [default] = rays in caller order on the one-ray-per-lane kernel are dealt to the 8 XCDs by the digit sum of
 * their chunk index instead of round-robin -- a periodic pattern in the rays, such as the polar-axis column of a 1024-wide grid of
 * impact parameters, otherwise lands on one or two XCDs (38 against 21 ms) --, 0 = chunk b to workgroup b);
 * ("live_first", the order of an image launch's pixel tiles on the one-ray-per-lane kernel where rays are decided at their start
 * (one thin disc around the Kerr metric, misses ignored): 1 [default] = launches of at least as many tiles as the device holds
 * waves take the tiles with a corner ray that is traced first and the tiles decided at the start last -- the order is built on
 * the device ahead of each launch from that launch's own parameters --, 2 = launches of any size, 0 = tile order; same pixels
 * and statistics either way; GRADUS_MI355X_LIVE_FIRST=0, 1 or 2 in the environment takes the knob's place);
 * ("sky_deal", 1 [default] = gr_corona_trace deals the rays of a sky source to the waves by what they will cost -- a counting sort
 * by a step count predicted from each ray's initial position and direction (its passage round the polar axis), the longest class
 * first, traced by the one-ray-per-lane kernel in 256-thread workgroups: a wave's rays take nearly the same number of steps and the
 * launch begins with its longest waves (10⁶ lamp-post samples: 5.9 against 8.4 ms in sample order) --, 0 = sample order; same
 * min / max and bins either way);
 * ("lds_points", 1 [default] = the one-ray-per-lane kernel sends a wave's 64 end-point records through LDS as runs of
 * consecutive addresses, 0 = every lane stores its own 152 bytes; same bytes either way); ("direct_host", 1 [default] =
 * gr_render_endpoints into a gr_host_alloc block lets the kernel store across the link itself -- no staging buffer, no
 * copy --, 0 = staged in HBM and copied in bands as for caller-owned memory); ("pinned_pool_mib", process-wide: bytes of freed
 * gr_host_alloc blocks kept page-locked for the next request, default 1024 in at most 4 blocks, 0 = empty the pool and keep nothing;
 * the pool is emptied when the last context is destroyed); ("pinned_max_mib", process-wide: bytes of gr_host_alloc blocks that may
 * be outstanding at once, default 8192 -- a request beyond it is refused with GR_ERR_OUT_OF_MEMORY and the caller falls back to
 * pageable memory: a garbage-collected caller sees a 100-byte wrapper, not the block behind it);
 * ("pinned_huge", process-wide: 1 [default] = gr_host_alloc blocks of 8 MiB and more are mappings on transparent huge pages
 * registered with the runtime (13 ms for 608 MiB), 0 = every block from hipHostMalloc (122-365 ms));
 * ("tf_chunk", annuli per workgroup of gr_tf_lineprofile / gr_tf_lagtransfer, 0 = auto [default], at most 65536: the launch
 * shape only, the results are the same bits for every value). */
int32_t gr_ctx_set(gr_ctx* ctx, const char* key, int64_t value);

/* ---- pinned result buffers (ABI 5).  The reference allocates the result of ensemble_solve_tracing_problem itself
 * (`Vector{GeodesicPoint{T}}(undef, n)`, src/tracing/tracing.jl:179-183): pageable memory, which the D2H copy crosses at
 * ~30 GB/s after its pages have been faulted in.  A binding that lets the LIBRARY allocate that block (page-locked, mapped
 * for DMA once) and wraps it as its array -- Julia: unsafe_wrap(Array, Ptr{GeodesicPoint}(p), n) + a finalizer calling
 * gr_host_free -- lets the trace kernel store the records into it directly, across the link (gr_render_endpoints, gr_render:
 * no staging buffer, no copy; gr_ctx_set "direct_host").  Any host entry point accepts such a pointer wherever it takes a
 * caller-owned output buffer; callers that bring their own memory are served as before.  Blocks are registered
 * process-wide: gr_host_free does not look at `ctx` (it may be NULL, or a context that has been destroyed meanwhile --
 * finalizers of a garbage-collected host language run in no particular order), and destroying a context does not free them.
 * gr_host_free(ctx, NULL) is a no-op.  Blocks of 8 MiB and more are anonymous mappings on transparent huge pages that the
 * library registers with the runtime (608 MiB: 13 ms; hipHostMalloc takes 122-365 ms for the same block), and freed blocks
 * wait in a bounded process-wide pool for the next request of a similar size (gr_ctx_set "pinned_pool_mib"), which then
 * costs nothing.  The memory of a reused block holds the previous result until the next call overwrites it -- a call that
 * writes only PART of a block (a gr_range that is not the whole plane) leaves the rest as it found it.
 * PROCESS-WIDE STATE, the one exception to "no global state but the context handle" (SURVEY §8b): the registry of blocks, the
 * pool and its two limits ("pinned_pool_mib", "pinned_max_mib": set through any context, they apply to all) belong to the
 * process because the blocks must outlive contexts.  The library counts the bytes it has handed out and REFUSES
 * (GR_ERR_OUT_OF_MEMORY) a request that would take them past "pinned_max_mib" (default 8 GiB): bindings for garbage-collected
 * languages collect and retry, or fall back to pageable memory.  The pool is emptied when the last context is destroyed.
 * Only a destination that lies ENTIRELY inside one block is written by a kernel directly; anything else -- a pointer near the end
 * of a block, a block too small for the result -- takes the staged copy like caller-owned memory. */
int32_t gr_host_alloc(gr_ctx* ctx, int64_t bytes, void** out);
int32_t gr_host_free(gr_ctx* ctx, void* p);

/* ---- fused render: rendergeodesics / render_into_image! (rendering.jl:28-54,89-107) ----
 * image[j] (j local, see gr_range) = pf(m, trace(ray i), λ_max). */
int32_t gr_render_device(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane,
                         const gr_pointfunction* pf, const gr_range* range,
                         double* d_image /* device, range->count doubles */,
                         gr_stats* d_stats /* device, may be NULL */, void* hip_stream);
int32_t gr_render(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane,
                  const gr_pointfunction* pf, const gr_range* range,
                  double* image /* host, range->count doubles */, gr_stats* stats /* host, may be NULL */);

/* ---- ONE host thread, SEVERAL devices: what a Julia caller gets from `ensemble = EnsembleMI355X(devices)` at every entry
 * of the boundary (bench.py uses one process per GPU and an RCCL gather instead).  Every *_multi call has the same shape:
 *   phase 1  for each context: stage its inputs, launch its kernel on its own stream -- nothing here waits for a device
 *            (gr_stats.enqueue_ms records the host time each context took);
 *   phase 2  for each context: queue the copy of its share into its place in the caller's buffer (a copy into pageable memory
 *            may block the host until THAT device's kernel has finished -- every other device is already running);
 *   phase 3  wait for all of them.
 * There is no exchange between devices at all.  ctxs must be distinct contexts; they may live on different devices or (for
 * testing) on the same one.  stats[k] receives the counters of ctxs[k] (may be NULL).  With n = 1 a call produces the bytes of
 * its single-context entry point -- which, the two image-plane renders apart, IS this call on its one context: the same checks,
 * the same timings (kernel_ms / call_ms from before the staging of the inputs), nothing left in flight on an error, a ray set
 * taken as it is given (the refusals below concern sharing rays out: n > 1), and enqueue_ms = 0.
 *
 * Image planes (gr_render_multi, gr_render_endpoints_multi): the columns are dealt to the n contexts block-cyclically in
 * groups of `block_cols` columns (0 = default 8, halved until it divides width / n) -- centre columns hold the long rays, so
 * a contiguous split would leave the middle devices working after the outer ones have finished.  Into caller-owned (pageable)
 * memory each device's share goes home with one strided D2H copy; into a block from gr_host_alloc every device's KERNEL
 * stores its pixels / records at their final place across the link (no staging buffer, no copy). */
int32_t gr_render_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_plane* plane,
                        const gr_pointfunction* pf, int64_t block_cols,
                        double* image /* host, width*height doubles */, gr_stats* stats /* n entries or NULL */);
/* prerendergeodesics / ensemble_solve_tracing_problem on the render closure (src/rendering/rendering.jl:56-87,
 * src/tracing/tracing.jl:151-196): the whole plane's end points, 152 B per ray in image order. */
int32_t gr_render_endpoints_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_plane* plane,
                                  int64_t block_cols, gr_point* points /* host, width*height */,
                                  gr_stats* stats /* n entries or NULL */);
/* tracegeodesics(m, xs, vs, ...) (tracing.jl:151-196 on the array inputs of geodesic-problem.jl:121-150): context k takes
 * the k-th contiguous share of the rays (shares are multiples of 64 rays, the last may be short or empty). */
int32_t gr_trace_endpoints_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const double* x, int64_t x_stride,
                                 const double* v, int64_t n_rays, gr_point* points /* host, n_rays */,
                                 gr_stats* stats /* n entries or NULL */);
/* (the ray-set entry points -- gr_rayset_endpoints_multi, gr_ray_summary_multi, gr_ray_tangent_multi,
 * gr_redshift_radius_multi, gr_lineprofile_multi -- are declared at the end of this header, behind gr_rayset) */

/* ---- endpoints of an image plane: prerendergeodesics / EndpointRenderCache
 * (rendering.jl:56-87,121-138) ---- */
int32_t gr_render_endpoints_device(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane,
                                   const gr_range* range, gr_point* d_points, gr_stats* d_stats,
                                   void* hip_stream);
int32_t gr_render_endpoints(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane,
                            const gr_range* range, gr_point* points, gr_stats* stats);

/* ---- tracegeodesics(m, xs, vs, ...; ensemble) -> Vector{GeodesicPoint}
 * (tracing.jl:151-196; input shapes of geodesic-problem.jl:121-150).
 * x: n x 4 positions, or a single position when x_stride == 0 (else x_stride == 4);
 * v: n x 4 UNCONSTRAINED velocities -- constrain_all (constraints.jl:14-15) is applied on
 * the device. */
int32_t gr_trace_endpoints_device(gr_ctx* ctx, const gr_config* cfg, const double* d_x,
                                  int64_t x_stride, const double* d_v, int64_t n,
                                  gr_point* d_points, gr_stats* d_stats, void* hip_stream);
int32_t gr_trace_endpoints(gr_ctx* ctx, const gr_config* cfg, const double* x, int64_t x_stride,
                           const double* v, int64_t n, gr_point* points, gr_stats* stats);

/* ---- covariant radiative transfer (additive within ABI 8): TraceRadiativeTransfer through an optically thick disc ----
 * src/tracing/radiative-transfer-problem.jl.  The ray carries a ninth state component I, integrated with the geodesic:
 *     dI/dλ = s (-a_ν I + j_ν / ν³),   s = -g_μν(x) k^μ u^ν,   ν = nu0 s,
 * with u the fluid velocity at ρ = r sin θ (CircularOrbits.fourvelocity outside the ISCO, CircularOrbits.plunging_fourvelocity
 * inside) while the ray is inside the geometry, and dI/dλ = 0 outside.  The ray does not end on the surface: every crossing
 * is located on the dense output, the state (I included) moved there, and the trace goes on -- to the chart, to lambda1, to
 * maxiters, or to the 65th crossing (GR_FLAG_MAXITERS).  Coefficients are power laws,
 *     a_ν = a0 ρ^-pa ν^-sa,   j_ν = j0 ρ^-pj ν^-sj
 * (all exponents zero: the constant coefficients of the reference's doughnut example).  transfer->r_isco separates the two
 * velocity laws (pf->r_isco is not read).
 * Refused with GR_ERR_UNSUPPORTED: cfg->disc_id other than GR_DISC_SHAKURA_SUNYAEV / GR_DISC_TABULATED (a warped table,
 * disc_params[3] != 0, included), GR_METRIC_TABULATED and compiled metrics, metrics without an ISCO (kernels exist for Kerr,
 * Johannsen, Bumblebee, Kerr-Newman, Johannsen-Psaltis, dilaton-axion and Kerr-refractive), "precision" 32, cfg->q != 0,
 * cfg->count_windings, and in the render a pf_id other than GR_PF_INTENSITY. */
typedef struct gr_transfer {
    double nu0;               /* TraceRadiativeTransfer.ν                                  */
    double I0;                /* TraceRadiativeTransfer.I₀: the intensity every ray starts with */
    double a0, j0;            /* absorption / emissivity amplitudes                        */
    double pa, pj;            /* ... their exponents in ρ                                  */
    double sa, sj;            /* ... and in ν                                              */
    double r_isco;            /* isco(m), host-computed: fluid_velocity's switch between the two laws */
    double reserved;          /* zero                                                      */
} gr_transfer;
/* the image of I over `range` of the plane (pf->pf_id = GR_PF_INTENSITY; filter and fill as in gr_render) */
int32_t gr_transfer_render_device(gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer, const gr_plane* plane,
                                  const gr_pointfunction* pf, const gr_range* range, double* d_image /* device */,
                                  gr_stats* d_stats /* device, may be NULL */, void* hip_stream);
int32_t gr_transfer_render(gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer, const gr_plane* plane,
                           const gr_pointfunction* pf, const gr_range* range, double* image /* host, range->count doubles */,
                           gr_stats* stats /* host, may be NULL */);
/* the end-point records of n rays given by (x, v) as in gr_trace_endpoints, and their intensities beside them */
int32_t gr_transfer_endpoints(gr_ctx* ctx, const gr_config* cfg, const gr_transfer* transfer, const double* x,
                              int64_t x_stride, const double* v, int64_t n, gr_point* points,
                              double* intensity /* host, n doubles */, gr_stats* stats);

/* ---- tracegeodesics(m, x::SVector, v::SVector, ...): ONE geodesic with every accepted step
 * saved (the reference's single-problem solve with save_on = true, src/tracing/tracing.jl:88-110).
 * Used on its own and by interpolate_plunging_velocities (src/orbits/orbit-solving.jl:137-167),
 * which traces the μ = 1 plunge from the ISCO on the same integrator.
 * path: cap rows of 9 doubles (λ, x[4], v[4]); row 0 is the initial state, the last row the
 * final state (after any event).  *n_rows receives the number of rows the solve produced
 * (rows beyond cap are dropped but still counted). */
int32_t gr_trace_path(gr_ctx* ctx, const gr_config* cfg, const double* x /* 4 */,
                      const double* v /* 4, unconstrained */, int64_t cap, double* path /* host, cap x 9 */,
                      int64_t* n_rows, gr_point* endpoint /* host, may be NULL */);
/* The same for n geodesics at once (tracegeodesics(m, xs, vs, ...) with save_on = true, the
 * EnsembleProblem solve of src/tracing/tracing.jl:113-149; the reference's benchmark suite
 * benchmark/integrator/benchmark-tracing.jl "many-geodesic" cases): ray j fills path[j * cap * 9 ...],
 * n_rows[j], endpoints[j].  x_stride = 0: one position for all rays, 4: one per ray. */
int32_t gr_trace_paths(gr_ctx* ctx, const gr_config* cfg, const double* x, int64_t x_stride,
                       const double* v /* n x 4, unconstrained */, int64_t n, int64_t cap,
                       double* path /* host, n x cap x 9 */, int64_t* n_rows /* host, n */,
                       gr_point* endpoints /* host, n, may be NULL */);

/* ---- lineprofile(bins, ε, m, x, d, BinningMethod(); plane, callback) --
 * src/line-profiles.jl:152-198.  The rays are an AbstractImagePlane given by its impact parameters
 * (src/image-planes/planes.jl:70-184); velocities are map_impact_parameters(m, x, α_i, β_i) with no
 * pixel offset (planes.jl:180-184). */
typedef struct gr_rayset {
    double x_obs[4];
    double Mx[16];            /* as in gr_plane                                            */
    const double* alpha;      /* n impact parameters α                                     */
    const double* beta;       /* n impact parameters β                                     */
    const double* area;       /* n unnormalized_areas(plane), or NULL for 1                */
    int64_t n;
    const double* height;     /* GR_DISC_DATUM only: n plane heights, one DatumPlane per ray
                                 (datumplane(d, rₑ), datum-plane.jl:14-17: what the thick-disc
                                 transfer-function solvers trace against, one plane per emission
                                 radius), or NULL for cfg->disc_params[0]                   */
    /* Separable ray sets (ABI 4): a PolarPlane (src/image-planes/planes.jl:96-131) is the outer product of Nr radii and
     * Nθ angles -- α = r_i cos θ_j, β = r_i sin θ_j, unnormalized_areas = r_i² -- so its rays need not be materialised:
     * with sep_r != NULL the library forms them on the device from the three small tables (alpha / beta / area are
     * ignored; products are plain IEEE multiplies, i.e. bit-identical to the arrays the
     * reference builds).  Ray k of the set is visited in 8 x 8 tiles of (i, j) (sep_tiled = 1: 64 neighbouring rays per
     * wave; the order in which a histogram receives its rays is immaterial) or column-major, k = i + sep_nr j
     * (sep_tiled = 0: the order of vec(αs), for outputs that are indexed by ray). */
    const double* sep_r;      /* sep_nr radii                                              */
    const double* sep_cos;    /* sep_nt cosines                                            */
    const double* sep_sin;    /* sep_nt sines                                              */
    int64_t sep_nr, sep_nt;
    int32_t sep_tiled;
    int32_t sep_reserved;
    /* Which rays of the set's order this launch traces (one plane sharded over devices, each adding its partial
     * histogram -- gradus.jl_amd/distributed.py): local ray j is ray
     *     k = sep_first + (j / sep_block) * sep_stride + j % sep_block          (sep_block > 0: a block-cyclic deal)
     *     k = sep_first + j                                                     (sep_block = 0: a contiguous range)
     * and every k must be below sep_nr * sep_nt.  All zero and n = sep_nr * sep_nt: the whole plane. */
    int64_t sep_first, sep_block, sep_stride;
    /* Rays FROM A SOURCE INTO ITS SKY (ABI 7): tracegeodesics(m, model::AbstractCoronaModel, ...) / tracecorona
     * (src/corona/corona-models.jl:1-33,143-190) for a source at ONE position (lamp post, beamed point source, a ring's
     * representative point).  sky_sampler != 0 selects it: x_obs is the source position, Mx = T · diag(1, J) with T =
     * tetradframe(g, v_source) and J the Cartesian -> spherical Jacobian at the source (samplers.jl:81-99: v = T (E0, E0 J k̂));
     * ray j (sample number j + 1, 1-based as in samplers.jl:30-44) leaves in the direction k̂ = -(sinθ cosϕ, sinθ sinϕ, cosθ) with
     *   i     = j + 1 (sky_generator 0: GoldenSpiralGenerator) | (j + 1) / n (1: EvenGenerator) | sky_i[j] (2: the caller's
     *           numbers, e.g. RandomGenerator's rand() * n)
     *   θ     = EvenSampler (sky_sampler 1): acos(1 - i / n) lower hemisphere, acos(1 - 2 i / n) both;
     *           WeierstrassSampler (2): 2 atan(sqrt(sky_resolution / i)), mirrored to π - θ for odd i on both hemispheres
     *   ϕ     = mod(π (1 + √5) i, 2π) for the golden spiral, mod(2π i, 2π) otherwise.
     * alpha / beta / area / height / sep_* are not read. */
    int32_t sky_sampler;      /* 0 = off, 1 = EvenSampler, 2 = WeierstrassSampler */
    int32_t sky_both;         /* 0 = LowerHemisphere, 1 = BothHemispheres */
    int32_t sky_generator;    /* 0 = golden spiral, 1 = even, 2 = sky_i */
    int32_t sky_reserved;
    double sky_resolution;
    const double* sky_i;      /* n values for sky_generator 2 (host / device pointer like alpha), else NULL */
    /* ABI 8 -- a SHARE of a source's samples (what the *_multi entry points hand each context; a caller that shards by hand --
     * one process per GPU -- sets them itself): the n rays of this set are samples sky_first + 1 .. sky_first + n of sky_total in
     * all, i.e. the `n` of the formulas above is sky_total and ray j has sample number sky_first + j + 1 (sky_i still has one
     * entry per ray of THIS set).  sky_total = 0: the whole source (first 0, total n). */
    int64_t sky_first, sky_total;
    /* ABI 8 -- a source WITHOUT one position (the reference's DiscCorona, src/corona/models/extended.jl:165-181: every sample leaves
     * from a point of its own, sample_position_velocity per ray, corona-models.jl:1-33): GR_SKY_ROW doubles per ray,
     *     x[4]       the sample's position
     *     Mx[16]     its matrix T diag(1, J), row-major as above (x_obs and Mx of the set are then not read)
     *     u_cov[4]   g_μν(x) u_src^ν, the source's four-velocity there with its index lowered
     *     gt[4]      g_tμ(x)
     * and the rows of gr_ray_summary / gr_corona_trace hold g = energy_ratio against THAT sample's source velocity (pf->has_u_src
     * must be 0: the library forms (u_cov · v) / (gt · v) per ray and scales the static-observer ratio with it).  Host or device
     * pointer like alpha; NULL: one position.
     * Two rules go with it:
     *   - ONLY gr_ray_summary / gr_corona_trace (and their _device / _multi forms) form that per-sample ratio; gr_rayset_endpoints
     *     takes such a set too (its records carry no g).  gr_lineprofile, gr_redshift_radius and gr_ray_tangent -- host, _device
     *     and _multi forms -- would return g against the static observer: they refuse a set with sky_rows
     *     (GR_ERR_INVALID_ARGUMENT) before anything is staged.
     *   - Under GR_METRIC_TABULATED every sample's start radius x[1] must lie inside the table's radial range (x_obs is not
     *     read, so it is not what is checked).  The entry points that take HOST pointers check all n rows before staging and
     *     refuse a set with a start outside [r_min, r_max] (GR_ERR_INVALID_ARGUMENT, the radius in the message); the _device
     *     forms cannot see the rows: there the caller vouches that every row starts inside the table. */
    const double* sky_rows;
} gr_rayset;
#define GR_SKY_ROW 28

typedef struct gr_binning {
    double r_min, r_max;      /* minrₑ, maxrₑ: only hits with r_min <= ρ <= r_max count    */
    double emissivity_index;  /* ε(r) = r^-q                                               */
    int64_t n_bins;
    const double* bin_edges;  /* n_bins values, ascending (the `bins` argument)            */
    /* ABI 4: a tabulated emissivity instead of the power law -- emissivity_at(prof::RadialDiscProfile, r)
     * (src/corona/radial.jl:15-18): r clamped to [eps_r[0], eps_r[eps_n-1]], then the NaNLinearInterpolator of
     * src/interpolations.jl:1-30 (linear between the neighbouring radii; a NaN node falls back to the nearer finite
     * neighbour, else 0).  eps_n >= 2 selects it; eps_n = 0: ε(r) = r^-emissivity_index. */
    const double* eps_r;      /* eps_n radii, ascending                                    */
    const double* eps_v;      /* eps_n emissivities                                        */
    int64_t eps_n;
} gr_binning;

/* flux[k] += ε(ρ) g³ area for every counted hit whose redshift g falls in bin k
 * (bucket(Simple(), g, f, bins): last edge <= g, clamped to the first / last bin).  NOT normalised;
 * the caller divides by sum(flux) (line-profiles.jl:197).  Device variant: rays->alpha/beta/area,
 * b->bin_edges and d_flux are device pointers; d_flux is zeroed by the call. */
int32_t gr_lineprofile_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                              const gr_pointfunction* pf, const gr_binning* b, double* d_flux,
                              gr_stats* d_stats, void* hip_stream);
int32_t gr_lineprofile(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                       const gr_pointfunction* pf, const gr_binning* b, double* flux, gr_stats* stats);
/* generic emissivity: (g, ρ) per ray (NaN, NaN for rays that do not count), n x 2 doubles */
int32_t gr_redshift_radius_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                                  const gr_pointfunction* pf, double r_min, double r_max,
                                  double* d_pairs, gr_stats* d_stats, void* hip_stream);
int32_t gr_redshift_radius(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                           const gr_pointfunction* pf, double r_min, double r_max, double* pairs,
                           gr_stats* stats);

/* ---- ray summaries for the precision solvers (find_offset_for_radius, jacobian_∂αβ_∂gr,
 * src/tracing/precision-solvers.jl:135-236,401-451): per ray of an impact-parameter set, 4 doubles
 * (g, ρ, t, status) = (redshift of the end point or NaN if the ray did not reach the geometry,
 * r |sinθ| and coordinate time of the end point, status code) -- everything one solver iteration
 * reads, in one launch and 32 B per ray. ---- */
int32_t gr_ray_summary_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                              const gr_pointfunction* pf, double* d_out /* n x 4 */, gr_stats* d_stats,
                              void* hip_stream);
int32_t gr_ray_summary(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                       const gr_pointfunction* pf, double* out /* host, n x 4 */, gr_stats* stats);

/* ---- The same rays with DUAL NUMBERS THROUGH THE INTEGRATOR: what jacobian_∂αβ_∂gr obtains from ForwardDiff.jacobian around
 * tracegeodesics (src/tracing/precision-solvers.jl:401-451) and the Cunningham transfer functions divide by
 * (src/transfer-functions/cunningham-transfer-functions.jl:337-387).  The integrator is instantiated on a scalar that carries
 * ∂/∂α and ∂/∂β (gr_tangent.hpp): the tangent equations are integrated with the very Tsit5 steps of the value, the event
 * time's dependence on (α, β) is added by implicit differentiation at the disc.  out: n x 8 doubles
 * (g, ρ, ∂g/∂α, ∂g/∂β, ∂ρ/∂α, ∂ρ/∂β, t, status); g = NaN unless the ray met the geometry.  cfg->disc_id must not be NONE. */
int32_t gr_ray_tangent_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                              const gr_pointfunction* pf, double* d_out /* n x 8 */, gr_stats* d_stats,
                              void* hip_stream);
int32_t gr_ray_tangent(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                       const gr_pointfunction* pf, double* out /* host, n x 8 */, gr_stats* stats);

/* ---- THE ITERATIONS AROUND THOSE RAYS, on the device (ABI 8): the emission-radius offset solve and the redshift-extremum search of
 * the Cunningham transfer functions, every problem carried from start to finish by one lane pair of ONE launch (gr_offsetsolve.hpp).
 *
 * gr_offset_solve: _find_offset_for_radius (src/tracing/precision-solvers.jl:135-236) for n problems (r_target, θ) -- the offset r
 * along the image-plane direction (cos θ, sin θ) from (alpha0, beta0) whose ray meets the geometry at ρ = r_target: the cold start
 * max(20, r_target), Newton with dρ/dr from the dual numbers, the contrapoint and the biased bisection step, the "converge failed"
 * stop, the six-entry cycle test, the bracket finish (at most 60 bisections), the late bracket after max_iter rounds, the exit at the
 * first |ρ - r_target| <= zero_atol.  cos_theta / sin_theta come from the caller, so that a host route that forms them itself works
 * on the same bits.  `rays` gives the observer (x_obs, Mx); its per-ray fields are not read.  out: n x 10 doubles
 *     r (NaN: no acceptable offset -- r >= 0, |ρ - r_target| <= 1e-4 r_target, the ray met the geometry), the 8 doubles of
 *     gr_ray_tangent for the ray the iteration ended on, the number of rays the iteration traced.
 * gr_offset_search: _search_extremal! (src/transfer-functions/cunningham-transfer-functions.jl:390-438), Optim's golden section over
 * θ on sign·g, for n searches (r_target, lower, upper, sign): the first point lower + GOLDEN (upper - lower), then `iterations` steps;
 * every visited θ is nudged by +1e-4 when within 1e-4 of 0 or ±π, cos θ and sin θ are formed on the device, and every evaluation is
 * one whole offset solve.  out: n x (12 (iterations + 1) + 1) doubles -- per evaluation, in call order,
 *     θ after the nudge, r, the 8 doubles of the ray, rays traced, failure flag (1: no acceptable offset: the search ends there, its
 *     later records are not written -- the host forms return them as NaN -- and its minimum is NaN),
 * then the minimum of sign·g found.
 * A solve's result does not depend on which other problems share its launch or its context.  gr_stats as for gr_ray_tangent.
 * GR_ERR_UNSUPPORTED for a set with sky rows, for cfg->disc_id other than GR_DISC_THIN / GR_DISC_DATUM and with "precision" 32;
 * GR_ERR_INVALID_ARGUMENT for a null pointer, a negative n, iterations outside 0 ... 4096, per_wave outside 0 ... 32. */
typedef struct gr_offset_problems {
    int64_t n;
    const double* r_target;   /* n */
    const double* cos_theta;  /* n */
    const double* sin_theta;  /* n */
    const double* height;     /* GR_DISC_DATUM only: n plane heights, one DatumPlane per problem, or NULL for cfg->disc_params[0] */
    double alpha0, beta0;
    double zero_atol;         /* the reference's 1e-7 */
    double r_min;             /* inner_radius(m): a ray that ends within r_min + 1 of it falls short */
    int64_t max_iter;         /* the reference's 50 */
    double contrapoint_bias;  /* the reference's 2 */
    int64_t per_wave;         /* problems a wave carries, 1 ... 32; 0 = the library's choice */
} gr_offset_problems;
typedef struct gr_offset_searches {
    int64_t n;
    const double* r_target;   /* n */
    const double* lower;      /* n */
    const double* upper;      /* n */
    const double* sign;       /* n: +1 searches the minimum of g, -1 its maximum */
    const double* height;     /* as above */
    double alpha0, beta0;
    double zero_atol;
    double r_min;
    int64_t max_iter;
    double contrapoint_bias;
    int64_t per_wave;
    int64_t iterations;       /* golden-section steps behind the first point */
} gr_offset_searches;
int32_t gr_offset_solve_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                               const gr_offset_problems* problems /* device arrays */, double* d_out /* n x 10 */,
                               gr_stats* d_stats, void* hip_stream);
int32_t gr_offset_solve(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                        const gr_offset_problems* problems, double* out /* host, n x 10 */, gr_stats* stats);
int32_t gr_offset_search_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                                const gr_offset_searches* searches /* device arrays */,
                                double* d_out /* n x (12 (iterations + 1) + 1) */, gr_stats* d_stats, void* hip_stream);
int32_t gr_offset_search(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                         const gr_offset_searches* searches, double* out /* host, n x (12 (iterations + 1) + 1) */,
                         gr_stats* stats);

/* ---- end points of an impact-parameter ray set: tracegeodesics(m, x, i -> map_impact_parameters(m, x,
 * α[i], β[i]), d, ...; ensemble = EnsembleEndpointThreads()) as impact_parameters_for_radius_obscured
 * (src/tracing/precision-solvers.jl:363-372) and the thick-disc transfer-function workhorse
 * (src/transfer-functions/cunningham-transfer-functions.jl:253-300) call it. ---- */

int32_t gr_rayset_endpoints_device(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                                   gr_point* d_points /* n */, gr_stats* d_stats, void* hip_stream);
int32_t gr_rayset_endpoints(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays,
                            gr_point* points /* host, n */, gr_stats* stats);

/* ---- apply(pf, cache): evaluate a built-in point function on endpoint records
 * (point-functions.jl:98-101, rendering.jl:103-107) ---- */
int32_t gr_apply_pointfunction_device(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf,
                                      const gr_point* d_points, int64_t n, double max_time,
                                      double* d_out, void* hip_stream);
int32_t gr_apply_pointfunction(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf,
                               const gr_point* points, int64_t n, double max_time, double* out);

/* ---- corona -> disc on the device (ABI 7): emissivity_profile(m, d, model; n_samples, sampler) (src/corona/emissivity.jl:118-168,
 * src/corona/radial.jl:38-100) for a source at one position.  Two calls on ONE context, nothing else on that context in between:
 *   gr_corona_trace  traces the rays of a sky source (gr_rayset.sky_*) against the disc and keeps (g, ρ, t, status) per ray ON THE
 *                    DEVICE -- g = energy_ratio against pf->u_src and the disc's Keplerian / plunging velocity, ρ = r |sinθ| and
 *                    t = coordinate time of the hit -- and returns min / max ρ over the rays that hit and their number (what
 *                    the radial grid of radial.jl:60-66 is built from);
 *   gr_corona_bin    bins those rays by ρ into the caller's edges (bucket(Simple()): last edge <= ρ, clamped) and returns, per
 *                    bin, the count, Σ g and Σ t (radial.jl:70-84 takes the means).  out: 3 x n_edges doubles, n_edges <= 65536.
 *                    The sums are accumulated as integers on a fixed-point grid finer than an ulp of the values, so they do
 *                    not depend on the order of the additions: the same rays give the same bits on every run.             */
int32_t gr_corona_trace(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                        double* rho_min_max /* 2 */, int64_t* n_hits, gr_stats* stats);
int32_t gr_corona_bin(gr_ctx* ctx, const double* edges, int64_t n_edges, double* out /* 3 x n_edges */);
/* ABI 8 -- the same two calls over SEVERAL contexts from one host thread (see gr_render_multi for the shape every *_multi call
 * has): context k traces a contiguous share of the source's samples (gr_rayset.sky_first / sky_total) and keeps its rows; min / max ρ
 * and the hit count are those of all shares.  gr_corona_bin_multi bins every context's rows into the caller's edges on ONE common
 * fixed-point grid (from the largest |g|, |t| and the hit count of all shares) and adds the integer accumulators: the result is
 * bit for bit what one context gives for the whole source.  stats: n entries or NULL. */
int32_t gr_corona_trace_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                              double* rho_min_max /* 2 */, int64_t* n_hits, gr_stats* stats);
int32_t gr_corona_bin_multi(gr_ctx* const* ctxs, int32_t n, const double* edges, int64_t n_edges, double* out /* 3 x n_edges */);

/* ---- observer -> disc on the device (added within ABI 8, nothing else changes): the second half of lagtransfer and binflux
 * (src/transfer-functions/transfer-functions-2d.jl:141-242) without the 152-byte end points.  Calls on ONE context:
 *   gr_lagtransfer_trace    traces an observer's plane (impact parameters or a separable set, not a sky source) against the disc
 *                           and keeps (g, ρ, t, area) per ray ON THE DEVICE, in a buffer of its own: the corona calls above and
 *                           these do not disturb each other.  g = NaN unless the ray met the geometry; area = rays->area, r_i² of
 *                           a separable plane, or 1.  Returns the number of hits.  A refused trace leaves no rows.
 *   gr_lagtransfer_extrema  over the hits, with E = g E0, t = coordtime(ρ) + t and f = g³ ε(ρ) area: min / max of E and of t (the
 *                           limits bin_transfer_function takes when none are given) and Σ f (the normalisation of binflux).
 *                           An error if the trace had no hit.
 *   gr_lagtransfer_bin      Σ f per cell of the caller's edges (per axis: last edge <= value, clamped to the first / last bin),
 *                           NOT normalised.  n_E, n_t >= 2, ascending, n_E * n_t <= 2^22.  The sums are integers on a fixed-point
 *                           grid like those of gr_corona_bin: the same rows give the same bits for every launch shape.
 *   gr_lagtransfer_rows     the kept rows, n x 4 doubles (for tests and debugging).
 * ε and coordtime are gr_binning's: ρ clamped to the table, then the NaNLinearInterpolator; eps_n = 0: ε(ρ) = ρ^-emissivity_index.
 * Tables and edges are host pointers, staged per call.  Without a trace on the context: GR_ERR_INVALID_ARGUMENT. */
typedef struct gr_lagprofile {
    double E0;                /* energy of the line: E = g E0                               */
    double emissivity_index;  /* ε(ρ) = ρ^-q                                                */
    const double* eps_r;      /* eps_n radii, ascending (eps_n >= 2: tabulated ε)           */
    const double* eps_v;      /* eps_n emissivities                                         */
    int64_t eps_n;
    const double* time_r;     /* time_n >= 2 radii, ascending: the coordtime_at table       */
    const double* time_v;     /* time_n source -> disc coordinate times                     */
    int64_t time_n;
} gr_lagprofile;
int32_t gr_lagtransfer_trace(gr_ctx* ctx, const gr_config* cfg, const gr_rayset* rays, const gr_pointfunction* pf,
                             int64_t* n_hits, gr_stats* stats);
int32_t gr_lagtransfer_extrema(gr_ctx* ctx, const gr_lagprofile* profile, double* lims /* E_min, E_max, t_min, t_max */,
                               double* flux_sum);
int32_t gr_lagtransfer_bin(gr_ctx* ctx, const gr_lagprofile* profile, const double* E_edges, int64_t n_E,
                           const double* t_edges, int64_t n_t, double* out /* host, n_E x n_t, row-major [E][t], raw Σf */);
int32_t gr_lagtransfer_rows(gr_ctx* ctx, double* out /* host, n x 4 */);

/* ---- transfer functions integrated on the device (added within ABI 8, nothing else changes): integrate_lineprofile and
 * integrate_lagtransfer (src/transfer-functions/integration.jl:161-453) for one or many parameter sets in one call -- the
 * shape of a spectral fit, which integrates a table point, an emissivity and an inner radius per iteration.
 * A gr_tfset is self-contained:
 *   transfer functions  n_r >= 2 emission radii (ascending) with their gmin / gmax, and per radius a lower and an upper branch:
 *                       branch (k, lower) owns the knots [off[2k], off[2k+1]), (k, upper) the knots [off[2k+1], off[2k+2]) of
 *                       knot_g (g✶, ascending), knot_f and knot_t; 2 ... 1024 knots per branch, off ascending from off[0] >= 0.
 *                       A CunninghamTransferGrid is the case where every branch has the same knots: the caller replicates them.
 *   annuli              n_int >= 2 integration radii r_int (the caller forms the grid: inverse for a line profile, geometric
 *                       for a lag transfer function), ε(rₑ) and coordtime(rₑ) - t0 at each of them (any emissivity the caller
 *                       can evaluate), r_min (the first annulus is as wide as the second) and g_scale.
 * gr_tfquad: the edge width h of integrate_bin and a quadrature rule on [-1, 1] of n_q <= 32 nodes.
 * Per annulus the branches of the two radii around rₑ are blended linearly (NaNLinearInterpolator per branch, then
 * (1 - w) y1 + w y2), the bin integrals get the weight (rₑ - r_prev) rₑ ε π / (gmax - gmin), and a lag deposit goes to the first
 * t edge >= its arrival time (dropped past the last edge).  Results are RAW sums: _normalize! stays with the caller.  Row
 * n_g - 1 of every set is 0 (n_g edges bound n_g - 1 bins).
 * The sums are integers on a fixed-point grid chosen per set from its largest deposit, like those of gr_lagtransfer_bin: the
 * same arguments give the same bits on every run and for every launch shape, and a set gives the same bits alone or in a batch.
 * All pointers are host pointers, staged per call; the calls keep nothing on the context and disturb nothing it holds.
 * GR_ERR_INVALID_ARGUMENT, before anything touches the device, for: a null pointer, n_sets < 1, n_r < 2, n_int < 2, n_g < 2,
 * n_t < 2, n_q outside 1 ... 32, a branch with fewer than 2 or more than 1024 knots, offsets that do not ascend, and more than
 * 2^24 cells (n_sets n_g n_t). */
typedef struct gr_tfset {
    int64_t n_r;              /* emission radii                                             */
    const double* radii;      /* n_r, ascending                                             */
    const double* gmin;       /* n_r                                                        */
    const double* gmax;       /* n_r                                                        */
    const int64_t* off;       /* 2 n_r + 1 offsets into the knot arrays                     */
    const double* knot_g;     /* off[2 n_r] knots g✶, ascending within a branch             */
    const double* knot_f;     /* transfer function on the knots                             */
    const double* knot_t;     /* disc -> observer coordinate time on the knots              */
    int64_t n_int;            /* annuli                                                     */
    const double* r_int;      /* n_int integration radii                                    */
    const double* eps_int;    /* n_int emissivities ε(rₑ)                                   */
    const double* tsd_int;    /* n_int source -> disc times minus t0 (lag transfer only)    */
    double r_min;             /* inner radius of the integration                            */
    double g_scale;           /* the g edges are divided by it                              */
} gr_tfset;
typedef struct gr_tfquad {
    double h;                 /* integrate_bin's edge width in g✶                           */
    int64_t n_q;              /* 1 ... 32 nodes                                             */
    const double* x;          /* nodes on [-1, 1]                                           */
    const double* w;          /* weights                                                    */
} gr_tfquad;
int32_t gr_tf_lineprofile(gr_ctx* ctx, const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges,
                          int64_t n_g, double* out /* host, n_sets x n_g, raw sums */);
int32_t gr_tf_lagtransfer(gr_ctx* ctx, const gr_tfset* sets, int64_t n_sets, const gr_tfquad* quad, const double* g_edges,
                          int64_t n_g, const double* t_edges, int64_t n_t, double* out /* host, n_sets x n_g x n_t, raw sums */);

/* ---- the lag transfer function of a time-dependent emissivity (added within ABI 8, nothing else changes):
 * integrate_lagtransfer for the RingCoronaProfile / DiscCoronaProfile of an extended corona (src/corona/radial.jl:164-324,
 * src/corona/models/ring.jl:857-950).  A gr_tfprofile is n_rings rings of two arms; an arm is a run of 2 ... 1024 curves
 * (one per slice of the source's sky), a curve >= 2 knots (ρ ascending, t, ε) on the disc.  At an annulus every curve that
 * covers rₑ gives a knot (t, ε) by NaNLinearInterpolator, a curve that does not a NaN; an arm's ε(t) interpolates its knots
 * sorted by t (stable, NaN last) between the first and the last of them and is 0 outside -- so everywhere, if any slice
 * misses rₑ.  The profile at time x is Σ_i (left_i(x - ring_dt[i]) + right_i(x - ring_dt[i])) ring_weight[i]; its limits are
 * the extrema over the arms of the knots' times plus ring_dt, an arm without a knot counting as (0, 0).
 * One set per call; eps_int and tsd_int of the set are not read (they may be null).  Per annulus the weight is
 * (rₑ - r_prev) rₑ π / (gmax - gmin); every g bin is cut into g_upscale fine bins, and each branch of each fine bin deposits
 * ((integrate_bin weight) ε(time_k)) (t_hi - t_lo) / n_time at the first t edge >= (branch time + time_k) - t0 for the n_time
 * samples time_k of linspace(t_lo, t_hi, n_time) (dropped past the last edge).  Results are RAW sums on a fixed-point grid,
 * as gr_tf_lagtransfer forms them: the same arguments give the same bits on every run and for every "tf_chunk".
 * em_out, unless null, receives per annulus t_lo, t_hi and the n_time values ε(time_k).
 * All pointers are host pointers, staged per call; nothing is kept on the context.
 * GR_ERR_INVALID_ARGUMENT, before anything touches the device, for: what gr_tf_lagtransfer refuses, a null pointer, n_rings
 * outside 1 ... 1024, an arm with fewer than 2 or more than 1024 curves, a curve with fewer than 2 knots, offsets that do not
 * ascend, n_time outside 2 ... 1024 and g_upscale outside 1 ... 64. */
typedef struct gr_tfprofile {
    int64_t n_rings;            /* 1 ... 1024                                                                   */
    const double* ring_weight;  /* n_rings (1 for a single RingCoronaProfile)                                   */
    const double* ring_dt;      /* n_rings (0 for a single RingCoronaProfile)                                   */
    const int64_t* arm_off;     /* 2 n_rings + 1: arm (i, left) owns curves [arm_off[2i], arm_off[2i+1]), (i, right) the next run */
    const int64_t* curve_off;   /* arm_off[2 n_rings] + 1 offsets into the knot arrays                          */
    const double* knot_r;       /* ρ, ascending within a curve                                                  */
    const double* knot_t;       /* source -> disc coordinate time on the knots                                  */
    const double* knot_e;       /* emissivity on the knots                                                      */
} gr_tfprofile;
int32_t gr_tf_lagtransfer_td(gr_ctx* ctx, const gr_tfset* set, const gr_tfprofile* prof, const gr_tfquad* quad,
                             const double* g_edges, int64_t n_g, const double* t_edges, int64_t n_t,
                             int64_t g_upscale, int64_t n_time, double t0,
                             double* out /* host, n_g x n_t raw sums */,
                             double* em_out /* host or NULL: n_int x (2 + n_time): t_lo, t_hi, em[k] */);

/* ---- the longitudinal arms of ring coronae (added within ABI 8, nothing else changes): corona_arms for a RingCorona
 * (src/corona/models/ring.jl:1-485) and for the concentric rings of a DiscCorona (src/corona/models/extended.jl:185-200).
 * A ring is one representative point; its sky is cut into slices by the angle β about the point's radial direction, and in
 * a slice a ray leaves at the local angle θ (rotatorfunctor, ring.jl:105-118).  A gr_ringset holds per ring a FRAME of
 * GR_SKY_ROW doubles, laid out as a row of gr_rayset.sky_rows -- position x[4] (x[2] is the angle of the axis), the matrix
 * T diag(1, J) [16], the source velocity with its index lowered [4] and (g_tt, 0, 0, g_tϕ) at x [4] -- the n_slices angles β
 * and the n_base = n_samples - 2 extrema_iter local angles of every slice's base rays, ascending.
 * Every ray is written as (x, v) on the device and traced by the ray-summary launch of gr_ray_summary (any metric, either
 * kernel); g of a row is the energy ratio against ITS ring's source velocity and the disc's Keplerian / plunging velocity, as
 * gr_corona_trace forms it for a source of many positions: pf->pf_id = GR_PF_REDSHIFT and pf->has_u_src = 0.
 * Only cfg->disc_id == GR_DISC_THIN is accepted (GR_ERR_UNSUPPORTED otherwise).  All pointers are host pointers, staged per
 * call; nothing is kept on the context.
 *
 * gr_ring_rays forms and traces n rays, ray j at the local angle angles[j] in slice ring_slice[2 j + 1] of ring
 * ring_slice[2 j]: rows_out[j] = (g, ρ, t, status), v_out[j] (unless null) the formed, unconstrained velocity.  n_base,
 * extrema_iter and base_angles of the set are not read.
 *
 * gr_ring_arms is the producer in one call: the base rays of every slice of every ring in one launch, then per slice two
 * golden-section searches side by side -- for the minimal and for the maximal ρ (_determine_bracket, _golden_bracket!,
 * ring.jl:131-237) -- all slices in lock-step: per iteration one launch forms the two probe rays of every search that is
 * still live, one traces them and one updates the brackets, until no search is live (at most 2 extrema_iter + 1 iterations).
 *   rows_out[ring][slice][n_base + 2 extrema_iter][5] = (θ as probed, g, ρ, t, status): the n_base base rows, then the probes
 *       the minima search kept, then those the maxima search kept (the reference's order); zeros behind them.
 *   counts_out[ring][slice][3] = (n_base, kept by the minima search, kept by the maxima search); a slice none of whose base
 *       rays met the disc -- an error in the reference -- has (n_base, -1, -1) and no search.
 * GR_ERR_INVALID_ARGUMENT for: a null pointer, n_rings, n_slices or extrema_iter < 1, n_base < 2, more than 2^31 - 1 base rays,
 * a ring or slice index out of range, pf->has_u_src != 0. */
typedef struct gr_ringset {
    int64_t n_rings;
    int64_t n_slices;
    int64_t n_base;             /* base rays per slice (gr_ring_arms)                                           */
    int64_t extrema_iter;       /* the searches' iteration count (gr_ring_arms)                                 */
    const double* frames;       /* n_rings x GR_SKY_ROW                                                         */
    const double* betas;        /* n_slices                                                                     */
    const double* base_angles;  /* n_base, ascending (gr_ring_arms)                                             */
} gr_ringset;
int32_t gr_ring_rays(gr_ctx* ctx, const gr_config* cfg, const gr_ringset* rings, const gr_pointfunction* pf, int64_t n,
                     const int64_t* ring_slice /* host, n x 2 */, const double* angles /* host, n */,
                     double* rows_out /* host, n x 4 */, double* v_out /* host, n x 4, or NULL */, gr_stats* stats);
int32_t gr_ring_arms(gr_ctx* ctx, const gr_config* cfg, const gr_ringset* rings, const gr_pointfunction* pf,
                     double* rows_out /* host, n_rings x n_slices x (n_base + 2 extrema_iter) x 5 */,
                     int64_t* counts_out /* host, n_rings x n_slices x 3 */, gr_stats* stats);

/* ---- the cells of a source's adaptive sky (added within ABI 8; AdaptiveSky, src/corona/adaptive-sample.jl:43-81) ----
 * Cell j is the direction (θ_j = acos(cos_theta[j]), ϕ_j = phi[j]) on the local sky of a source at x_src with the sky frame
 * Mx = T diag(1, J) (the matrix a gr_rayset's sky source carries): v = Mx (1, -k̂), k̂ = (sin θ cos ϕ, sin θ sin ϕ, cos θ).  The
 * TANGENT kernels trace it with ∂/∂θ and ∂/∂ϕ of the sky angles seeded on that velocity (closed form, formed on the device) --
 * the reference's dual numbers through the integrator -- and write one CoronaGridValues row of 6 doubles per cell:
 *     t, r = x^r |sin x^θ|, ϕ = x^ϕ (unwrapped, as integrated), g, J = |∂(r, ϕ)/∂(θ, ϕ_sky)| / sin θ, status
 * with g the redshift point function's energy ratio against pf->u_src and status the reference's float code: 1 = the ray met
 * the geometry, -3 = within the inner boundary, 7 = out of the domain, 0 = anything else.  A cell whose ray does not meet the
 * geometry has NaN in t, r, ϕ, g and J.  gr_ctx_set "tangent_pairs" / "tangent_norm" apply as for gr_ray_tangent.
 * GR_ERR_INVALID_ARGUMENT, before anything touches the device, for: a null pointer, cfg->disc_id == GR_DISC_NONE, a point
 * function other than the redshift or without has_u_src, a source outside the radial range of a GR_METRIC_TABULATED table and
 * (where the angles are host arrays: not gr_sky_cells_device) |cos θ| >= 1.
 * gr_sky_cells_multi: contiguous shares of the cells, one per context, the rows of one context bit for bit. */
typedef struct gr_skycells {
    double x_src[4];          /* the source's position                                                       */
    double Mx[16];            /* row-major 4 x 4: tetrad of the source times diag(1, Cartesian -> spherical) */
    const double* cos_theta;  /* n (gr_sky_cells_device: device memory)                                      */
    const double* phi;        /* n (gr_sky_cells_device: device memory)                                      */
    int64_t n;
} gr_skycells;
int32_t gr_sky_cells(gr_ctx* ctx, const gr_config* cfg, const gr_skycells* cells, const gr_pointfunction* pf,
                     double* out /* host, n x 6 */, gr_stats* stats);
int32_t gr_sky_cells_device(gr_ctx* ctx, const gr_config* cfg, const gr_skycells* cells, const gr_pointfunction* pf,
                            double* d_out /* device, n x 6 */, gr_stats* d_stats, void* hip_stream);
int32_t gr_sky_cells_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_skycells* cells,
                           const gr_pointfunction* pf, double* out /* host, n x 6 */, gr_stats* stats /* n, or NULL */);

/* ---- an adaptive sky resident on the device (added within ABI 8; AdaptiveSky, src/image-planes/adaptive-sky.jl, and the
 * drivers of src/corona/adaptive-sample.jl:486-842) ----
 * A gr_sky is the 3 x 3 refinement tree of Grids.AdaptiveGrid over (cos θ, ϕ) with one row of 6 doubles per cell, kept in the
 * context's device memory between refinement steps: cells count from 1 in the order they were made, row 0 is a null cell, the
 * children of the k-th cell of a refinement list take the indices n + 1 + 9 k ... n + 9 + 9 k (column order; the middle child
 * inherits its parent's row), neighbours are (top, right, bottom, left).  It keeps COPIES of cfg, cells (x_src, Mx) and pf:
 * the tables they point to must outlive the sky.  One context; the calls of one sky come from one thread at a time.
 *
 * A criterion decides per pair (leaf, bordering leaf) whether the BORDERING leaf is refined.  A pair of cells that both miss
 * (NaN r) is always left alone.  GR_SKY_CRIT_DEFAULT: g or J of the two rows are not isapprox at rtol (false on NaN);
 * GR_SKY_CRIT_FUNCTION: either row lies in one of the boxes; GR_SKY_CRIT_FINE: both of these; GR_SKY_CRIT_LEVEL: the bordering
 * leaf's level is below `level`.  A box is an r interval and zero, one or two intervals of fmod(ϕ, 2π) (+ 2π where negative),
 * every bound open or closed. */
#define GR_SKY_MAX_BOXES 8
enum { GR_SKY_CRIT_DEFAULT = 0, GR_SKY_CRIT_FUNCTION = 1, GR_SKY_CRIT_FINE = 2, GR_SKY_CRIT_LEVEL = 3,
       GR_SKY_CRIT_PLANE = 4 /* a plane sky's (gr_sky_create_plane, below) */ };
typedef struct gr_sky_box {
    double r_lo, r_hi;
    double phi_lo[2], phi_hi[2];
    int32_t r_open_lo, r_open_hi;      /* 1: the bound itself lies outside                                   */
    int32_t phi_open_lo, phi_open_hi;  /* ... of every ϕ interval                                            */
    int32_t n_phi;                     /* 0: any ϕ                                                           */
    int32_t reserved;
} gr_sky_box;
typedef struct gr_sky_criterion {
    int32_t kind;                      /* GR_SKY_CRIT_*                                                      */
    int32_t level;                     /* GR_SKY_CRIT_LEVEL                                                  */
    double rtol;                       /* percentage / 100                                                   */
    int32_t n_boxes;                   /* 0 ... GR_SKY_MAX_BOXES                                             */
    int32_t reserved;
    gr_sky_box boxes[GR_SKY_MAX_BOXES];
} gr_sky_criterion;
typedef struct gr_sky gr_sky;
/* The nine top cells over limits = (x1, x2, y1, y2); nothing is traced.  Refused as gr_sky_cells_device refuses. */
int32_t gr_sky_create(gr_ctx* ctx, const gr_config* cfg, const gr_skycells* source /* x_src, Mx */, const gr_pointfunction* pf,
                      const double* limits /* 4 */, int32_t x_periodic, gr_sky** sky);
int32_t gr_sky_destroy(gr_sky* sky);
int32_t gr_sky_size(gr_sky* sky, int64_t* n_cells);
/* trace_initial!: the nine cells, then every leaf refined level - 1 times; launch_sizes receives the cells each of the `level`
 * launches traced (9, 72, 648 for level 3) */
int32_t gr_sky_trace_initial(gr_sky* sky, int32_t level, int64_t* launch_sizes /* level, or NULL */);
/* find_need_refine: the bordering leaves the criterion names, ascending, left in a device list; only their number comes back.
 * gr_sky_need_refine_list copies that list out. */
int32_t gr_sky_find_need_refine(gr_sky* sky, const gr_sky_criterion* criterion, int64_t* count);
int32_t gr_sky_need_refine_list(gr_sky* sky, int64_t* cells /* host, count */);
/* every (leaf, bordering leaf) pair in the reference's visiting order: leaves ascending, each with its bordering leaves top,
 * right, bottom, left.  n receives their number; the pairs are written if cap >= n (i1, i2 may be NULL to ask for n only). */
int32_t gr_sky_pairs(gr_sky* sky, int64_t* i1 /* host, cap */, int64_t* i2 /* host, cap */, int64_t cap, int64_t* n);
/* refine_and_trace!: the list of the last gr_sky_find_need_refine (cells = NULL; n is ignored) or n cells of a host list.  The
 * eight outer children of every cell are traced in ONE gr_sky_cells_device launch (`traced` receives its size).
 * GR_ERR_INVALID_ARGUMENT, with the sky as it was, for an index outside 1 ... n_cells, a cell that is refined already, a cell
 * named twice, a cell at level GR_SKY_MAX_LEVEL (20) and for cells = NULL without a list. */
int32_t gr_sky_refine_and_trace(gr_sky* sky, const int64_t* cells /* host, n, or NULL */, int64_t n, int64_t* traced,
                                gr_stats* stats);
/* per (r, ϕ) bin the number of leaves that land in it (adaptive-sample.jl:337-348: r not NaN and not above the largest edge,
 * the last edge <= r and <= fmod(ϕ, 2π)) and whose J g^Γ is not ±0; gamma = NULL leaves the redshift out.  bin_emissivity_grid
 * is non-zero exactly in the bins counted here.  Integer sums: the same counts on every run. */
int32_t gr_sky_occupancy(gr_sky* sky, const double* r_bins, int64_t n_r, const double* phi_bins, int64_t n_phi,
                         const double* gamma /* 1, or NULL */, int64_t* counts /* host, n_r x n_phi */);
/* the arrays of cells first_cell ... first_cell + count - 1 (row 0 included if first_cell = 0), and -- for first_cell >= 10,
 * where every nine cells are the children of one refined cell -- those cells and their rows of `children` */
int32_t gr_sky_download(gr_sky* sky, int64_t first_cell, int64_t count, double* pos /* count x 2 */, void* level /* count int32_t */,
                        int64_t* children /* count x 9 */, int64_t* neighbours /* count x 4 */, int64_t* parent,
                        void* location /* count int8_t */, double* rows /* count x 6 */, int64_t* refined /* count / 9, or NULL */,
                        int64_t* refined_children /* count / 9 x 9, or NULL */);

/* ---- the (r, ϕ) maps and the filled image of a resident sky (added within ABI 8) ----
 * γ(r) A(r) of the disc in the equatorial plane at n radii: γ the Lorentz factor of the disc's velocity in the LNRF (Keplerian
 * from pf->r_isco out; inside it the plunging table of pf clamped to its ends, or Kerr's analytic plunge when pf brings no
 * table -- the branches of the REDSHIFT point function), A = 2π √(g_rr g_ϕϕ).  pf as gr_apply_pointfunction takes it.
 * gr_disc_area_factor_device: r and out are device memory, nothing is waited for. */
int32_t gr_disc_area_factor_device(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf, const double* d_r, int64_t n,
                                   double* d_out, void* hip_stream);
int32_t gr_disc_area_factor(gr_ctx* ctx, const gr_config* cfg, const gr_pointfunction* pf, const double* r /* host, n */, int64_t n,
                            double* out /* host, n */);
/* bin_emissivity_grid / bin_redshift_grid / bin_time_grid (adaptive-sample.jl:266-450): over the leaves gr_sky_occupancy keeps,
 * with ΔΩ = wx wy / sin(acos(cos θ)) of a leaf, out = Σ ΔΩ w / Σ ΔΩ per bin (0 where Σ ΔΩ = 0) for w = J g^Γ γ(r) A(r)
 * (gamma = NULL leaves g^Γ out), w = g or w = t; solid_angle receives Σ ΔΩ.  The sums are integer sums on a fixed-point grid
 * (two integers per value): the same bits on every run and for every launch shape.  A bin with a NaN term is NaN; an infinite
 * term makes it ±∞ (NaN for both signs).  An empty sky gives zeros.
 * GR_ERR_INVALID_ARGUMENT, before anything touches the device, for: r_bins, phi_bins or out null, a bin count outside
 * 1 ... 46340, a sky that has not been traced, edges that do not ascend, `what` outside the enum.
 * GR_ERR_UNSUPPORTED if a bin with non-zero terms and no NaN sums to 0: its terms lie below the resolution of the sums (2^(2 en - 124)
 * of the map's largest term rounded up to a power of two, 2^en >= the cell count: 2^-86 at half a million cells), and a map that
 * is 0 where gr_sky_occupancy counts would read as unlit. */
enum { GR_SKY_MAP_EMISSIVITY = 0, GR_SKY_MAP_REDSHIFT = 1, GR_SKY_MAP_TIME = 2 };
int32_t gr_sky_bin_grid(gr_sky* sky, int32_t what, const double* r_bins, int64_t n_r, const double* phi_bins, int64_t n_phi,
                        const double* gamma /* 1, or NULL: leave g^Γ out */, double* out /* host, n_r x n_phi */,
                        double* solid_angle /* host, n_r x n_phi, or NULL */);
/* fill_sky_values (adaptive-sample.jl:196-250): per column ϕ_k the distinct leaves that hold (cos θ_j, ϕ_k), ordered by
 * θ = acos(cos θ of the leaf); every point takes the interval of searchsorted(θ_j, side = right) clipped to [1, cells - 1] and
 * interpolates the six row fields linearly in θ.  The θ grid may come in any order (it is walked in ascending order, the results
 * land at the caller's indices).  A column with fewer than two leaves is NaN.  `cells`: the lower and the upper
 * leaf of every point (0, 0 in a NaN column).  GR_ERR_INVALID_ARGUMENT for a null grid or out, a count outside 1 ... 46340, a sky
 * that has not been traced; GR_ERR_UNSUPPORTED if a column does not meet its leaves in ascending θ (no tree of disjoint
 * rectangles does that). */
int32_t gr_sky_fill(gr_sky* sky, const double* phi_grid, int64_t n_phi, const double* theta_grid, int64_t n_theta,
                    double* out /* host, n_theta x n_phi x 6 */, int64_t* cells /* host, n_theta x n_phi x 2, or NULL */);

/* ---- an observer's adaptive image plane (added within ABI 8; AdaptivePlane, src/image-planes/adaptive-plane.jl) ----
 * Cell j is the ray of impact parameters (alpha[j], beta[j]) of an observer at plane->x_obs: the unconstrained velocity
 * v = Mx local_momentum(x_obs[1], -alpha, beta) (the sign of alpha: adaptive-plane.jl:81) is formed on the device and traced to its
 * end point, one gr_point per cell.  Of `plane` only x_obs and Mx are read.  cfg->disc_id may be GR_DISC_NONE.
 * GR_ERR_INVALID_ARGUMENT, before anything touches the device, for a null pointer and for an observer outside the radial range
 * of a GR_METRIC_TABULATED table.  gr_plane_cells_device: alpha, beta and the points are device memory, nothing is waited for.
 * gr_plane_cells_multi: contiguous shares of the cells, one per context, the points of one context bit for bit. */
int32_t gr_plane_cells(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane /* x_obs, Mx */, const double* alpha /* host, n */,
                       const double* beta /* host, n */, int64_t n, gr_point* out /* host, n */, gr_stats* stats);
int32_t gr_plane_cells_device(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane, const double* d_alpha, const double* d_beta,
                              int64_t n, gr_point* d_out, gr_stats* d_stats, void* hip_stream);
int32_t gr_plane_cells_multi(gr_ctx* const* ctxs, int32_t n_ctx, const gr_config* cfg, const gr_plane* plane, const double* alpha,
                             const double* beta, int64_t n, gr_point* out /* host, n */, gr_stats* stats /* n_ctx, or NULL */);
/* A gr_sky over (alpha, beta) whose rows are gr_point records -- row 0 a NoStatus one with NaN fields: the tree of gr_sky_create with every new
 * cell traced by gr_plane_cells_device; the middle child of a refined cell inherits its parent's whole point.  gr_sky_size,
 * gr_sky_trace_initial, gr_sky_find_need_refine, gr_sky_need_refine_list, gr_sky_pairs, gr_sky_refine_and_trace, gr_sky_destroy
 * and the tree arrays of gr_sky_download work on it as on a corona sky.  Its criteria are GR_SKY_CRIT_PLANE (adaptive-plane.jl:24-50:
 * with "hit" = status IntersectedWithGeometry, a pair that both miss is left alone, a pair of which one hits is refined, a pair
 * that both hit is refined if log10 x[1] or fmod(x[2], 2π) (+ 2π where negative) of the two points are not isapprox at rtol) and
 * GR_SKY_CRIT_LEVEL (a pair that both miss is left alone).  GR_ERR_INVALID_ARGUMENT, with the sky untouched, for the corona kinds
 * DEFAULT / FUNCTION / FINE on a plane sky, for GR_SKY_CRIT_PLANE on a corona sky, for gr_sky_occupancy, gr_sky_bin_grid,
 * gr_sky_fill and the `rows` of gr_sky_download on a plane sky, and for the two calls below on a corona sky. */
int32_t gr_sky_create_plane(gr_ctx* ctx, const gr_config* cfg, const gr_plane* plane /* x_obs, Mx */, const double* limits /* 4 */,
                            int32_t x_periodic, gr_sky** sky);
int32_t gr_sky_download_points(gr_sky* sky, int64_t first_cell, int64_t count, gr_point* out /* host, count */);
/* fill_sky_values of a plane (adaptive-plane.jl:100-181) from one value per cell: pf evaluated on the resident points
 * (gr_apply_pointfunction_device, max_time = cfg->lambda1), or cell_values, or -- both NULL -- x[0] of every point (the
 * reference's default pf).  Per column x_k the y grid is walked ascending and every run of points held by one cell c is recorded;
 * c's value is interpolated in x with its left (x_k < pos_x(c)) or right neighbour unless there is none, it lies across the
 * periodic wrap or its ray did not hit; the column's abscissae are pos_y(c); every point takes the interval
 * clamp(searchsortedlast(column, y), 1, cells - 1) and interpolates linearly in y.  out[j * n_x + k] belongs to (x_k, y_j); a
 * column with fewer than two cells is NaN (cells 0, 0).  The y grid may come in any order.  Refused as gr_sky_fill refuses. */
int32_t gr_sky_fill_plane(gr_sky* sky, const gr_pointfunction* pf /* or NULL */, const double* cell_values /* host, n_cells + 1, or NULL */,
                          const double* x_grid, int64_t n_x, const double* y_grid, int64_t n_y, double* out /* host, n_y x n_x */,
                          int64_t* cells /* host, n_y x n_x x 2, or NULL */);

/* ---- tabulated metrics (ABI 7; segments, axis terms: ABI 8; GR_METRIC_TABULATED): the AbstractMetric plugin interface on the device ----
 * Host-only functions (no context, no device): plan a grid, learn its nodes, fit, check.
 *
 *   gr_metric_grid g;  gr_metric_grid_plan(r_min, r_max, r0, m_r, n_theta, &g);
 *   gr_metric_grid_nodes(&g, r_nodes, theta_nodes);                 // g.n_r_nodes radii, g.n_theta_nodes angles
 *   samples[(a * g.n_theta_nodes + b) * 5 + k] = metric_components(m, (r_nodes[a], theta_nodes[b]))[k];   // the caller's metric
 *   gr_metric_table_fit(&g, samples, table, err);                   // table: g.table_doubles doubles
 *   cfg.metric_id = GR_METRIC_TABULATED; cfg.metric_table = table; cfg.metric_table_n = g.table_doubles;
 *
 * Radial patches are the m_r equal parts of every octave [2^e, 2^(e+1)) of r - r0 between r_min and r_max: choose r0 at (or just
 * inside) the event horizon -- inner_radius(m) -- and r_min = the chart's inner radius, so that the patches shrink geometrically
 * towards the pole of g_rr; r_max = the chart's outer radius (the entry points refuse a chart, an observer or a source outside
 * [r_min, r_max]: polynomials do not extrapolate).  Polar patches: n_theta equal parts of [0, π]; the components are
 * taken to be even about both poles (θ outside [0, π] is folded).  err[0..2] receive the fit's own estimates of the largest
 * truncation error of a component, of its ∂/∂ln(r - r0) and of its ∂/∂θ, each relative to the component's magnitude on the
 * patch: refine (m_r, n_theta) until they are below what the integration tolerance needs.
 *
 * ABI 8 -- metrics that are PIECEWISE in r (the reference's KerrDarkMatter, src/metrics/kerr-dark-matter.jl:12-20: kinks at rₛ and
 * rₛ + Δr; KerrRefractive, kerr-refractive-ad.jl:26 with utils.jl:158-168: jumps at corona_radius ± δx/2 and an arctangent step
 * of width δx/10⁴ between them) name their break radii: gr_metric_grid_plan_breaks starts a new radial SEGMENT at every break,
 * anchored there (octaves of r - break, behind a core of m_r equal parts of the first octave's width), so that no patch straddles
 * a break and the rows next to one are fitted on their own side only.  A break with scale > 0 is a feature of that width centred
 * there: the patches shrink geometrically towards it from BOTH sides, down to that scale.  Radii may be negative (a chart through
 * the throat of src/metrics/morris-thorne-ad.jl's wormhole: a break at 0 with scale b): a segment measures distances from its
 * anchor.  gr_metric_grid_plan is the call without breaks: one segment, anchored at r0. */
#define GR_METRIC_MAX_SEG 12
typedef struct gr_metric_break {
    double radius;            /* where metric_components changes form                                         */
    double scale;             /* 0: a kink or a jump AT radius; > 0: a smooth feature of this width centred at radius */
} gr_metric_break;
typedef struct gr_metric_segment {
    double r_lo, r_hi;        /* radii r_lo <= r < r_hi take this segment                                    */
    double anchor;            /* x = dir (r - anchor) > 0 inside the segment                                 */
    double xmin;              /* 2^e_lo                                                                       */
    double fit_lo, fit_hi;    /* the metric is smooth on (fit_lo, fit_hi) ⊇ [r_lo, r_hi): no node lies outside (±inf: no limit) */
    int32_t e_lo, e_hi;       /* octaves 2^e_lo .. 2^(e_hi + 1) of x                                          */
    int32_t first_row, n_rows; /* radial rows (core + e_hi - e_lo + 1) m_r of the table                       */
    int32_t dir;              /* +1 | -1                                                                      */
    int32_t core;             /* 1: m_r equal parts of [0, 2^e_lo) come first                                 */
} gr_metric_segment;
typedef struct gr_metric_grid {
    double r0;                /* origin of the radial octaves of segment 0                                   */
    double r_min, r_max;      /* radii the table covers (patch edges are rounded outwards)                   */
    int32_t e_min, n_oct;     /* segment 0: octaves 2^e_min .. 2^(e_min + n_oct) of r - r0                   */
    int32_t m_r, n_theta;     /* patches per octave, patches over [0, π]                                     */
    int32_t degree, fit_nodes; /* total degree of a patch polynomial (5), Chebyshev nodes per patch and direction (12) */
    int32_t pole_factor;      /* the form g_ϕϕ and g_tϕ are stored in (the caller may change it between plan and fit):
                                 1 [set by gr_metric_grid_plan]: divided by sin²θ -- both vanish like sin²θ on the axis of a regular
                                 axis-symmetric metric, and a polynomial with an ABSOLUTE error would leave g^ϕϕ with an unbounded
                                 RELATIVE one for rays that graze the axis; the kernels multiply the factor (and its derivative) back.
                                 2: g = K_m(r) + K_d(r) cos θ + sin²θ h(r, θ) -- a metric whose g_ϕϕ, g_tϕ do NOT vanish on the axis
                                 (an axion charge: the reference's DilatonAxion with β != 0): K_m ± K_d, the limits on the two poles,
                                 are taken from the samples nearest the poles and stored as polynomials per radial row.
                                 0: stored as sampled (the reference's MorrisThorneWormhole, g_ϕϕ ∝ sin θ)                        */
    int32_t n_seg;            /* radial segments (1 without breaks)                                          */
    int64_t n_r_nodes;        /* n_rows * fit_nodes                                                          */
    int64_t n_theta_nodes;    /* n_theta * fit_nodes                                                         */
    int64_t table_doubles;    /* length of the table gr_metric_table_fit writes                              */
    int32_t n_rows;           /* radial rows of all segments                                                 */
    int32_t reserved;
    gr_metric_segment seg[GR_METRIC_MAX_SEG];
} gr_metric_grid;
int32_t gr_metric_grid_plan(double r_min, double r_max, double r0, int32_t m_r, int32_t n_theta, gr_metric_grid* grid);
int32_t gr_metric_grid_plan_breaks(double r_min, double r_max, double r0, int32_t m_r, int32_t n_theta, int32_t n_breaks,
                                   const gr_metric_break* breaks /* n_breaks, any order */, gr_metric_grid* grid);
int32_t gr_metric_grid_nodes(const gr_metric_grid* grid, double* r_nodes, double* theta_nodes);
int32_t gr_metric_table_fit(const gr_metric_grid* grid, const double* samples /* n_r_nodes x n_theta_nodes x 5 */,
                            double* table /* table_doubles */, double* err /* 3, may be NULL */);
/* the table's value at one point, by the arithmetic the kernels use: (g, ∂r g, ∂θ g) of the five components -- for checking a
 * table against the caller's own Jacobian (Julia: Gradus.metric_jacobian) before tracing with it */
int32_t gr_metric_table_eval(const double* table, int64_t table_n, double r, double theta, double* g /* 5 */, double* dr /* 5 */,
                             double* dth /* 5 */);

/* ---- compiled metrics (additive within ABI 8; GR_METRIC_COMPILED): a user's component function as kernels of its own ----
 * The tabulated route carries a metric across this ABI as samples.  This one carries it as CODE: the five components written
 * as the body of GenericMetricT<GR_METRIC_COMPILED>::components (csrc/gr_usermetric.hpp: + - * on typed dual numbers, inv_,
 * dsqrt, dexp, dlog, dpowi<N>, sin θ and cos θ as `s` and `c`, run-time parameters as P[0..5], results through dput(g[i], ...)),
 * compiled with the library's own kernels_tu.hip (-DGR_TU_METRIC=12 -DGR_TU_USER -DGR_USER_COMPONENTS_FILE=\"...\", the seven
 * flavours fp64 / area factor / two tangent shapes / two sky-cell shapes / offset solve) and linked into ONE shared module that
 * exports the launchers gr64_launch_{trace,path,apply,classify,areafactor}_m12, grt_, grt1_, grts_, grts1_launch_trace_m12,
 * grv1_launch_offset_m12 and gr_user_module_info.  The Python host writes the body from a numpy callable
 * (metrics.CompiledMetric); any tool that emits C expressions can.
 *
 *   int64_t id;  gr_metric_module_load("/path/to/module.so", &id);     // GR_METRIC_COMPILED + slot
 *   cfg.metric_id = (int32_t)id;  cfg.params[0..5] = ...;                        // then every entry point as for the catalogue
 *   gr_metric_module_unload(id);
 *
 * A compiled metric is traced by eval() + the generic contraction like the catalogue's dual-number form, takes no miss cull
 * (like every metric but Kerr) and has no fp32 flavour.  Learned state that is keyed by a configuration (the longest-first
 * tile order) keys a compiled metric by its module's BUILD ID, not by its slot: slots are reused after an unload. */
typedef struct gr_user_module_info_t {
    int32_t abi_version;      /* GR_ABI_VERSION the module was compiled against */
    int32_t metric_id;        /* GR_METRIC_COMPILED */
    int64_t build_id;         /* > 0, unique per generated source + kernel sources + flags + compiler: what caches key on */
    int64_t header_hash[4];   /* sha256 of the csrc/ sources and this header the module was compiled against, as four words */
} gr_user_module_info_t;
/* every module exports `gr_user_module_info`: a C function without arguments that returns a pointer to one of these */

typedef struct gr_metric_resources {
    int32_t vgprs;            /* vector registers per lane (hipFuncGetAttributes numRegs) */
    int32_t scratch_bytes;    /* private memory per lane: > 0 means the kernel spills */
    int32_t lds_bytes;        /* static LDS per workgroup */
    int32_t max_threads;      /* maxThreadsPerBlock */
} gr_metric_resources;
enum { GR_MODULE_KERNEL_TRACE_LANE = 0, GR_MODULE_KERNEL_TRACE_PERSISTENT = 1, GR_MODULE_KERNEL_TANGENT = 2,
       GR_MODULE_KERNEL_TANGENT_PAIRS = 3, GR_MODULE_KERNEL_COUNT = 4 };

/* dlopen `path` (RTLD_LOCAL), check gr_user_module_info against this library (ABI version and header hash must be equal:
 * GR_ERR_INVALID_ARGUMENT with both values in the message otherwise; so for a file that is not a module or lacks a launcher of
 * the fp64 set) and keep it in a process-wide registry of GR_METRIC_MODULE_SLOTS slots.  *metric_id = GR_METRIC_COMPILED + slot.
 * GR_ERR_UNSUPPORTED when every slot is taken.  Needs no device.  Thread-safe. */
int32_t gr_metric_module_load(const char* path, int64_t* metric_id);
/* free the slot (the module's code stays mapped: a launch in flight may still be running it).  A config that names the id
 * afterwards is refused (GR_ERR_UNSUPPORTED), like any unknown metric_id.  GR_ERR_INVALID_ARGUMENT for an id that is not loaded. */
int32_t gr_metric_module_unload(int32_t metric_id);
/* the module's build id (0 and GR_ERR_INVALID_ARGUMENT for an id that is not loaded) */
int32_t gr_metric_module_build_id(int32_t metric_id, int64_t* build_id);
/* registers and scratch of the module's trace kernels as compiled for `cfg` (the kernels are instantiated per disc type):
 * out[GR_MODULE_KERNEL_*].  Needs a device (hipFuncGetAttributes). */
int32_t gr_metric_module_resources(int32_t metric_id, const gr_config* cfg, gr_metric_resources* out /* GR_MODULE_KERNEL_COUNT */);

/* ---- ONE host thread, SEVERAL devices, ray sets (see gr_render_multi for the shape every *_multi call has) ---- */
/* Ray sets with one output row per ray (gr_rayset_endpoints, gr_ray_summary, gr_ray_tangent, gr_redshift_radius): contiguous
 * shares as above.  A separable ray set must come whole and in ray order (sep_block = 0, sep_tiled = 0). */
int32_t gr_rayset_endpoints_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                                  gr_point* points /* host, rays->n */, gr_stats* stats);
int32_t gr_ray_summary_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                             const gr_pointfunction* pf, double* out /* host, rays->n x 4 */, gr_stats* stats);
int32_t gr_ray_tangent_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                             const gr_pointfunction* pf, double* out /* host, rays->n x 8 */, gr_stats* stats);
int32_t gr_redshift_radius_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                                 const gr_pointfunction* pf, double r_min, double r_max,
                                 double* pairs /* host, rays->n x 2 */, gr_stats* stats);
/* gr_offset_solve / gr_offset_search: the problems are dealt in contiguous shares (multiples of 64), the results land at the
 * caller's indices and are the bytes one context gives. */
int32_t gr_offset_solve_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                              const gr_pointfunction* pf, const gr_offset_problems* problems,
                              double* out /* host, problems->n x 10 */, gr_stats* stats);
int32_t gr_offset_search_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                               const gr_pointfunction* pf, const gr_offset_searches* searches,
                               double* out /* host, searches->n x (12 (iterations + 1) + 1) */, gr_stats* stats);
/* lineprofile(bins, ε, m, x, d, BinningMethod(); plane) (src/line-profiles.jl:152-198): the rays are dealt block-cyclically
 * (a separable plane: one block = one strip of 8 x 8 tiles, all radii of 8 neighbouring angles, so every device sees every
 * radius; ray arrays: contiguous shares), each device bins its own rays into its own histogram and the host adds the n
 * histograms in context order.  The order in which a bin receives its rays differs from the one-context call, so the sums
 * agree to rounding (1e-13 relative), not bit for bit.  A separable ray set must come whole (sep_block = 0). */
int32_t gr_lineprofile_multi(gr_ctx* const* ctxs, int32_t n, const gr_config* cfg, const gr_rayset* rays,
                             const gr_pointfunction* pf, const gr_binning* b, double* flux /* host, n_bins */,
                             gr_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* GRADUS_MI355X_H */
