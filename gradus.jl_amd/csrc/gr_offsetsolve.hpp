// gr_offsetsolve.hpp -- the emission-radius offset solve and the redshift-extremum search of the Cunningham transfer functions as
// RESUMABLE STATE MACHINES, one problem each, for the host and the device.
//
//   Solve   _find_offset_for_radius (src/tracing/precision-solvers.jl:135-236) for ONE (r_target, θ): transfer_functions.py's
//           find_offsets_for_radius_newton_ad restated step for step.  That function advances a batch in lock-step, one launch of
//           gr_ray_tangent per round, and no problem of the batch depends on its neighbours: a problem's iteration index is the
//           round index.  Here the iteration is turned inside out: `solve_start` names the first offset to trace, `solve_feed`
//           takes the 8-double row of that ray (g, ρ, ∂g/∂α, ∂g/∂β, ∂ρ/∂α, ∂ρ/∂β, t, status: out_mode 5) and names the next one or
//           says that the iteration is over.  Whoever traces -- a lane pair of k_offset_solve, a loop of the host harness -- holds no
//           other state.
//   Search  _search_extremal! (src/transfer-functions/cunningham-transfer-functions.jl:390-438) as _golden_section_batch runs it
//           with depth 1: golden section on sign·g over θ, every evaluation a whole Solve at that θ.
//
// Every update has to be the number numpy makes from the same numbers: one rounding per operation, nothing contracted into an fma
// (GR_OS_NO_CONTRACT; the discipline of gr_skygrid.hpp / gr_planegrid.hpp), comparisons that are false on NaN where numpy's are, and
// np.maximum's NaN.  The functions read no array with a runtime index: the six `previous` slots are members picked by a switch, a
// row is copied by unrolled loops (a runtime-indexed private array is scratch memory on the device).
//
// The device kernels (k_offset_solve, k_offset_search) are at the end, compiled into objects of their own (kernels_tu.hip,
// -DGR_TU_TAN1 -DGR_TU_SOLVE).
#pragma once

#include <cmath>
#include <cstdint>

#ifdef GR_HOST_HARNESS
#define GR_OS_FN inline
#else
#define GR_OS_FN __host__ __device__ __forceinline__
#endif
#if defined(__clang__)
#define GR_OS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GR_OS_NO_CONTRACT      // (g++ fuses only with -mfma / -march)
#endif

namespace gr_os {

constexpr int kRow = 8;               // doubles of a tangent summary
constexpr int kSolveOut = 10;         // doubles per problem of a solve: r, the row the iteration ended on, rays traced
constexpr int kRecord = 12;           // doubles per evaluation of a search: θ after the nudge, r, row, rays traced, failure flag
constexpr int kBracketRounds = 60;    // Roots.find_zero's bisection, as find_offsets_for_radius_newton_ad bounds it
constexpr double kGolden = 0.5 * (3.0 - 2.23606797749979);      // transfer_functions.GOLDEN: the literal is sqrt(5.0) to the bit
constexpr double kPi = 3.141592653589793;
constexpr double kHit = 2.0;          // GR_STATUS_INTERSECTED_WITH_GEOMETRY as a row holds it

// doubles of a search's output: iterations + 1 records, then the minimum found
GR_OS_FN int64_t search_stride(int64_t iterations) { return (iterations + 1) * kRecord + 1; }

// what a launch shares among its problems
struct Setup {
    double alpha0, beta0, zero_atol, r_min, contrapoint_bias;
    int32_t max_iter;
    int32_t iterations;      // golden-section steps of a search
};

enum Phase : int32_t { kFirst = 0, kNewton = 1, kBiased = 2, kBracket = 3 };

struct Solve {
    // one problem
    double r_target, c, s;
    // the iteration's variables, named as find_offsets_for_radius_newton_ad names them
    double x, y, df, contra;
    double point[kRow];      // (indexed by constants only)
    double p0, p1, p2, p3, p4, p5;      // previous[0..5]
    double lo, hi;           // the bracket of the bisection finish
    double cur;              // the offset of the ray being traced
    int32_t i, it, phase, n_rays;
};

GR_OS_FN double np_maximum(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}
GR_OS_FN double np_abs(double a) { return __builtin_fabs(a); }

// the impact parameters of the offset `r` of a problem
GR_OS_FN void aim(const Solve& q, const Setup& st, double r, double& alpha, double& beta)
{
    GR_OS_NO_CONTRACT
    const double a = r * q.c, b = r * q.s;
    alpha = a + st.alpha0;
    beta = b + st.beta0;
}

// -> the first offset to trace: the reference's cold start
GR_OS_FN double solve_start(Solve& q, double r_target, double c, double s)
{
    q.r_target = r_target; q.c = c; q.s = s;
    q.x = np_maximum(20.0, r_target);
    q.y = 0.0; q.df = 0.0; q.contra = 0.0;
#pragma unroll
    for (int k = 0; k < kRow; ++k) q.point[k] = 0.0;
    q.p0 = q.p1 = q.p2 = q.p3 = q.p4 = q.p5 = 0.0;
    q.lo = q.hi = 0.0;
    q.i = 0; q.it = 0; q.phase = kFirst; q.n_rays = 0;
    q.cur = q.x;
    return q.cur;
}

GR_OS_FN void set_point(Solve& q, const double* row)
{
#pragma unroll
    for (int k = 0; k < kRow; ++k) q.point[k] = row[k];
}

// Roots.find_zero(..., (contra, x), atol = zero_atol) begins: the first midpoint
GR_OS_FN bool bracket_begin(Solve& q)
{
    GR_OS_NO_CONTRACT
    q.lo = q.contra; q.hi = q.x; q.it = 0;
    q.phase = kBracket;
    const double sum = q.lo + q.hi;
    q.cur = 0.5 * sum;
    return false;
}

// the head of the loop `while active.any() and i <= max_iter` for this problem, and what follows the loop
GR_OS_FN bool next_round(Solve& q, const Setup& st)
{
    GR_OS_NO_CONTRACT
    const bool active = np_abs(q.y) > st.zero_atol;
    if (active && q.i <= st.max_iter) {
        const double quot = q.y / q.df;
        q.cur = q.x - quot;
        q.phase = kNewton;
        return false;
    }
    // "Exceeded max iter": still iterating and far off
    if (q.i >= st.max_iter && active && q.y > 10.0) return bracket_begin(q);
    return true;
}

// the part of a round behind `step(next_x)` and the biased bisection step, if one was taken
GR_OS_FN bool after_step(Solve& q, const Setup& st, double next_x, double next_y, double df2, const double* row)
{
    GR_OS_NO_CONTRACT
    const double ny = -q.y;
    const double push = ny / df2;
    const bool stop = (next_y < 0.0) && (q.y < 0.0) && (push < 0.0);
    const double dy = q.y - next_y;
    const double next_dy = dy / q.y;
    const double tol = st.zero_atol * 100.0;
    const bool seen = (np_abs(q.p0 - next_dy) <= tol) || (np_abs(q.p1 - next_dy) <= tol) || (np_abs(q.p2 - next_dy) <= tol)
                      || (np_abs(q.p3 - next_dy) <= tol) || (np_abs(q.p4 - next_dy) <= tol) || (np_abs(q.p5 - next_dy) <= tol);
    const bool cycle = !stop && (q.y > 0.0) && seen;
    if (stop) {
        // "Converge failed": x and y stay, the point is the new one; the problem leaves the loop
        set_point(q, row);
        q.df = df2;
        return true;
    }
    if (cycle) return bracket_begin(q);      // ... finished off by bracketing, and the loop is left
    q.x = next_x; q.y = next_y; q.df = df2;
    set_point(q, row);
    switch (q.i % 6) {
    case 0: q.p0 = next_dy; break;
    case 1: q.p1 = next_dy; break;
    case 2: q.p2 = next_dy; break;
    case 3: q.p3 = next_dy; break;
    case 4: q.p4 = next_dy; break;
    default: q.p5 = next_dy; break;
    }
    q.i += 1;
    return next_round(q, st);
}

// the row of the ray at offset q.cur -> true: the iteration is over (solve_result), false: trace q.cur next
GR_OS_FN bool solve_feed(Solve& q, const Setup& st, const double* row)
{
    GR_OS_NO_CONTRACT
    q.n_rays += 1;
    const double da = row[4] * q.c, db = row[5] * q.s;
    const double df_new = da + db;
    const double y_new = row[1] - q.r_target;
    if (q.phase == kFirst) {
        set_point(q, row);
        q.df = df_new; q.y = y_new;
        return next_round(q, st);
    }
    if (q.phase == kNewton) {
        const double next_x = q.cur;
        const bool fell_short = (next_x < 0.0) || ((y_new < 0.0) && (q.y > 0.0));
        if (fell_short) q.contra = np_maximum(q.contra, next_x);
        const double hole = st.r_min + 1.0;
        if (fell_short && ((next_x < 0.0) || (row[1] < hole))) {
            const double num = q.contra * st.contrapoint_bias;
            const double sum = num + q.x, den = 1.0 + st.contrapoint_bias;
            q.cur = sum / den;
            q.phase = kBiased;
            return false;
        }
        return after_step(q, st, next_x, y_new, df_new, row);
    }
    if (q.phase == kBiased) return after_step(q, st, q.cur, y_new, df_new, row);
    // kBracket: one more midpoint; the reference re-evaluates step(x) at the last one -- its values are these
    q.x = q.cur; q.y = y_new; q.df = df_new;
    set_point(q, row);
    if (y_new < 0.0) q.lo = q.cur; else q.hi = q.cur;
    q.it += 1;
    if (np_abs(y_new) <= st.zero_atol || q.it >= kBracketRounds) return true;
    const double sum = q.lo + q.hi;
    q.cur = 0.5 * sum;
    return false;
}

// the accepted offset, or NaN: x >= 0 && |y| <= 1e-4 r_target && IntersectedWithGeometry
GR_OS_FN double solve_result(const Solve& q)
{
    GR_OS_NO_CONTRACT
    const double worst = 1e-4 * q.r_target;
    const bool ok = (q.x >= 0.0) && (np_abs(q.y) <= worst) && ((int32_t)q.point[7] == (int32_t)kHit);
    return ok ? q.x : __builtin_nan("");
}

// out[kSolveOut]: r, the row, rays traced
GR_OS_FN void solve_store(const Solve& q, double* out)
{
    out[0] = solve_result(q);
#pragma unroll
    for (int k = 0; k < kRow; ++k) out[1 + k] = q.point[k];
    out[1 + kRow] = (double)q.n_rays;
}

// ---- the extremum search ----
struct Search {
    double r_target, sign;
    double lower, upper, xmin, fmin, new_x;
    double theta;            // the angle being solved at, after the pole nudge
    int32_t k;               // evaluations recorded
    int32_t failed;
};

// θ -> θ after the pole nudge, and the solve at it begins: -> the first offset to trace
GR_OS_FN double search_eval(Search& s, Solve& q, double theta)
{
    GR_OS_NO_CONTRACT
    const double at = np_abs(theta);
    const bool pole = (at < 1e-4) || (np_abs(at - kPi) < 1e-4);
    s.theta = pole ? theta + 1e-4 : theta;
    return solve_start(q, s.r_target, ::cos(s.theta), ::sin(s.theta));
}

GR_OS_FN double search_start(Search& s, Solve& q, double r_target, double lower, double upper, double sign)
{
    GR_OS_NO_CONTRACT
    s.r_target = r_target; s.sign = sign; s.lower = lower; s.upper = upper;
    s.k = 0; s.failed = 0; s.fmin = 0.0;
    const double w = upper - lower, gw = kGolden * w;
    s.xmin = lower + gw;
    s.new_x = s.xmin;
    return search_eval(s, q, s.xmin);
}

// A solve of the search has ended: its record goes to rec[kRecord]; -> true: the search is over (*minimum is written), false: the
// next solve has begun and q.cur is its first offset.
GR_OS_FN bool search_feed(Search& s, Solve& q, const Setup& st, double* rec, double* minimum)
{
    GR_OS_NO_CONTRACT
    const double r = solve_result(q);
    rec[0] = s.theta;
    rec[1] = r;
#pragma unroll
    for (int k = 0; k < kRow; ++k) rec[2 + k] = q.point[k];
    rec[2 + kRow] = (double)q.n_rays;
    const bool bad = r != r;
    rec[3 + kRow] = bad ? 1.0 : 0.0;
    if (bad) {
        s.failed = 1;
        *minimum = __builtin_nan("");
        return true;
    }
    const double f = s.sign * q.point[0];
    if (s.k == 0) {
        s.fmin = f;
    } else {
        const bool right = (s.upper - s.xmin) > (s.xmin - s.lower);
        const bool better = f < s.fmin;
        const double lo = (right && better) ? s.xmin : ((!right && !better) ? s.new_x : s.lower);
        const double up = (right && !better) ? s.new_x : ((!right && better) ? s.xmin : s.upper);
        s.lower = lo; s.upper = up;
        if (better) { s.xmin = s.new_x; s.fmin = f; }
    }
    s.k += 1;
    if (s.k > st.iterations) {
        *minimum = s.fmin;
        return true;
    }
    const double above = s.upper - s.xmin, below = s.xmin - s.lower;
    const double ga = kGolden * above, gb = kGolden * below;
    s.new_x = (above > below) ? s.xmin + ga : s.xmin - gb;
    search_eval(s, q, s.new_x);
    return false;
}

// device pointers of a launch (work block: alpha | beta | rows, n each)
struct OffsetDev {
    const double* r_target;      // n
    const double* a;             // solve: cos θ        search: lower
    const double* b;             // solve: sin θ        search: upper
    const double* sign;          // search only
    double* alpha;               // n (Cold::alpha)
    double* beta;                // n (Cold::beta)
    double* rows;                // n x 8 (Cold::lp_pairs)
    double* out;                 // solve: n x kSolveOut        search: n x search_stride(iterations)
    Setup st;
    int32_t per_wave;            // problems a wave carries, 1 ... 32
};

}  // namespace gr_os

// ---------------------------------------------------------------------------------------------------------------------------
// The kernels.  Included by kernels_tu.hip behind gr_kernels.hpp with -DGR_TU_TAN1 -DGR_TU_SOLVE: the pair shape only (GR_TAN_W = 1,
// one wave per SIMD), one shape for every launch size -- what keeps a root independent of how many problems share its launch.
//
// A lane PAIR carries one problem from its cold start to its accepted root (k_offset_solve), or one golden-section search -- its
// iterations + 1 root finds -- from start to finish (k_offset_search).  Both lanes of a pair run the same state machine on the same
// numbers: the value part of a pair's ray is computed twice anyway (gr_tangent.hpp), the solver's handful of operations per ray
// likewise, and no state crosses lanes but the partner's column of the row.
//
// ONE step loop per wave (the idiom of k_trace_persistent): a pair whose ray has ended finalizes it, feeds the row to its state
// machine, re-initialises the ray and goes on stepping; the loop ends when no pair of the wave is live.  With the ray loop nested
// inside the solver loop a wave would pay, iterate by iterate, its slowest ray; flattened it pays the slowest SUM.
//
// The ray itself is Ray<Metric, DISC> as gr_ray_tangent drives it (src_mode 2, out_mode 5) and is not touched: its impact
// parameters are read from Cold::alpha / beta [problem], its row is written to Cold::lp_pairs [8 problem] -- slots of the launch's
// work block that only this pair uses.  Both lanes store the same α, β before init() reads them back (a lane reads its own store).
// The row is written half by each lane (finalize: the even lane the values and ∂/∂α, the odd one ∂/∂β); both lanes are in finalize
// together (same values, same branches), and a workgroup-scope release / acquire fence stands between those stores and the volatile
// loads that read the whole row back.
// ---------------------------------------------------------------------------------------------------------------------------
#if defined(GR_TU_SOLVE) && !defined(GR_HOST_HARNESS)
namespace GR_NS {
namespace {

constexpr int kOffsetBlock = 64;      // many small workgroups: one wave each

struct OffsetNoSearch {};
template <bool SEARCH>
struct OffsetLaneState {
    gr_os::Solve q;
    typename std::conditional<SEARCH, gr_os::Search, OffsetNoSearch>::type s;
};

template <class Metric, int DISC, bool SEARCH>
__device__ __forceinline__ void offset_wave(const Params& p, const gr_os::OffsetDev& d)
{
    Metric m;
    m.load(p.cfg);
    const int lane = (int)(threadIdx.x & 63u);
    const int slot = lane >> 1;
    const int64_t j = (int64_t)blockIdx.x * d.per_wave + slot;
    bool live = slot < d.per_wave && j < p.n;
    LaneStats<Metric, DISC> ls;
    const LdsView lds = lds_prologue<ColdSel<Metric>::kBytesPerThread>(p);
    const typename ColdSel<Metric>::type cs = cold_store_of<ColdSel<Metric>>(p);
    Ray<Metric, DISC> ray;
    // The solver's state lives in LDS, a slot per lane: the ray takes the registers (the Kerr search had 36 bytes of scratch per lane
    // with the state in registers beside it), and the state is touched once per RAY, not per step.
    __shared__ OffsetLaneState<SEARCH> state[kOffsetBlock];
    gr_os::Solve& q = state[threadIdx.x].q;
    auto& s = state[threadIdx.x].s;
    const gr_os::Setup st = d.st;
    const int64_t stride = SEARCH ? gr_os::search_stride(st.iterations) : gr_os::kSolveOut;

    if (live) {
        if constexpr (SEARCH) gr_os::search_start(s, q, d.r_target[j], d.a[j], d.b[j], d.sign[j]);
        else gr_os::solve_start(q, d.r_target[j], d.a[j], d.b[j]);
    }
    bool fresh = true;      // the pair's next ray, at the offset q.cur, has yet to be set up
    while (__any(live)) {
        if (live) {
            if (fresh) {
                double al, be;
                gr_os::aim(q, st, q.cur, al, be);
                d.alpha[j] = al;
                d.beta[j] = be;
                ray.init(m, p, j);      // never decided at the start: the tangent launches leave Params::r_cull_start at +inf
                fresh = false;
            }
            if (ray.step(m, p, cs)) {
                ray.finalize(m, p, lds);
                if (tan_dir() == 0) ls.add(ray);      // a ray is counted once
                // the partner's column of the row: its stores are behind the release, the loads below behind the acquire
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const volatile double* vr = d.rows + gr_os::kRow * j;
                double row[gr_os::kRow];
#pragma unroll
                for (int k = 0; k < gr_os::kRow; ++k) row[k] = vr[k];
                bool done = gr_os::solve_feed(q, st, row);
                if (done) {
                    if constexpr (SEARCH) {
                        // both lanes hold the same record: the even lane stores it
                        double rec[gr_os::kRecord], fmin = 0.0;
                        const int k_rec = s.k;
                        done = gr_os::search_feed(s, q, st, rec, &fmin);
                        if (tan_dir() == 0) {
                            double* o = d.out + stride * j + (int64_t)gr_os::kRecord * k_rec;
#pragma unroll
                            for (int k = 0; k < gr_os::kRecord; ++k) o[k] = rec[k];
                            if (done) d.out[stride * j + stride - 1] = fmin;
                        }
                    } else {
                        if (tan_dir() == 0) gr_os::solve_store(q, d.out + stride * j);
                    }
                }
                if (done) live = false;
                else fresh = true;
            }
        }
    }
    ls.template flush<false>(p.stats);
}

template <class Metric, int DISC>
__global__ void __launch_bounds__(kOffsetBlock) k_offset_solve(const Params p, const gr_os::OffsetDev d)
{
    offset_wave<Metric, DISC, false>(p, d);
}
template <class Metric, int DISC>
__global__ void __launch_bounds__(kOffsetBlock) k_offset_search(const Params p, const gr_os::OffsetDev d)
{
    offset_wave<Metric, DISC, true>(p, d);
}

template <class Metric, int DISC>
hipError_t launch_offset_tmpl(Params& p, const gr_os::OffsetDev& d, bool search, hipStream_t stream)
{
    // the LDS of a one-wave workgroup of the lane kernel (launch_tmpl): the plunging table, a tabulated metric's patch cache
    p.lds_points = 0;
    p.lds_bins = 0;
    if (ColdSel<Metric, true>::kTab) p.lds_plunge_rows = 0;
    size_t lds = sizeof(double) * 4 * (size_t)p.lds_plunge_rows + ColdSel<Metric, true>::kBytesPerThread * (size_t)kOffsetBlock;
    lds = (lds + 15) & ~(size_t)15;
    p.lds_tab_off = (int32_t)lds;
    lds += ColdSel<Metric, true>::kTabBytesPerWave;
    const int64_t grid = (p.n + d.per_wave - 1) / d.per_wave;
    if (search) hipLaunchKernelGGL((k_offset_search<Metric, DISC>), dim3((unsigned)grid), dim3(kOffsetBlock), lds, stream, p, d);
    else hipLaunchKernelGGL((k_offset_solve<Metric, DISC>), dim3((unsigned)grid), dim3(kOffsetBlock), lds, stream, p, d);
    return hipGetLastError();
}

template <class Metric>
hipError_t launch_offset_metric(Params& p, const gr_os::OffsetDev& d, bool search, hipStream_t stream)
{
    switch (p.cfg.disc_id) {
    case GR_DISC_THIN: return launch_offset_tmpl<Metric, GR_DISC_THIN>(p, d, search, stream);
    case GR_DISC_DATUM: return launch_offset_tmpl<Metric, GR_DISC_DATUM>(p, d, search, stream);
    default: return hipErrorInvalidValue;      // the host unit refuses every other geometry before it gets here
    }
}

}  // namespace
}  // namespace GR_NS
#endif
