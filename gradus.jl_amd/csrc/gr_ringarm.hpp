// gr_ringarm.hpp -- the arithmetic of the producer of a ring corona's longitudinal arms (corona_arms,
// src/corona/models/ring.jl:1-485) outside the trace itself: forming the ray of a (ring, slice β, local angle θ) triple
// (rotatorfunctor, ring.jl:105-118, through sky_angles_to_velocity, samplers.jl:81-99), the initial bracket of an extremum of
// ρ(θ) from a slice's traced base rows (_determine_bracket, ring.jl:131-166) and one iteration of the golden-section search
// on it (_golden_bracket!, ring.jl:172-237).
// Plain functions for the host and the device: k_ring_rays / k_ring_bracket / k_ring_probe / k_ring_update
// (gradus_mi355x.hip) call them, and tests/host_harness_ringarm.cpp compiles the same text with g++ against numpy.  The
// bracket and the golden update are sums, differences and one product by INVPHI: with nothing contracted into an fma numpy
// forms the same bits (gr_lagbin.hpp); the ray formation goes through libm (sin, cos, atan2) and agrees to rounding.
#pragma once
#include "gr_lagbin.hpp"

namespace gr_ring {

constexpr int kFrame = 28;                        // doubles of a ring's frame: the layout of a gr_rayset.sky_rows row
constexpr int kHit = 2;                           // GR_STATUS_INTERSECTED_WITH_GEOMETRY
constexpr double kInvPhi = 0.6180339887498949;    // (sqrt(5) - 1) / 2, ring.jl:1
constexpr double kPi = 3.14159265358979323846;
constexpr int kMinima = 0, kMaxima = 1;

// One search: the bracket [a, b], the counter n the loop ends on, the iterations made, the too_many_iters flag and the
// estimate the bracket was found with -- never updated inside the loop (ring.jl:186-236).
struct Search {
    double a, b, best;
    int32_t n, iters, too_many, done;
};

// comparator of a target (ring.jl:178-184): strict
GR_LAG_DEV bool better(int target, double x, double y) { return target == kMinima ? x < y : x > y; }

// The unconstrained velocity of the ray that leaves a ring's representative point at local angle θ in the slice β, and the
// factor f that turns the trace's energy ratio against the static observer into the ratio against the ring's own velocity.
// frame: x[4], Mx[16] = T diag(1, J) (tetrad times Cartesian -> spherical Jacobian), u_μ[4] of the source, g_tμ[4] at x.
//   q = dir(θ + axis, 0), k = dir(axis, 0), b = q cos β + (k × q) sin β + k (k · q) (1 - cos β)      (emissivity.jl:220)
//   ph = atan2(b₂, b₁), th = atan2(sqrt(b₂² + b₁²), b₃), k̂ = -dir(th, ph), v = Mx (1, k̂)
GR_LAG_DEV void form_ray(const double* frame, double beta, double theta, double v[4], double& f)
{
    GR_LAG_NO_CONTRACT
    const double axis = frame[2];
    const double k[3] = { ::sin(axis) * ::cos(0.0), ::sin(axis) * ::sin(0.0), ::cos(axis) };
    const double tq = theta + axis;
    const double q[3] = { ::sin(tq) * ::cos(0.0), ::sin(tq) * ::sin(0.0), ::cos(tq) };
    const double cb = ::cos(beta), sb = ::sin(beta);
    const double kxq[3] = { k[1] * q[2] - k[2] * q[1], k[2] * q[0] - k[0] * q[2], k[0] * q[1] - k[1] * q[0] };
    const double kq = k[0] * q[0] + k[1] * q[1] + k[2] * q[2];
    double b[3];
    for (int i = 0; i < 3; ++i) b[i] = q[i] * cb + kxq[i] * sb + k[i] * kq * (1.0 - cb);
    const double ph = ::atan2(b[1], b[0]);
    const double th = ::atan2(::sqrt(b[1] * b[1] + b[0] * b[0]), b[2]);
    const double st = ::sin(th), ct = ::cos(th), sp = ::sin(ph), cp = ::cos(ph);
    const double pb[4] = { 1.0, -(st * cp), -(st * sp), -ct };
    const double* M = frame + 4;
    for (int r = 0; r < 4; ++r) v[r] = M[r * 4 + 0] * pb[0] + M[r * 4 + 1] * pb[1] + M[r * 4 + 2] * pb[2] + M[r * 4 + 3] * pb[3];
    double eu = 0.0, et = 0.0;
    for (int r = 0; r < 4; ++r) { eu += frame[20 + r] * v[r]; et += frame[24 + r] * v[r]; }
    f = eu / et;
}

// _determine_bracket (ring.jl:131-166) on a slice's N base rows (g, ρ, t, status), traced at `angles` in ascending order.
// Returns false when no row of the slice met the geometry (the reference then fails converting `nothing`).
GR_LAG_DEV bool bracket(const double* rows, const double* angles, int N, int target, double& a, double& b, double& best)
{
    GR_LAG_NO_CONTRACT
    a = b = angles[0];
    bool have = false;
    double estimate = 0.0;
    for (int i = 0; i < N; ++i) {
        if ((int)rows[4 * i + 3] != kHit) continue;
        const double rho = rows[4 * i + 1];
        if (!have || better(target, rho, estimate)) {
            have = true;
            estimate = rho;
            a = b = angles[i];
            if (i < N - 1 && (int)rows[4 * (i + 1) + 3] != kHit) b = angles[i + 1];      // likely a better upper limit
            if (i > 0 && (int)rows[4 * (i - 1) + 3] != kHit) a = angles[i - 1];          // likely a better lower limit
        }
    }
    const double delta = kPi / (double)(N < 32 ? N : 32);
    a = a - 2.0 * delta;
    b = b + 2.0 * delta;
    best = estimate;
    return have;
}

// the two probe angles of the next iteration (ring.jl:207-208)
GR_LAG_DEV void probes(const Search& s, double& c, double& d)
{
    GR_LAG_NO_CONTRACT
    c = s.b - (s.b - s.a) * kInvPhi;
    d = s.a + (s.b - s.a) * kInvPhi;
}

// One iteration of _golden_bracket! (ring.jl:206-236) given the outcomes of the probes at c and d.  A probe that missed
// takes the value `best`; a probe joins the slice's cache only when it beats `best`; n also counts every iteration once
// iters has passed extrema_iter.  Returns 0: nothing to append, 1: the probe at c, 2: the probe at d.
GR_LAG_DEV int golden_update(Search& s, int target, int extrema_iter, int c_status, double c_rho, int d_status, double d_rho)
{
    double c, d;
    probes(s, c, d);
    const double c_value = c_status == kHit ? c_rho : s.best;
    const double d_value = d_status == kHit ? d_rho : s.best;
    int append = 0;
    if (better(target, c_value, d_value)) {
        if (better(target, c_value, s.best)) { s.n += 1; append = 1; }
        else if (s.too_many) s.n += 1;
        s.b = d;
    } else {
        if (better(target, d_value, s.best)) { s.n += 1; append = 2; }
        else if (s.too_many) s.n += 1;
        s.a = c;
    }
    s.iters += 1;
    if (!s.too_many && s.iters > extrema_iter) s.too_many = 1;
    s.done = s.n < extrema_iter ? 0 : 1;
    return append;
}

}      // namespace gr_ring
