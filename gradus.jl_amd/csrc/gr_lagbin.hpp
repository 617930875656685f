// gr_lagbin.hpp -- the per-hit arithmetic of the 2-D lag-energy transfer function (binflux / bin_transfer_function,
// src/transfer-functions/transfer-functions-2d.jl:98-121,211-241) and the fixed-point grid its sums are formed on.
// Plain functions for the host and the device: k_lag_extrema / k_lag_bin (gradus_mi355x.hip) call them per row, and
// tests/host_harness_lagbin.cpp compiles the same text with g++ against numpy.
//
// A row is (g, ρ, t_obs, area) with g = NaN unless the ray met the geometry.  For a hit
//     E = g E0,   t = coordtime(ρ) + t_obs,   f = g³ ε(ρ) area
// and its cell is (last E edge <= E, last t edge <= t), each clamped to the first / last bin.  The cell of a hit has to be the
// one numpy finds from the same row, so nothing here may be contracted into an fma: E and t are compared with edges that numpy
// formed with one rounding per operation (the library is built with -ffp-contract=on, which would fuse (1 - w) y1 + w y2).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GR_LAG_DEV __host__ __device__ __forceinline__
#else
#define GR_LAG_DEV inline
#endif
#if defined(__clang__)
#define GR_LAG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GR_LAG_NO_CONTRACT      // (g++ fuses only with -mfma / -march; the harness is built with -ffp-contract=off all the same)
#endif

namespace gr_lag {

// what turns a row into (E, t, f): gr_lagprofile with its tables where the caller of these functions can read them
struct Profile {
    double E0;
    double q;                               // ε(ρ) = ρ^-q unless eps_n >= 2
    const double *eps_r, *eps_v;
    int64_t eps_n;
    const double *time_r, *time_v;          // coordtime_at: time_n >= 2 radii, ascending, and times
    int64_t time_n;
};

// emissivity_at / coordtime_at of a radial profile: ρ clamped to the table, then the NaNLinearInterpolator of
// src/interpolations.jl:1-30 exactly as corona._nan_linear_interp evaluates it -- (1 - w) y1 + w y2 between the nodes around ρ
// (the last node <= ρ and its successor); a NaN result falls back to the nearer node, and to 0 if that is NaN too.
GR_LAG_DEV double table_at(const double* r, const double* v, int64_t n, double rho)
{
    GR_LAG_NO_CONTRACT
    const double rc = fmin(fmax(rho, r[0]), r[n - 1]);
    int64_t a = 0, b = n;                   // number of nodes <= rc (searchsorted, side = "right")
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (r[mid] <= rc) a = mid + 1; else b = mid;
    }
    const int64_t i0 = (a < 1 ? 1 : (a > n - 1 ? n - 1 : a)) - 1;
    const double x1 = r[i0], x2 = r[i0 + 1], y1 = v[i0], y2 = v[i0 + 1];
    const double w = (rc - x1) / (x2 - x1);
    const double lo = (1.0 - w) * y1, hi = w * y2;
    double y = lo + hi;
    if (y != y) {
        const double pick = w < 0.5 ? y1 : y2;
        y = (pick != pick) ? 0.0 : pick;
    }
    return y;
}

GR_LAG_DEV double emissivity(const Profile& p, double rho)
{
    return p.eps_n >= 2 ? table_at(p.eps_r, p.eps_v, p.eps_n, rho) : pow(rho, -p.q);
}

struct Hit { double E, t, f; };

// false for a row that is no hit (g is NaN)
GR_LAG_DEV bool hit_of(const Profile& p, const double* row, Hit& h)
{
    GR_LAG_NO_CONTRACT
    const double g = row[0], rho = row[1];
    if (!(g == g)) return false;
    h.E = g * p.E0;
    const double tc = table_at(p.time_r, p.time_v, p.time_n, rho);
    h.t = tc + row[2];
    const double g3 = (g * g) * g, ge = g3 * emissivity(p, rho);
    h.f = ge * row[3];
    return true;
}

// reverberation._bucket_index: the last edge <= v, clamped to the first / last bin (the binary search of k_corona_bin)
GR_LAG_DEV int bucket(const double* edges, int n, double v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo > 0 ? lo - 1 : 0;
}

// Radius index of local ray jl of a separable ray set (gr_rayset.sep_*): the row part of the map Ray::sep_global / Ray::sep_index
// (gr_device.hpp) apply when they form the ray -- column-major over (radius, angle), walked in 8 x 8 tiles inside the block of
// core_rows x core_cols when the set is tiled -- so that a row's area is r_i² of ITS ray.
struct LagSep { const double* r; int64_t nr, core_rows, core_cols, first, block, stride; };
GR_LAG_DEV int64_t sep_row(const LagSep& p, int64_t jl)
{
    int64_t k = p.first + jl;
    if (p.block > 0) {
        const int64_t b = jl / p.block;
        k = p.first + b * p.stride + (jl - b * p.block);
    }
    const int64_t R = p.core_rows, Cc = p.core_cols, core = R * Cc;
    if (k < core) return ((((k >> 6) % (R >> 3)) << 3) + (k & 7));
    k -= core;
    const int64_t tail = p.nr - R;
    if (k < Cc * tail) return R + k % tail;
    return (k - Cc * tail) % p.nr;
}

// A double as an unsigned integer whose order is the order of the values (negative ones included), for integer atomicMin / Max
GR_LAG_DEV unsigned long long ordered_bits(double v)
{
    union { double d; unsigned long long u; } c;
    c.d = v;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
GR_LAG_DEV double ordered_value(unsigned long long k)
{
    union { double d; unsigned long long u; } c;
    c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.d;
}

// A double as two integers of a fixed-point grid whose step is a power of two chosen from the largest magnitude and the number
// of values (CoronaScale): hi = round(v / step), lo = round((v / step - hi) 2^K).  Integer sums do not depend on the order of
// the additions, so the per-bin sums -- and with them the whole profile -- are the same bits on every run and for every launch
// shape, which floating-point atomics are not; the grid resolves step 2^-K, below one ulp of any value within 2^10 of the
// largest, so the sums are also as accurate as a sorted pairwise fp64 sum.
struct CoronaScale { double inv_step, two_k; };
GR_LAG_DEV void corona_split(double v, const CoronaScale& sc, long long& hi, long long& lo)
{
    const double s = v * sc.inv_step;             // exact: a power of two
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __double2ll_rn(s);
    lo = __double2ll_rn((s - (double)hi) * sc.two_k);
#else
    hi = llrint(s);                               // (round to nearest even, the mode the host runs in)
    lo = llrint((s - (double)hi) * sc.two_k);
#endif
}

// step = 2^(e + en - 62) with vmax < 2^e and n <= 2^en: Σ |hi| < 2^62, every hi below 2^(62 - en) <= 2^52 (exact in a double),
// K = 62 - en: Σ |lo| < 2^61.
struct CoronaGrid { CoronaScale sc; double step, lo_unit; };
inline CoronaGrid corona_grid(double vmax, int64_t n)
{
    int en = 10;
    while (en < 40 && ((int64_t)1 << en) < n) ++en;
    int e = 0;
    if (vmax > 0.0 && std::isfinite(vmax)) (void)std::frexp(vmax, &e);      // vmax = f 2^e, f in [0.5, 1)
    const int k = 62 - en;
    CoronaGrid g;
    g.step = std::ldexp(1.0, e + en - 62);
    g.sc.inv_step = std::ldexp(1.0, -(e + en - 62));
    g.sc.two_k = std::ldexp(1.0, k);
    g.lo_unit = std::ldexp(1.0, -k);
    return g;
}
// the sum the two accumulators of a cell stand for
inline double corona_sum(long long hi, long long lo, const CoronaGrid& g)
{
    return (double)(((long double)hi + (long double)lo * (long double)g.lo_unit) * (long double)g.step);
}

}  // namespace gr_lag
