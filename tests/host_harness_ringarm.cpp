// host_harness_ringarm.cpp -- TEST INFRASTRUCTURE.  The arithmetic of gr_ring_rays / gr_ring_arms (gr_ringarm.hpp) compiled for
// the host with g++: ray formation, the bracket of a slice and a whole golden-section search over a caller's objective table,
// with the header's functions in the order the kernels call them.  Never linked into libgradus_mi355x.so.
#include <cstdint>

#include "../gradus.jl_amd/csrc/gr_ringarm.hpp"

extern "C" {

double hring_invphi() { return gr_ring::kInvPhi; }

// v[n][4], f[n] of the rays at local angles theta[n] in the slice beta of one frame
void hring_form_rays(const double* frame, double beta, const double* theta, int64_t n, double* v, double* f)
{
    for (int64_t j = 0; j < n; ++j) gr_ring::form_ray(frame, beta, theta[j], v + 4 * j, f[j]);
}

// out = (a, b, best); returns 0 when no row of the slice met the geometry
int hring_bracket(const double* rows, const double* angles, int N, int target, double* out)
{
    return gr_ring::bracket(rows, angles, N, target, out[0], out[1], out[2]) ? 1 : 0;
}

// one update: state = (a, b, best, n, iters, too_many, done) in and out; returns what to append (0 | 1 | 2)
int hring_update(double* state, int target, int extrema_iter, int c_status, double c_rho, int d_status, double d_rho)
{
    gr_ring::Search s{ state[0], state[1], state[2], (int32_t)state[3], (int32_t)state[4], (int32_t)state[5], (int32_t)state[6] };
    const int append = gr_ring::golden_update(s, target, extrema_iter, c_status, c_rho, d_status, d_rho);
    state[0] = s.a; state[1] = s.b; state[2] = s.best;
    state[3] = s.n; state[4] = s.iters; state[5] = s.too_many; state[6] = s.done;
    return append;
}

// the two probe angles of a state
void hring_probes(const double* state, double* cd)
{
    const gr_ring::Search s{ state[0], state[1], state[2], (int32_t)state[3], (int32_t)state[4], (int32_t)state[5], (int32_t)state[6] };
    gr_ring::probes(s, cd[0], cd[1]);
}

}      // extern "C"
