// gr_tile_order.hpp -- the order in which the one-ray-per-lane kernel takes the pixel tiles of an image launch: the tiles whose
// rays are traced ("live") first, the tiles the start cull decides ("dead") last, each class in ascending tile index.
//
// Under the start cull (Ray::init) most waves of a deep image launch end without a step: 61 % of the 2048² bench
// render's waves, about 4 % of its work, scattered among the live ones in tile order; each holds a wave slot for some 14 µs and
// issues next to nothing.  Taken last they hold slots while the last live waves drain, when slots are free anyway.
//
// Two small kernels ahead of the trace launch, on its stream (gr_kernels.hpp, gradus_mi355x.hip):
//   k_tile_classify   four threads per tile ask Ray::init's own start decision (Ray::decided_at_start) of the tile's four CORNER
//                     rays and write one flag byte: 1 = all four are decided at the start, 0 = the tile is traced (a ray left
//                     to the defer cull is traced);
//   k_tile_partition  turns the flags into Cold::tile_perm (queue position -> tile) by a stable partition: thread t owns the flags
//                     [chunk_lo(t), chunk_lo(t + 1)) -- one tile on the device, a thread per tile --, learns how many flags are
//                     set before its chunk and in all, and places its tiles -- no atomics, so the order is the same at every
//                     launch.
// The flag is a guess about the other 60 rays, nothing more: tile_swizzle only reads the permutation, every ray is still decided
// or traced by the trace kernel itself, and a misplaced tile merely runs in the other class.  Which way a guess may be wrong is
// not indifferent, though: a live tile called dead starts among the last waves of the launch and may be its tail.  On the bench
// render (host census, scripts/live_first_model.py) one inner ray per tile calls 345 of the 25 325 live tiles dead, the four
// corners call two -- single undecided rays 45 tiles away from any other, which nothing short of asking all 64 rays finds -- and
// no dead tile live.
//
// Plain C++ with no device types: the partition's arithmetic is compiled for the host as well (tests/host_harness_tile_order.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GR_ORDER_FN __host__ __device__ inline
#else
#define GR_ORDER_FN inline
#endif

namespace gr_order {

constexpr int kPartitionThreads = 1024;      // threads of a workgroup of k_tile_partition (a multiple of 64 and of 8)
constexpr int kClassLanes = 4;               // rays of a tile that k_tile_classify asks (a power of two: a group of lanes per tile)

// lane of the k-th corner of a tile of 2^rows_log2 rows (Cold::swizzle: 3 = 8 x 8, 4 = 16 x 4; lane = column * rows + row)
GR_ORDER_FN int class_lane(int rows_log2, int k)
{
    const int rows = 1 << rows_log2;
    return k == 0 ? 0 : k == 1 ? rows - 1 : k == 2 ? 64 - rows : 63;
}

// first flag of thread t's chunk; chunk_lo(threads) = tiles.  Chunks are ceil(tiles / threads) long, the last ones short or empty.
GR_ORDER_FN int64_t chunk_lo(int64_t tiles, int threads, int t)
{
    const int64_t per = (tiles + threads - 1) / threads;
    const int64_t lo = (int64_t)t * per;
    return lo < tiles ? lo : tiles;
}

// bit 8 b of the result = byte b of w is not zero
GR_ORDER_FN uint64_t nonzero_bytes(uint64_t w)
{
    w |= w >> 4;
    w |= w >> 2;
    w |= w >> 1;
    return w & 0x0101010101010101ull;
}

// how many of the flags [lo, hi) are set (eight at a time where the chunk allows: `flags` is 8-byte aligned)
GR_ORDER_FN uint32_t chunk_ones(const uint8_t* flags, int64_t lo, int64_t hi)
{
    uint32_t n = 0;
    int64_t i = lo;
    for (; i < hi && (i & 7); ++i) n += flags[i] ? 1u : 0u;
    for (; i + 8 <= hi; i += 8) n += (uint32_t)__builtin_popcountll(nonzero_bytes(*(const uint64_t*)(flags + i)));
    for (; i < hi; ++i) n += flags[i] ? 1u : 0u;
    return n;
}

// Place the tiles [lo, hi): `ones_before` flags are set in [0, lo), `zeros_total` flags are clear in all.  A tile with a clear
// flag goes behind the clear ones before it, a tile with a set flag behind every clear one and the set ones before it.
GR_ORDER_FN void chunk_place(const uint8_t* flags, int64_t lo, int64_t hi, uint32_t ones_before, uint32_t zeros_total, uint32_t* perm)
{
    uint32_t z = (uint32_t)lo - ones_before, o = zeros_total + ones_before;
    int64_t i = lo;
    for (; i < hi && (i & 7); ++i) {
        if (flags[i]) perm[o++] = (uint32_t)i;
        else perm[z++] = (uint32_t)i;
    }
    for (; i + 8 <= hi; i += 8) {
        const uint64_t w = nonzero_bytes(*(const uint64_t*)(flags + i));
        for (int b = 0; b < 8; ++b) {
            if ((w >> (8 * b)) & 1u) perm[o++] = (uint32_t)(i + b);
            else perm[z++] = (uint32_t)(i + b);
        }
    }
    for (; i < hi; ++i) {
        if (flags[i]) perm[o++] = (uint32_t)i;
        else perm[z++] = (uint32_t)i;
    }
}

// what k_tile_partition does, one thread after the other (the counts before a chunk as a running sum); `threads` chunks, on the
// device as many as tiles rounded up to whole workgroups; returns the number of clear flags
GR_ORDER_FN uint32_t partition_serial(const uint8_t* flags, int64_t tiles, int threads, uint32_t* perm)
{
    uint32_t ones_total = 0;
    for (int t = 0; t < threads; ++t) ones_total += chunk_ones(flags, chunk_lo(tiles, threads, t), chunk_lo(tiles, threads, t + 1));
    const uint32_t zeros_total = (uint32_t)tiles - ones_total;
    uint32_t run = 0;
    for (int t = 0; t < threads; ++t) {
        const int64_t lo = chunk_lo(tiles, threads, t), hi = chunk_lo(tiles, threads, t + 1);
        chunk_place(flags, lo, hi, run, zeros_total, perm);
        run += chunk_ones(flags, lo, hi);
    }
    return zeros_total;
}

}  // namespace gr_order
