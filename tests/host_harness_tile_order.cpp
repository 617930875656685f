// host_harness_tile_order.cpp -- TEST INFRASTRUCTURE.  The arithmetic of the live-first tile order (gr_tile_order.hpp: a stable
// partition of the tiles by one flag each, in chunks as the one workgroup of k_tile_partition takes them) compiled for the host
// with g++.  Never linked into libgradus_mi355x.so.
#include <cstdint>

#include "../gradus.jl_amd/csrc/gr_tile_order.hpp"

extern "C" {

int hto_threads(void) { return gr_order::kPartitionThreads; }
int hto_class_lanes(void) { return gr_order::kClassLanes; }
int hto_class_lane(int rows_log2, int k) { return gr_order::class_lane(rows_log2, k); }
int64_t hto_chunk_lo(int64_t tiles, int threads, int t) { return gr_order::chunk_lo(tiles, threads, t); }

// k_tile_partition (gradus_mi355x.hip), one thread after the other; returns the number of clear flags
uint32_t hto_partition(const uint8_t* flags, int64_t tiles, int threads, uint32_t* perm)
{
    return gr_order::partition_serial(flags, tiles, threads, perm);
}

// one thread's share alone, given what a scan of the other threads' counts hands it
void hto_chunk_place(const uint8_t* flags, int64_t lo, int64_t hi, uint32_t ones_before, uint32_t zeros_total, uint32_t* perm)
{
    gr_order::chunk_place(flags, lo, hi, ones_before, zeros_total, perm);
}

}      // extern "C"
