// gr_stats_fold.hpp -- where the trace kernels leave a launch's statistics, and how they reach the caller's nine counters.
//
// Every wave of a trace kernel used to add its sums to the caller's nine counters directly: 65 536 waves of the 2048² bench
// render, three to six 64-bit atomics each, all aimed at the same 72 bytes (two cache lines, one memory channel).  Now a wave
// adds them to ONE OF kStatRows ROWS of a partials block on the context (row = workgroup index modulo kStatRows; a row has a
// 128-byte line of its own, so neighbouring workgroups meet in different lines), and a one-workgroup kernel enqueued behind
// the trace kernel (k_stats_fold, gradus_mi355x.hip) adds the column sums to the caller's counters and leaves the block zero
// for the next launch.  The counters' layout (gr_stats) and their accumulation over launches are what they were.
//
// Plain C++ with no device types: the fold's arithmetic is compiled for the host as well (tests/host_harness_stats_fold.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GR_FOLD_FN __host__ __device__ inline
#else
#define GR_FOLD_FN inline
#endif

namespace gr_fold {

constexpr int kStatCols = 9;       // = N_STAT (gr_device.hpp): rays, accepted, rejected, rhs, flagged, status[4]
constexpr int kStatRows = 64;      // S, a power of two (DESIGN_measurements.md §M26 for the choice)
constexpr int kStatStride = 16;    // 64-bit words from one row to the next: 128 bytes, nine of them used
constexpr int kStatWords = kStatRows * kStatStride;

// the row of the partials block that workgroup `block` adds to
GR_FOLD_FN unsigned row_of(unsigned block) { return block & (unsigned)(kStatRows - 1); }

// Σ over the rows of column `col` of a rows x stride block (wrapping 64-bit sums, like the atomics that filled it)
GR_FOLD_FN unsigned long long column_sum(const unsigned long long* part, int rows, int stride, int col)
{
    unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;      // four chains: the loads of a column do not wait for one another
    int r = 0;
    for (; r + 4 <= rows; r += 4) {
        s0 += part[(r + 0) * stride + col];
        s1 += part[(r + 1) * stride + col];
        s2 += part[(r + 2) * stride + col];
        s3 += part[(r + 3) * stride + col];
    }
    for (; r < rows; ++r) s0 += part[r * stride + col];
    return (s0 + s1) + (s2 + s3);
}

// what the fold kernel does, one thread after the other: counters += column sums, then the block is zero again
GR_FOLD_FN void fold_serial(unsigned long long* part, int rows, int stride, int cols, unsigned long long* counters)
{
    for (int c = 0; c < cols; ++c) counters[c] += column_sum(part, rows, stride, c);
    for (int i = 0; i < rows * stride; ++i) part[i] = 0;
}

}  // namespace gr_fold
