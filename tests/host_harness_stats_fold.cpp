// host_harness_stats_fold.cpp -- TEST INFRASTRUCTURE.  The arithmetic of the statistics fold (gr_stats_fold.hpp: column sums of
// the partials block added into the nine counters, the block zero afterwards) compiled for the host with g++.  Never linked into
// libgradus_mi355x.so.
#include <cstdint>

#include "../gradus.jl_amd/csrc/gr_stats_fold.hpp"

extern "C" {

int hsf_cols(void) { return gr_fold::kStatCols; }
int hsf_rows(void) { return gr_fold::kStatRows; }
int hsf_stride(void) { return gr_fold::kStatStride; }
unsigned hsf_row_of(unsigned block) { return gr_fold::row_of(block); }

unsigned long long hsf_column_sum(const unsigned long long* part, int rows, int stride, int col)
{
    return gr_fold::column_sum(part, rows, stride, col);
}

// k_stats_fold (gradus_mi355x.hip), one thread after the other
void hsf_fold(unsigned long long* part, int rows, int stride, int cols, unsigned long long* counters)
{
    gr_fold::fold_serial(part, rows, stride, cols, counters);
}

}      // extern "C"
