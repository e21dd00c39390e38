// Chains-on-chains partitioning (CCP): optimal contiguous partition of
// weighted items onto p workers minimizing the max part weight.
// Capability parity: reference src/thread_partition.c (lprobe:83-121,
// bisection:124-151, partition_weighted:156-195, partition_simple:198-217).
// Fresh design: integer binary search over the bottleneck bound (exact,
// no epsilon), probe via upper_bound on the prefix sums.
#pragma once

#include "types.hpp"

namespace splatt {

// returns true iff items can be split into <= nparts contiguous parts each
// of weight <= bound; fills parts[0..nparts] boundaries greedily.
bool ccp_probe(const int64_t * prefix, int64_t n, int nparts, int64_t bound,
               int64_t * parts);

// optimal boundaries (size nparts+1, parts[0]=0, parts[nparts]=n)
std::vector<int64_t> partition_weighted(const int64_t * weights, int64_t n,
                                        int nparts, int64_t * bottleneck = nullptr);

std::vector<int64_t> partition_simple(int64_t n, int nparts);

// Strips of the strip/window MTTKRP layout (csrc/hip/mttkrp_strip.hip): a
// strip is a contiguous range of output rows, at most tile_rows of them, and
// the stream range [p0, p1) of their nonzeros, at most nnz_cap long. A row
// with more than nnz_cap nonzeros is split between consecutive strips; every
// other row lies in one strip. flags bit 0: the strip's first row continues
// from the strip before; bit 1: its last row continues in the strip after.
struct Strips {
  std::vector<int32_t> row0, nrows, flags;
  std::vector<int64_t> p0, p1;
};
// rowptr: nrows + 1 stream positions, non-decreasing, rowptr[0] = 0.
// Every row, empty ones included, is in a strip. O(nrows + strips).
Strips plan_strips(const int64_t * rowptr, int64_t nrows, int64_t tile_rows,
                   int64_t nnz_cap);

}  // namespace splatt
