// Points in the order of the cells of a uniform lattice (cell_order.hip): the device pipeline under the
// correspondence search (icp.cpp), the voxel filter and the normal estimation (cloud.cpp).  All pointers
// are device memory.
//   cloudBoundingBox    min / max of m packed points (synchronises the stream)
//   sortByCell          order.d_perm[k] = original index of the k-th point in (cell id, original index)
//                       order; order.d_cell_start (optional) [cells + 1] offsets into that order
//                       (synchronises the stream)
//   gatherByOrder       out[k] = xyz[d_perm[k]], packed (3) or padded to 4 scalars
//   exclusiveScan       in-place exclusive scan of `length` counters with the sort's scan kernels
//                       (synchronises the stream)
//   countOccupiedCells  cells of the lattice that hold at least one point (synchronises the stream)
#pragma once

#include <hip/hip_runtime.h>

#include "cell_lattice.hpp"

namespace mopt {

// what sortByCell leaves: the arrays it fills and what it is asked to do about non-finite points
struct CellOrder {
  int *d_perm = nullptr;                  // [m]
  int *d_cell_start = nullptr;            // optional: [cells + 1]
  unsigned int *d_sorted_keys = nullptr;  // optional: receives the m sorted keys
  // points with a non-finite coordinate take a key one past the last cell (one more value for the sort's
  // passes to cover), so they sort last, and are counted
  bool park_non_finite = false;
  long long parked = 0;  // written by the call (0 without park_non_finite)
};

template <typename S>
hipError_t cloudBoundingBox(const S *d_xyz, long long m, double lo[3], double hi[3], hipStream_t stream,
                            bool whole_points = false);  // true: a point with any non-finite coordinate
                                                         // shapes no axis of the box
template <typename S>
hipError_t sortByCell(const S *d_xyz, long long m, const CellLattice &lattice, CellOrder &order,
                      hipStream_t stream);
template <typename S>
hipError_t gatherByOrder(const S *d_xyz, const int *d_perm, long long m, S *d_out, bool padded,
                         hipStream_t stream);
hipError_t exclusiveScan(unsigned int *d_data, long long length, hipStream_t stream);
hipError_t countOccupiedCells(const int *d_cell_start, long long ncells, long long *occupied,
                              hipStream_t stream);

}  // namespace mopt
