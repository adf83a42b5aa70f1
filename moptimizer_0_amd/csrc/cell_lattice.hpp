// The uniform lattice that the correspondence search, the voxel filter and the normal estimation bin
// their points on (cell_order.hpp sorts by it), and the host rules that choose its resolution from a
// cloud's bounding box: icp.cpp and cloud.cpp call them with the box the device took,
// tests/cpp/host_logic.cpp with literals.  Host arithmetic only — no HIP header, no project header.
#pragma once

#include <cmath>

namespace mopt {

// cell of a coordinate v along axis a: floor((v - origin[a]) / edge), clamped into [0, dims[a]);
// cell id = x + dims[0] * (y + dims[1] * z).  (A kernel argument as it stands: cellKeyKernel.)
struct CellLattice {
  double origin[3] = {0, 0, 0};
  double edge = 1.0;
  int dims[3] = {1, 1, 1};
  long long cells() const { return (long long)dims[0] * dims[1] * dims[2]; }
};

// 2^31 - 1 voxels: the sort's keys are 32 bits, and one is the parked key
constexpr double kMostVoxels = 2147483647.0;
// 2^26 cells where a table of cell offsets is kept (the search, the normals): 256 MB of offsets at most
constexpr int kMostCellsLog2 = 26;
constexpr double kMostCells = double(1ll << kMostCellsLog2);

// ---- the voxel filter -------------------------------------------------------------------------------
// The lattice of edge `leaf` anchored at the world origin that covers [lo, hi]; `cells` is its cell
// count, which may be beyond what dims can say: the dims are only to be read when cells <= kMostVoxels.
inline CellLattice voxelLattice(const double lo[3], const double hi[3], double leaf, double &cells) {
  CellLattice g;
  g.edge = leaf;
  cells = 1.0;
  for (int a = 0; a < 3; ++a) {
    g.origin[a] = std::floor(lo[a] / leaf) * leaf;
    const double d = std::floor((hi[a] - g.origin[a]) / leaf) + 1.0;
    cells *= d;
    g.dims[a] = d <= kMostVoxels ? int(d) : 0;
  }
  return g;
}

inline bool voxelLatticeFits(const double lo[3], const double hi[3], double leaf) {
  double cells;
  (void)voxelLattice(lo, hi, leaf, cells);
  return cells <= kMostVoxels;
}

// the smallest leaf >= `leaf` whose lattice fits, by bisection between this one and one that surely does
inline double smallestLeafThatFits(const double lo[3], const double hi[3], double leaf) {
  double small = leaf, large = leaf;
  while (!voxelLatticeFits(lo, hi, large)) large *= 2.0;
  for (int it = 0; it < 60; ++it) {
    const double mid = 0.5 * (small + large);
    (voxelLatticeFits(lo, hi, mid) ? large : small) = mid;
  }
  return large;
}

// ---- the normal estimation --------------------------------------------------------------------------
// The voxel lattice rule over [lo, hi] with the cell edge doubled until there are at most kMostCells.  The
// edge starts a millionth above the radius, not at it: cell = floor((v - origin) / edge) is rounded
// twice, and with edge == radius a point one ulp in front of a cell face and a neighbour exactly a
// (rounded) radius behind it come out two cells apart — with the margin the two quotients differ by
// less than 1, so the 3 x 3 x 3 cells around a point's own always hold its neighbourhood (the search
// widens its cells the same way: SearchBox::radius_cell).
inline CellLattice normalsLattice(const double lo[3], const double hi[3], double radius) {
  double cells;
  double edge = radius * (1.0 + 0x1p-20);
  for (;;) {
    const CellLattice g = voxelLattice(lo, hi, edge, cells);
    if (cells <= kMostCells) return g;
    edge *= 2.0;
  }
}

// ---- the correspondence search ----------------------------------------------------------------------
// Cell edge: a hair above the search radius over `reach`, so that the (2 reach + 1)^3 cells around a
// query hold every target within the radius.  reach = 1 while that leaves about one target per cell;
// where the radius spans many targets the cells are made finer (up to 8 to the radius, and never more
// than `most_cells`): the search's first round looks at 2 x 2 x 2 cells whatever the radius, and what it
// costs goes with the targets in them.  Enlarged instead when even cells of the radius's size would be
// more than that.
constexpr int kMostReach = 8;

// the cap on the search's cells from MOPT_ICP_MAX_CELLS_LOG2 (measurements: 20 ... 28)
inline double searchCellCap(int cells_log2) {
  return double(1ll << (cells_log2 < 20 ? 20 : cells_log2 > 28 ? 28 : cells_log2));
}

struct SearchBox {
  double lo[3], hi[3];  // of the targets
  double radius_cell;   // the cell edge at reach 1
  double most_cells;
  SearchBox(const double lo_[3], const double hi_[3], double max_distance, double most_cells_)
      : radius_cell(max_distance * 1.001), most_cells(most_cells_) {
    for (int a = 0; a < 3; ++a) lo[a] = lo_[a], hi[a] = hi_[a];
  }
  double cellsAt(double edge) const {
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) cells *= std::floor((hi[a] - lo[a]) / edge) + 1.0;
    return cells;
  }
  // the largest reach <= wanted the cell budget allows
  int mostReach(int wanted) const {
    while (wanted > 1 && cellsAt(radius_cell / wanted) > most_cells) --wanted;
    return wanted;
  }
  // a box thinner than a cell along some axis — a wall, a line, coincident points — says nothing about
  // the targets per cell by its volume: there the resolution comes from the occupied cells alone
  bool thin() const {
    bool thin_box = false;
    for (int a = 0; a < 3; ++a) thin_box = thin_box || !(hi[a] - lo[a] >= radius_cell);
    return thin_box;
  }
  // the reach of the first binning of m targets: MOPT_ICP_REACH where set (> 0), else by the box's
  // volume — finer while there are more than 1.5 targets per cell of the box
  int firstReach(long long m, int forced_reach) const {
    int reach = 1;
    if (forced_reach > 0) {
      reach = mostReach(forced_reach > kMostReach ? kMostReach : forced_reach);
    } else if (!thin()) {
      while (reach < kMostReach && double(m) > 1.5 * cellsAt(radius_cell / reach) &&
             mostReach(reach + 1) > reach)
        ++reach;
    }
    return reach;
  }
  // the lattice at that reach, anchored at the box's corner
  CellLattice latticeAt(int reach) const {
    CellLattice g;
    g.edge = radius_cell / reach;
    while (cellsAt(g.edge) > most_cells) g.edge *= 1.26;  // (only ever with reach == 1)
    for (int a = 0; a < 3; ++a) {
      g.origin[a] = lo[a];
      g.dims[a] = int(std::floor((hi[a] - lo[a]) / g.edge)) + 1;
    }
    return g;
  }
};

// The box's volume says little about how the targets fill it (a scanned surface occupies a thin sheet
// of the cells): after a binning the cells that hold anything are counted, and while they hold more than
// three targets each on average the grid is made finer and the targets are binned again (at most twice
// more; a binning is ~0.25 ms per million).  Finer cells that do not thin the targets out (coincident
// points; fewer than 1.5 times fewer per occupied cell) only add empty rows to every search: the grid
// then goes back to the resolution before, and stays.

// is a binning of m targets at `reach` worth counting the occupied cells of?  (`reach_before`: 0 until a
// refinement was made)
inline bool refinementPossible(int reach, int reach_before, int forced_reach, long long m) {
  if (forced_reach > 0 || m == 0) return false;
  return !(reach == kMostReach && reach_before == 0);  // by the volume rule, nothing finer to try
}

// What follows binning number `attempt` (0, 1, 2) at `reach`, which left `per_cell` targets per occupied
// cell (`per_cell_before` at `reach_before`, the resolution before the last refinement).
struct Refinement {
  enum What { kStop, kStepBack, kFiner } what;
  int reach;  // kStepBack: the reach to settle at; kFiner: the reach wanted, for mostReach to allow
};
inline Refinement refineReach(int reach, int reach_before, double per_cell_before, int attempt,
                              double per_cell) {
  if (reach_before > 0 && per_cell * 1.5 > per_cell_before) return {Refinement::kStepBack, reach_before};
  if (per_cell <= 3.0 || attempt >= 2) return {Refinement::kStop, reach};
  const int wanted = int(std::ceil(reach * std::sqrt(per_cell / 1.5)));
  const int next = wanted > reach + 1 ? wanted : reach + 1;
  return {Refinement::kFiner, next < kMostReach ? next : kMostReach};
}

}  // namespace mopt
