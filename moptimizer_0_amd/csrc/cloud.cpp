// Point-cloud filters (mopt_cloud_*): what a registration pipeline runs on a raw scan before it builds
// a cost.  The voxel filter bins with the search's own bounding box, cell keys and stable sort
// (icp_grid.hip) and reduces the sorted order to one centroid per occupied voxel (cloud_voxel.hip); the
// normal estimation bins the same way into cells at least a radius wide, gathers the points cell by cell
// and leaves the rest to one kernel (cloud_normals.hip); this file is the host side of both.  (The reference has no counterpart: model.h:24-26 leaves correspondences and
// everything before them to the user.)
#include "cost_state.hpp"

#include <cmath>
#include <cstdio>
#include <limits>

using namespace mopt_detail;

namespace {

constexpr double kMostVoxels = 2147483647.0;  // 2^31 - 1: the sort's keys are 32 bits, one is the parked key
constexpr int kStages = MOPT_CLOUD_VOXEL_STAGES;

// stage boundaries of the calling thread's last call, when it asked for them (mopt_cloud_voxel_profile)
thread_local bool t_profiling = false;
thread_local double t_stage_ms[kStages] = {0};

struct StageClock {
  hipEvent_t marks[kStages + 1] = {};
  hipStream_t stream = nullptr;
  bool on = false;
  int next = 0;
  explicit StageClock(hipStream_t s) : stream(s), on(t_profiling) {
    for (int k = 0; k < kStages; ++k) t_stage_ms[k] = 0.0;
    if (!on) return;
    for (auto &m : marks)
      if (hipEventCreate(&m) != hipSuccess) on = false;
    mark();
  }
  void mark() {  // the end of a stage (and the start of the next)
    if (on && next <= kStages) (void)hipEventRecord(marks[next], stream);
    ++next;
  }
  void skipTo(int stage_end) {
    while (next <= stage_end) mark();
  }
  ~StageClock() {
    if (on) {
      skipTo(kStages);
      (void)hipStreamSynchronize(stream);
      for (int k = 0; k < kStages; ++k) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, marks[k], marks[k + 1]) == hipSuccess) t_stage_ms[k] = ms;
      }
    }
    for (auto &m : marks)
      if (m) (void)hipEventDestroy(m);
  }
};

struct Lattice {
  double origin[3];
  int dims[3];
  double cells;
};

// the lattice anchored at the world origin that covers [lo, hi]
Lattice latticeFor(const double lo[3], const double hi[3], double leaf) {
  Lattice g;
  g.cells = 1.0;
  for (int a = 0; a < 3; ++a) {
    g.origin[a] = std::floor(lo[a] / leaf) * leaf;
    const double d = std::floor((hi[a] - g.origin[a]) / leaf) + 1.0;
    g.cells *= d;
    g.dims[a] = d <= kMostVoxels ? int(d) : 0;  // (only read when the product fits)
  }
  return g;
}

template <typename S>
int voxelDownsample(const S *xyz, long long count, double leaf, unsigned flags, S *out_xyz,
                    int32_t *out_counts, long long capacity, int64_t *out_count, hipStream_t s) {
  StageClock clock(s);
  DeviceScratch d_in(s), d_perm(s), d_keys(s), d_flags(s), d_carry(s), d_out(s), d_counts(s);
  const S *d_xyz = xyz;
  if (!(flags & MOPT_CLOUD_INPUT_DEVICE)) {
    MOPT_HIP_TRY(d_in.alloc(size_t(count) * 3 * sizeof(S)));
    MOPT_HIP_TRY(hipMemcpyAsync(d_in.p, xyz, size_t(count) * 3 * sizeof(S), hipMemcpyHostToDevice, s));
    d_xyz = d_in.as<S>();
  }
  clock.mark();  // 0: stage-in
  double lo[3], hi[3];
  MOPT_HIP_TRY(mopt::icpBoundingBox<S>(d_xyz, count, lo, hi, s, /*whole_points=*/true));
  clock.mark();  // 1: bounding box
  const Lattice g = latticeFor(lo, hi, leaf);
  if (!(g.cells <= kMostVoxels)) {
    // the smallest leaf whose lattice fits, by bisection between this one and one that surely does
    double small = leaf, large = leaf;
    while (!(latticeFor(lo, hi, large).cells <= kMostVoxels)) large *= 2.0;
    for (int it = 0; it < 60; ++it) {
      const double mid = 0.5 * (small + large);
      (latticeFor(lo, hi, mid).cells <= kMostVoxels ? large : small) = mid;
    }
    char msg[320];
    std::snprintf(msg, sizeof msg,
                  "leaf %g is too small for the input: the extent %g x %g x %g would take %.4g voxels, "
                  "more than 2^31 - 1; the smallest leaf that fits is about %.6g",
                  leaf, hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], g.cells, large);
    return fail(MOPT_ERR_INVALID_ARGUMENT, msg);
  }
  MOPT_HIP_TRY(d_perm.alloc(size_t(count) * sizeof(int)));
  MOPT_HIP_TRY(d_keys.alloc(size_t(count) * sizeof(unsigned int)));
  long long parked = 0;
  MOPT_HIP_TRY(mopt::icpSortByCell<S>(d_xyz, count, g.origin, leaf, g.dims, d_perm.as<int>(), nullptr, s,
                                      &parked, d_keys.as<unsigned int>()));
  clock.mark();  // 2: keys and sort
  const long long kept = count - parked;  // the points with finite coordinates: the first of the order
  if (kept <= 0) return MOPT_OK;
  MOPT_HIP_TRY(d_flags.alloc(size_t(kept + 1) * sizeof(unsigned int)));
  MOPT_HIP_TRY(mopt::launchVoxelHeadFlags(d_keys.as<unsigned int>(), kept, d_flags.as<unsigned int>(), s));
  MOPT_HIP_TRY(mopt::icpExclusiveScan(d_flags.as<unsigned int>(), kept + 1, s));
  unsigned int voxels = 0;
  MOPT_HIP_TRY(hipMemcpyAsync(&voxels, d_flags.as<unsigned int>() + kept, sizeof voxels,
                              hipMemcpyDeviceToHost, s));
  MOPT_HIP_TRY(hipStreamSynchronize(s));
  clock.mark();  // 3: head flags and scan
  *out_count = int64_t(voxels);
  if (!out_xyz || int64_t(voxels) > capacity) return MOPT_OK;  // the count alone
  const bool to_device = (flags & MOPT_CLOUD_OUTPUT_DEVICE) != 0;
  S *d_out_xyz = out_xyz;
  int32_t *d_out_counts = out_counts;
  if (!to_device) {
    MOPT_HIP_TRY(d_out.alloc(size_t(voxels) * 3 * sizeof(S)));
    d_out_xyz = d_out.as<S>();
    if (out_counts) {
      MOPT_HIP_TRY(d_counts.alloc(size_t(voxels) * sizeof(int32_t)));
      d_out_counts = d_counts.as<int32_t>();
    }
  }
  MOPT_HIP_TRY(d_carry.alloc(mopt::voxelCarryBytes(kept)));
  MOPT_HIP_TRY(mopt::launchVoxelCentroids<S>(d_xyz, d_perm.as<int>(), d_keys.as<unsigned int>(),
                                             d_flags.as<unsigned int>(), kept, d_out_xyz, d_out_counts,
                                             d_carry.p, s));
  clock.mark();  // 4: centroids
  if (!to_device) {
    MOPT_HIP_TRY(hipMemcpyAsync(out_xyz, d_out_xyz, size_t(voxels) * 3 * sizeof(S), hipMemcpyDeviceToHost, s));
    if (out_counts)
      MOPT_HIP_TRY(hipMemcpyAsync(out_counts, d_out_counts, size_t(voxels) * sizeof(int32_t),
                                  hipMemcpyDeviceToHost, s));
  }
  clock.mark();  // 5: copy-out
  MOPT_HIP_TRY(hipStreamSynchronize(s));
  return MOPT_OK;
}

// ---- mopt_cloud_estimate_normals -----------------------------------------------------------------
constexpr double kMostNormalCells = 67108864.0;  // 2^26: the search grid's own cap (icp.cpp), a 256 MB offset table

struct NormalsLattice {
  double origin[3];
  double edge;
  int dims[3];
};

// The voxel lattice rule over [lo, hi] with the cell edge doubled until there are at most 2^26 cells.  The
// edge starts a millionth above the radius, not at it: cell = floor((v - origin) / edge) is rounded
// twice, and with edge == radius a point one ulp in front of a cell face and a neighbour exactly a
// (rounded) radius behind it come out two cells apart — with the margin the two quotients differ by
// less than 1, so the 3 x 3 x 3 cells around a point's own always hold its neighbourhood (the search
// widens its cells the same way: icp.cpp, radius_cell).
NormalsLattice normalsLatticeFor(const double lo[3], const double hi[3], double radius) {
  NormalsLattice g;
  g.edge = radius * (1.0 + 0x1p-20);
  for (;;) {
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {
      g.origin[a] = std::floor(lo[a] / g.edge) * g.edge;
      const double d = std::floor((hi[a] - g.origin[a]) / g.edge) + 1.0;
      cells *= d;
      g.dims[a] = d <= kMostNormalCells ? int(d) : 0;  // (only read when the product fits)
    }
    if (cells <= kMostNormalCells) return g;
    g.edge *= 2.0;
  }
}

template <typename S>
int estimateNormals(const S *xyz, long long count, double radius, int min_neighbors, const double view[3],
                    unsigned flags, S *out_normals, S *out_curvature, int32_t *out_counts, hipStream_t s) {
  DeviceScratch d_in(s), d_perm(s), d_keys(s), d_cell_start(s), d_cells(s), d_normals(s), d_curvature(s),
      d_counts(s);
  const S *d_xyz = xyz;
  if (!(flags & MOPT_CLOUD_INPUT_DEVICE)) {
    MOPT_HIP_TRY(d_in.alloc(size_t(count) * 3 * sizeof(S)));
    MOPT_HIP_TRY(hipMemcpyAsync(d_in.p, xyz, size_t(count) * 3 * sizeof(S), hipMemcpyHostToDevice, s));
    d_xyz = d_in.as<S>();
  }
  double lo[3], hi[3];
  MOPT_HIP_TRY(mopt::icpBoundingBox<S>(d_xyz, count, lo, hi, s, /*whole_points=*/true));
  const NormalsLattice g = normalsLatticeFor(lo, hi, radius);
  const long long ncells = (long long)g.dims[0] * g.dims[1] * g.dims[2];
  MOPT_HIP_TRY(d_perm.alloc(size_t(count) * sizeof(int)));
  MOPT_HIP_TRY(d_keys.alloc(size_t(count) * sizeof(unsigned int)));
  MOPT_HIP_TRY(d_cell_start.alloc(size_t(ncells + 1) * sizeof(int)));
  long long parked = 0;  // the points with a non-finite coordinate: the last of the order
  MOPT_HIP_TRY(mopt::icpSortByCell<S>(d_xyz, count, g.origin, g.edge, g.dims, d_perm.as<int>(),
                                      d_cell_start.as<int>(), s, &parked, d_keys.as<unsigned int>()));
  const long long kept = count - parked;
  MOPT_HIP_TRY(d_cells.alloc(size_t(kept) * 4 * sizeof(S)));
  MOPT_HIP_TRY(mopt::icpGatherPoints<S>(d_xyz, d_perm.as<int>(), kept, d_cells.as<S>(), /*padded=*/true, s));
  const bool to_device = (flags & MOPT_CLOUD_OUTPUT_DEVICE) != 0;
  S *d_out_normals = out_normals, *d_out_curvature = out_curvature;
  int32_t *d_out_counts = out_counts;
  if (!to_device) {
    MOPT_HIP_TRY(d_normals.alloc(size_t(count) * 3 * sizeof(S)));
    d_out_normals = d_normals.as<S>();
    if (out_curvature) {
      MOPT_HIP_TRY(d_curvature.alloc(size_t(count) * sizeof(S)));
      d_out_curvature = d_curvature.as<S>();
    }
    if (out_counts) {
      MOPT_HIP_TRY(d_counts.alloc(size_t(count) * sizeof(int32_t)));
      d_out_counts = d_counts.as<int32_t>();
    }
  }
  MOPT_HIP_TRY(mopt::launchCloudNormals<S>(d_cells.as<S>(), d_perm.as<int>(), d_keys.as<unsigned int>(),
                                           d_cell_start.as<int>(), count, kept, g.dims, radius, min_neighbors,
                                           view, d_out_normals, d_out_curvature, d_out_counts, s));
  if (!to_device) {
    MOPT_HIP_TRY(hipMemcpyAsync(out_normals, d_out_normals, size_t(count) * 3 * sizeof(S),
                                hipMemcpyDeviceToHost, s));
    if (out_curvature)
      MOPT_HIP_TRY(hipMemcpyAsync(out_curvature, d_out_curvature, size_t(count) * sizeof(S),
                                  hipMemcpyDeviceToHost, s));
    if (out_counts)
      MOPT_HIP_TRY(hipMemcpyAsync(out_counts, d_out_counts, size_t(count) * sizeof(int32_t),
                                  hipMemcpyDeviceToHost, s));
  }
  MOPT_HIP_TRY(hipStreamSynchronize(s));
  return MOPT_OK;
}

}  // namespace

extern "C" {

int mopt_cloud_voxel_downsample(int device, int scalar_bytes, const void *xyz, int64_t count, double leaf,
                                unsigned flags, void *out_xyz, int32_t *out_counts, int64_t capacity,
                                int64_t *out_count) {
  if (!out_count) return fail(MOPT_ERR_INVALID_ARGUMENT, "out_count is NULL");
  *out_count = 0;
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 (float) or 8 (double)");
  if (flags & ~unsigned(MOPT_CLOUD_INPUT_DEVICE | MOPT_CLOUD_OUTPUT_DEVICE))
    return fail(MOPT_ERR_INVALID_ARGUMENT,
                "unknown flags bits (MOPT_CLOUD_INPUT_DEVICE, MOPT_CLOUD_OUTPUT_DEVICE)");
  if (count < 0) return fail(MOPT_ERR_INVALID_ARGUMENT, "count must be >= 0");
  if (count > std::numeric_limits<int>::max())
    return fail(MOPT_ERR_INVALID_ARGUMENT, "count must be below 2^31 (the sorted order holds 32-bit indices)");
  if (!std::isfinite(leaf) || !(leaf > 0.0))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "leaf must be finite and > 0");
  if (count > 0 && !xyz) return fail(MOPT_ERR_INVALID_ARGUMENT, "xyz is NULL with count > 0");
  if (count == 0) return MOPT_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MOPT_ERR_NO_DEVICE, "no HIP device is visible to this process");
  if (device < 0 || device >= ndev) return fail(MOPT_ERR_INVALID_ARGUMENT, "device index out of range");
  MOPT_HIP_TRY(hipSetDevice(device));
  hipStream_t s = nullptr;
  MOPT_HIP_TRY(acquireStream(device, &s));
  const int rc = withScalar(scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    return voxelDownsample<S>(static_cast<const S *>(xyz), count, leaf, flags, static_cast<S *>(out_xyz),
                              out_counts, capacity, out_count, s);
  });
  (void)hipStreamSynchronize(s);
  releaseStream(device, s);
  return rc;
}

int mopt_cloud_voxel_profile(int enabled, double *stage_ms) {
  if (stage_ms)
    for (int k = 0; k < kStages; ++k) stage_ms[k] = t_stage_ms[k];
  t_profiling = enabled != 0;
  return MOPT_OK;
}

int mopt_cloud_estimate_normals(int device, int scalar_bytes, const void *xyz, int64_t count, double radius,
                                int min_neighbors, const double *viewpoint, unsigned flags, void *out_normals,
                                void *out_curvature, int32_t *out_counts) {
  if (count > 0 && !out_normals) return fail(MOPT_ERR_INVALID_ARGUMENT, "out_normals is NULL with count > 0");
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 (float) or 8 (double)");
  if (flags & ~unsigned(MOPT_CLOUD_INPUT_DEVICE | MOPT_CLOUD_OUTPUT_DEVICE))
    return fail(MOPT_ERR_INVALID_ARGUMENT,
                "unknown flags bits (MOPT_CLOUD_INPUT_DEVICE, MOPT_CLOUD_OUTPUT_DEVICE)");
  if (count < 0) return fail(MOPT_ERR_INVALID_ARGUMENT, "count must be >= 0");
  if (count > std::numeric_limits<int>::max())
    return fail(MOPT_ERR_INVALID_ARGUMENT, "count must be below 2^31 (the sorted order holds 32-bit indices)");
  if (!std::isfinite(radius) || !(radius > 0.0))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "radius must be finite and > 0");
  if (min_neighbors < 0) return fail(MOPT_ERR_INVALID_ARGUMENT, "min_neighbors must be >= 0");
  if (count > 0 && !xyz) return fail(MOPT_ERR_INVALID_ARGUMENT, "xyz is NULL with count > 0");
  double view[3] = {0.0, 0.0, 0.0};
  for (int a = 0; viewpoint && a < 3; ++a) {
    if (!std::isfinite(viewpoint[a])) return fail(MOPT_ERR_INVALID_ARGUMENT, "viewpoint must be finite");
    view[a] = viewpoint[a];
  }
  if (count == 0) return MOPT_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MOPT_ERR_NO_DEVICE, "no HIP device is visible to this process");
  if (device < 0 || device >= ndev) return fail(MOPT_ERR_INVALID_ARGUMENT, "device index out of range");
  MOPT_HIP_TRY(hipSetDevice(device));
  hipStream_t s = nullptr;
  MOPT_HIP_TRY(acquireStream(device, &s));
  const int rc = withScalar(scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    return estimateNormals<S>(static_cast<const S *>(xyz), count, radius, min_neighbors, view, flags,
                              static_cast<S *>(out_normals), static_cast<S *>(out_curvature), out_counts, s);
  });
  (void)hipStreamSynchronize(s);
  releaseStream(device, s);
  return rc;
}

}  // extern "C"
