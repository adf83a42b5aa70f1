// Point-cloud filters (mopt_cloud_*): what a registration pipeline runs on a raw scan before it builds
// a cost.  The voxel filter bins with the bounding box, cell keys and stable sort the search uses
// (cell_order.hip), on a lattice anchored at the world origin (cell_lattice.hpp), and reduces the sorted
// order to one centroid per occupied voxel (cloud_voxel.hip); the normal estimation bins the same way
// into cells at least a radius wide, gathers the points cell by cell and leaves the rest to one kernel
// (cloud_normals.hip); this file is the host side of both.  (The reference has no counterpart:
// model.h:24-26 leaves correspondences and everything before them to the user.)
#include "cell_order.hpp"
#include "cost_state.hpp"

#include <cmath>
#include <cstdio>
#include <limits>

using namespace mopt_detail;

namespace {

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

// ---- what the two calls share ------------------------------------------------------------------------
// The refusals both calls give for the arguments both take, in the order both give them; `own_refusal`
// (or NULL) is the call's refusal of its own parameters, whose place is between the count's and xyz's.
int checkCloudArgs(int scalar_bytes, unsigned flags, int64_t count, const void *xyz, const char *own_refusal) {
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 (float) or 8 (double)");
  if (flags & ~unsigned(MOPT_CLOUD_INPUT_DEVICE | MOPT_CLOUD_OUTPUT_DEVICE))
    return fail(MOPT_ERR_INVALID_ARGUMENT,
                "unknown flags bits (MOPT_CLOUD_INPUT_DEVICE, MOPT_CLOUD_OUTPUT_DEVICE)");
  if (count < 0) return fail(MOPT_ERR_INVALID_ARGUMENT, "count must be >= 0");
  if (count > std::numeric_limits<int>::max())
    return fail(MOPT_ERR_INVALID_ARGUMENT, "count must be below 2^31 (the sorted order holds 32-bit indices)");
  if (own_refusal) return fail(MOPT_ERR_INVALID_ARGUMENT, own_refusal);
  if (count > 0 && !xyz) return fail(MOPT_ERR_INVALID_ARGUMENT, "xyz is NULL with count > 0");
  return MOPT_OK;
}

// the device selected and a pooled stream for one call; on exit the stream is synchronised and goes back
struct CloudCall {
  int device = 0;
  hipStream_t stream = nullptr;
  CloudCall() = default;
  CloudCall(const CloudCall &) = delete;
  CloudCall &operator=(const CloudCall &) = delete;
  int open(int on_device) {
    if (const int rc = selectDevice(on_device)) return rc;
    device = on_device;
    MOPT_HIP_TRY(acquireStream(device, &stream));
    return MOPT_OK;
  }
  ~CloudCall() {
    if (!stream) return;
    (void)hipStreamSynchronize(stream);
    releaseStream(device, stream);
  }
};

// the caller's points on the device: copied into `d_in`, or adopted under MOPT_CLOUD_INPUT_DEVICE
template <typename S>
int stageIn(const S *xyz, long long count, unsigned flags, DeviceScratch &d_in, const S **d_xyz) {
  *d_xyz = xyz;
  if (flags & MOPT_CLOUD_INPUT_DEVICE) return MOPT_OK;
  MOPT_HIP_TRY(d_in.alloc(size_t(count) * 3 * sizeof(S)));
  MOPT_HIP_TRY(hipMemcpyAsync(d_in.p, xyz, size_t(count) * 3 * sizeof(S), hipMemcpyHostToDevice, d_in.stream));
  *d_xyz = d_in.as<S>();
  return MOPT_OK;
}

// Where the kernels write one output array: the caller's own pointer under MOPT_CLOUD_OUTPUT_DEVICE (or
// NULL, an output not asked for), else scratch that copyBack() queues to the caller's host array.
template <typename T>
struct CloudOutput {
  DeviceScratch scratch;
  T *dev = nullptr, *host = nullptr;
  size_t bytes = 0;
  explicit CloudOutput(hipStream_t s) : scratch(s) {}
  hipError_t open(T *callers, size_t values, bool to_device) {
    dev = callers;
    if (!callers || to_device) return hipSuccess;
    host = callers;
    bytes = values * sizeof(T);
    const hipError_t e = scratch.alloc(bytes);
    dev = scratch.as<T>();
    return e;
  }
  hipError_t copyBack() const {
    return host ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, scratch.stream) : hipSuccess;
  }
};

// ---- mopt_cloud_voxel_downsample ---------------------------------------------------------------------
template <typename S>
int voxelDownsample(const S *xyz, long long count, double leaf, unsigned flags, S *out_xyz,
                    int32_t *out_counts, long long capacity, int64_t *out_count, hipStream_t s) {
  StageClock clock(s);
  DeviceScratch d_in(s), d_perm(s), d_keys(s), d_flags(s), d_carry(s);
  CloudOutput<S> centroids(s);
  CloudOutput<int32_t> counts(s);
  const S *d_xyz = nullptr;
  if (const int rc = stageIn(xyz, count, flags, d_in, &d_xyz)) return rc;
  clock.mark();  // 0: stage-in
  double lo[3], hi[3];
  MOPT_HIP_TRY(mopt::cloudBoundingBox<S>(d_xyz, count, lo, hi, s, /*whole_points=*/true));
  clock.mark();  // 1: bounding box
  double cells = 0.0;
  const mopt::CellLattice g = mopt::voxelLattice(lo, hi, leaf, cells);
  if (!(cells <= mopt::kMostVoxels)) {
    char msg[320];
    std::snprintf(msg, sizeof msg,
                  "leaf %g is too small for the input: the extent %g x %g x %g would take %.4g voxels, "
                  "more than 2^31 - 1; the smallest leaf that fits is about %.6g",
                  leaf, hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], cells,
                  mopt::smallestLeafThatFits(lo, hi, leaf));
    return fail(MOPT_ERR_INVALID_ARGUMENT, msg);
  }
  MOPT_HIP_TRY(d_perm.alloc(size_t(count) * sizeof(int)));
  MOPT_HIP_TRY(d_keys.alloc(size_t(count) * sizeof(unsigned int)));
  mopt::CellOrder order;
  order.d_perm = d_perm.as<int>();
  order.d_sorted_keys = d_keys.as<unsigned int>();
  order.park_non_finite = true;
  MOPT_HIP_TRY(mopt::sortByCell<S>(d_xyz, count, g, order, s));
  clock.mark();  // 2: keys and sort
  const long long kept = count - order.parked;  // the points with finite coordinates: the first of the order
  if (kept <= 0) return MOPT_OK;
  MOPT_HIP_TRY(d_flags.alloc(size_t(kept + 1) * sizeof(unsigned int)));
  MOPT_HIP_TRY(mopt::launchVoxelHeadFlags(order.d_sorted_keys, kept, d_flags.as<unsigned int>(), s));
  MOPT_HIP_TRY(mopt::exclusiveScan(d_flags.as<unsigned int>(), kept + 1, s));
  unsigned int voxels = 0;
  MOPT_HIP_TRY(hipMemcpyAsync(&voxels, d_flags.as<unsigned int>() + kept, sizeof voxels,
                              hipMemcpyDeviceToHost, s));
  MOPT_HIP_TRY(hipStreamSynchronize(s));
  clock.mark();  // 3: head flags and scan
  *out_count = int64_t(voxels);
  if (!out_xyz || int64_t(voxels) > capacity) return MOPT_OK;  // the count alone
  const bool to_device = (flags & MOPT_CLOUD_OUTPUT_DEVICE) != 0;
  MOPT_HIP_TRY(centroids.open(out_xyz, size_t(voxels) * 3, to_device));
  MOPT_HIP_TRY(counts.open(out_counts, size_t(voxels), to_device));
  MOPT_HIP_TRY(d_carry.alloc(mopt::voxelCarryBytes(kept)));
  MOPT_HIP_TRY(mopt::launchVoxelCentroids<S>(d_xyz, order.d_perm, order.d_sorted_keys,
                                             d_flags.as<unsigned int>(), kept, centroids.dev, counts.dev,
                                             d_carry.p, s));
  clock.mark();  // 4: centroids
  MOPT_HIP_TRY(centroids.copyBack());
  MOPT_HIP_TRY(counts.copyBack());
  clock.mark();  // 5: copy-out
  MOPT_HIP_TRY(hipStreamSynchronize(s));
  return MOPT_OK;
}

// ---- mopt_cloud_estimate_normals -----------------------------------------------------------------
template <typename S>
int estimateNormals(const S *xyz, long long count, double radius, int min_neighbors, const double view[3],
                    unsigned flags, S *out_normals, S *out_curvature, int32_t *out_counts, hipStream_t s) {
  DeviceScratch d_in(s), d_perm(s), d_keys(s), d_cell_start(s), d_cells(s);
  CloudOutput<S> normals(s), curvature(s);
  CloudOutput<int32_t> counts(s);
  const S *d_xyz = nullptr;
  if (const int rc = stageIn(xyz, count, flags, d_in, &d_xyz)) return rc;
  double lo[3], hi[3];
  MOPT_HIP_TRY(mopt::cloudBoundingBox<S>(d_xyz, count, lo, hi, s, /*whole_points=*/true));
  const mopt::CellLattice g = mopt::normalsLattice(lo, hi, radius);
  MOPT_HIP_TRY(d_perm.alloc(size_t(count) * sizeof(int)));
  MOPT_HIP_TRY(d_keys.alloc(size_t(count) * sizeof(unsigned int)));
  MOPT_HIP_TRY(d_cell_start.alloc(size_t(g.cells() + 1) * sizeof(int)));
  mopt::CellOrder order;
  order.d_perm = d_perm.as<int>();
  order.d_cell_start = d_cell_start.as<int>();
  order.d_sorted_keys = d_keys.as<unsigned int>();
  order.park_non_finite = true;  // the points with a non-finite coordinate: the last of the order
  MOPT_HIP_TRY(mopt::sortByCell<S>(d_xyz, count, g, order, s));
  const long long kept = count - order.parked;
  MOPT_HIP_TRY(d_cells.alloc(size_t(kept) * 4 * sizeof(S)));
  MOPT_HIP_TRY(mopt::gatherByOrder<S>(d_xyz, order.d_perm, kept, d_cells.as<S>(), /*padded=*/true, s));
  const bool to_device = (flags & MOPT_CLOUD_OUTPUT_DEVICE) != 0;
  MOPT_HIP_TRY(normals.open(out_normals, size_t(count) * 3, to_device));
  MOPT_HIP_TRY(curvature.open(out_curvature, size_t(count), to_device));
  MOPT_HIP_TRY(counts.open(out_counts, size_t(count), to_device));
  MOPT_HIP_TRY(mopt::launchCloudNormals<S>(d_cells.as<S>(), order.d_perm, order.d_sorted_keys,
                                           order.d_cell_start, count, kept, g, radius, min_neighbors, view,
                                           normals.dev, curvature.dev, counts.dev, s));
  MOPT_HIP_TRY(normals.copyBack());
  MOPT_HIP_TRY(curvature.copyBack());
  MOPT_HIP_TRY(counts.copyBack());
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
  const char *bad_leaf = (!std::isfinite(leaf) || !(leaf > 0.0)) ? "leaf must be finite and > 0" : nullptr;
  if (const int rc = checkCloudArgs(scalar_bytes, flags, count, xyz, bad_leaf)) return rc;
  if (count == 0) return MOPT_OK;
  CloudCall call;
  if (const int rc = call.open(device)) return rc;
  return withScalar(scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    return voxelDownsample<S>(static_cast<const S *>(xyz), count, leaf, flags, static_cast<S *>(out_xyz),
                              out_counts, capacity, out_count, call.stream);
  });
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
  const char *bad_parameter = (!std::isfinite(radius) || !(radius > 0.0)) ? "radius must be finite and > 0"
                              : min_neighbors < 0                         ? "min_neighbors must be >= 0"
                                                                          : nullptr;
  if (const int rc = checkCloudArgs(scalar_bytes, flags, count, xyz, bad_parameter)) return rc;
  double view[3] = {0.0, 0.0, 0.0};
  for (int a = 0; viewpoint && a < 3; ++a) {
    if (!std::isfinite(viewpoint[a])) return fail(MOPT_ERR_INVALID_ARGUMENT, "viewpoint must be finite");
    view[a] = viewpoint[a];
  }
  if (count == 0) return MOPT_OK;
  CloudCall call;
  if (const int rc = call.open(device)) return rc;
  return withScalar(scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    return estimateNormals<S>(static_cast<const S *>(xyz), count, radius, min_neighbors, view, flags,
                              static_cast<S *>(out_normals), static_cast<S *>(out_curvature), out_counts,
                              call.stream);
  });
}

}  // extern "C"
