// Point-cloud filters on the device, on packed xyz vectors — the layout cloud_io.hpp loads and the
// device models take.  voxelDownsample is mopt_cloud_voxel_downsample (moptimizer_hip.h has the
// semantics: lattice anchored at the world origin, one centroid per occupied voxel in ascending voxel
// id, points with a non-finite coordinate dropped, bit-identical from call to call); estimateNormals is
// mopt_cloud_estimate_normals (radius-neighbourhood PCA normals, row for row).  The reference has
// no counterpart: model.h:24-26 leaves correspondences and everything before them to the user.
// Needs no Eigen.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "moptimizer_hip.h"

namespace moptimizer {
namespace io {

// One point per occupied voxel of edge `leaf`; `counts` (optional) receives the voxels' populations.
// Throws std::runtime_error with mopt_last_error() where the call refuses.
template <typename Scalar>
inline std::vector<Scalar> voxelDownsample(const std::vector<Scalar> &xyz, double leaf, int device = 0,
                                           std::vector<int32_t> *counts = nullptr) {
  static_assert(std::is_same<Scalar, float>::value || std::is_same<Scalar, double>::value,
                "float or double clouds");
  const auto tried = [](int rc) {
    if (rc != MOPT_OK) throw std::runtime_error(std::string("voxelDownsample: ") + mopt_last_error());
  };
  const int64_t count = int64_t(xyz.size() / 3);
  int64_t voxels = 0;
  tried(mopt_cloud_voxel_downsample(device, int(sizeof(Scalar)), xyz.data(), count, leaf, 0u, nullptr,
                                    nullptr, 0, &voxels));
  std::vector<Scalar> out(size_t(voxels) * 3);
  if (counts) counts->assign(size_t(voxels), 0);
  if (voxels > 0)
    tried(mopt_cloud_voxel_downsample(device, int(sizeof(Scalar)), xyz.data(), count, leaf, 0u, out.data(),
                                      counts ? counts->data() : nullptr, voxels, &voxels));
  return out;
}

// One unit normal per point (packed xyz, the caller's order) from the PCA of its neighbours within
// `radius`, turned towards `viewpoint` (3 values; NULL: the origin) — mopt_cloud_estimate_normals.  Rows
// with fewer than max(min_neighbors, 3) neighbours, and rows of points with a non-finite coordinate, are
// NaN.  `curvature` and `counts` (optional) receive the surface variation and the neighbourhood sizes.
// Throws std::runtime_error with mopt_last_error() where the call refuses.
template <typename Scalar>
inline std::vector<Scalar> estimateNormals(const std::vector<Scalar> &xyz, double radius,
                                           int min_neighbors = 3, const double *viewpoint = nullptr,
                                           int device = 0, std::vector<Scalar> *curvature = nullptr,
                                           std::vector<int32_t> *counts = nullptr) {
  static_assert(std::is_same<Scalar, float>::value || std::is_same<Scalar, double>::value,
                "float or double clouds");
  const int64_t count = int64_t(xyz.size() / 3);
  std::vector<Scalar> normals(size_t(count) * 3);
  if (curvature) curvature->assign(size_t(count), Scalar(0));
  if (counts) counts->assign(size_t(count), 0);
  if (mopt_cloud_estimate_normals(device, int(sizeof(Scalar)), xyz.data(), count, radius, min_neighbors,
                                  viewpoint, 0u, normals.data(), curvature ? curvature->data() : nullptr,
                                  counts ? counts->data() : nullptr) != MOPT_OK)
    throw std::runtime_error(std::string("estimateNormals: ") + mopt_last_error());
  return normals;
}

}  // namespace io
}  // namespace moptimizer
