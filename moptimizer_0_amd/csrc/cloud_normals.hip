// Radius-neighbourhood PCA normals (mopt_cloud_estimate_normals, cloud.cpp): the device half
// that follows the sort and the gather of cell_order.hip.  The finite points arrive cell by cell (a lattice
// whose cell edge is >= radius, 32- or 16-byte padded rows) with their sorted cell keys and the cells'
// offsets into that order.
//   cloudNormalsKernel   one lane per position of the sorted order.  A lane in front of `kept` takes its
//                        point and, from its key, its cell; the 3 x 3 x 3 cells around it are nine runs of
//                        consecutive positions (the three cells along x are neighbours in the order), which
//                        it walks in ascending (z, y) offset: 16-byte loads, d2 as the header defines it,
//                        the nine moment sums and the count in registers.  Then the covariance, the Jacobi
//                        eigen-solve (normals_device.hpp), the orientation towards the viewpoint, and the
//                        rows scattered through perm to the caller's order.  A lane from `kept` on holds a
//                        point with a non-finite coordinate: NaN rows, count 0.
// The lanes of a wave hold consecutive positions, so they sit in the same or adjacent cells and read
// nearly the same runs.  Every sum is taken by one lane in the order of the positions: no atomics, two
// calls give the same bits.  (The reference has no counterpart: model.h:24-26 leaves everything in front
// of the cost to the user.)
#include <hip/hip_runtime.h>

#include <limits>

#include "normals_device.hpp"
#include "sweep.hpp"

namespace mopt {
namespace {

struct NormalsArgs {
  int dims[3];
  int min_k;     // max(min_neighbors, 3)
  double r2;     // radius * radius, rounded once
  double view[3];
};

// a padded row of the cell-ordered copy, widened: 16-byte loads
__device__ __forceinline__ void loadPoint(const double *rows, long long j, double &x, double &y, double &z) {
  const double2 *row = reinterpret_cast<const double2 *>(rows + 4 * j);
  const double2 xy = row[0], zw = row[1];
  x = xy.x, y = xy.y, z = zw.x;
}
__device__ __forceinline__ void loadPoint(const float *rows, long long j, double &x, double &y, double &z) {
  const float4 v = *reinterpret_cast<const float4 *>(rows + 4 * j);
  x = double(v.x), y = double(v.y), z = double(v.z);
}

template <typename S>
__global__ __launch_bounds__(kBlockThreads) void cloudNormalsKernel(
    const S *__restrict__ cell_xyz, const int *__restrict__ perm, const unsigned int *__restrict__ keys,
    const int *__restrict__ cell_start, long long count, long long kept, const NormalsArgs g,
    S *__restrict__ normals, S *__restrict__ curvature, int32_t *__restrict__ counts) {
  const long long k = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
  if (k >= count) return;
  const size_t row = size_t(perm[k]);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double nx = nan, ny = nan, nz = nan, curv = nan;
  normals::Moments m;
  if (k < kept) {
    double px, py, pz;
    loadPoint(cell_xyz, k, px, py, pz);
    const unsigned int key = keys[k];
    const int dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    const int cx = int(key % unsigned(dx)), cyz = int(key / unsigned(dx));
    const int cy = cyz % dy, cz = cyz / dy;
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < dx ? cx + 1 : dx - 1;
    for (int oz = -1; oz <= 1; ++oz) {
      const int z = cz + oz;
      if (z < 0 || z >= dz) continue;
      for (int oy = -1; oy <= 1; ++oy) {
        const int y = cy + oy;
        if (y < 0 || y >= dy) continue;
        const long long base = ((long long)z * dy + y) * dx;  // (below 2^26: the host's cap on the cells)
        const int begin = cell_start[base + x0], end = cell_start[base + x1 + 1];
        for (int j = begin; j < end; ++j) {
          double qx, qy, qz;
          loadPoint(cell_xyz, j, qx, qy, qz);
          const double ddx = qx - px, ddy = qy - py, ddz = qz - pz;
          if (normals::distance2(ddx, ddy, ddz) <= g.r2) normals::accumulate(m, ddx, ddy, ddz);
        }
      }
    }
    if (m.k >= g.min_k) {
      normals::normalFromMoments(m, nx, ny, nz, curv);
      const double towards = nx * (g.view[0] - px) + ny * (g.view[1] - py) + nz * (g.view[2] - pz);
      if (towards < 0.0) nx = -nx, ny = -ny, nz = -nz;
    }
  }
  normals[3 * row + 0] = S(nx);  // (the one rounding to the scalar type)
  normals[3 * row + 1] = S(ny);
  normals[3 * row + 2] = S(nz);
  if (curvature) curvature[row] = S(curv);
  if (counts) counts[row] = m.k;
}

}  // namespace

template <typename S>
hipError_t launchCloudNormals(const S *d_cell_xyz, const int *d_perm, const unsigned int *d_sorted_keys,
                              const int *d_cell_start, long long count, long long kept,
                              const CellLattice &lattice, double radius, int min_neighbors,
                              const double viewpoint[3], S *d_normals, S *d_curvature, int32_t *d_counts,
                              hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  NormalsArgs g;
  for (int a = 0; a < 3; ++a) {
    g.dims[a] = lattice.dims[a];
    g.view[a] = viewpoint[a];
  }
  g.min_k = min_neighbors > 3 ? min_neighbors : 3;
  g.r2 = radius * radius;
  const unsigned blocks = unsigned((count + kBlockThreads - 1) / kBlockThreads);
  hipLaunchKernelGGL(cloudNormalsKernel<S>, dim3(blocks), dim3(kBlockThreads), 0, stream, d_cell_xyz,
                     d_perm, d_sorted_keys, d_cell_start, count, kept, g, d_normals, d_curvature, d_counts);
  return hipGetLastError();
}

template hipError_t launchCloudNormals<double>(const double *, const int *, const unsigned int *, const int *,
                                               long long, long long, const CellLattice &, double, int,
                                               const double[3], double *, double *, int32_t *, hipStream_t);
template hipError_t launchCloudNormals<float>(const float *, const int *, const unsigned int *, const int *,
                                              long long, long long, const CellLattice &, double, int,
                                              const double[3], float *, float *, int32_t *, hipStream_t);

}  // namespace mopt
