// The per-point arithmetic of the normal estimation (csrc/normals_device.hpp: the neighbourhood test, the
// one-pass moments about the query point, the Jacobi eigen-solve) on the CPU, over brute-force
// neighbourhoods in the caller's order (test_cloud_normals_abi.py compiles and runs this, with
// contraction off, and holds the result to the bound the GPU tests use):
//   normals_solver <in.bin> <radius> <min_neighbors> <vx> <vy> <vz> <normals.bin> <curvature.bin> <counts.bin>
// reads packed fp64 xyz, writes fp64 normals and curvature and int32 counts.  Links nothing of the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "normals_device.hpp"

namespace {

template <typename T>
std::vector<T> readAll(const char *path) {
  std::vector<T> data;
  FILE *f = std::fopen(path, "rb");
  if (!f) return data;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  data.resize(size_t(bytes) / sizeof(T));
  if (std::fread(data.data(), sizeof(T), data.size(), f) != data.size()) data.clear();
  std::fclose(f);
  return data;
}

template <typename T>
bool writeAll(const char *path, const std::vector<T> &data) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(data.data(), sizeof(T), data.size(), f) == data.size();
  return std::fclose(f) == 0 && ok;
}

bool finitePoint(const double *p) {
  return std::fabs(p[0]) <= 1e300 && std::fabs(p[1]) <= 1e300 && std::fabs(p[2]) <= 1e300;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 10) return 2;
  const std::vector<double> xyz = readAll<double>(argv[1]);
  const double radius = std::atof(argv[2]);
  const int min_k = std::atoi(argv[3]) > 3 ? std::atoi(argv[3]) : 3;
  const double view[3] = {std::atof(argv[4]), std::atof(argv[5]), std::atof(argv[6])};
  const size_t n = xyz.size() / 3;
  const double r2 = radius * radius, nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> normals(3 * n, nan), curvature(n, nan);
  std::vector<int32_t> counts(n, 0);
  for (size_t i = 0; i < n; ++i) {
    const double *p = &xyz[3 * i];
    if (!finitePoint(p)) continue;
    mopt::normals::Moments m;
    for (size_t j = 0; j < n; ++j) {
      const double *q = &xyz[3 * j];
      if (!finitePoint(q)) continue;
      const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
      if (mopt::normals::distance2(dx, dy, dz) <= r2) mopt::normals::accumulate(m, dx, dy, dz);
    }
    counts[i] = m.k;
    if (m.k < min_k) continue;
    double nx, ny, nz;
    mopt::normals::normalFromMoments(m, nx, ny, nz, curvature[i]);
    const double towards = nx * (view[0] - p[0]) + ny * (view[1] - p[1]) + nz * (view[2] - p[2]);
    const double sign = towards < 0.0 ? -1.0 : 1.0;
    normals[3 * i + 0] = sign * nx, normals[3 * i + 1] = sign * ny, normals[3 * i + 2] = sign * nz;
  }
  return writeAll(argv[7], normals) && writeAll(argv[8], curvature) && writeAll(argv[9], counts) ? 0 : 3;
}
