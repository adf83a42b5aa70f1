// moptimizer::io::estimateNormals from C++ (test_gpu_cloud_normals.py compiles and runs this):
//   cloud_normals <f64|f32> <radius> <in.bin> <out_normals.bin> <out_curvature.bin> <out_counts.bin>
// reads packed xyz of that scalar type, writes normals and curvature in it and the neighbour counts as
// int32; the viewpoint is (0, 0, 10).  Without arguments it needs no device: the wrapper must throw what
// the C ABI refuses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "moptimizer_amd/cloud_filter.hpp"

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

template <typename S>
int run(double radius, char **paths) {
  const std::vector<S> xyz = readAll<S>(paths[0]);
  const double viewpoint[3] = {0.0, 0.0, 10.0};
  std::vector<S> curvature;
  std::vector<int32_t> counts;
  const std::vector<S> normals = moptimizer::io::estimateNormals<S>(xyz, radius, 3, viewpoint, 0, &curvature, &counts);
  if (!writeAll(paths[1], normals) || !writeAll(paths[2], curvature) || !writeAll(paths[3], counts)) return 3;
  std::printf("normals of %zu points\n", counts.size());
  return 0;
}

template <typename S>
int refused() {
  try {
    (void)moptimizer::io::estimateNormals<S>(std::vector<S>(3, S(0)), -1.0);
  } catch (const std::runtime_error &e) {
    return std::strstr(e.what(), "radius") ? 1 : 0;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 1) {
    std::printf("refused %d of 2\n", refused<double>() + refused<float>());
    return 0;
  }
  if (argc != 7) return 2;
  try {
    const double radius = std::atof(argv[2]);
    return std::string(argv[1]) == "f32" ? run<float>(radius, argv + 3) : run<double>(radius, argv + 3);
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
}
