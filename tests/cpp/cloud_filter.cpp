// moptimizer::io::voxelDownsample from C++ (test_gpu_cloud_voxel.py compiles and runs this):
//   cloud_filter <f64|f32> <leaf> <in.bin> <out_xyz.bin> <out_counts.bin>
// reads packed xyz of that scalar type, writes the centroids in it and the populations as int32.
// Without arguments it needs no device: the wrapper must throw what the C ABI refuses.
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
int run(double leaf, char **paths) {
  const std::vector<S> xyz = readAll<S>(paths[0]);
  std::vector<int32_t> counts;
  const std::vector<S> out = moptimizer::io::voxelDownsample<S>(xyz, leaf, 0, &counts);
  if (!writeAll(paths[1], out) || !writeAll(paths[2], counts)) return 3;
  std::printf("voxels %zu of %zu points\n", counts.size(), xyz.size() / 3);
  return 0;
}

template <typename S>
int refused() {
  try {
    (void)moptimizer::io::voxelDownsample<S>(std::vector<S>(3, S(0)), -1.0);
  } catch (const std::runtime_error &e) {
    return std::strstr(e.what(), "leaf") ? 1 : 0;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 1) {
    std::printf("refused %d of 2\n", refused<double>() + refused<float>());
    return 0;
  }
  if (argc != 6) return 2;
  try {
    const double leaf = std::atof(argv[2]);
    return std::string(argv[1]) == "f32" ? run<float>(leaf, argv + 3) : run<double>(leaf, argv + 3);
  } catch (const std::exception &e) {
    std::printf("FAIL %s\n", e.what());
    return 1;
  }
}
