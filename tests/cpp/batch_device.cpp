// moptimizer::hip::Point2PointBatchDevice<Scalar> (mopt_batch) from C++: compiled and linked for double
// and float by tests/test_batch_abi.py; run with the argument `run` (on a GPU) it solves a batch of four
// problems and compares every problem with a LevenbergMarquadtDevice solve of the same cost.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "moptimizer_amd/cost_function_hip.hpp"
#include "moptimizer_amd/levenberg_marquadt_device.hpp"

namespace mh = moptimizer::hip;
using moptimizer::OptimizationStatus;

static int g_fail = 0;
static void expectTrue(const char *what, bool ok) {
  if (!ok) ++g_fail;
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", what);
}

// problem i: sizes[i] points in [0, 10)^3 (a fixed linear congruential sequence), turned about z by
// 0.1 (i + 1) and moved by (0.5, -0.25 i, 0.125)
template <typename S>
static void makeProblems(const std::vector<int> &sizes, std::vector<S> &src, std::vector<S> &tgt,
                         std::vector<std::int64_t> &offsets) {
  std::uint32_t state = 12345u;
  auto next = [&]() {
    state = state * 1664525u + 1013904223u;
    return S(double(state >> 8) / double(1u << 24) * 10.0);
  };
  offsets.assign(1, 0);
  for (std::size_t i = 0; i < sizes.size(); ++i) {
    const double a = 0.1 * double(i + 1), c = std::cos(a), s = std::sin(a);
    for (int k = 0; k < sizes[i]; ++k) {
      const S p[3] = {next(), next(), next()};
      src.insert(src.end(), p, p + 3);
      tgt.push_back(S(c * p[0] - s * p[1] + 0.5));
      tgt.push_back(S(s * p[0] + c * p[1] - 0.25 * double(i)));
      tgt.push_back(S(p[2] + 0.125));
    }
    offsets.push_back(offsets.back() + sizes[i]);
  }
}

template <typename S>
static void solveAndCompare(const char *name) {
  const std::vector<int> sizes = {5, 700, 1025, 2048};
  std::vector<S> src, tgt;
  std::vector<std::int64_t> offsets;
  makeProblems<S>(sizes, src, tgt, offsets);
  const int B = int(sizes.size());
  mh::Point2PointBatchDevice<S> batch(src.data(), tgt.data(), offsets);
  batch.setMaximumIterations(5);
  std::vector<S> xs(std::size_t(B) * 6, S(0));
  const std::vector<OptimizationStatus> status = batch.minimize(xs.data(), MOPT_JAC_ANALYTIC);
  char label[160];
  for (int i = 0; i < B; ++i) {
    auto model = std::make_shared<mh::Point2PointDeviceModel<S>>(src.data() + 3 * offsets[i], tgt.data() + 3 * offsets[i],
                                                                 std::size_t(sizes[i]));
    mh::CostFunctionAnalyticalHip<S> cost(model, 6, 3, sizes[i]);
    mh::LevenbergMarquadtDevice<S> lone(6);
    lone.setMaximumIterations(5);
    lone.addCost(&cost);
    S x[6] = {0, 0, 0, 0, 0, 0};
    const OptimizationStatus lone_status = lone.minimize(x);
    std::snprintf(label, sizeof label, "%s problem %d: status %d and %u iterations as the lone solve (%d, %u)", name, i,
                  int(status[i]), batch.getExecutedIterations(i), int(lone_status), lone.getExecutedIterations());
    expectTrue(label, status[i] == lone_status && batch.getExecutedIterations(i) == lone.getExecutedIterations() &&
                          batch.sweeps(i) == lone.sweeps());
    std::snprintf(label, sizeof label, "%s problem %d: x and cost bit for bit the lone solve's", name, i);
    const double cost_batch = batch.finalCost(i), cost_lone = lone.finalCost();
    expectTrue(label, std::memcmp(x, &xs[std::size_t(i) * 6], sizeof x) == 0 &&
                          std::memcmp(&cost_batch, &cost_lone, sizeof cost_lone) == 0);
  }
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "run") == 0) {
    solveAndCompare<double>("double");
    solveAndCompare<float>("float");
    std::printf("%d failed\n", g_fail);
    return g_fail ? 1 : 0;
  }
  // without a device: the classes exist for both scalars and refuse what the C ABI refuses
  int refused = 0;
  try {
    const double xyz[3] = {0, 0, 0};
    mh::Point2PointBatchDevice<double> batch(xyz, xyz, std::vector<std::int64_t>{0, 0});  // an empty problem
  } catch (const moptimizer::Exception &) {
    ++refused;
  }
  try {
    const float xyz[3] = {0, 0, 0};
    mh::Point2PointBatchDevice<float> batch(xyz, xyz, std::vector<std::int64_t>{1, 2});  // does not start at 0
  } catch (const moptimizer::Exception &) {
    ++refused;
  }
  std::printf("refused %d of 2\n", refused);
  return refused == 2 ? 0 : 1;
}
