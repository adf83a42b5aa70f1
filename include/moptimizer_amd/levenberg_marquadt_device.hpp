// LevenbergMarquadtDynamic with the iteration resident on the GPU.
//
// Same surface as the reference's optimizer (include/moptimizer/optimizer.h:12-89,
// include/moptimizer/levenberg_marquadt_dyn.h:8-50): addCost / clearCosts / setMaximumIterations /
// setLevenbergMarquadtIterations / minimize / getExecutedIterations, same OptimizationStatus
// values, same arithmetic (src/levenberg_marquadt_dyn.cpp:34-119) — but minimize() hands the whole
// loop to mopt_lm_minimize: the damped solve, the trial point, the gain ratio and the stopping
// tests run in a one-workgroup kernel behind every sweep, sweeps are queued ahead, and the host
// sees only the final x.  It accepts the HIP cost classes of cost_function_hip.hpp (a host cost
// has nothing to run on the device and is refused).  Where the optimizer must stay the reference's
// own class, the boundary CostFunctionBase::linearize / computeCost is unchanged and that class
// keeps working; this one is the additive fast path.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "moptimizer_amd/cost_function_hip.hpp"

namespace moptimizer {
namespace hip {

template <class Scalar = double>
class LevenbergMarquadtDevice {
 public:
  using CostFunctionType = CostFunctionBase<Scalar>;

  explicit LevenbergMarquadtDevice(int num_parameters) : num_parameters_(num_parameters) {}
  LevenbergMarquadtDevice(const LevenbergMarquadtDevice &) = delete;
  LevenbergMarquadtDevice &operator=(const LevenbergMarquadtDevice &) = delete;

  void setMaximumIterations(int max_iterations) {  // optimizer.h:33-37
    if (max_iterations < 0)
      throw std::invalid_argument("Optimization::max_iterations cannot be less than 0.");
    maximum_iterations_ = static_cast<unsigned int>(max_iterations);
  }
  unsigned int getMaximumIterations() const { return maximum_iterations_; }
  unsigned int getExecutedIterations() const { return executed_iterations_; }
  unsigned int getLevenbergMarquadtIterations() const { return lm_max_iterations_; }
  void setLevenbergMarquadtIterations(int max_iterations) { lm_max_iterations_ = max_iterations; }
  // xi = x0 (+) delta on SE(3) (mopt_se3_plus) instead of the reference's xi = x0 + delta
  // (levenberg_marquadt_dyn.cpp:82-83, "TODO Manifold operation"); 6-parameter poses, to be used
  // with CostFunctionAnalyticalLeftHip costs.
  void setManifoldUpdate(bool on) { manifold_update_ = on ? 1 : 0; }
  // The same composed on the right — R <- R Exp(delta_w), t <- t + delta_t, the form of the
  // reference's own sketches (tst/manifold.cpp:47, tst/state_model.cpp:28-34) — to be used with
  // CostFunctionAnalyticalRightHip costs.
  void setRightManifoldUpdate(bool on) { manifold_update_ = on ? 2 : 0; }

  // Non-owning, as Optimizer::addCost (optimizer.h:58).
  void addCost(CostFunctionType *cost) {
    auto *access = dynamic_cast<DeviceCostAccess *>(cost);
    if (!access || !access->deviceCost())
      throw Exception(
          "LevenbergMarquadtDevice drives single-device HIP costs (moptimizer::hip::CostFunction*); "
          "use LevenbergMarquadtDynamic for host costs and device groups");
    costs_.push_back(cost);
    access_.push_back(access);
  }
  void clearCosts(bool delete_costs = false) {  // optimizer.h:62-68
    if (delete_costs)
      for (auto *c : costs_) delete c;
    costs_.clear();
    access_.clear();
  }

  OptimizationStatus step(Scalar *) { return OptimizationStatus::NUMERIC_ERROR; }  // as the reference's stub

  OptimizationStatus minimize(Scalar *x0) {
    if (costs_.empty()) throw std::runtime_error("No cost function added!");  // optimizer.h:48-54
    std::vector<mopt_cost *> handles;
    std::vector<int> modes;
    for (std::size_t k = 0; k < costs_.size(); ++k) {
      costs_[k]->update(x0);  // the model's per-iteration hook: empty for every device model here
      access_[k]->syncDeviceState();
      handles.push_back(access_[k]->deviceCost());
      modes.push_back(access_[k]->deviceJacobianMode());
    }
    mopt_lm_options options;
    options.max_iterations = int(maximum_iterations_);
    options.lm_max_iterations = int(lm_max_iterations_);
    options.manifold = manifold_update_;
    options.window = 0;
    mopt_lm_report report;
    (void)num_parameters_;
    throwOnError(mopt_lm_minimize(handles.data(), int(handles.size()), modes.data(), x0, &options,
                                  &report),
                 "mopt_lm_minimize");
    executed_iterations_ = static_cast<unsigned int>(report.iterations);
    sweeps_ = report.sweeps;
    final_cost_ = report.cost;
    return static_cast<OptimizationStatus>(report.status);
  }

  long long sweeps() const { return sweeps_; }   // points evaluated by the last minimize()
  double finalCost() const { return final_cost_; }

 private:
  int num_parameters_;
  unsigned int maximum_iterations_ = 15;  // optimizer.h:19
  unsigned int lm_max_iterations_ = 3;    // levenberg_marquadt_dyn.cpp:9
  unsigned int executed_iterations_ = 0;
  int manifold_update_ = 0;  // mopt_lm_options.manifold
  long long sweeps_ = 0;
  double final_cost_ = 0.0;
  std::vector<CostFunctionType *> costs_;
  std::vector<DeviceCostAccess *> access_;
};

// B independent small point2point registrations — B times a Point2Point model, its cost and a
// LevenbergMarquadtDevice of its own — laid out once and minimised together in one launch of B
// workgroups (mopt_batch).  Problems of at most four tiles (2048 double / 4096 float correspondences);
// one covariance and one loss for the batch; each problem has its own x, status and iteration count,
// and computes what LevenbergMarquadtDevice computes for it alone.
//   src_xyz / tgt_xyz: packed xyz of all problems behind one another; problem i owns correspondences
//   [offsets[i], offsets[i + 1]), offsets.size() = B + 1.
template <class Scalar = double>
class Point2PointBatchDevice {
 public:
  Point2PointBatchDevice(const Scalar *src_xyz, const Scalar *tgt_xyz, const std::vector<std::int64_t> &offsets,
                         int device = 0) {
    throwOnError(mopt_point2point_batch_create(&handle_, device, int(sizeof(Scalar)), src_xyz, tgt_xyz,
                                               offsets.data(), int(offsets.size()) - 1, MOPT_INPUT_HOST),
                 "mopt_point2point_batch_create");
    num_problems_ = int(offsets.size()) - 1;
  }
  ~Point2PointBatchDevice() { mopt_batch_destroy(handle_); }
  Point2PointBatchDevice(const Point2PointBatchDevice &) = delete;
  Point2PointBatchDevice &operator=(const Point2PointBatchDevice &) = delete;

  int numProblems() const { return num_problems_; }
  void setMaximumIterations(int max_iterations) {  // optimizer.h:33-37
    if (max_iterations < 0)
      throw std::invalid_argument("Optimization::max_iterations cannot be less than 0.");
    maximum_iterations_ = max_iterations;
  }
  void setLevenbergMarquadtIterations(int max_iterations) { lm_max_iterations_ = max_iterations; }
  void setManifoldUpdate(bool on) { manifold_update_ = on ? 1 : 0; }       // with MOPT_JAC_ANALYTIC_LEFT
  void setRightManifoldUpdate(bool on) { manifold_update_ = on ? 2 : 0; }  // with MOPT_JAC_ANALYTIC_RIGHT
  // CostFunctionBase::setCovariance (3 x 3 column-major; nullptr: identity) / setLossFunction
  void setCovariance(const Scalar *cov_colmajor) {
    throwOnError(mopt_batch_set_covariance(handle_, cov_colmajor), "mopt_batch_set_covariance");
  }
  void setLoss(int loss_kind, double parameter) {
    throwOnError(mopt_batch_set_loss(handle_, loss_kind, parameter), "mopt_batch_set_loss");
  }

  // x: numProblems() x 6, a row per problem; start poses in, results out.  jacobian_mode: the cost class
  // the caller would have used for every problem (MOPT_JAC_*).  Returns each problem's status.
  std::vector<OptimizationStatus> minimize(Scalar *x, int jacobian_mode = MOPT_JAC_ANALYTIC) {
    mopt_lm_options options;
    options.max_iterations = maximum_iterations_;
    options.lm_max_iterations = lm_max_iterations_;
    options.manifold = manifold_update_;
    options.window = 0;
    reports_.resize(std::size_t(num_problems_));
    throwOnError(mopt_batch_lm_minimize(handle_, jacobian_mode, x, &options, reports_.data()),
                 "mopt_batch_lm_minimize");
    std::vector<OptimizationStatus> status;
    for (const mopt_lm_report &r : reports_) status.push_back(static_cast<OptimizationStatus>(r.status));
    return status;
  }
  // of problem i in the last minimize()
  unsigned int getExecutedIterations(int i) const { return unsigned(reports_.at(std::size_t(i)).iterations); }
  long long sweeps(int i) const { return reports_.at(std::size_t(i)).sweeps; }
  double finalCost(int i) const { return reports_.at(std::size_t(i)).cost; }
  // evaluated points whose forward-difference form was chosen on the device, and how many were literal
  void choiceStats(long long *points, long long *literal_points) const {
    std::int64_t p = 0, l = 0;
    throwOnError(mopt_batch_lm_choice_stats(handle_, &p, &l), "mopt_batch_lm_choice_stats");
    if (points) *points = p;
    if (literal_points) *literal_points = l;
  }
  mopt_batch *handle() const { return handle_; }

 private:
  mopt_batch *handle_ = nullptr;
  int num_problems_ = 0;
  int maximum_iterations_ = 15;  // optimizer.h:19
  int lm_max_iterations_ = 3;    // levenberg_marquadt_dyn.cpp:9
  int manifold_update_ = 0;
  std::vector<mopt_lm_report> reports_;
};

}  // namespace hip
}  // namespace moptimizer
