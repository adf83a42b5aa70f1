// Host-side logic of the drop-in, without a GPU and without the HIP library: the LM caller's
// status / error behaviour (levenberg_marquadt_dyn.cpp:34-119, optimizer.h:26-54), the pivoted
// LDL^T it solves with, the dense matrix subset, SO(3) exp / log, loss weights, the logger and
// the exception type; and the library's host-only headers (csrc/dispatch.hpp, csrc/sweep_choice.hpp: the
// rules that choose a sweep, csrc/cell_lattice.hpp: the rules that choose a lattice of cells).  Costs here are tiny closed-form CostFunctionBase subclasses written for
// the test; nothing from oracle/ or the device path is involved.
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>
#include <random>
#include <sstream>
#include <stdexcept>
#include <type_traits>

#include "cell_lattice.hpp"
#include "dispatch.hpp"
#include "sweep_choice.hpp"
#include "moptimizer_amd/cost_function_hip.hpp"
#include "moptimizer_caller/levenberg_marquadt.hpp"
#include "moptimizer_amd/so3.hpp"

using moptimizer::LevenbergMarquadtDynamic;
using moptimizer::OptimizationStatus;
namespace dense = moptimizer::dense;

static int g_fail = 0, g_checks = 0;
static void expectTrue(const char *what, bool ok) {
  ++g_checks;
  if (!ok) ++g_fail;
  std::printf("%s %s\n", ok ? "PASS" : "FAIL", what);
}
static void expectNear(const char *what, double got, double want, double tol) {
  ++g_checks;
  const bool ok = std::fabs(got - want) <= tol && !std::isnan(got);
  if (!ok) ++g_fail;
  std::printf("%s %-58s got % .12g want % .12g tol %.1e\n", ok ? "PASS" : "FAIL", what, got, want, tol);
}

// r_i = a_i . x - y_i  (linear least squares): LM must land on the normal-equation solution.
class LinearCost : public moptimizer::CostFunctionBase<double> {
 public:
  LinearCost(int n, int rows, unsigned seed) : CostFunctionBase<double>(nullptr, rows), n_(n) {
    std::mt19937 gen(seed);
    std::normal_distribution<double> dist(0.0, 1.0);
    a_.resize(rows, n);
    y_.resize(rows, 1);
    truth_.resize(n, 1);
    for (int j = 0; j < n; ++j) truth_[j] = 0.5 + j;
    for (int i = 0; i < rows; ++i) {
      double v = 0;
      for (int j = 0; j < n; ++j) {
        a_(i, j) = dist(gen);
        v += a_(i, j) * truth_[j];
      }
      y_[i] = v;
    }
  }
  double computeCost(const double *x) override {
    double s = 0;
    for (int i = 0; i < a_.rows(); ++i) s += residual(x, i) * residual(x, i);
    return s;
  }
  double linearize(const double *x, double *H, double *b) override {
    for (int k = 0; k < n_ * n_; ++k) H[k] = 0;
    for (int k = 0; k < n_; ++k) b[k] = 0;
    double s = 0;
    for (int i = 0; i < a_.rows(); ++i) {
      const double r = residual(x, i);
      for (int c = 0; c < n_; ++c) {
        for (int rr = 0; rr < n_; ++rr) H[c * n_ + rr] += a_(i, rr) * a_(i, c);
        b[c] += a_(i, c) * r;
      }
      s += r * r;
    }
    return s;
  }
  const dense::Matrix<double> &truth() const { return truth_; }

 private:
  double residual(const double *x, int i) const {
    double v = -y_[i];
    for (int j = 0; j < n_; ++j) v += a_(i, j) * x[j];
    return v;
  }
  int n_;
  dense::Matrix<double> a_, y_, truth_;
};

// cost whose trial evaluation is NaN: the optimizer must stop with NUMERIC_ERROR (:88-91)
class NanTrialCost : public moptimizer::CostFunctionBase<double> {
 public:
  NanTrialCost() : CostFunctionBase<double>(nullptr, 1) {}
  double computeCost(const double *) override { return std::numeric_limits<double>::quiet_NaN(); }
  double linearize(const double *, double *H, double *b) override {
    H[0] = 1.0;
    b[0] = 1.0;
    return 1.0;
  }
};

// cost that never decreases: every trial is rejected (rho < 0)
class StubbornCost : public moptimizer::CostFunctionBase<double> {
 public:
  explicit StubbornCost(double gradient) : CostFunctionBase<double>(nullptr, 1), g_(gradient) {}
  double computeCost(const double *) override { return 2.0; }
  double linearize(const double *, double *H, double *b) override {
    H[0] = 1.0;
    b[0] = g_;
    return 1.0;
  }
  int linearizations = 0;

 private:
  double g_;
};

static void optimizerStatuses() {
  {
    LevenbergMarquadtDynamic<double> lm(3);
    bool threw = false;
    double x[3] = {0, 0, 0};
    try {
      lm.minimize(x);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    expectTrue("minimize without costs throws std::runtime_error (optimizer.h:48-54)", threw);
    threw = false;
    try {
      lm.setMaximumIterations(-1);
    } catch (const std::invalid_argument &) {
      threw = true;
    }
    expectTrue("setMaximumIterations(-1) throws std::invalid_argument (optimizer.h:33-37)", threw);
    expectTrue("default maximum iterations is 15", lm.getMaximumIterations() == 15);
    expectTrue("default inner LM iterations is 3", lm.getLevenbergMarquadtIterations() == 3);
  }
  {
    LinearCost cost(4, 40, 7);
    LevenbergMarquadtDynamic<double> lm(4);
    lm.addCost(&cost);
    double x[4] = {0, 0, 0, 0};
    const OptimizationStatus st = lm.minimize(x);
    expectTrue("linear least squares: CONVERGED (cost below 8 eps)", st == OptimizationStatus::CONVERGED);
    for (int j = 0; j < 4; ++j) expectNear("linear least squares x[j]", x[j], cost.truth()[j], 1e-9);
    expectTrue("linear least squares: a handful of iterations", lm.getExecutedIterations() <= 5);
  }
  {
    // two costs are summed (multi-objective, levenberg_marquadt_dyn.cpp:48-60)
    LinearCost a(3, 20, 1), b(3, 25, 2);
    LevenbergMarquadtDynamic<double> lm(3);
    lm.addCost(&a);
    lm.addCost(&b);
    double x[3] = {5, -5, 5};
    lm.minimize(x);
    for (int j = 0; j < 3; ++j) expectNear("two summed costs x[j]", x[j], a.truth()[j], 1e-9);
    lm.clearCosts();
    bool threw = false;
    try {
      lm.minimize(x);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    expectTrue("clearCosts() empties the optimizer", threw);
  }
  {
    NanTrialCost cost;
    LevenbergMarquadtDynamic<double> lm(1);
    std::ostringstream sink;
    lm.setLogger(std::make_shared<duna::Logger>(sink, duna::Logger::L_ERROR, "test"));
    lm.addCost(&cost);
    double x[1] = {1.0};
    expectTrue("NaN trial cost -> NUMERIC_ERROR", lm.minimize(x) == OptimizationStatus::NUMERIC_ERROR);
    expectTrue("x is left untouched by a rejected NaN trial", x[0] == 1.0);
    expectTrue("the error is logged at L_ERROR", sink.str().find("Numeric Error") != std::string::npos);
  }
  {
    StubbornCost cost(1.0);
    LevenbergMarquadtDynamic<double> lm(1);
    lm.setMaximumIterations(4);
    lm.addCost(&cost);
    double x[1] = {3.0};
    expectTrue("always-rejected steps -> MAXIMUM_ITERATIONS_REACHED",
               lm.minimize(x) == OptimizationStatus::MAXIMUM_ITERATIONS_REACHED);
    expectTrue("rejected steps never move x", x[0] == 3.0);
    expectTrue("executed iterations == maximum", lm.getExecutedIterations() == 4);
  }
  {
    StubbornCost cost(1e-12);  // delta = -b / H(1 + lambda) is below sqrt(eps): SMALL_DELTA (delta.h:11-16)
    LevenbergMarquadtDynamic<double> lm(1);
    lm.addCost(&cost);
    double x[1] = {3.0};
    expectTrue("rejected step with |delta| < sqrt(eps) -> SMALL_DELTA",
               lm.minimize(x) == OptimizationStatus::SMALL_DELTA);
  }
}

static void ldlt() {
  std::mt19937 gen(11);
  std::normal_distribution<double> dist(0.0, 1.0);
  for (int n : {1, 2, 6, 8}) {
    // SPD: A = B^T B + I
    dense::Matrix<double> B(n + 3, n), A(n, n), x(n, 1), rhs(n, 1);
    for (int i = 0; i < n + 3; ++i)
      for (int j = 0; j < n; ++j) B(i, j) = dist(gen);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double v = i == j ? 1.0 : 0.0;
        for (int k = 0; k < n + 3; ++k) v += B(k, i) * B(k, j);
        A(i, j) = v;
      }
    for (int i = 0; i < n; ++i) x[i] = dist(gen);
    for (int i = 0; i < n; ++i) {
      double v = 0;
      for (int j = 0; j < n; ++j) v += A(i, j) * x[j];
      rhs[i] = v;
    }
    const auto got = dense::PivotedLDLT<double>(A).solve(rhs);
    double err = 0;
    for (int i = 0; i < n; ++i) err = std::max(err, std::fabs(got[i] - x[i]));
    char label[64];
    std::snprintf(label, sizeof label, "PivotedLDLT SPD n=%d max error", n);
    expectNear(label, err, 0.0, 1e-10);
  }
  {
    // indefinite but non-singular, needs the diagonal pivoting
    dense::Matrix<double> A(3, 3), rhs(3, 1);
    const double a[3][3] = {{1e-12, 2, 0}, {2, -3, 1}, {0, 1, 5}};
    const double want[3] = {1.0, -2.0, 0.5};
    for (int i = 0; i < 3; ++i) {
      rhs[i] = 0;
      for (int j = 0; j < 3; ++j) {
        A(i, j) = a[i][j];
        rhs[i] += a[i][j] * want[j];
      }
    }
    const auto got = dense::PivotedLDLT<double>(A).solve(rhs);
    for (int i = 0; i < 3; ++i) expectNear("PivotedLDLT indefinite x[i]", got[i], want[i], 1e-9);
  }
  {
    // rank-deficient (a zero row / column, as the as-written point2point Jacobian produces,
    // SURVEY 8a-9): the step is finite and zero along the null direction
    dense::Matrix<double> A(3, 3), rhs(3, 1);
    A.setZero();
    A(0, 0) = 4;
    A(2, 2) = 2;
    rhs[0] = 8;
    rhs[1] = 0;
    rhs[2] = -2;
    const auto got = dense::PivotedLDLT<double>(A).solve(rhs);
    expectNear("PivotedLDLT singular x[0]", got[0], 2.0, 1e-14);
    expectNear("PivotedLDLT singular x[1] (null direction)", got[1], 0.0, 0.0);
    expectNear("PivotedLDLT singular x[2]", got[2], -1.0, 1e-14);
  }
}

static void denseAndSo3() {
  dense::Matrix<double> m(2, 3);
  m.setConstant(2.0);
  m(1, 2) = 7.0;
  expectTrue("Matrix is column-major (data()[c * rows + r])", m.data()[2 * 2 + 1] == 7.0 && m(5) == 7.0);
  m *= 0.5;
  expectNear("Matrix *= scalar", m(1, 2), 3.5, 0);
  m.setIdentity();
  expectTrue("setIdentity on a 2x3", m(0, 0) == 1 && m(1, 1) == 1 && m(0, 1) == 0 && m(1, 2) == 0);
  moptimizer::covariance::Matrix<float> cov;
  cov.resize(3, 3);
  cov.setIdentity();
  cov *= 0.25f;
  expectNear("covariance::Matrix scaling", cov(2, 2), 0.25, 0);

  // exp / log round trip and the small-angle branch (so3.cpp:43-57: identity below 10 eps)
  const double w[3] = {0.3, -0.2, 0.5};
  double R[9], back[3];
  moptimizer::so3::expSO3(w, R);
  moptimizer::so3::logSO3(R, back);
  for (int a = 0; a < 3; ++a) expectNear("log(exp(w)) == w", back[a], w[a], 1e-14);
  double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
               R[2] * (R[3] * R[7] - R[4] * R[6]);
  expectNear("det exp(w) == 1", det, 1.0, 1e-14);
  const double tiny[3] = {1e-17, 0, 0};
  moptimizer::so3::expSO3(tiny, R);
  expectTrue("exp of a rotation below 10 eps is exactly I", R[0] == 1 && R[4] == 1 && R[8] == 1 && R[1] == 0 && R[5] == 0);
  double x[6] = {1, 2, 3, 0, 0, M_PI / 2}, T[16];
  moptimizer::so3::convert6DOFParameterToMatrix(x, T);  // column-major 4x4
  expectNear("convert6DOFParameterToMatrix translation", T[12] + T[13] + T[14], 6.0, 0);
  expectNear("convert6DOFParameterToMatrix Rz(90): R(1,0)", T[1], 1.0, 1e-15);
  expectNear("convert6DOFParameterToMatrix Rz(90): R(0,1)", T[4], -1.0, 1e-15);
  expectNear("convert6DOFParameterToMatrix bottom row", T[3] + T[7] + T[11] + T[15], 1.0, 0);

  moptimizer::loss::GemmanMCClure<double> gm(100.0);
  expectNear("GemmanMCClure weight t^2/(s+t)^2", gm.weight(25.0), 100.0 * 100.0 / (125.0 * 125.0), 1e-16);
  moptimizer::loss::NoLoss<double> none;
  expectNear("NoLoss weight", none.weight(1e9), 1.0, 0);

  std::ostringstream sink;
  duna::Logger log(sink, duna::Logger::L_WARN, "unit");
  log.log(duna::Logger::L_DEBUG, "hidden");
  log.log(duna::Logger::L_ERROR, "shown ", 42);
  expectTrue("Logger filters by level and prefixes the line",
             sink.str() == "[ERROR] duna::unit::shown 42\n");
  log.setLogLevel(duna::Logger::L_DEBUG);
  log.log(duna::Logger::L_DEBUG, "now");
  expectTrue("Logger::setLogLevel", sink.str().find("[DEBUG] duna::unit::now") != std::string::npos);

  try {
    throw moptimizer::Exception("boom");
  } catch (const std::exception &e) {
    expectTrue("moptimizer::Exception is a std::exception carrying its text", std::string(e.what()) == "boom");
  }
}

// The binding's recovery of a Geman-McClure threshold from a loss object that keeps it private, as
// the reference's class does (loss_function/geman_mcclure.h:6-19: no accessor): one probe of
// weight(1) = t^2 / (1 + t)^2 gives t = sqrt(w) / (1 - sqrt(w)) (cost_function_hip.hpp,
// gemanMcClureThreshold).  Against a class of the reference's shape here, since its headers are not in
// this image; the class of host_api.hpp has an accessor and must come back exactly.
template <typename T>
class ReferenceShapedGemanMcClure : public moptimizer::loss::ILossFunction<T> {
 public:
  explicit ReferenceShapedGemanMcClure(T threshold) : threshold_(threshold) {}
  T weight(T errorSquaredNorm) override {
    const T den = errorSquaredNorm + threshold_;
    return (threshold_ * threshold_) / (den * den);
  }

 private:
  T threshold_;
};

template <typename T>
static void lossThresholdRecoveryFor(const char *type_name, double tolerance_at_1, double tolerance_at_1e4) {
  const double thresholds[] = {0.05, 0.8, 1.0, 100.0, 1e4};
  for (double t : thresholds) {
    ReferenceShapedGemanMcClure<T> hidden{T(t)};
    const double got = moptimizer::hip::gemanMcClureThreshold(&hidden, 0);
    // 1 - sqrt(w) cancels as t grows: the error is ~ t * eps relative
    const double tolerance = t <= 1.0 ? tolerance_at_1 : tolerance_at_1 + (tolerance_at_1e4 - tolerance_at_1) * t / 1e4;
    expectTrue((std::string("threshold recovered from weight(1), ") + type_name + ", t = " + std::to_string(t)).c_str(),
               std::fabs(got - double(T(t))) <= tolerance * t);
    moptimizer::loss::GemmanMCClure<T> open{T(t)};
    expectTrue((std::string("threshold through the accessor, ") + type_name).c_str(),
               moptimizer::hip::gemanMcClureThreshold(&open, 0) == double(T(t)));
  }
}

static void lossThresholdRecovery() {
  lossThresholdRecoveryFor<double>("double", 1e-14, 1e-11);
  lossThresholdRecoveryFor<float>("float", 1e-6, 2e-3);
}

// csrc/dispatch.hpp: a run-time value reaches the lambda as the compile-time tag of that same value, an
// unlisted one takes what the call states (the default's tag, or the failure value without running the
// lambda), and the lambda's return value comes back.
template <typename Tag>
static int tagValue(Tag) { return Tag::value; }
template <typename T>
static int typeBytes(mopt::dispatch::Type<T>) {
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "a scalar type");
  return std::is_same<T, double>::value ? 8 : 4;
}

static void dispatchPrimitives() {
  namespace dispatch = mopt::dispatch;
  for (int v : {-1, 0, 3, 7}) {
    int calls = 0;
    const int got = dispatch::intOrFail<-1, 0, 3, 7>(v, -100, [&](auto tag) {
      static_assert(decltype(tag)::value == tag(), "tag() is the value, a constant expression");
      constexpr int as_template_argument = tag();
      ++calls;
      return 10 * as_template_argument + 1;
    });
    expectTrue("intOrFail: a listed value reaches its own tag, once", got == 10 * v + 1 && calls == 1);
    expectTrue("intOrDefault: a listed value reaches its own tag",
               (dispatch::intOrDefault<3, -1, 0, 7>(v, [](auto tag) { return tagValue(tag); })) == v);
  }
  for (int v : {-2, 1, 2, 8, 1 << 30}) {
    int calls = 0;
    const int got = dispatch::intOrFail<-1, 0, 3, 7>(v, -100, [&](auto tag) {
      ++calls;
      return tagValue(tag);
    });
    expectTrue("intOrFail: an unlisted value returns the failure value, the lambda not run",
               got == -100 && calls == 0);
    expectTrue("intOrDefault: an unlisted value takes the default's tag",
               (dispatch::intOrDefault<3, -1, 0, 7>(v, [](auto tag) { return tagValue(tag); })) == 3);
  }
  expectTrue("intOrDefault: the default itself need not be listed",
             (dispatch::intOrDefault<2, 0, 1>(2, [](auto tag) { return tagValue(tag); })) == 2);
  expectTrue("intOrFail: one listed value",
             (dispatch::intOrFail<5>(5, -1, [](auto tag) { return tagValue(tag); })) == 5 &&
                 (dispatch::intOrFail<5>(4, -1, [](auto tag) { return tagValue(tag); })) == -1);
  // the return type is the lambda's, not int
  const std::string text = dispatch::intOrDefault<0, 1>(1, [](auto tag) { return std::to_string(tag()) + "!"; });
  expectTrue("the lambda's return value comes back (a std::string)", text == "1!");

  expectTrue("byBool(true) -> std::true_type",
             dispatch::byBool(true, [](auto flag) { return std::is_same<decltype(flag), std::true_type>::value; }));
  expectTrue("byBool(false) -> std::false_type",
             dispatch::byBool(false, [](auto flag) { return std::is_same<decltype(flag), std::false_type>::value; }));
  expectTrue("byBool: flag() is a constant expression", dispatch::byBool(true, [](auto flag) {
    constexpr bool as_template_argument = flag();
    return std::integral_constant<bool, as_template_argument>::value;
  }));

  expectTrue("widthOrFail(8) -> double", dispatch::widthOrFail(8, -1, [](auto s) { return typeBytes(s); }) == 8);
  expectTrue("widthOrFail(4) -> float", dispatch::widthOrFail(4, -1, [](auto s) { return typeBytes(s); }) == 4);
  for (int bytes : {0, 2, 16, -8}) {
    int calls = 0;
    const int got = dispatch::widthOrFail(bytes, -1, [&](auto s) {
      ++calls;
      return typeBytes(s);
    });
    expectTrue("widthOrFail: another width returns the failure value, the lambda not run", got == -1 && calls == 0);
    expectTrue("widthOrDefault<float>: another width is float",
               dispatch::widthOrDefault<float>(bytes, [](auto s) { return typeBytes(s); }) == 4);
    expectTrue("widthOrDefault<double>: another width is double",
               dispatch::widthOrDefault<double>(bytes, [](auto s) { return typeBytes(s); }) == 8);
  }
  expectTrue("widthOrDefault<float>(8) -> double",
             dispatch::widthOrDefault<float>(8, [](auto s) { return typeBytes(s); }) == 8);
  expectTrue("widthOrDefault<double>(4) -> float",
             dispatch::widthOrDefault<double>(4, [](auto s) { return typeBytes(s); }) == 4);
  // nested, as the launchers use it: every combination reaches its own pair of tags
  for (int a : {0, 1, 2})
    for (bool b : {false, true}) {
      const int got = dispatch::intOrDefault<2, 0, 1>(a, [&](auto x) {
        return dispatch::byBool(b, [&](auto y) { return std::integral_constant<int, 2 * x() + (y() ? 1 : 0)>::value; });
      });
      expectTrue("nested dispatch reaches the pair's own instantiation", got == 2 * a + (b ? 1 : 0));
    }
}

// csrc/sweep_choice.hpp: the rules that decide which sweep runs, at the values their comments state.
// Expected values are worked out here from those formulas, never by calling a rule twice.
static void sweepChoiceRules() {
  namespace choice = mopt::choice;
  // forward differences: literal where some |x_j| (0 judged as 1) is below 0.08 max(1, rho / 30),
  // rho = src_bound + |t|.  Here |t| = |(1, 2, 2)| = 3 and src_bound = 10: rho = 13, threshold 0.08.
  {
    double x[6] = {1, 2, 2, 0.5, 0.5, 0.079};
    expectTrue("forward step, rho <= 30: |x_j| = 0.079 is small", choice::hasSmallForwardStep(10.0, x));
    x[5] = -0.079;
    expectTrue("forward step, rho <= 30: x_j = -0.079 is small", choice::hasSmallForwardStep(10.0, x));
    x[5] = 0.081;
    expectTrue("forward step, rho <= 30: |x_j| = 0.081 is not", !choice::hasSmallForwardStep(10.0, x));
    x[5] = 0.0;
    expectTrue("forward step, rho <= 30: x_j = 0 is judged as 1, not small", !choice::hasSmallForwardStep(10.0, x));
    x[5] = 0.079;
    expectTrue("forward step: rho = 27 + 3 = 30 still has the threshold 0.08", choice::hasSmallForwardStep(27.0, x));
    x[5] = 0.081;
    expectTrue("forward step: rho = 30, 0.081 is not small", !choice::hasSmallForwardStep(27.0, x));
  }
  // rho = 300: threshold 0.08 * 300 / 30 = 0.8
  expectNear("forwardStepThreshold(300)", mopt::forwardStepThreshold(300.0), 0.8, 1e-15);
  expectNear("forwardStepThreshold(30)", mopt::forwardStepThreshold(30.0), 0.08, 0);
  expectNear("forwardStepThreshold(3)", mopt::forwardStepThreshold(3.0), 0.08, 0);
  expectNear("forwardStepThreshold(3000)", mopt::forwardStepThreshold(3000.0), 8.0, 1e-14);
  {
    double x[6] = {0, 0, 0, 2, 2, 0.79};
    expectTrue("forward step, bound 300: 0.79 < 0.8 is small", choice::hasSmallForwardStep(300.0, x));
    x[5] = 0.81;
    expectTrue("forward step, bound 300: 0.81 is not (and the zeros are judged as 1 > 0.8)",
               !choice::hasSmallForwardStep(300.0, x));
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    expectTrue("forward step, bound 300: all-zero x is not small (1 > 0.8)", !choice::hasSmallForwardStep(300.0, zero));
    expectTrue("forward step, bound 3000: all-zero x is small (1 < 8)", choice::hasSmallForwardStep(3000.0, zero));
    // the |t| term: src_bound = 295 alone gives 0.08 * 295 / 30 = 0.7867 < 0.79; |t| = |(3, 4, 0)| = 5
    // brings rho to 300 and the threshold to 0.8 > 0.79
    const double still[6] = {0, 0, 0, 2, 2, 0.79}, moved[6] = {3, 4, 0, 2, 2, 0.79};
    expectTrue("forward step, bound 295 and t = 0: 0.79 > 0.7867 is not small", !choice::hasSmallForwardStep(295.0, still));
    expectTrue("forward step, bound 295 and |t| = 5: 0.79 < 0.8 is small", choice::hasSmallForwardStep(295.0, moved));
  }
  // the left-perturbation basis cancels where |t|^2 > 1e3 rho_w^2, rho_w = |R c0 + t| + r
  {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, c0[3] = {1000, 0, 0};
    const double back[3] = {-1000, 0, 0}, none[3] = {0, 0, 0};
    expectTrue("leftBasisCancels: t = -c0, rho_w = 1, |t|^2 = 1e6 > 1e3", choice::leftBasisCancels(c0, 1.0, I, back));
    expectTrue("leftBasisCancels: t = 0 does not (0 > 1e3 * 1001^2 is false)", !choice::leftBasisCancels(c0, 1.0, I, none));
    // t = (-1000, y, 0): rho_w = y + 1, |t|^2 = 1e6 + y^2.  y = 30: 1000900 > 961000; y = 31: 1000961 < 1024000
    const double y30[3] = {-1000, 30, 0}, y31[3] = {-1000, 31, 0};
    expectTrue("leftBasisCancels: 1000900 > 1e3 * 31^2", choice::leftBasisCancels(c0, 1.0, I, y30));
    expectTrue("leftBasisCancels: 1000961 < 1e3 * 32^2", !choice::leftBasisCancels(c0, 1.0, I, y31));
    // a quarter turn about z maps c0 = (1000, 0, 0) to (0, 1000, 0): it is R c0 + t that counts
    const double Rz[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, back_y[3] = {0, -1000, 0};
    expectTrue("leftBasisCancels: R c0 + t = 0 under a rotation", choice::leftBasisCancels(c0, 1.0, Rz, back_y));
    expectTrue("leftBasisCancels: the same t without the rotation (rho_w = 1000 sqrt 2 + 1)",
               !choice::leftBasisCancels(c0, 1.0, I, back_y));
    // may cancel at some pose only where |c0|^2 > 1e3 r^2: sqrt(1000) = 31.62
    const double c31[3] = {31, 0, 0}, c32[3] = {0, 0, -32}, c62[3] = {0, 62, 0}, c64[3] = {0, 64, 0};
    expectTrue("leftBasisMayCancel: |c0| = 31 r does not", !choice::leftBasisMayCancel(c31, 1.0));
    expectTrue("leftBasisMayCancel: |c0| = 32 r does", choice::leftBasisMayCancel(c32, 1.0));
    expectTrue("leftBasisMayCancel: |c0| = 31 r, r = 2", !choice::leftBasisMayCancel(c62, 2.0));
    expectTrue("leftBasisMayCancel: |c0| = 32 r, r = 2", choice::leftBasisMayCancel(c64, 2.0));
  }
  // usesMoments / residentPerIterate: rows AUTO, LITERAL, MOMENTS, MOMENTS_ALWAYS (the values 0..3 of the
  // header); columns ANALYTIC, ANALYTIC_TST_LAYOUT, NUMERIC, ANALYTIC_LEFT, ANALYTIC_RIGHT (0..4)
  static_assert(MOPT_KERNEL_AUTO == 0 && MOPT_KERNEL_LITERAL == 1 && MOPT_KERNEL_MOMENTS == 2 &&
                    MOPT_KERNEL_MOMENTS_ALWAYS == 3 && MOPT_JAC_ANALYTIC == 0 && MOPT_JAC_ANALYTIC_TST_LAYOUT == 1 &&
                    MOPT_JAC_NUMERIC == 2 && MOPT_JAC_ANALYTIC_LEFT == 3 && MOPT_JAC_ANALYTIC_RIGHT == 4,
                "the order of the tables below");
  static const bool moments_p2p_may_cancel[4][5] = {{1, 1, 1, 0, 1}, {0, 0, 0, 0, 0}, {1, 1, 1, 0, 1}, {1, 1, 1, 1, 1}};
  static const bool moments_p2p_near[4][5] = {{1, 1, 1, 1, 1}, {0, 0, 0, 0, 0}, {1, 1, 1, 1, 1}, {1, 1, 1, 1, 1}};
  // another model never takes the left-basis exception, whatever its sources' sphere says
  static const bool moments_other[4][5] = {{1, 1, 1, 1, 1}, {0, 0, 0, 0, 0}, {1, 1, 1, 1, 1}, {1, 1, 1, 1, 1}};
  static const bool per_iterate_p2p[4][5] = {{0, 0, 1, 0, 0}, {0, 0, 0, 0, 0}, {0, 0, 1, 0, 0}, {0, 0, 0, 0, 0}};
  bool moments_ok = true, per_iterate_ok = true, switched_off_ok = true;
  for (int variant = 0; variant < 4; ++variant)
    for (int jac = 0; jac < 5; ++jac)
      for (int may_cancel = 0; may_cancel < 2; ++may_cancel)
        for (int p2p = 0; p2p < 2; ++p2p) {
          const bool want_moments = !p2p ? moments_other[variant][jac]
                                         : (may_cancel ? moments_p2p_may_cancel : moments_p2p_near)[variant][jac];
          if (choice::usesMoments(p2p, variant, jac, may_cancel) != want_moments) {
            moments_ok = false;
            std::printf("  usesMoments(p2p=%d, variant=%d, jac=%d, may_cancel=%d) != %d\n", p2p, variant, jac,
                        may_cancel, int(want_moments));
          }
          const bool want_per_iterate = p2p && per_iterate_p2p[variant][jac];
          if (choice::residentPerIterate(p2p, variant, jac, true) != want_per_iterate) {
            per_iterate_ok = false;
            std::printf("  residentPerIterate(p2p=%d, variant=%d, jac=%d) != %d\n", p2p, variant, jac,
                        int(want_per_iterate));
          }
          if (choice::residentPerIterate(p2p, variant, jac, false)) switched_off_ok = false;
        }
  expectTrue("usesMoments: the whole table (variant x jac_mode x may cancel x model)", moments_ok);
  expectTrue("residentPerIterate: the whole table", per_iterate_ok);
  expectTrue("residentPerIterate: never with MOPT_LM_PER_ITERATE off", switched_off_ok);
  // speculation pays while fewer than two kept results went unused, or no more unused than used
  {
    const int unused[4] = {1, 2, 2, 3}, used[4] = {0, 2, 1, 2};
    const bool pays[4] = {true, true, false, false};
    for (int k = 0; k < 4; ++k) {
      expectTrue("speculationPays, not free: (1,0) (2,2) pay, (2,1) (3,2) do not",
                 choice::speculationPays(false, unused[k], used[k]) == pays[k]);
      expectTrue("speculationPays, free: always", choice::speculationPays(true, unused[k], used[k]));
    }
  }
  // gridFor: num_cus * blocks_per_cu, clamped to the tiles, to max_grid, and to at least 1
  expectTrue("gridFor: 256 CUs x 2 with room", choice::gridFor(256, 2, 19532, 4096) == 512);
  expectTrue("gridFor: clamped to num_tiles", choice::gridFor(256, 2, 17, 4096) == 17);
  expectTrue("gridFor: clamped to max_grid", choice::gridFor(256, 32, 19532, 4096) == 4096);
  expectTrue("gridFor: tiles below max_grid below the product", choice::gridFor(256, 32, 5000, 4096) == 4096);
  expectTrue("gridFor: no tile still launches one workgroup", choice::gridFor(256, 1, 0, 4096) == 1);
  expectTrue("gridFor: no overflow in num_cus * blocks_per_cu", choice::gridFor(1 << 20, 1 << 20, 1000, 4096) == 1000);
}

// csrc/cell_lattice.hpp: the lattices the voxel filter, the normal estimation and the correspondence
// search bin on.  Expected values are worked out here by hand from the rules.
static void cellLatticeRules() {
  using mopt::CellLattice;
  // voxelLattice, leaf 0.5: origin = floor(lo / leaf) * leaf = (floor(-2.4), floor(0), floor(0.6)) * 0.5;
  // dims = floor((hi - origin) / leaf) + 1 = (floor(8.2), floor(0), floor(0.6)) + 1
  {
    const double lo[3] = {-1.2, 0.0, 0.3}, hi[3] = {2.6, 0.0, 0.3};
    double cells = 0.0;
    const CellLattice g = mopt::voxelLattice(lo, hi, 0.5, cells);
    expectTrue("voxelLattice: origin (-1.5, 0, 0)", g.origin[0] == -1.5 && g.origin[1] == 0.0 && g.origin[2] == 0.0);
    expectTrue("voxelLattice: dims (9, 1, 1)", g.dims[0] == 9 && g.dims[1] == 1 && g.dims[2] == 1);
    expectTrue("voxelLattice: edge is the leaf, 9 cells", g.edge == 0.5 && cells == 9.0 && g.cells() == 9);
    bool covers = true;
    for (int a = 0; a < 3; ++a)
      covers = covers && g.origin[a] <= lo[a] && g.origin[a] + g.dims[a] * g.edge > hi[a];
    expectTrue("voxelLattice: origin <= lo and origin + dims * leaf > hi on every axis", covers);
  }
  // [0, 2000]^3: leaf 1 gives 2001^3 = 8.012e9 cells, over 2^31 - 1; 1290^3 = 2146689000 <= 2147483647 <
  // 1291^3 = 2151685171, so the smallest leaf that fits has floor(2000 / leaf) = 1289: just above 2000 / 1290
  {
    const double lo[3] = {0, 0, 0}, hi[3] = {2000, 2000, 2000};
    double cells = 0.0;
    (void)mopt::voxelLattice(lo, hi, 1.0, cells);
    expectTrue("voxelLattice: 2001^3 cells are counted, and are over the cap",
               cells == 2001.0 * 2001.0 * 2001.0 && !(cells <= mopt::kMostVoxels));
    expectTrue("kMostVoxels is 2^31 - 1", mopt::kMostVoxels == 2147483647.0);
    const double leaf = mopt::smallestLeafThatFits(lo, hi, 1.0);
    const CellLattice g = mopt::voxelLattice(lo, hi, leaf, cells);
    expectTrue("smallestLeafThatFits: dims (1290, 1290, 1290)",
               g.dims[0] == 1290 && g.dims[1] == 1290 && g.dims[2] == 1290 && cells == 2146689000.0);
    expectNear("smallestLeafThatFits: just above 2000 / 1290", leaf, 2000.0 / 1290.0, 1e-12);
    (void)mopt::voxelLattice(lo, hi, leaf - 1e-6, cells);
    expectTrue("smallestLeafThatFits: a leaf 1e-6 smaller takes 1291^3 cells and does not fit",
               cells == 2151685171.0 && !(cells <= mopt::kMostVoxels));
    const double lo2[3] = {-1.2, 0.0, 0.3}, hi2[3] = {2.6, 0.0, 0.3};
    expectTrue("smallestLeafThatFits: a leaf that fits comes back as it is",
               mopt::smallestLeafThatFits(lo2, hi2, 0.5) == 0.5);
  }
  // normalsLattice over [0, 1000]^3, radius 1: edges (1 + 2^-20) x 1, 2, 4 give floor(1000 / edge) + 1 =
  // 1000, 500, 250 cells an axis; 1000^3 and 500^3 = 1.25e8 exceed 2^26 = 67108864, 250^3 = 15625000 does not
  {
    const double lo[3] = {0, 0, 0}, hi[3] = {1000, 1000, 1000};
    expectTrue("kMostCells is 2^26", mopt::kMostCells == 67108864.0 && mopt::kMostCellsLog2 == 26);
    const CellLattice g = mopt::normalsLattice(lo, hi, 1.0);
    expectTrue("normalsLattice: two doublings, edge 4 (1 + 2^-20) exactly", g.edge == 4.0 * (1.0 + 0x1p-20));
    expectTrue("normalsLattice: dims (250, 250, 250)", g.dims[0] == 250 && g.dims[1] == 250 && g.dims[2] == 250);
    expectTrue("normalsLattice: anchored at the world origin", g.origin[0] == 0.0 && g.origin[1] == 0.0 && g.origin[2] == 0.0);
    // radius 10: floor(1000 / 10.0000095) + 1 = 100 an axis, 1e6 cells
    const CellLattice h = mopt::normalsLattice(lo, hi, 10.0);
    expectTrue("normalsLattice: radius 10 needs no doubling, edge 10 (1 + 2^-20) > radius",
               h.edge == 10.0 * (1.0 + 0x1p-20) && h.edge > 10.0);
    expectTrue("normalsLattice: radius 10, dims (100, 100, 100)", h.dims[0] == 100 && h.dims[1] == 100 && h.dims[2] == 100);
  }
  // the search: radius_cell = 1.001 max_distance; a cube of side 100 searched within 1
  {
    const double lo[3] = {0, 0, 0}, hi[3] = {100, 100, 100};
    const mopt::SearchBox box(lo, hi, 1.0, mopt::kMostCells);
    expectTrue("SearchBox: radius_cell = 1.001 max_distance", box.radius_cell == 1.0 * 1.001);
    // floor(100 / 1.001) + 1 = 99 + 1 an axis
    expectTrue("SearchBox: cellsAt(1.001) = 100^3", box.cellsAt(1.001) == 1e6);
    expectTrue("searchCellCap: 26 is 2^26, clamped to 2^20 ... 2^28",
               mopt::searchCellCap(26) == mopt::kMostCells && mopt::searchCellCap(3) == 1048576.0 &&
                   mopt::searchCellCap(31) == 268435456.0);
    expectTrue("SearchBox: the cube is not thin", !box.thin());
    expectTrue("firstReach: m = 1e6 is not above 1.5 x 1e6 cells: reach 1", box.firstReach(1000000, 0) == 1);
    // m = 1e7 > 1.5e6: reach 2, whose edge 0.5005 gives (floor(199.8) + 1)^3 = 8e6 cells; 1e7 < 1.2e7 stops there
    const int reach = box.firstReach(10000000, 0);
    expectTrue("firstReach: m = 1e7 gives reach 2", reach > 1 && reach == 2);
    expectTrue("firstReach: the cells at that reach are within the cap",
               box.cellsAt(box.radius_cell / reach) == 8e6 && box.cellsAt(box.radius_cell / reach) <= box.most_cells);
    // forced: 20 is clamped to 8; edge 1.001 / 4 gives 400^3 = 6.4e7 <= 2^26 < 500^3 at reach 5
    expectTrue("firstReach: forced 20 -> 8 -> 4 under 2^26 cells", box.firstReach(10, 20) == 4);
    expectTrue("mostReach(8) under 2^26 cells", box.mostReach(8) == 4);
    // ... and under 2^20 = 1048576 only reach 1 (100^3) fits: 200^3 = 8e6 at reach 2
    const mopt::SearchBox tight(lo, hi, 1.0, mopt::searchCellCap(20));
    expectTrue("firstReach: forced 20 -> 8 -> 1 under 2^20 cells", tight.firstReach(10, 20) == 1);
    expectTrue("firstReach: forced 1 stays, whatever m is", box.firstReach(100000000, 1) == 1);
    const CellLattice g = box.latticeAt(2);
    expectTrue("latticeAt(2): edge radius_cell / 2, dims 200^3, anchored at lo",
               g.edge == box.radius_cell / 2 && g.dims[0] == 200 && g.dims[1] == 200 && g.dims[2] == 200 &&
                   g.origin[0] == 0.0 && g.cells() == 8000000);
    // a box thinner than radius_cell on one axis: reach 1, whatever m is
    const double flat_hi[3] = {100, 100, 1.0};
    const mopt::SearchBox wall(lo, flat_hi, 1.0, mopt::kMostCells);
    expectTrue("SearchBox: 1.0 < 1.001 on one axis is thin", wall.thin());
    expectTrue("firstReach: a thin box gives reach 1 for m = 10", wall.firstReach(10, 0) == 1);
    expectTrue("firstReach: a thin box gives reach 1 for m = 1e9", wall.firstReach(1000000000, 0) == 1);
    const double exact_hi[3] = {100, 100, 1.0 * 1.001};
    expectTrue("SearchBox: an extent of exactly radius_cell is not thin",
               !mopt::SearchBox(lo, exact_hi, 1.0, mopt::kMostCells).thin());
  }
  // [0, 1000]^3 searched within 1 under 2^20 = 1048576 cells: 1000^3 at edge 1.001; the edge grows by 1.26
  // until dims <= 101 (101^3 = 1030301), i.e. edge > 1000 / 101 = 9.90: 1.001 x 1.26^9 = 8.01 (125 an axis)
  // does not, 1.001 x 1.26^10 = 10.10 (floor(99.05) + 1 = 100 an axis) does
  {
    const double lo[3] = {0, 0, 0}, hi[3] = {1000, 1000, 1000};
    const mopt::SearchBox box(lo, hi, 1.0, mopt::searchCellCap(20));
    expectTrue("firstReach: 1e9 cells at reach 1 are over the cap, reach stays 1", box.firstReach(5000000, 0) == 1);
    double edge = 1.0 * 1.001;
    for (int k = 0; k < 10; ++k) edge *= 1.26;
    const CellLattice g = box.latticeAt(1);
    expectTrue("latticeAt(1): ten growths by 1.26", g.edge == edge);
    expectTrue("latticeAt(1): dims (100, 100, 100) fit 2^20", g.dims[0] == 100 && g.dims[1] == 100 && g.dims[2] == 100 &&
                                                                 double(g.cells()) <= box.most_cells);
  }
  // the refinement by occupied cells
  {
    using mopt::Refinement;
    expectTrue("refinementPossible: a first binning of some targets", mopt::refinementPossible(1, 0, 0, 1000));
    expectTrue("refinementPossible: not with a forced reach", !mopt::refinementPossible(1, 0, 2, 1000));
    expectTrue("refinementPossible: not without targets", !mopt::refinementPossible(1, 0, 0, 0));
    expectTrue("refinementPossible: not at reach 8 by the volume rule", !mopt::refinementPossible(8, 0, 0, 1000));
    expectTrue("refinementPossible: at reach 8 after a refinement (it may step back)", mopt::refinementPossible(8, 3, 0, 1000));
    Refinement r = mopt::refineReach(1, 0, 0.0, 0, 2.9);
    expectTrue("refineReach: 2.9 targets per occupied cell stop", r.what == Refinement::kStop);
    r = mopt::refineReach(1, 0, 0.0, 0, 3.0);
    expectTrue("refineReach: 3 stop too", r.what == Refinement::kStop);
    r = mopt::refineReach(1, 0, 0.0, 0, 12.0);
    expectTrue("refineReach: 12 per cell at reach 1 want ceil(sqrt(8)) = 3", r.what == Refinement::kFiner && r.reach == 3);
    r = mopt::refineReach(2, 0, 0.0, 0, 3.5);  // ceil(2 sqrt(3.5 / 1.5)) = ceil(3.06) = 4
    expectTrue("refineReach: 3.5 per cell at reach 2 want 4", r.what == Refinement::kFiner && r.reach == 4);
    r = mopt::refineReach(4, 0, 0.0, 0, 3.1);  // ceil(4 sqrt(3.1 / 1.5)) = ceil(5.75) = 6
    expectTrue("refineReach: 3.1 per cell at reach 4 want 6", r.what == Refinement::kFiner && r.reach == 6);
    r = mopt::refineReach(2, 0, 0.0, 0, 600.0);  // ceil(2 sqrt(400)) = 40
    expectTrue("refineReach: never beyond reach 8", r.what == Refinement::kFiner && r.reach == 8);
    // second reading: 9 x 1.5 = 13.5 > 12, thinned out by less than 1.5 times
    r = mopt::refineReach(3, 1, 12.0, 1, 9.0);
    expectTrue("refineReach: 12 -> 9 per cell steps back to the reach before", r.what == Refinement::kStepBack && r.reach == 1);
    r = mopt::refineReach(3, 1, 12.0, 1, 2.0);  // 3 <= 12: thinned out; 2 <= 3 stops
    expectTrue("refineReach: 12 -> 2 per cell stays and stops", r.what == Refinement::kStop);
    r = mopt::refineReach(3, 1, 12.0, 1, 6.0);  // 9 <= 12; ceil(3 sqrt(4)) = 6
    expectTrue("refineReach: 12 -> 6 per cell refines once more, to 6", r.what == Refinement::kFiner && r.reach == 6);
    r = mopt::refineReach(6, 3, 6.0, 2, 3.5);  // 5.25 <= 6: thinned out, but two refinements were made
    expectTrue("refineReach: never a third refinement", r.what == Refinement::kStop);
    r = mopt::refineReach(6, 3, 6.0, 2, 5.0);  // 7.5 > 6
    expectTrue("refineReach: the third binning may still step back", r.what == Refinement::kStepBack && r.reach == 3);
  }
}

int main() {
  optimizerStatuses();
  dispatchPrimitives();
  sweepChoiceRules();
  cellLatticeRules();
  ldlt();
  denseAndSo3();
  lossThresholdRecovery();
  std::printf("SUMMARY %d checks, failures=%d\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
