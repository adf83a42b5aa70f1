// mopt_batch: B independent small point2point problems laid out once and minimised together — lifetime,
// configuration and mopt_batch_lm_minimize.  One launch of B workgroups runs the one-launch solve of a
// small cost (finalize_kernels.hip: p2pSolveBatchKernel, the body of p2pSolveSmallKernel with a workgroup
// index) on every problem at once; each problem has its own x, LM state, report and stopping decision.
// The host takes no decision and copies nothing per iteration: it writes the batch's one problem
// description and the start poses, launches, waits for the B reports and copies them out.
#include "cost_state.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <new>

using namespace mopt_detail;

struct mopt_batch {
  int device = 0;
  int scalar_bytes = 8;
  int num_problems = 0;
  long long total_count = 0;
  int total_tiles = 0;
  // covariance and loss of the batch, held by a cost that owns no device memory: the setters and the
  // argument / basis filling are then the lone cost's own (mopt_cost_set_covariance, fillP2PArgs, fillBasis)
  mopt_cost config;
  hipStream_t stream = nullptr;
  std::vector<long long> offsets;   // [B + 1]
  std::vector<int> first_tile;      // [B + 1]
  std::vector<double> src_center;   // [B][3]: each problem's source bounding sphere, as a cost stores its own
  std::vector<double> src_radius;   // [B]
  std::vector<double> src_bound;    // [B]
  // device memory, one allocation per kind
  void *d_tiles = nullptr;
  long long *d_offsets = nullptr;
  int *d_first_tile = nullptr;
  double *d_bounds = nullptr;
  void *d_args = nullptr;                 // P2PSweepArgs<S>[B]
  mopt::AffineBasis *d_basis = nullptr;   // [B]
  double *d_results = nullptr;            // [B][kBatchResultStride]
  mopt::LmControl *d_controls = nullptr;  // [B][kLmControlBlocks]
  // per call: the problem description followed by the start poses, written into pinned host memory
  // and copied to the device in one piece
  unsigned char *h_stage = nullptr;
  unsigned char *d_stage = nullptr;
  size_t stage_bytes = 0;
  mopt::LmReport *h_reports = nullptr;      // mapped host memory, [B]
  mopt::LmReport *h_reports_dev = nullptr;  // as the device addresses it
  unsigned long long uploaded_version = ~0ull;  // the configuration d_args / d_basis hold
  int uploaded_mode = -1;
  long long stat_choice_points = 0, stat_literal_points = 0;
};

namespace {

constexpr size_t kStageStarts = (sizeof(mopt::LmProblem) + 255) & ~size_t(255);  // offset of the start poses

int tilePoints(int scalar_bytes) {
  return scalar_bytes == 8 ? mopt::TileShape<double>::kPoints : mopt::TileShape<float>::kPoints;
}

void destroyBatch(mopt_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  deviceRelease(b->d_tiles);
  deviceRelease(b->d_offsets);
  deviceRelease(b->d_first_tile);
  deviceRelease(b->d_bounds);
  deviceRelease(b->d_args);
  deviceRelease(b->d_basis);
  deviceRelease(b->d_results);
  deviceRelease(b->d_controls);
  deviceRelease(b->d_stage);
  if (b->h_stage) (void)hipHostFree(b->h_stage);
  if (b->h_reports) (void)hipHostFree(b->h_reports);
  releaseStream(b->device, b->stream);  // synchronised above
  delete b;
}

using BatchPtr = std::unique_ptr<mopt_batch, void (*)(mopt_batch *)>;

// the per-problem argument and basis blocks for this Jacobian mode, when the configuration they were
// filled from has changed (once per configuration, not per call)
template <typename S>
int uploadBlocks(mopt_batch *b, int jac_mode) {
  const int B = b->num_problems;
  std::vector<mopt::P2PSweepArgs<S>> args(B);
  std::vector<mopt::AffineBasis> basis(B);
  const S zero[kNumParams] = {0, 0, 0, 0, 0, 0};
  mopt::P2PSweepArgs<S> common;
  fillP2PArgs<S>(&b->config, zero, false, common);  // loss, covariance; the step writes T, 1 / h
  common.partials = nullptr;                        // (one workgroup a problem: no partial rows)
  mopt::AffineBasis common_basis;
  // as residentPrepareP2P: constant for the analytic modes in the Euclidean parameters, else rewritten
  // per point by the step, of which only the covariance stays
  const bool per_point = jac_mode == MOPT_JAC_NUMERIC || jac_mode == MOPT_JAC_ANALYTIC_LEFT ||
                         jac_mode == MOPT_JAC_ANALYTIC_RIGHT;
  fillBasis<S>(&b->config, per_point ? MOPT_JAC_ANALYTIC : jac_mode, common, common_basis);
  const size_t tile_scalars = size_t(mopt::TileShape<S>::kP2PScalars);
  for (int i = 0; i < B; ++i) {
    args[i] = common;
    args[i].tiles = static_cast<const S *>(b->d_tiles) + size_t(b->first_tile[i]) * tile_scalars;
    args[i].count = b->offsets[i + 1] - b->offsets[i];
    args[i].num_tiles = b->first_tile[i + 1] - b->first_tile[i];
    basis[i] = common_basis;
  }
  MOPT_HIP_TRY(hipMemcpyAsync(b->d_args, args.data(), sizeof(args[0]) * B, hipMemcpyHostToDevice, b->stream));
  MOPT_HIP_TRY(hipMemcpyAsync(b->d_basis, basis.data(), sizeof(basis[0]) * B, hipMemcpyHostToDevice, b->stream));
  MOPT_HIP_TRY(hipStreamSynchronize(b->stream));  // the vectors go out of scope
  return MOPT_OK;
}

inline unsigned long long reportWord(const mopt::LmReport *r) {
  return __atomic_load_n(&r->flag, __ATOMIC_ACQUIRE);
}

}  // namespace

extern "C" {

int mopt_point2point_batch_create(mopt_batch **out, int device, int scalar_bytes, const void *src_xyz,
                                  const void *tgt_xyz, const int64_t *offsets, int num_problems, int flags) {
  if (!out) return fail(MOPT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (!src_xyz || !tgt_xyz || !offsets) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL point arrays / offsets");
  if (num_problems < 1) return fail(MOPT_ERR_INVALID_ARGUMENT, "a batch holds at least one problem");
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 or 8");
  if (unsigned(flags) & ~unsigned(MOPT_INPUT_DEVICE))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown flag bits (MOPT_INPUT_HOST or MOPT_INPUT_DEVICE)");
  if (offsets[0] != 0) return fail(MOPT_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  for (int i = 0; i < num_problems; ++i) {
    if (offsets[i + 1] < offsets[i])
      return fail(MOPT_ERR_INVALID_ARGUMENT, "offsets decrease at problem " + std::to_string(i));
    if (offsets[i + 1] == offsets[i])
      return fail(MOPT_ERR_INVALID_ARGUMENT, "problem " + std::to_string(i) + " is empty");
  }
  const int tile_points = tilePoints(scalar_bytes);
  const int max_tiles = mopt::solveSmallMaxTiles();
  for (int i = 0; i < num_problems; ++i) {
    const long long n = offsets[i + 1] - offsets[i];
    if (n > (long long)max_tiles * tile_points)
      return fail(MOPT_ERR_UNSUPPORTED,
                  "problem " + std::to_string(i) + " has " + std::to_string(n) +
                      " correspondences: a batch solves problems of at most " + std::to_string(max_tiles) +
                      " tiles of " + std::to_string(tile_points) + " (use a mopt_cost and mopt_lm_minimize)");
  }
  BatchPtr b(new (std::nothrow) mopt_batch, destroyBatch);
  if (!b) return fail(MOPT_ERR_HIP, "out of host memory");
  const int B = num_problems;
  b->scalar_bytes = b->config.scalar_bytes = scalar_bytes;
  b->num_problems = B;
  b->total_count = offsets[B];
  b->offsets.assign(offsets, offsets + B + 1);
  b->first_tile.resize(B + 1);
  b->first_tile[0] = 0;
  for (int i = 0; i < B; ++i)
    b->first_tile[i + 1] =
        b->first_tile[i] + int((b->offsets[i + 1] - b->offsets[i] + tile_points - 1) / tile_points);
  b->total_tiles = b->first_tile[B];

  if (const int rc = selectDevice(device)) return rc;
  b->device = b->config.device = device;
  MOPT_HIP_TRY(acquireStream(device, &b->stream));
  hipStream_t s = b->stream;

  const size_t tile_bytes = size_t(tile_points) * 6 * scalar_bytes;
  const size_t args_bytes = scalar_bytes == 8 ? sizeof(mopt::P2PSweepArgs<double>) : sizeof(mopt::P2PSweepArgs<float>);
  MOPT_HIP_TRY(deviceAlloc(&b->d_tiles, tile_bytes * size_t(b->total_tiles)));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&b->d_offsets), sizeof(long long) * (B + 1)));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&b->d_first_tile), sizeof(int) * (B + 1)));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&b->d_bounds), sizeof(double) * B));
  MOPT_HIP_TRY(deviceAlloc(&b->d_args, args_bytes * B));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&b->d_basis), sizeof(mopt::AffineBasis) * B));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&b->d_results),
                           sizeof(double) * mopt::kBatchResultStride * B));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&b->d_controls),
                           sizeof(mopt::LmControl) * mopt::kLmControlBlocks * B));
  b->stage_bytes = kStageStarts + size_t(B) * mopt::kMaxWideParams * scalar_bytes;
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&b->d_stage), b->stage_bytes));
  MOPT_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_stage), b->stage_bytes, hipHostMallocDefault));
  MOPT_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_reports), sizeof(mopt::LmReport) * B,
                             hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(b->h_reports, 0, sizeof(mopt::LmReport) * B);
  MOPT_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->h_reports_dev), b->h_reports, 0));

  MOPT_HIP_TRY(hipMemcpyAsync(b->d_offsets, b->offsets.data(), sizeof(long long) * (B + 1),
                              hipMemcpyHostToDevice, s));
  MOPT_HIP_TRY(hipMemcpyAsync(b->d_first_tile, b->first_tile.data(), sizeof(int) * (B + 1),
                              hipMemcpyHostToDevice, s));
  // the boxes land in the result slots, idle until the first solve: 6 of a problem's 48 doubles
  static_assert(mopt::kBatchResultStride >= 6, "a problem's bounding box");
  std::vector<double> boxes(size_t(B) * 6);
  {
    Staging st;
    const size_t bytes = size_t(b->total_count) * 3 * scalar_bytes;
    const int rc = stageInputs(src_xyz, bytes, tgt_xyz, bytes, unsigned(flags), s, st);
    if (rc != MOPT_OK) return rc;
    MOPT_HIP_TRY(withScalar(scalar_bytes, [&](auto scalar) {
      using S = typename decltype(scalar)::type;
      hipError_t e = mopt::launchRelayoutP2PBatch<S>(static_cast<const S *>(st.a), static_cast<const S *>(st.b),
                                                     b->d_offsets, b->d_first_tile, B, b->total_tiles,
                                                     static_cast<S *>(b->d_tiles), s);
      if (e != hipSuccess) return e;
      // the scale of each scene (leftBasisMayCancel, forwardStepThreshold), as a cost takes its own
      return mopt::launchSourceBoxBatch<S>(static_cast<const S *>(b->d_tiles), b->d_offsets, b->d_first_tile, B,
                                           b->d_results, s);
    }));
    MOPT_HIP_TRY(hipMemcpyAsync(boxes.data(), b->d_results, sizeof(double) * 6 * B, hipMemcpyDeviceToHost, s));
    MOPT_HIP_TRY(hipStreamSynchronize(s));
  }
  b->src_center.resize(size_t(B) * 3);
  b->src_radius.resize(B);
  b->src_bound.resize(B);
  for (int i = 0; i < B; ++i) {  // (the arithmetic of mopt_point2point_set_data)
    double diag2 = 0.0, center2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double lo = boxes[size_t(i) * 6 + k], hi = boxes[size_t(i) * 6 + 3 + k];
      const double c = 0.5 * (lo + hi);
      b->src_center[size_t(i) * 3 + k] = c;
      diag2 += (hi - lo) * (hi - lo);
      center2 += c * c;
    }
    b->src_radius[i] = 0.5 * std::sqrt(diag2);
    b->src_bound[i] = std::sqrt(center2) + b->src_radius[i];
  }
  MOPT_HIP_TRY(hipMemcpyAsync(b->d_bounds, b->src_bound.data(), sizeof(double) * B, hipMemcpyHostToDevice, s));
  MOPT_HIP_TRY(hipStreamSynchronize(s));
  b->config.state_version = 0;
  *out = b.release();
  return MOPT_OK;
}

int mopt_batch_destroy(mopt_batch *batch) {
  destroyBatch(batch);
  return MOPT_OK;
}

int mopt_batch_info(const mopt_batch *batch, int *num_problems, int64_t *total_count, int *scalar_bytes) {
  if (!batch) return fail(MOPT_ERR_INVALID_ARGUMENT, "batch is NULL");
  if (num_problems) *num_problems = batch->num_problems;
  if (total_count) *total_count = batch->total_count;
  if (scalar_bytes) *scalar_bytes = batch->scalar_bytes;
  return MOPT_OK;
}

int mopt_batch_set_covariance(mopt_batch *batch, const void *cov_colmajor) {
  if (!batch) return fail(MOPT_ERR_INVALID_ARGUMENT, "batch is NULL");
  return mopt_cost_set_covariance(&batch->config, cov_colmajor);
}

int mopt_batch_set_loss(mopt_batch *batch, int loss_kind, double parameter) {
  if (!batch) return fail(MOPT_ERR_INVALID_ARGUMENT, "batch is NULL");
  return mopt_cost_set_loss(&batch->config, loss_kind, parameter);
}

int mopt_batch_lm_choice_stats(const mopt_batch *batch, int64_t *points, int64_t *literal_points) {
  if (!batch) return fail(MOPT_ERR_INVALID_ARGUMENT, "batch is NULL");
  if (points) *points = batch->stat_choice_points;
  if (literal_points) *literal_points = batch->stat_literal_points;
  return MOPT_OK;
}

int mopt_batch_lm_minimize(mopt_batch *b, int jacobian_mode, void *x, const mopt_lm_options *options,
                           mopt_lm_report *reports) {
  if (!b || !x) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  if (jacobian_mode < MOPT_JAC_ANALYTIC || jacobian_mode > MOPT_JAC_ANALYTIC_RIGHT)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown jacobian_mode");
  mopt_lm_options opt;
  opt.max_iterations = 15;    // optimizer.h:19
  opt.lm_max_iterations = 3;  // levenberg_marquadt_dyn.cpp:9
  opt.manifold = 0;
  opt.window = 0;
  if (options) opt = *options;
  if (opt.max_iterations < 0 || opt.lm_max_iterations < 0)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "Optimization::max_iterations cannot be less than 0.");
  if (opt.manifold < 0 || opt.manifold > 2)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "mopt_lm_options.manifold is 0 (none), 1 (left) or 2 (right)");
  const int B = b->num_problems;
  mopt_lm_report blank;
  std::memset(&blank, 0, sizeof blank);
  blank.status = MOPT_LM_MAXIMUM_ITERATIONS_REACHED;
  if (opt.max_iterations == 0) {  // the reference's loop body never runs
    for (int i = 0; reports && i < B; ++i) reports[i] = blank;
    return MOPT_OK;
  }
  // The left-basis rule: a cloud far from its frame's origin is one the lone solve sweeps literally, launch
  // per point (sweep_choice.hpp leftBasisMayCancel); the batch holds the moments only.
  if (jacobian_mode == MOPT_JAC_ANALYTIC_LEFT)
    for (int i = 0; i < B; ++i)
      if (mopt::choice::leftBasisMayCancel(&b->src_center[size_t(i) * 3], b->src_radius[i]))
        return fail(MOPT_ERR_UNSUPPORTED,
                    "problem " + std::to_string(i) +
                        ": MOPT_JAC_ANALYTIC_LEFT over a cloud far from its frame's origin (|c0|^2 > 1e3 r^2) is "
                        "evaluated literally, which a batch does not hold (use a mopt_cost and mopt_lm_minimize)");
  // only the linearization at x0 when no trial point is ever formed (lm_max_iterations == 0, below)
  const bool x0_only = opt.lm_max_iterations == 0;
  const long long max_points = x0_only ? 1 : 1 + (long long)opt.max_iterations * opt.lm_max_iterations;
  if (max_points > 4096)  // (the bound of the lone one-launch solve, lm.cpp)
    return fail(MOPT_ERR_UNSUPPORTED,
                "a batch evaluates at most 4096 points per problem (1 + max_iterations * lm_max_iterations)");
  MOPT_HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = b->stream;
  if (b->uploaded_version != b->config.state_version || b->uploaded_mode != jacobian_mode) {
    const int rc = withScalar(b->scalar_bytes, [&](auto scalar) {
      return uploadBlocks<typename decltype(scalar)::type>(b, jacobian_mode);
    });
    if (rc != MOPT_OK) return rc;
    b->uploaded_version = b->config.state_version;
    b->uploaded_mode = jacobian_mode;
  }

  mopt::LmProblem problem;  // control, state, report, cost[0].args / basis / result: per workgroup, on the device
  problem.num_costs = 1;
  problem.n = kNumParams;
  problem.max_iterations = opt.max_iterations;
  problem.lm_max_iterations = opt.lm_max_iterations;
  problem.manifold = opt.manifold;
  problem.cost[0].model = mopt::kLmPoint2Point;
  problem.cost[0].jac_mode = jacobian_mode;
  problem.cost[0].n_out = 3;
  problem.cost[0].moments = 1;
  problem.fd_per_iterate = residentPerIterate(&b->config, jacobian_mode) ? 1 : 0;
  std::memcpy(b->h_stage, &problem, sizeof problem);
  unsigned char *starts = b->h_stage + kStageStarts;
  std::memset(starts, 0, size_t(B) * mopt::kMaxWideParams * b->scalar_bytes);
  for (int i = 0; i < B; ++i)
    std::memcpy(starts + size_t(i) * mopt::kMaxWideParams * b->scalar_bytes,
                static_cast<const unsigned char *>(x) + size_t(i) * kNumParams * b->scalar_bytes,
                size_t(kNumParams) * b->scalar_bytes);
  MOPT_HIP_TRY(hipMemcpyAsync(b->d_stage, b->h_stage, b->stage_bytes, hipMemcpyHostToDevice, s));
  for (int i = 0; i < B; ++i) __atomic_store_n(&b->h_reports[i].flag, 0ull, __ATOMIC_RELEASE);

  mopt::BatchSolveLaunch launch;
  launch.tiles = b->d_tiles;
  launch.first_tile = b->d_first_tile;
  launch.problem = reinterpret_cast<const mopt::LmProblem *>(b->d_stage);
  launch.args = b->d_args;
  launch.basis = b->d_basis;
  launch.results = b->d_results;
  launch.controls = b->d_controls;
  launch.reports = b->h_reports_dev;
  launch.starts = b->d_stage + kStageStarts;
  launch.source_bounds = b->d_bounds;
  launch.num_problems = B;
  launch.max_points = int(max_points);
  launch.fd_per_iterate = problem.fd_per_iterate;
  MOPT_HIP_TRY(withScalar(b->scalar_bytes, [&](auto scalar) {
    return mopt::launchP2PSolveBatch<typename decltype(scalar)::type>(launch, b->config.cov_mode, s);
  }));

  if (x0_only) {
    // every outer iteration would linearize at the same x0 and find the same cost: the loop runs into its
    // limit — unless that cost is already ~0 (mopt_lm_minimize; levenberg_marquadt_dyn.cpp:62-64, :77)
    std::vector<double> results(size_t(B) * mopt::kBatchResultStride);
    MOPT_HIP_TRY(hipMemcpyAsync(results.data(), b->d_results, sizeof(double) * results.size(),
                                hipMemcpyDeviceToHost, s));
    MOPT_HIP_TRY(hipStreamSynchronize(s));
    const double eps = b->scalar_bytes == 8 ? 2.220446049250313e-16 : 1.1920929e-7;
    for (int i = 0; reports && i < B; ++i) {
      const double sum_sq = results[size_t(i) * mopt::kBatchResultStride + kResultDoubles - 1];
      const double y0 = b->scalar_bytes == 8 ? sum_sq : double(float(sum_sq));
      mopt_lm_report rep = blank;
      rep.status = std::fabs(y0) < 8.0 * eps ? MOPT_LM_CONVERGED : MOPT_LM_MAXIMUM_ITERATIONS_REACHED;
      rep.iterations = rep.status == MOPT_LM_CONVERGED ? 0 : opt.max_iterations;
      rep.sweeps = 1;
      rep.cost = y0;
      reports[i] = rep;
    }
    return MOPT_OK;
  }

  // wait for the B reports: each is complete once its word has the low bit (payload first, then the word)
  const auto started = std::chrono::steady_clock::now();
  unsigned long long spins = 0;
  for (int next = 0; next < B;) {
    if (reportWord(&b->h_reports[next]) & 1ull) {
      ++next;
      continue;
    }
    if ((++spins & 0x3fff) == 0) {
      const hipError_t q = hipStreamQuery(s);
      if (q != hipSuccess && q != hipErrorNotReady)
        return fail(MOPT_ERR_HIP, std::string("batch solve failed: ") + hipGetErrorString(q));
      if (q == hipSuccess && !(reportWord(&b->h_reports[next]) & 1ull))
        return fail(MOPT_ERR_HIP, "batch solve drained without a status for problem " + std::to_string(next));
      if (std::chrono::steady_clock::now() - started > std::chrono::seconds(120))
        return fail(MOPT_ERR_HIP, "timed out waiting for the batch solve (120 s)");
    }
    __builtin_ia32_pause();
  }
  for (int i = 0; i < B; ++i) {
    mopt::LmReport snap;
    std::memcpy(&snap, &b->h_reports[i], sizeof snap);
    if (problem.fd_per_iterate) {
      b->stat_choice_points += (long long)snap.trials;
      b->stat_literal_points += (long long)snap.pad[0];
    }
    if (b->scalar_bytes == 8)
      for (int k = 0; k < kNumParams; ++k) static_cast<double *>(x)[size_t(i) * kNumParams + k] = snap.x[k];
    else
      for (int k = 0; k < kNumParams; ++k) static_cast<float *>(x)[size_t(i) * kNumParams + k] = float(snap.x[k]);
    if (reports) {
      mopt_lm_report rep = blank;
      rep.status = int(snap.status);
      rep.iterations = int(snap.iterations);
      rep.sweeps = (long long)snap.trials;
      rep.cost = snap.cost;
      rep.lambda = snap.lambda;
      reports[i] = rep;
    }
  }
  return MOPT_OK;
}

}  // extern "C"
