// Launching one sweep: the once-per-x host work (SE(3) transforms, forward-difference steps, the affine
// Jacobian basis), the choice between the moments and the literal kernels, the grid, the timing of a
// profiled launch, and per model the sweep + finalize pair enqueued on a stream.  Each model's argument
// filling stands beside its launch; blocking.cpp and group.cpp enter through linearizeAsyncImpl /
// costAsyncImpl at the end, resident.cpp uses the argument filling and the grid rules.
#include "cost_state.hpp"

#include <cmath>
#include <cstring>
#include <limits>

#include "moptimizer_amd/so3.hpp"

namespace mopt_detail {

// MOPT_BLOCKS_PER_CU (tuning override of the workgroups launched per CU) is read once per process.
int blocksPerCu(int fallback) {
  static const int forced = envInt("MOPT_BLOCKS_PER_CU", 0);
  return forced > 0 ? forced : fallback;
}

int gridFor(const mopt_cost *c, int blocks_per_cu) {
  return mopt::choice::gridFor(c->num_cus, blocks_per_cu, c->num_tiles, c->max_grid);
}

// Every pair leaves pending_events exactly once, whatever fails: a pair whose timing cannot be read
// is dropped from the statistics and its events destroyed (not recycled: they may still be pending).
int resolvePendingEvents(mopt_cost *c) {
  int rc = MOPT_OK;
  for (auto &pr : c->pending_events) {
    float ms = 0.f;
    hipError_t e = rc == MOPT_OK ? hipEventSynchronize(pr.second) : hipErrorUnknown;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.first, pr.second);
    if (e == hipSuccess) {
      c->sweep_ms_total += double(ms);
      c->sweep_launches += 1;
      c->free_events.push_back(pr.first);
      c->free_events.push_back(pr.second);
    } else {
      if (rc == MOPT_OK)
        rc = fail(MOPT_ERR_HIP, std::string("sweep timing events: ") + hipGetErrorString(e));
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  }
  c->pending_events.clear();
  return rc;
}

namespace {
// Times the dominant kernel of a sweep with a pair of HIP events on the launch stream when
// profiling samples this launch.  The moments / cost sweeps have their dispatch timestamped into
// the events (hipExtLaunchKernelGGL: agrees with rocprofv3's kernel trace to 0.2 us, costs the
// host ~10 us, which is why launches are sampled); the other sweeps get a recorded pair around
// the launch (reads 1-3 us longer than the kernel, costs ~6 us).
struct SweepTimer {
  mopt_cost *c;
  mopt::LaunchSite site;
  hipEvent_t start = nullptr, stop_ev = nullptr;
  bool dispatch_stamped = false;
  bool aql_used = false;  // the sweep kernel went to the cost's own queue (aql.hpp): so must its finalize
  mopt_detail::AqlSite finalize_site;  // the same queue, never timed (the timing is the sweep's)
  const mopt_detail::AqlSite *aql() {
    if (!aql_used) return nullptr;
    c->stat_direct_sweeps += 1;
    c->sweep_went_direct = true;
    finalize_site = site.aql;
    finalize_site.timed_for = nullptr;
    return &finalize_site;
  }
  SweepTimer(const SweepTimer &) = delete;
  SweepTimer(mopt_cost *cost, hipStream_t stream, bool stamp_dispatch = false) : c(cost) {
    site.stream = stream;
    if (cost->aql_now.queue && stream == cost->stream) {
      site.aql = cost->aql_now;
      site.aql_used = &aql_used;
    }
    // Streaming (non-temporal) loads once the tiles exceed the 32 MiB of aggregate L2: measured
    // faster both beyond the 256 MiB Infinity Cache (10 M points: 82 -> 77 us) and inside it
    // (1 M points: 12.3 -> 11.6 us); below that the default policy lets sweeps re-hit L2.
    static const int force = envInt("MOPT_STREAMING_LOADS", 0);  // 1 = never, 2 = always (tuning)
    const size_t bytes = size_t(cost->count) * 6 * size_t(cost->scalar_bytes);
    site.streaming = force == 2 || (force != 1 && bytes > (size_t(32) << 20));
    if (cost->profiling <= 0 || (cost->profiling_tick++ % cost->profiling) != 0) return;
    if (site.aql.queue && stamp_dispatch) {
      // the direct path stamps its own dispatch: the packet processor's start and end of this very
      // kernel, read after the call's results have arrived (blockingSweep)
      site.aql.timed_for = cost;
      cost->aql_timed = true;
      return;
    }
    site.aql = mopt_detail::AqlSite();  // (a sweep timed with recorded events goes to the stream)
    site.aql_used = nullptr;
    if (cost->pending_events.size() >= 4096 && resolvePendingEvents(cost) != MOPT_OK) return;
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (auto &e : ev) {
      if (!cost->free_events.empty()) {
        e = cost->free_events.back();
        cost->free_events.pop_back();
      } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
      }
    }
    if (!ev[0] || !ev[1]) {  // keep the one that was obtained
      for (auto e : ev)
        if (e) cost->free_events.push_back(e);
      return;
    }
    if (stamp_dispatch) {
      start = site.time_start = ev[0];
      stop_ev = site.time_stop = ev[1];
      dispatch_stamped = true;
    } else if (hipEventRecord(ev[0], stream) == hipSuccess) {
      start = ev[0];
      stop_ev = ev[1];
    } else {
      cost->free_events.push_back(ev[0]);
      cost->free_events.push_back(ev[1]);
    }
  }
  void stop() {
    if (!start || !stop_ev) return;
    if (dispatch_stamped || hipEventRecord(stop_ev, site.stream) == hipSuccess)
      c->pending_events.emplace_back(start, stop_ev);
  }
};
}  // namespace

// Forward-difference points of the reference (linearization.h:78-92): h_j = sqrt(eps) |x_j|,
// or sqrt(eps) when that is zero; x_plus_j = x + h_j e_j.
template <typename S>
void forwardSteps(const S *x, S h[kNumParams], S x_plus[kNumParams][kNumParams]) {
  MOPT_SO3_EXACT_BODY  // x + h is a rounded product added to x, never a fused multiply-add
  const S min_step = std::sqrt(std::numeric_limits<S>::epsilon());
  for (int j = 0; j < kNumParams; ++j) {
    h[j] = min_step * std::fabs(x[j]);
    if (h[j] == S(0)) h[j] = min_step;
    for (int k = 0; k < kNumParams; ++k) x_plus[j][k] = x[k];
    x_plus[j][j] += h[j];
  }
}

template <typename S>
void fillP2PArgs(const mopt_cost *c, const S *x, bool with_steps, mopt::P2PSweepArgs<S> &a) {
  a.tiles = static_cast<const S *>(c->d_tiles);
  a.count = c->count;
  a.num_tiles = c->num_tiles;
  a.loss_kind = c->loss_kind;
  a.loss_param = S(c->loss_param);
  a.partials = c->d_partials;
  const auto T0 = moptimizer::so3::rigidFrom6DOF<S>(x);
  std::memcpy(a.T[0], T0.m, sizeof T0.m);
  for (int j = 0; j < kNumParams; ++j) {
    std::memcpy(a.T[1 + j], T0.m, sizeof T0.m);
    a.inv_h[j] = S(0);
  }
  if (with_steps) {
    S h[kNumParams], xp[kNumParams][kNumParams];
    forwardSteps<S>(x, h, xp);
    for (int j = 0; j < kNumParams; ++j) {
      const auto Tj = moptimizer::so3::rigidFrom6DOF<S>(xp[j]);
      std::memcpy(a.T[1 + j], Tj.m, sizeof Tj.m);
      a.inv_h[j] = S(1) / h[j];
    }
  }
  for (int k = 0; k < 9; ++k) a.cov[k] = S(c->cov[k]);
}

// The 3x6 row-major Jacobian pattern of a point, host copy of the device formulas; used to
// derive the affine basis J(p) = J0 + px Jx + py Jy + pz Jz.
static void analyticPattern(int jac_mode, const double p[3], double J[18]) {
  for (int k = 0; k < 18; ++k) J[k] = 0.0;
  if (jac_mode == MOPT_JAC_ANALYTIC) {
    J[0 * 6 + 0] = 1; J[1 * 6 + 1] = 1; J[2 * 6 + 2] = 1;
    J[0 * 6 + 4] = p[2];  J[0 * 6 + 5] = -p[1];
    J[1 * 6 + 3] = -p[2]; J[1 * 6 + 5] = p[0];
    J[2 * 6 + 3] = p[1];  J[2 * 6 + 4] = -p[0];
  } else {
    J[0 * 6 + 0] = 1; J[0 * 6 + 4] = 1;
    J[1 * 6 + 2] = 1; J[1 * 6 + 4] = -p[2]; J[1 * 6 + 5] = p[1];
    J[2 * 6 + 0] = p[2]; J[2 * 6 + 2] = -p[0]; J[2 * 6 + 3] = -p[1]; J[2 * 6 + 4] = p[0];
  }
}

template <typename S>
void fillBasis(const mopt_cost *c, int jac_mode, const mopt::P2PSweepArgs<S> &a,
               mopt::AffineBasis &B) {
  if (jac_mode == MOPT_JAC_NUMERIC) {
    // column j of J is ((R_j - R) p + (t_j - t)) / h_j
    for (int r = 0; r < 3; ++r)
      for (int j = 0; j < kNumParams; ++j) {
        B.J[0][r * 6 + j] = double((a.T[1 + j][r * 4 + 3] - a.T[0][r * 4 + 3]) * a.inv_h[j]);
        for (int k = 0; k < 3; ++k)
          B.J[1 + k][r * 6 + j] = double((a.T[1 + j][r * 4 + k] - a.T[0][r * 4 + k]) * a.inv_h[j]);
      }
  } else if (jac_mode == MOPT_JAC_ANALYTIC_LEFT) {
    // J(p) = [I | -skew(R p + t)] is the conformant pattern taken at the warped point, which is
    // affine in p: J0 at t, J_k the change along column k of R
    double w[3] = {double(a.T[0][3]), double(a.T[0][7]), double(a.T[0][11])};
    analyticPattern(MOPT_JAC_ANALYTIC, w, B.J[0]);
    for (int k = 0; k < 3; ++k) {
      const double wk[3] = {w[0] + double(a.T[0][0 * 4 + k]), w[1] + double(a.T[0][1 * 4 + k]),
                            w[2] + double(a.T[0][2 * 4 + k])};
      analyticPattern(MOPT_JAC_ANALYTIC, wk, B.J[1 + k]);
      for (int q = 0; q < 18; ++q) B.J[1 + k][q] -= B.J[0][q];
    }
  } else if (jac_mode == MOPT_JAC_ANALYTIC_RIGHT) {
    // J(p) = [I | -R skew(p)]: J0 = [I | 0], J_k = [0 | -R skew(e_k)]
    for (int q = 0; q < 18; ++q) B.J[0][q] = B.J[1][q] = B.J[2][q] = B.J[3][q] = 0.0;
    B.J[0][0 * 6 + 0] = B.J[0][1 * 6 + 1] = B.J[0][2 * 6 + 2] = 1.0;
    for (int k = 0; k < 3; ++k) {
      double e[3] = {0, 0, 0};
      e[k] = 1.0;
      const double skew[3][3] = {{0, -e[2], e[1]}, {e[2], 0, -e[0]}, {-e[1], e[0], 0}};
      for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 3; ++col) {
          double v = 0.0;
          for (int m = 0; m < 3; ++m) v += double(a.T[0][r * 4 + m]) * skew[m][col];
          B.J[1 + k][r * 6 + 3 + col] = -v;
        }
    }
  } else {
    const double origin[3] = {0, 0, 0};
    analyticPattern(jac_mode, origin, B.J[0]);
    for (int k = 0; k < 3; ++k) {
      double e[3] = {0, 0, 0};
      e[k] = 1.0;
      analyticPattern(jac_mode, e, B.J[1 + k]);
      for (int q = 0; q < 18; ++q) B.J[1 + k][q] -= B.J[0][q];
    }
  }
  for (int k = 0; k < 9; ++k) B.cov[k] = c->cov[k];
}

// AUTO's choice for forward differences (sweep_choice.hpp), at the cost's stored bound of |p|
template <typename S>
static bool hasSmallForwardStep(const mopt_cost *c, const S *x) {
  double xd[kNumParams];
  for (int j = 0; j < kNumParams; ++j) xd[j] = double(x[j]);
  return mopt::choice::hasSmallForwardStep(c->src_bound, xd);
}

template <typename S>
static int p2pLinearizeAsync(mopt_cost *c, int jac_mode, const S *x, double *d_result, hipStream_t s,
                      const mopt::HostPublish &pub) {
  mopt::P2PSweepArgs<S> args;
  fillP2PArgs<S>(c, x, jac_mode == MOPT_JAC_NUMERIC, args);
  bool moments = c->variant != MOPT_KERNEL_LITERAL;
  if (moments && c->variant != MOPT_KERNEL_MOMENTS_ALWAYS) {
    if (jac_mode == MOPT_JAC_NUMERIC) {
      moments = !hasSmallForwardStep<S>(c, x);
    } else if (jac_mode == MOPT_JAC_ANALYTIC_LEFT) {
      double R[9], t[3];
      for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) R[r * 3 + k] = double(args.T[0][r * 4 + k]);
        t[r] = double(args.T[0][r * 4 + 3]);
      }
      moments = !mopt::choice::leftBasisCancels(c->src_center, c->src_radius, R, t);
    }
  }
  if (moments) {
    mopt::AffineBasis basis;
    fillBasis<S>(c, jac_mode, args, basis);
    const int grid = gridFor(c, blocksPerCu(1));
    SweepTimer timer(c, s, true);
    MOPT_HIP_TRY(mopt::launchP2PMoments<S>(args, grid, timer.site));
    timer.stop();
    MOPT_HIP_TRY(mopt::launchFinalizeMoments(c->d_partials, grid, basis, d_result, pub, s, c->launch_peers,
                                             timer.aql()));
  } else {
    // forward differences: two workgroups per CU (VALU-heavy: the second wave per SIMD pays); the
    // analytic patterns stream like the moments sweep: one (70.8 vs 72.1 us at 10 M, and half the
    // partial rows for the finalize kernel)
    const int grid = gridFor(c, blocksPerCu(jac_mode == MOPT_JAC_NUMERIC ? 2 : 1));
    const int nacc = mopt::denseRowLength(c->cov_mode);
    // (tiled launch signature: dispatch timestamps like the moments sweep)
    SweepTimer timer(c, s, true);
    MOPT_HIP_TRY(mopt::launchP2PLinearizeLiteral<S>(args, jac_mode, c->cov_mode, grid, timer.site));
    timer.stop();
    MOPT_HIP_TRY(mopt::launchFinalizeDense(c->d_partials, grid, nacc, kNumParams, d_result, pub, s,
                                           c->launch_peers, timer.aql()));
  }
  return MOPT_OK;
}

template <typename S>
static int p2pCostAsync(mopt_cost *c, const S *x, double *d_sum, hipStream_t s,
                 const mopt::HostPublish &pub) {
  mopt::P2PSweepArgs<S> args;
  fillP2PArgs<S>(c, x, false, args);
  const int grid = gridFor(c, blocksPerCu(1));
  SweepTimer timer(c, s, true);
  MOPT_HIP_TRY(mopt::launchP2PCost<S>(args, grid, timer.site));
  timer.stop();
  MOPT_HIP_TRY(mopt::launchFinalizeCost(c->d_partials, grid, d_sum, pub, s, c->launch_peers, timer.aql()));
  return MOPT_OK;
}

// (K * T) * C, row-major 3x4, the matrix products of tst/camera_calibration.cpp:37.
static void projectionFor(const mopt_cost *c, const double *x, double M[12]) {
  MOPT_SO3_EXACT_BODY  // bit-identical to the oracle's products: forward differences amplify an ulp
  const auto T = moptimizer::so3::rigidFrom6DOF<double>(x);
  double T4[16];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) T4[r * 4 + k] = T.m[r * 4 + k];
  T4[12] = T4[13] = T4[14] = 0.0;
  T4[15] = 1.0;
  double KT[12];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) {
      double v = 0.0;
      for (int q = 0; q < 4; ++q) v += c->camera[r * 4 + q] * T4[q * 4 + k];
      KT[r * 4 + k] = v;
    }
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) {
      double v = 0.0;
      for (int q = 0; q < 4; ++q) v += KT[r * 4 + q] * c->frame[q * 4 + k];
      M[r * 4 + k] = v;
    }
}

void fillReprojArgs(const mopt_cost *c, const double *x, bool with_steps,
                    mopt::ReprojSweepArgs &a) {
  a.tiles = static_cast<const unsigned char *>(c->d_tiles);
  a.count = c->count;
  a.num_tiles = c->num_tiles;
  a.loss_kind = c->loss_kind;
  a.loss_param = c->loss_param;
  a.partials = c->d_partials;
  projectionFor(c, x, a.M[0]);
  for (int j = 0; j < kNumParams; ++j) {
    std::memcpy(a.M[1 + j], a.M[0], sizeof a.M[0]);
    a.inv_h[j] = 0.0;
  }
  if (with_steps) {
    double h[kNumParams], xp[kNumParams][kNumParams];
    forwardSteps<double>(x, h, xp);
    for (int j = 0; j < kNumParams; ++j) {
      projectionFor(c, xp[j], a.M[1 + j]);
      a.inv_h[j] = 1.0 / h[j];
    }
  }
  // row-major 2x2 out of the 3x3 slot
  a.cov[0] = c->cov[0]; a.cov[1] = c->cov[1];
  a.cov[2] = c->cov[3]; a.cov[3] = c->cov[4];
}

static int reprojLinearizeAsync(mopt_cost *c, int jac_mode, const double *x, double *d_result,
                         hipStream_t s, const mopt::HostPublish &pub) {
  if (jac_mode != MOPT_JAC_NUMERIC)
    return fail(MOPT_ERR_UNSUPPORTED,
                "the reprojection model has no analytic Jacobian (BaseModel, numeric only)");
  mopt::ReprojSweepArgs args;
  fillReprojArgs(c, x, true, args);
  const int grid = gridFor(c, blocksPerCu(2));
  const int nacc = mopt::denseRowLength(c->cov_mode);
  SweepTimer timer(c, s, true);
  MOPT_HIP_TRY(mopt::launchReprojLinearize(args, c->cov_mode, grid, timer.site));
  timer.stop();
  MOPT_HIP_TRY(mopt::launchFinalizeDense(c->d_partials, grid, nacc, kNumParams, d_result, pub, s,
                                         c->launch_peers, timer.aql()));
  return MOPT_OK;
}

static int reprojCostAsync(mopt_cost *c, const double *x, double *d_sum, hipStream_t s,
                    const mopt::HostPublish &pub) {
  mopt::ReprojSweepArgs args;
  fillReprojArgs(c, x, false, args);
  const int grid = gridFor(c, blocksPerCu(2));
  SweepTimer timer(c, s, true);
  MOPT_HIP_TRY(mopt::launchReprojCost(args, grid, timer.site));
  timer.stop();
  MOPT_HIP_TRY(mopt::launchFinalizeCost(c->d_partials, grid, d_sum, pub, s, c->launch_peers, timer.aql()));
  return MOPT_OK;
}

template <typename S>
void fillScalarArgs(const mopt_cost *c, const S *x, mopt::ScalarSweepArgs<S> &a) {
  a.data = static_cast<const S *>(c->d_tiles);
  a.count = c->count;
  a.stride = c->data_stride;
  a.loss_kind = c->loss_kind;
  a.loss_param = S(c->loss_param);
  a.partials = c->d_partials;
  const S min_step = std::sqrt(std::numeric_limits<S>::epsilon());  // linearization.h:78
  for (int j = 0; j < mopt::kMaxParams; ++j) {
    a.x[j] = j < c->n_params ? x[j] : S(0);
    S h = min_step * std::fabs(a.x[j]);  // :85
    if (h == S(0)) h = min_step;         // :87
    a.h[j] = h;
  }
  for (int k = 0; k < 16; ++k) a.cov[k] = S(c->cov_m[k]);
}

static bool scalarModelHasJacobian(int kind) {
  return kind != mopt::kScalarExpCurve && kind != mopt::kScalarExpCurveMarked;
}

// The Jacobian modes of the generic models (built-in scalar and run-time compiled; blocking calls and
// the device-resident loop): forward differences always, the model's own where it has one.
int checkModelJacobian(const mopt_cost *c, int jac_mode) {
  if (jac_mode == MOPT_JAC_ANALYTIC_TST_LAYOUT || jac_mode == MOPT_JAC_ANALYTIC_LEFT ||
      jac_mode == MOPT_JAC_ANALYTIC_RIGHT)
    return fail(MOPT_ERR_UNSUPPORTED,
                "the as-written layout and the perturbation Jacobians apply to point2point only");
  const bool has_jacobian =
      c->model == kModelJit ? c->jit.has_jacobian : scalarModelHasJacobian(c->scalar_model);
  if (jac_mode == MOPT_JAC_ANALYTIC && !has_jacobian)
    return fail(MOPT_ERR_UNSUPPORTED, "Non implemented non-jacobian model function `f_df` being used.");
  return MOPT_OK;
}

// workgroups (= partial rows) of a built-in scalar model's sweep: a workgroup per 256 packs of 16
// bytes, at most four per CU
int scalarGrid(const mopt_cost *c) {
  const long long per_block = (long long)mopt::kBlockThreads * (16 / c->scalar_bytes);
  long long blocks = (c->count + per_block - 1) / per_block;
  if (blocks > c->num_cus * 4) blocks = c->num_cus * 4;
  return blocks < 1 ? 1 : int(blocks);
}

template <typename S>
static int scalarSweepAsync(mopt_cost *c, bool cost_only, int jac_mode, const S *x, double *d_out,
                     hipStream_t s, const mopt::HostPublish &pub) {
  if (!cost_only) {
    const int rc = checkModelJacobian(c, jac_mode);
    if (rc != MOPT_OK) return rc;
  }
  mopt::ScalarSweepArgs<S> args;
  fillScalarArgs<S>(c, x, args);
  const int grid = scalarGrid(c);
  const int n = c->n_params;
  SweepTimer timer(c, s);
  MOPT_HIP_TRY(mopt::launchScalarModel<S>(args, c->scalar_model, cost_only, jac_mode, c->cov_mode,
                                          grid, timer.site));
  timer.stop();
  if (cost_only) {
    MOPT_HIP_TRY(mopt::launchFinalizeCost(c->d_partials, grid, d_out, pub, s, c->launch_peers, timer.aql()));
  } else {
    MOPT_HIP_TRY(mopt::launchFinalizeDense(c->d_partials, grid, mopt::denseRowLength(n, c->cov_mode), n,
                                           d_out, pub, s, c->launch_peers, timer.aql()));
  }
  return MOPT_OK;
}

template <typename S>
void fillJitArgs(const mopt_cost *c, const S *x, mopt::JitArgs<S> &args) {
  mopt::ScalarSweepArgs<S> filled;
  fillScalarArgs<S>(c, x, filled);
  args.data = filled.data;
  args.count = filled.count;
  args.stride = filled.stride;
  args.loss_kind = filled.loss_kind;
  args.pad_[0] = args.pad_[1] = args.pad_[2] = 0;
  args.loss_param = filled.loss_param;
  for (int k = 0; k < 8; ++k) {
    args.x[k] = filled.x[k];
    args.h[k] = filled.h[k];
  }
  for (int k = 0; k < 16; ++k) args.cov[k] = filled.cov[k];
  args.partials = c->d_partials;
}

template <typename S>
void fillJitWideArgs(const mopt_cost *c, const S *x, mopt::JitWideArgs<S> &args) {
  args.data = static_cast<const S *>(c->d_tiles);
  args.count = c->count;
  args.stride = c->data_stride;
  args.loss_kind = c->loss_kind;
  args.pad_[0] = args.pad_[1] = args.pad_[2] = 0;
  args.loss_param = S(c->loss_param);
  const S min_step = std::sqrt(std::numeric_limits<S>::epsilon());  // linearization.h:78
  for (int j = 0; j < mopt::kMaxWideParams; ++j) {
    args.x[j] = j < c->n_params ? x[j] : S(0);
    S h = min_step * std::fabs(args.x[j]);  // :85
    if (h == S(0)) h = min_step;            // :87
    args.h[j] = h;
  }
  for (int k = 0; k < mopt::kMaxWideOutputs * mopt::kMaxWideOutputs; ++k) args.cov[k] = S(c->cov_m[k]);
  args.partials = c->d_partials;
}

int jitGrid(const mopt_cost *c) {
  if (c->jit.wide) {
    long long blocks = (c->count + mopt::kJitWideElementsPerBlock - 1) / mopt::kJitWideElementsPerBlock;
    if (blocks > c->num_cus * 2) blocks = c->num_cus * 2;  // rows of up to 273 doubles
    return blocks < 1 ? 1 : int(blocks);
  }
  const long long per_block = (long long)mopt::kBlockThreads * (16 / c->scalar_bytes);
  long long blocks = (c->count + per_block - 1) / per_block;
  if (blocks > c->num_cus * 4) blocks = c->num_cus * 4;
  if (blocks < 1) blocks = 1;
  return int(blocks);
}

// rows of a run-time compiled model's sweep (the column-per-lane sweep of a wide one has one form)
int jitDenseRow(const mopt_cost *c) {
  return mopt::denseRowLength(c->n_params, c->jit.wide ? int(mopt::kCovGeneral) : c->cov_mode);
}

// User-defined (hipRTC) model: same sweep shape as the built-in scalar models, full-form rows.
template <typename S>
static int jitSweepAsync(mopt_cost *c, bool cost_only, int jac_mode, const S *x, double *d_out,
                  hipStream_t s, const mopt::HostPublish &pub) {
  if (!cost_only) {
    const int rc = checkModelJacobian(c, jac_mode);
    if (rc != MOPT_OK) return rc;
  }
  const int mode = cost_only ? 0 : (jac_mode == MOPT_JAC_NUMERIC ? 2 : 1);
  const mopt::JitVariant *variant = mopt::jitVariant(c->jit, mode, c->cov_mode);
  if (!variant) return fail(MOPT_ERR_INVALID_ARGUMENT, mopt::jitLastError());
  const int grid = jitGrid(c);
  const int n = c->n_params;
  SweepTimer timer(c, s);
  if (c->jit.wide) {
    mopt::JitWideArgs<S> args;
    fillJitWideArgs<S>(c, x, args);
    MOPT_HIP_TRY(mopt::jitLaunch(*variant, &args, sizeof args, grid, s));
  } else {
    mopt::JitArgs<S> args;
    fillJitArgs<S>(c, x, args);
    MOPT_HIP_TRY(mopt::jitLaunch(*variant, &args, sizeof args, grid, s));
  }
  timer.stop();
  if (cost_only) {
    MOPT_HIP_TRY(mopt::launchFinalizeCost(c->d_partials, grid, d_out, pub, s, c->launch_peers));
  } else {
    MOPT_HIP_TRY(mopt::launchFinalizeDense(c->d_partials, grid, jitDenseRow(c), n, d_out, pub, s,
                                           c->launch_peers));
  }
  return MOPT_OK;
}

int linearizeAsyncImpl(mopt_cost *c, int jac_mode, const void *x, double *d_result, hipStream_t s,
                       const mopt::HostPublish &pub) {
  if (jac_mode < MOPT_JAC_ANALYTIC || jac_mode > MOPT_JAC_ANALYTIC_RIGHT)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown jacobian_mode");
  if (c->model == kModelReprojection)
    return reprojLinearizeAsync(c, jac_mode, static_cast<const double *>(x), d_result, s, pub);
  return withScalar(c->scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    const S *xs = static_cast<const S *>(x);
    if (c->model == kModelJit) return jitSweepAsync<S>(c, false, jac_mode, xs, d_result, s, pub);
    if (c->model == kModelScalar) return scalarSweepAsync<S>(c, false, jac_mode, xs, d_result, s, pub);
    return p2pLinearizeAsync<S>(c, jac_mode, xs, d_result, s, pub);
  });
}

int costAsyncImpl(mopt_cost *c, const void *x, double *d_sum, hipStream_t s,
                  const mopt::HostPublish &pub) {
  if (c->model == kModelReprojection)
    return reprojCostAsync(c, static_cast<const double *>(x), d_sum, s, pub);
  return withScalar(c->scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    const S *xs = static_cast<const S *>(x);
    if (c->model == kModelJit) return jitSweepAsync<S>(c, true, 0, xs, d_sum, s, pub);
    if (c->model == kModelScalar) return scalarSweepAsync<S>(c, true, 0, xs, d_sum, s, pub);
    return p2pCostAsync<S>(c, xs, d_sum, s, pub);
  });
}

// the templates other units call (cost_state.hpp)
#define MOPT_INSTANTIATE_FILLS(S)                                                                  \
  template void forwardSteps<S>(const S *, S[kNumParams], S[kNumParams][kNumParams]);             \
  template void fillP2PArgs<S>(const mopt_cost *, const S *, bool, mopt::P2PSweepArgs<S> &);      \
  template void fillBasis<S>(const mopt_cost *, int, const mopt::P2PSweepArgs<S> &, mopt::AffineBasis &); \
  template void fillScalarArgs<S>(const mopt_cost *, const S *, mopt::ScalarSweepArgs<S> &);      \
  template void fillJitArgs<S>(const mopt_cost *, const S *, mopt::JitArgs<S> &);                 \
  template void fillJitWideArgs<S>(const mopt_cost *, const S *, mopt::JitWideArgs<S> &);
MOPT_INSTANTIATE_FILLS(float)
MOPT_INSTANTIATE_FILLS(double)
#undef MOPT_INSTANTIATE_FILLS

}  // namespace mopt_detail
