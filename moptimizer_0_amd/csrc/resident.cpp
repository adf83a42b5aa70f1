// Resident sweeps for the device-resident LM (lm.cpp): a cost's sweep constants uploaded once and
// rewritten by the step kernel per trial point, and the sweep + finalize kernels that read them and the
// loop's control block — per cost, or all costs of a problem in one launch.  The argument filling and the
// grid rules are those of the blocking calls (sweep_launch.cpp).
#include "cost_state.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>

namespace mopt_detail {

template <typename Args>
static int uploadArgs(mopt_cost *c, const Args &host_value, hipStream_t s) {
  if (!c->d_lm_args) MOPT_HIP_TRY(deviceAlloc(&c->d_lm_args, 4096));  // >= every Args struct
  static_assert(sizeof(Args) <= 4096, "resident argument block too small");
  MOPT_HIP_TRY(mopt::launchStoreArgs<Args>(host_value, static_cast<Args *>(c->d_lm_args), s));
  return MOPT_OK;
}

// A generic model's argument block (x[] | h[] inside it, of Args' own length): where the step kernel
// writes them, and, when `stale`, the static part (data, loss, covariance; filled at x = 0) uploaded.
template <typename Args, typename S>
static int residentPrepareModel(mopt_cost *c, void (*fill)(const mopt_cost *, const S *, Args &), bool stale,
                         double *partials, hipStream_t s, mopt::LmCostDesc *desc) {
  constexpr int kSlots = int(sizeof(Args::x) / sizeof(S));
  desc->x_slots = kSlots;
  desc->x_offset = int(offsetof(Args, x));
  if (!stale) return MOPT_OK;
  Args args;
  const S zero[kSlots] = {0};
  fill(c, zero, args);
  args.partials = partials;
  return uploadArgs(c, args, s);
}

template <typename S>
static int residentPrepareP2P(mopt_cost *c, int jac_mode, bool moments, double *partials, hipStream_t s) {
  mopt::P2PSweepArgs<S> args;
  const S zero[kNumParams] = {0, 0, 0, 0, 0, 0};
  fillP2PArgs<S>(c, zero, false, args);  // data, loss, covariance; the step kernel writes T, 1/h
  args.partials = partials;
  int rc = uploadArgs(c, args, s);
  if (rc != MOPT_OK) return rc;
  if (moments) {
    mopt::AffineBasis basis;
    // analytic modes in the Euclidean parameters: the whole basis is independent of x; forward
    // differences and the left-perturbation form: the step kernel rewrites J per point and only the
    // covariance stays
    const bool per_point = jac_mode == MOPT_JAC_NUMERIC || jac_mode == MOPT_JAC_ANALYTIC_LEFT ||
                           jac_mode == MOPT_JAC_ANALYTIC_RIGHT;
    fillBasis<S>(c, per_point ? MOPT_JAC_ANALYTIC : jac_mode, args, basis);
    if (!c->d_lm_basis)
      MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&c->d_lm_basis), sizeof(mopt::AffineBasis)));
    MOPT_HIP_TRY(mopt::launchStoreArgs<mopt::AffineBasis>(basis, c->d_lm_basis, s));
  }
  return MOPT_OK;
}

// rows of moments or dense rows: the rule of sweep_choice.hpp with this cost's fields
static bool usesMoments(const mopt_cost *c, int jac_mode) {
  return mopt::choice::usesMoments(c->model == kModelPoint2Point, c->variant, jac_mode,
                                   mopt::choice::leftBasisMayCancel(c->src_center, c->src_radius));
}

bool residentPerIterate(const mopt_cost *c, int jac_mode) {
  static const bool enabled = envInt("MOPT_LM_PER_ITERATE", 1) != 0;  // 0: moments at every point (round 5)
  return mopt::choice::residentPerIterate(c->model == kModelPoint2Point, c->variant, jac_mode, enabled);
}

int residentGrid(const mopt_cost *c, int jac_mode) {
  switch (c->model) {
    case kModelPoint2Point:
      return gridFor(c, blocksPerCu(usesMoments(c, jac_mode) ? 1 : 2));
    case kModelReprojection:
      return gridFor(c, blocksPerCu(2));
    case kModelScalar:
      return scalarGrid(c);
    case kModelJit:
      return jitGrid(c);
    default:
      return 1;
  }
}

int residentDenseRow(const mopt_cost *c, int jac_mode) {
  switch (c->model) {
    case kModelPoint2Point:
      if (usesMoments(c, jac_mode)) return 0;  // rows of moments, contracted by their own finalize kernel
      return mopt::denseRowLength(c->cov_mode);
    case kModelReprojection:
      return mopt::denseRowLength(c->cov_mode);
    case kModelJit:
      return jitDenseRow(c);
    case kModelScalar:
      return mopt::denseRowLength(c->n_params, c->cov_mode);
    default:
      return 0;
  }
}

int residentPrepare(mopt_cost *c, int jac_mode, hipStream_t s, mopt::LmCostDesc *desc,
                    double *partials_override) {
  double *const partials = partials_override ? partials_override : c->d_partials;
  if (jac_mode < MOPT_JAC_ANALYTIC || jac_mode > MOPT_JAC_ANALYTIC_RIGHT)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown jacobian_mode");
  desc->jac_mode = jac_mode;
  desc->n_out = c->n_out;
  desc->moments = 0;
  desc->result = c->d_result;
  int rc = MOPT_OK;
  const bool stale = c->lm_uploaded_version != c->state_version ||
                     c->lm_uploaded_mode != jac_mode || c->lm_uploaded_partials != partials ||
                     !c->d_lm_args;
  switch (c->model) {
    case kModelPoint2Point: {
      desc->model = mopt::kLmPoint2Point;
      desc->moments = usesMoments(c, jac_mode) ? 1 : 0;
      if (stale)
        rc = withScalar(c->scalar_bytes, [&](auto scalar) {
          return residentPrepareP2P<typename decltype(scalar)::type>(c, jac_mode, desc->moments, partials, s);
        });
      break;
    }
    case kModelReprojection: {
      if (jac_mode != MOPT_JAC_NUMERIC)
        return fail(MOPT_ERR_UNSUPPORTED,
                    "the reprojection model has no analytic Jacobian (BaseModel, numeric only)");
      desc->model = mopt::kLmReprojection;
      std::memcpy(desc->camera, c->camera, sizeof desc->camera);
      std::memcpy(desc->frame, c->frame, sizeof desc->frame);
      if (stale) {
        mopt::ReprojSweepArgs args;
        const double zero[kNumParams] = {0, 0, 0, 0, 0, 0};
        fillReprojArgs(c, zero, false, args);
        args.partials = partials;
        rc = uploadArgs(c, args, s);
      }
      break;
    }
    case kModelScalar: {
      rc = checkModelJacobian(c, jac_mode);
      if (rc != MOPT_OK) return rc;
      desc->model = mopt::kLmScalar;
      rc = withScalar(c->scalar_bytes, [&](auto scalar) {
        using S = typename decltype(scalar)::type;
        return residentPrepareModel<mopt::ScalarSweepArgs<S>>(c, fillScalarArgs<S>, stale, partials, s, desc);
      });
      break;
    }
    case kModelJit: {
      rc = checkModelJacobian(c, jac_mode);
      if (rc != MOPT_OK) return rc;
      // compile (first use) before anything is queued: a source error must surface here
      if (!mopt::jitVariant(c->jit, jac_mode == MOPT_JAC_NUMERIC ? 2 : 1, c->cov_mode))
        return fail(MOPT_ERR_INVALID_ARGUMENT, mopt::jitLastError());
      desc->model = mopt::kLmJit;
      rc = withScalar(c->scalar_bytes, [&](auto scalar) {
        using S = typename decltype(scalar)::type;
        if (c->jit.wide)  // x[16] | h[16] in the wide sweep's argument block
          return residentPrepareModel<mopt::JitWideArgs<S>>(c, fillJitWideArgs<S>, stale, partials, s, desc);
        return residentPrepareModel<mopt::JitArgs<S>>(c, fillJitArgs<S>, stale, partials, s, desc);
      });
      break;
    }
    default:
      return fail(MOPT_ERR_UNSUPPORTED, "mopt_lm_minimize: unknown model kind");
  }
  if (rc != MOPT_OK) return rc;
  c->lm_uploaded_version = c->state_version;
  c->lm_uploaded_mode = jac_mode;
  c->lm_uploaded_partials = partials;
  desc->args = c->d_lm_args;
  desc->basis = c->d_lm_basis;
  return MOPT_OK;
}

int residentFinalizeMerged(mopt_cost *last, int rows, int row_length, mopt::LmControl *control,
                           hipStream_t s, const mopt::LmProblem *step, int own_index) {
  MOPT_HIP_TRY(mopt::launchFinalizeDenseResident(last->d_partials, rows, row_length, last->n_params,
                                                 last->d_result, control, s, nullptr, step,
                                                 own_index, last->scalar_bytes));
  return MOPT_OK;
}

// Can the resident sweeps of these costs (whose rows already lie behind one another: `merged` in
// lm.cpp) go out as ONE launch?  They must run the same kernel: same model kind, scalar type,
// Jacobian mode and covariance form — and for run-time compiled models the same source.
bool residentSetSupported(mopt_cost *const *costs, int num_costs, const int *jac_modes) {
  if (num_costs < 2) return false;
  const mopt_cost *first = costs[0];
  for (int k = 0; k < num_costs; ++k) {
    const mopt_cost *c = costs[k];
    if (c->model != first->model || c->cov_mode != first->cov_mode ||
        c->scalar_bytes != first->scalar_bytes || jac_modes[k] != jac_modes[0] || c->matcher)
      return false;
    switch (c->model) {
      case kModelReprojection:
        break;
      case kModelPoint2Point:
        if (usesMoments(c, jac_modes[k])) return false;  // rows of moments: one finalize per cost anyway
        break;
      case kModelScalar:
        if (c->scalar_model != first->scalar_model) return false;
        break;
      case kModelJit:
        // the shape reaches the compiler as -D options, not as source text: two costs with the same
        // bodies and another m, plane or aux count are different kernels
        if (c->jit.wide || c->jit.source != first->jit.source ||
            c->jit.n_params != first->jit.n_params || c->jit.n_outputs != first->jit.n_outputs ||
            c->jit.n_planes != first->jit.n_planes || c->jit.n_aux != first->jit.n_aux)
          return false;
        break;
      default:
        return false;
    }
  }
  return true;
}

int residentSweepSet(mopt_cost *const *costs, int num_costs, const int *jac_modes,
                     const int *first_row, mopt::LmControl *control, hipStream_t s) {
  mopt::ResidentSweepSet set;
  set.num_costs = num_costs;
  size_t bytes = 0;
  for (int k = 0; k < num_costs; ++k) {
    set.args[k] = costs[k]->d_lm_args;
    set.first_block[k] = first_row[k];
    // bytes the launch streams: 40 per reprojection element, 6 scalars per correspondence
    bytes += costs[k]->model == kModelReprojection
                 ? size_t(costs[k]->count) * 40
                 : size_t(costs[k]->count) * 6 * size_t(costs[k]->scalar_bytes);
  }
  set.first_block[num_costs] = first_row[num_costs];
  mopt::LaunchSite site;
  site.stream = s;
  site.streaming = bytes > (size_t(32) << 20);
  mopt_cost *first = costs[0];
  const int jac_mode = jac_modes[0];
  switch (first->model) {
    case kModelReprojection:
      MOPT_HIP_TRY(mopt::launchReprojResidentSet(set, control, first->cov_mode, site));
      return MOPT_OK;
    case kModelPoint2Point:
      MOPT_HIP_TRY(withScalar(first->scalar_bytes, [&](auto scalar) {
        return mopt::launchP2PLiteralResidentSet<typename decltype(scalar)::type>(set, control, jac_mode,
                                                                                  first->cov_mode, site);
      }));
      return MOPT_OK;
    case kModelScalar:
      MOPT_HIP_TRY(withScalar(first->scalar_bytes, [&](auto scalar) {
        return mopt::launchScalarModelResidentSet<typename decltype(scalar)::type>(
            set, control, first->scalar_model, jac_mode, first->cov_mode, s);
      }));
      return MOPT_OK;
    case kModelJit: {
      const mopt::JitVariant *variant =
          mopt::jitVariant(first->jit, jac_mode == MOPT_JAC_NUMERIC ? 2 : 1, first->cov_mode);
      if (!variant) return fail(MOPT_ERR_INVALID_ARGUMENT, mopt::jitLastError());
      MOPT_HIP_TRY(mopt::jitLaunchResidentSet(*variant, set, control, s));
      return MOPT_OK;
    }
    default:
      return fail(MOPT_ERR_UNSUPPORTED, "no one-launch resident sweep for this model");
  }
}

template <typename S>
static int residentSweepFor(mopt_cost *c, int jac_mode, mopt::LmControl *control, hipStream_t s,
                     unsigned long long base_sequence, const mopt::LmProblem *step, int own_index,
                     bool finalize) {
  mopt::PeerCombine pc;
  const mopt::PeerCombine *peers = nullptr;
  if (c->combine.mode == MOPT_COMBINE_PEER) {
    // unlike a blocking sweep's (nextPeerCombine) the sequence is not advanced here: the device adds
    // control->trial to base_sequence, and lm.cpp moves the cost's counter on after the solve
    pc = peerCombineAt(c->combine, 0, base_sequence);
    peers = &pc;
  }
  mopt::LaunchSite site;
  site.stream = s;
  const size_t bytes = size_t(c->count) * 6 * size_t(c->scalar_bytes);
  site.streaming = bytes > (size_t(32) << 20);
  if (c->matcher) {
    // the model's update(x): re-search the correspondences at the point the step kernel has just
    // proposed, when it says so (a linearization point), before that point is swept
    mopt::IcpMatchArgs<S> a;
    fillIcpArgs<S>(c, a);
    MOPT_HIP_TRY(mopt::launchIcpMatchResident<S>(
        a, static_cast<const mopt::P2PSweepArgs<S> *>(c->d_lm_args), control, s));
  }
  // Each case launches its sweep and names the n of its dense rows; their one finalize kernel follows
  // the switch.  The two point2point forms with rows of moments bring their own and return.
  const int grid = residentGrid(c, jac_mode);
  int n = c->n_params;
  switch (c->model) {
    case kModelPoint2Point: {
      const S *tiles = static_cast<const S *>(c->d_tiles);
      const mopt::P2PSweepArgs<S> *d_args = static_cast<const mopt::P2PSweepArgs<S> *>(c->d_lm_args);
      if (residentPerIterate(c, jac_mode)) {
        // one sweep launch that holds both forward-difference forms and runs the one the step kernel named
        // for this point (sweep.hpp kLmGateMoments), and one finalize kernel that reads which it was
        const int grid_l = gridFor(c, blocksPerCu(2));
        // the moments form over the first half of the launch's workgroups (one per CU, as the single-purpose
        // moments sweep runs; the rest leave at once) or over all of them: MOPT_LM_EITHER_MOMENTS_BLOCKS = 1 /
        // 2 — measured 82.8-83.5 against 84.8-85.7 us per sweep at 10 M, 18.7 against 21.2 at 1 M
        static const int moments_blocks = envInt("MOPT_LM_EITHER_MOMENTS_BLOCKS", 1);
        const int grid_m = moments_blocks >= 2 ? grid_l : std::min(grid_l, grid);
        const int nacc = mopt::denseRowLength(c->cov_mode);
        MOPT_HIP_TRY(mopt::launchForwardDiffEitherResident<S>(tiles, c->num_tiles, d_args, control,
                                                              c->cov_mode, grid_l, grid_m, site));
        if (finalize)
          MOPT_HIP_TRY(mopt::launchFinalizeEitherResident(c->d_partials, grid_m, grid_l, nacc, c->d_lm_basis,
                                                          c->d_result, control, s, peers, step, own_index,
                                                          c->scalar_bytes));
        return MOPT_OK;
      }
      if (usesMoments(c, jac_mode)) {
        MOPT_HIP_TRY(mopt::launchP2PMomentsResident<S>(tiles, c->num_tiles, d_args, control, grid, site));
        if (finalize)
          MOPT_HIP_TRY(mopt::launchFinalizeMomentsResident(c->d_partials, grid, c->d_lm_basis,
                                                         c->d_result, control, s, peers, step,
                                                         own_index, c->scalar_bytes));
        return MOPT_OK;
      }
      MOPT_HIP_TRY(mopt::launchP2PLiteralResident<S>(d_args, control, jac_mode, c->cov_mode, grid, site));
      n = kNumParams;
      break;
    }
    case kModelReprojection:
      MOPT_HIP_TRY(mopt::launchReprojResident(
          static_cast<const mopt::ReprojSweepArgs *>(c->d_lm_args), control, c->cov_mode, grid, site));
      n = kNumParams;
      break;
    case kModelScalar:
      MOPT_HIP_TRY(mopt::launchScalarModelResident<S>(
          static_cast<const mopt::ScalarSweepArgs<S> *>(c->d_lm_args), control, c->scalar_model,
          jac_mode, c->cov_mode, grid, s));
      break;
    case kModelJit: {
      const mopt::JitVariant *variant =
          mopt::jitVariant(c->jit, jac_mode == MOPT_JAC_NUMERIC ? 2 : 1, c->cov_mode);
      if (!variant) return fail(MOPT_ERR_INVALID_ARGUMENT, mopt::jitLastError());
      MOPT_HIP_TRY(mopt::jitLaunchResident(*variant, c->d_lm_args, control, grid, s));
      break;
    }
    default:
      return fail(MOPT_ERR_UNSUPPORTED, "no resident sweep for this model");
  }
  if (finalize)
    MOPT_HIP_TRY(mopt::launchFinalizeDenseResident(c->d_partials, grid, residentDenseRow(c, jac_mode), n,
                                                   c->d_result, control, s, peers, step, own_index,
                                                   c->scalar_bytes));
  return MOPT_OK;
}

int residentSweep(mopt_cost *c, int jac_mode, mopt::LmControl *control, hipStream_t s,
                  unsigned long long base_sequence, const mopt::LmProblem *step, int own_index,
                  bool finalize) {
  return withScalar(c->scalar_bytes, [&](auto scalar) {
    return residentSweepFor<typename decltype(scalar)::type>(c, jac_mode, control, s, base_sequence,
                                                             step, own_index, finalize);
  });
}

void releaseResident(mopt_cost *c) {
  deviceRelease(c->d_lm_args);
  deviceRelease(c->d_lm_basis);
  deviceRelease(c->d_lm_control);
  deviceRelease(c->d_lm_state);
  c->d_lm_args = nullptr;
  c->d_lm_basis = nullptr;
  c->d_lm_control = nullptr;
  c->d_lm_state = nullptr;
  if (c->h_lm_report) (void)hipHostFree(c->h_lm_report);
  c->h_lm_report = c->h_lm_report_dev = nullptr;
}

}  // namespace mopt_detail
