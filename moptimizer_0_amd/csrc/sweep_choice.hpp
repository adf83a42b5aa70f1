// The rules that choose which sweep runs and how large it is launched, as functions of plain values:
// the blocking calls (sweep_launch.cpp, blocking.cpp) and the device-resident loop (resident.cpp) call
// them with a cost's fields, tests/cpp/host_logic.cpp with literals.  Host arithmetic only — no HIP
// header, no project header but the C ABI's constants; forwardStepThreshold alone is also device code
// (the step kernel of lm_device.hpp applies the same rule).
#pragma once

#include "moptimizer_hip.h"

#include <cmath>

namespace mopt {

// Below which |x_j| forward differences are evaluated literally: 0.08 where the warped cloud lies
// within rho = 30 of the origin (where it was measured), growing with rho = (bound of |p| stored when
// the data was laid out) + |t| beyond — the reference's noise is eps rho / h_j (derivation at
// choice::hasSmallForwardStep).  One rule for the blocking calls and the step kernel.
#if defined(__HIPCC__) || defined(__CUDACC__)
__host__ __device__
#endif
inline double forwardStepThreshold(double rho) {
  const double scale = rho * (1.0 / 30.0);
  return 0.08 * (scale > 1.0 ? scale : 1.0);
}

namespace choice {

// AUTO's choice for forward differences.  The moments sweep forms column j of J as
// ((R_j - R) p + (t_j - t)) / h_j — the reference's quotient without its per-point cancellation
// error eps |R p + t| / h_j.  With h_j = sqrt(eps) |x_j| (linearization.h:85) that error is part of
// what the reference computes once |x_j| is small: measured distance between the two evaluations
// 2e-8 / |x_j| (tests/tools/parity_table.py; the literal sweep matches the reference to 1e-14 at every
// step size).  So below |x_j| = 0.08, where 4 x that measurement would pass the 1e-6 bar, AUTO
// evaluates literally; x_j = 0 takes the fixed step sqrt(eps) and is fine.
// That measurement was taken on clouds with rho = |R p + t| = 10..30.  The distance is the
// reference's cancellation noise eps rho / h_j, linear in rho: the threshold is 0.08 rho / 30 beyond
// rho = 30 and stays 0.08 below (mopt::forwardStepThreshold), with rho = (the bound of |p| stored when
// the data was laid out) + |t|, a bound of |R p + t| that costs nothing per call.  At a large rho the
// fixed step of x_j = 0 is no longer fine either: sqrt(eps) is the step of |x_j| = 1 and is judged
// as that.  Same rule in the step kernel of the device-resident loop (lm_device.hpp).
inline bool hasSmallForwardStep(double src_bound, const double x[6]) {
  const double t_norm = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double threshold = forwardStepThreshold(src_bound + t_norm);
  for (int j = 0; j < 6; ++j) {
    const double a = std::fabs(x[j]);
    if ((a > 0.0 ? a : 1.0) < threshold) return true;
  }
  return false;
}

// AUTO's and MOMENTS' choice for the analytic modes: the moments, except where the left-perturbation
// Jacobian [I | -skew(R p + t)] would cancel.  Its affine basis about p = 0 is J0 = -skew(t),
// J_k = -skew(R e_k): where the pose brings a far source near the origin (a map-frame scan registered
// to a local target, t ~ -R c) terms of N |t|^2 cancel down to N |R p + t|^2 and H keeps
// eps |t|^2 / |R p + t|^2 of error (profiles/NOTES.md "Scene scale").  Literal, per point, when
// |t|^2 > 1e3 rho_w^2, rho_w = |R c0 + t| + r bounding |R p + t| from the sources' stored bounding
// sphere (c0, r): at most 1e3 eps = 2e-13 is then lost to the moments.  MOMENTS_ALWAYS keeps the
// moments to measure.
inline bool leftBasisCancels(const double center[3], double radius, const double R[9], const double t[3]) {
  double w2 = 0.0, t2 = 0.0;
  for (int r = 0; r < 3; ++r) {
    const double w = R[r * 3] * center[0] + R[r * 3 + 1] * center[1] + R[r * 3 + 2] * center[2] + t[r];
    w2 += w * w;
    t2 += t[r] * t[r];
  }
  const double rho_w = std::sqrt(w2) + radius;
  return t2 > 1e3 * rho_w * rho_w;
}

// The device-resident loop chooses once per solve, for every pose it may reach: |t| <= |w| + |c0| with
// w = R c0 + t, so the rule above can only fire where |c0| > sqrt(1e3) r, whatever the pose.  Such a
// cost (a cloud far from the origin of its own frame) is swept literally throughout the solve; every
// other keeps the moments, and a small one the one-launch solve.
inline bool leftBasisMayCancel(const double center[3], double radius) {
  const double c2 = center[0] * center[0] + center[1] * center[1] + center[2] * center[2];
  return c2 > 1e3 * radius * radius;
}

// Resident sweeps: rows of moments, except under MOPT_KERNEL_LITERAL.  Forward differences under AUTO /
// MOMENTS are the one case where that is not the whole answer: where some 0 < |x_j| < 0.08 the blocking
// calls evaluate literally (hasSmallForwardStep), and so does the device-resident loop, point by point —
// such a cost is swept by a kernel that holds both forms and the step kernel names the one that runs
// (residentPerIterate, sweep.hpp kLmGateMoments).  Literal forward differences at EVERY iterate were measured
// in round 5 at 21.5 against 17.9 us per evaluated point at 1 M, 101.6 against 84.4 at 10 M; the choice per
// point pays that only at the points that need it (and 0.6-2 us per point for the kernels that hold both
// forms: profiles/r6_device_loop_choice.txt).
// ... and the left-perturbation Jacobian of a cloud far from its frame's origin, which some pose of
// the solve may map near the origin (`left_may_cancel` = leftBasisMayCancel: the device writes the same
// basis about p = 0, lm_device.hpp writeSweepConstants).
inline bool usesMoments(bool is_point2point, int variant, int jac_mode, bool left_may_cancel) {
  if (variant == MOPT_KERNEL_LITERAL) return false;
  if (variant == MOPT_KERNEL_MOMENTS_ALWAYS || !is_point2point) return true;
  return !(jac_mode == MOPT_JAC_ANALYTIC_LEFT && left_may_cancel);
}

// point2point forward differences under AUTO / MOMENTS: moments or literal, chosen per evaluated point
// (`enabled`: MOPT_LM_PER_ITERATE, 0 = moments at every point as in round 5)
inline bool residentPerIterate(bool is_point2point, int variant, int jac_mode, bool enabled) {
  return enabled && is_point2point && jac_mode == MOPT_JAC_NUMERIC &&
         (variant == MOPT_KERNEL_AUTO || variant == MOPT_KERNEL_MOMENTS);
}

// Is a linearization sweep in place of a cost sweep (mopt_cost_compute's speculation) still worth it?
// Always where it costs nothing more (`is_free`); elsewhere until two kept results have gone unused and
// more have gone unused than were used.
inline bool speculationPays(bool is_free, int unused, int used) {
  return is_free || unused < 2 || unused <= used;
}

// workgroups of a tiled sweep: blocks_per_cu per CU, at most one per tile and max_grid (the rows of the
// partial buffer), at least one
inline int gridFor(int num_cus, int blocks_per_cu, int num_tiles, int max_grid) {
  long long g = (long long)num_cus * blocks_per_cu;
  if (g > num_tiles) g = num_tiles;
  if (g > max_grid) g = max_grid;
  if (g < 1) g = 1;
  return int(g);
}

}  // namespace choice
}  // namespace mopt
