// gfx950 (CDNA4, MI355X) kernels of the per-residual linearization sweep.
//
// What is computed follows /root/reference/include/moptimizer/linearization.h:
//   for every index i:  r_i, J_i  ->  w_i = loss(|r_i|^2)
//                       H += w_i J_i^T S J_i ;  b += w_i J_i^T S r_i ;  sum += r_i^T r_i
// (:101-117 forward-difference form, :143-154 analytic form, :36-47 cost only), with the
// point-to-point model of tst/point2point.cpp:32-78 and the reprojection model of
// tst/camera_calibration.cpp:35-41 built in as device code in place of the per-point virtual
// calls.  How it is computed is laid out for the hardware:
//
//   * HBM-bound streaming reduction (48 B in, O(1) out per correspondence): no MFMA, no LDS
//     staging of inputs — every lane issues 16-byte loads straight to VGPRs, six per tile, all
//     six landing in one contiguous 24 KiB tile (layout in sweep.hpp), with the next tile's loads
//     issued before the current tile's arithmetic so each wave keeps 2 x 96 B per lane in flight.
//   * 64-wide wavefronts: per-thread register accumulators -> one LDS transpose per workgroup
//     (every lane stores each value once, 32 x 8 threads add them up, three xor-shuffles finish;
//     blockReduceStore) -> one partial row per workgroup in HBM.
//   * A fixed grid (workgroups per CU x CUs) strides over tiles, so the summation tree — and
//     therefore the result — is deterministic for a given device and count.
//   * A second tiny kernel adds the workgroup partials in a fixed order and writes
//     H (column-major) | b | sum_sq; no atomics anywhere.
#include "sweep_device.hpp"

namespace mopt {
namespace {

// Which entries of a model's Jacobian are the literal zero, whatever the data: products with them
// add nothing to any sum (for finite data not even in the last bit), so the accumulation below
// leaves them out — the point-to-point patterns are half zeros, and an H entry none of whose terms
// survives is never touched.  (A product with a literal 1 the compiler folds by itself; x * 0 it may
// not.)
struct DensePattern {
  static constexpr bool zero(int, int) { return false; }
};
template <int JAC>
struct P2PJacobianPattern {
  static constexpr bool zero(int a, int j) {
    if (JAC == kJacAnalyticTst) {
      // {1,0,0,0,1,0}, {0,0,1,0,-z,y}, {z,0,-x,-y,x,0}  (tst/point2point.cpp:71-75 read row-major)
      return (a == 0 && (j == 1 || j == 2 || j == 3 || j == 5)) ||
             (a == 1 && (j == 0 || j == 1 || j == 3)) || (a == 2 && (j == 1 || j == 5));
    }
    if (j < 3) return a != j;                   // [ I3 | . ]
    if (JAC == kJacAnalyticRight) return false;  // -R skew(p): dense
    return a == j - 3;                           // -skew(.): zero diagonal
  }
};

// acc += w J^T S J (upper triangle, or all n*n entries when S is not symmetric), w J^T S r, r^T r.
// J is m x n (row index = output), cov row-major m x m.  NACC selects the n*n form.  In fp64 every
// sum is a chain of fused multiply-adds straight into its accumulator.
// `Acc`: double, or float where the caller adds the points of a pack in fp32 first and promotes
// their sum (the fp32 point-to-point sweep: a conversion and an fp64 add per entry and point
// otherwise).
template <typename S, int M, int N, int COV, typename Pattern = DensePattern, typename Acc, int NACC>
__device__ __forceinline__ void accumulateDense(const S (&J)[M][N], const S (&r)[M], S w, S rr,
                                                const S *cov, Acc (&acc)[NACC]) {
  S SJ[M][N];
  S Sr[M];
  if (COV == kCovIdentity) {
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
      for (int j = 0; j < N; ++j) SJ[a][j] = J[a][j];
      Sr[a] = r[a];
    }
  } else {
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        S v = 0;
#pragma unroll
        for (int c = 0; c < M; ++c)
          if (!Pattern::zero(c, j)) v += cov[a * M + c] * J[c][j];
        SJ[a][j] = v;
      }
      S v = 0;
#pragma unroll
      for (int c = 0; c < M; ++c) v += cov[a * M + c] * r[c];
      Sr[a] = v;
    }
  }
  S wJ[M][N];
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int i = 0; i < N; ++i) wJ[a][i] = Pattern::zero(a, i) ? S(0) : w * J[a][i];

  constexpr bool kFull = (NACC == N * N + N + 1);
  constexpr int kNH = kFull ? N * N : N * (N + 1) / 2;
  static_assert(NACC == kNH + N + 1, "accumulator count does not match the matrix form");
  // (S J)(a, j) is structurally zero only under the identity covariance
  constexpr bool kDirect = sizeof(S) == 8 || sizeof(Acc) == 4;  // one FMA per term into acc
  auto term = [&](Acc &dst, S &partial, S x, S y) {
    if constexpr (sizeof(Acc) == 4)
      dst = __builtin_fmaf(x, y, dst);
    else if constexpr (sizeof(S) == 8)
      dst = __builtin_fma(double(x), double(y), dst);
    else
      partial += x * y;
  };
#pragma unroll
  for (int j = 0; j < N; ++j) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (!kFull && i > j) continue;
      const int k = kFull ? (j * N + i) : (j * (j + 1) / 2 + i);
      S partial = 0;
      bool any = false;
#pragma unroll
      for (int a = 0; a < M; ++a) {
        if (Pattern::zero(a, i) || (COV == kCovIdentity && Pattern::zero(a, j))) continue;
        term(acc[k], partial, wJ[a][i], SJ[a][j]);
        any = true;
      }
      if (!kDirect && any) acc[k] += double(partial);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    S partial = 0;
#pragma unroll
    for (int a = 0; a < M; ++a) {
      if (Pattern::zero(a, i)) continue;
      term(acc[kNH + i], partial, wJ[a][i], Sr[a]);
    }
    if (!kDirect) acc[kNH + i] += double(partial);
  }
  acc[kNH + N] += Acc(rr);
}

// ---- point-to-point, literal evaluation ------------------------------------------------------
template <typename S, int JAC, int COV, typename Acc>
__device__ __forceinline__ void p2pPointLiteral(
    const P2PSweepArgs<S> &A, const S (&p)[3], const S (&q)[3], bool valid,
    Acc (&acc)[(COV == kCovGeneral) ? kAccFull : kAccSym]) {
  S r[3];
  p2pResidual<S>(A.T[0], p, q, r);
  S J[3][6];
  if (JAC == kJacAnalytic) {
    // [ I3 | -skew(p) ], row-major (model.h:35-42)
    const S z = S(0), o = S(1);
    const S Ja[3][6] = {{o, z, z, z, p[2], -p[1]}, {z, o, z, -p[2], z, p[0]}, {z, z, o, p[1], -p[0], z}};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < 6; ++j) J[a][j] = Ja[a][j];
  } else if (JAC == kJacAnalyticTst) {
    // the same 18 numbers written column-major and read row-major (tst/point2point.cpp:71-75
    // against linearization.h:17-18)
    const S z = S(0), o = S(1);
    const S Jt[3][6] = {{o, z, z, z, o, z}, {z, z, o, z, -p[2], p[1]}, {p[2], z, -p[0], -p[1], p[0], z}};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < 6; ++j) J[a][j] = Jt[a][j];
  } else if (JAC == kJacAnalyticLeft) {
    // derivative with respect to a left perturbation of the pose: [ I3 | -skew(R p + t) ], with
    // R p + t = r + q (levenberg_marquadt_dyn.cpp:82-83 "TODO Manifold operation")
    const S z = S(0), o = S(1);
    const S w0 = r[0] + q[0], w1 = r[1] + q[1], w2 = r[2] + q[2];
    const S Jl[3][6] = {{o, z, z, z, w2, -w1}, {z, o, z, -w2, z, w0}, {z, z, o, w1, -w0, z}};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < 6; ++j) J[a][j] = Jl[a][j];
  } else if (JAC == kJacAnalyticRight) {
    // derivative with respect to R <- R Exp(phi), t <- t + rho (tst/manifold.cpp:47,
    // tst/state_model.cpp:28-34): [ I3 | -R skew(p) ]
    const S z = S(0), o = S(1);
    S Jr[3][6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const S R0 = A.T[0][a * 4 + 0], R1 = A.T[0][a * 4 + 1], R2 = A.T[0][a * 4 + 2];
      Jr[a][0] = a == 0 ? o : z;
      Jr[a][1] = a == 1 ? o : z;
      Jr[a][2] = a == 2 ? o : z;
      Jr[a][3] = -(R1 * p[2] - R2 * p[1]);
      Jr[a][4] = -(R2 * p[0] - R0 * p[2]);
      Jr[a][5] = -(R0 * p[1] - R1 * p[0]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < 6; ++j) J[a][j] = Jr[a][j];
  } else {
    // forward differences are p2pForwardDiffKernel's (7 transforms do not fit the scalar registers)
    static_assert(JAC != kJacNumeric, "forward differences: p2pForwardDiffKernel");
  }
  const S rr = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  const S w = lossWeight<S>(A.loss_kind, A.loss_param, rr);
  accumulateDense<S, 3, 6, COV, P2PJacobianPattern<JAC>>(J, r, valid ? w : S(0), valid ? rr : S(0),
                                                          A.cov, acc);
}

template <typename S, int JAC, int COV, bool STREAMING = false>
__device__ __forceinline__ void p2pLinearizeLiteralBody(const P2PSweepArgs<S> &A, int block,
                                                        int num_blocks) {
  constexpr int NACC = (COV == kCovGeneral) ? kAccFull : kAccSym;
  constexpr int V = TileShape<S>::kVec;
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;

  // fp32: the four points of a pack are added in fp32 and their sums promoted once per pack
  using Local = typename std::conditional<sizeof(S) == 8, double, float>::type;
  sweepTiles<S, STREAMING>(A.tiles, A.num_tiles, [&](const Pack<S>(&cur)[6], long long first) {
    Local loc[sizeof(S) == 8 ? 1 : NACC];
    if constexpr (sizeof(S) == 4) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) loc[k] = 0.0f;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const S p[3] = {cur[0].v[e], cur[1].v[e], cur[2].v[e]};
      const bool ok = isCorrespondence(first + e, A.count, cur[3].v[e]);
      const S q[3] = {ok ? cur[3].v[e] : S(0), ok ? cur[4].v[e] : S(0), ok ? cur[5].v[e] : S(0)};
      if constexpr (sizeof(S) == 8)
        p2pPointLiteral<S, JAC, COV>(A, p, q, ok, acc);
      else
        p2pPointLiteral<S, JAC, COV>(A, p, q, ok, loc);
    }
    if constexpr (sizeof(S) == 4) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) acc[k] += double(loc[k]);
    }
  }, block, num_blocks);
  blockReduceStore<NACC>(acc, A.partials + size_t(block) * NACC);
}

// (tiles / num_tiles repeat the first members of A as preloaded leading arguments, as in the moments
// sweep; STREAMING: non-temporal loads once the data exceed the aggregate L2)
template <typename S, int JAC, int COV, bool STREAMING>
__global__ __launch_bounds__(kBlockThreads) void p2pLinearizeLiteralKernel(
    const S *tiles, int num_tiles, const P2PSweepArgs<S> A) {
  P2PSweepArgs<S> B = A;
  B.tiles = tiles;
  B.num_tiles = num_tiles;
  p2pLinearizeLiteralBody<S, JAC, COV, STREAMING>(B, blockIdx.x, gridDim.x);
}

// Resident form (device-resident LM, sweep.hpp): the per-x constants come from HBM, where the
// step kernel of the previous trial left them; a kernel queued past the end of the minimisation
// finds control->done set and returns.
template <typename S, int JAC, int COV>
__global__ __launch_bounds__(kBlockThreads) void p2pLinearizeLiteralResidentKernel(
    const P2PSweepArgs<S> *__restrict__ d_args, const LmControl *__restrict__ control) {
  if (control->done) return;
  const P2PSweepArgs<S> A = *d_args;
  p2pLinearizeLiteralBody<S, JAC, COV>(A, blockIdx.x, gridDim.x);
}

// The sweeps of several literally evaluated point2point costs of one problem in one launch (as
// reprojResidentSetKernel below): the loop of levenberg_marquadt_dyn.cpp:48-60 pays one launch per
// evaluated point, not one per cost.
template <typename S, int JAC, int COV>
__global__ __launch_bounds__(kBlockThreads) void p2pLinearizeLiteralResidentSetKernel(
    const ResidentSweepSet set, const LmControl *__restrict__ control) {
  if (control->done) return;
  const int k = costOfBlock(set);
  const P2PSweepArgs<S> A = *static_cast<const P2PSweepArgs<S> *>(set.args[k]);
  p2pLinearizeLiteralBody<S, JAC, COV>(A, int(blockIdx.x) - set.first_block[k],
                                       set.first_block[k + 1] - set.first_block[k]);
}

// ---- point-to-point, weighted moments --------------------------------------------------------
// Every Jacobian this model produces is affine in the source point p (analytic: [I | -skew(p)];
// forward differences: ((R_j - R) p + (t_j - t)) / h_j), so
//   sum_i w_i J_i^T S J_i  and  sum_i w_i J_i^T S r_i
// are linear in the 22 moments  sum w, sum w p, sum w p p^T, sum w r, sum w p r^T.  The sweep
// accumulates those (plus sum r^T r); finalizeMomentsKernel contracts them with the basis.
// `tiles` / `num_tiles` repeat the first members of A as leading scalar arguments: gfx950 can
// preload those into SGPRs at wave launch (-amdgpu-kernarg-preload-count), so the first tile's
// loads go out without waiting for a kernel-argument fetch.
// (momentsOfPack — the moments of the V correspondences one lane holds of a tile — is in sweep_device.hpp:
// the forward-difference translation unit sweeps with it too)
template <typename S, bool STREAMING>
__device__ __forceinline__ void p2pMomentsBody(const S *tiles, int num_tiles,
                                               const P2PSweepArgs<S> &A) {
  double acc[kAccMoments];
#pragma unroll
  for (int k = 0; k < kAccMoments; ++k) acc[k] = 0.0;
  sweepTiles<S, STREAMING>(tiles, num_tiles, [&](const Pack<S>(&cur)[6], long long first) {
    momentsOfPack<S>(acc, cur, first, A);
  });
  blockReduceStore<kAccMoments>(acc, A.partials + size_t(blockIdx.x) * kAccMoments);
}

template <typename S, bool STREAMING>
__global__ __launch_bounds__(kBlockThreads) void p2pMomentsKernel(const S *tiles, int num_tiles,
                                                                  const P2PSweepArgs<S> A) {
  p2pMomentsBody<S, STREAMING>(tiles, num_tiles, A);
}

template <typename S, bool STREAMING>
__global__ __launch_bounds__(kBlockThreads) void p2pMomentsResidentKernel(
    const S *tiles, int num_tiles, const P2PSweepArgs<S> *__restrict__ d_args,
    const LmControl *__restrict__ control) {
  if (control->done) return;
  const P2PSweepArgs<S> A = *d_args;
  p2pMomentsBody<S, STREAMING>(tiles, num_tiles, A);
}

// ---- point-to-point, cost only (linearization.h:36-63) ----------------------------------------
template <typename S, bool STREAMING>
__global__ __launch_bounds__(kBlockThreads) void p2pCostKernel(const S *tiles, int num_tiles,
                                                               const P2PSweepArgs<S> A) {
  constexpr int V = TileShape<S>::kVec;
  double acc[1] = {0.0};
  sweepTiles<S, STREAMING>(tiles, num_tiles, [&](const Pack<S>(&cur)[6], long long first) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const S p[3] = {cur[0].v[e], cur[1].v[e], cur[2].v[e]};
      const bool valid = isCorrespondence(first + e, A.count, cur[3].v[e]);
      const S q[3] = {valid ? cur[3].v[e] : S(0), valid ? cur[4].v[e] : S(0),
                      valid ? cur[5].v[e] : S(0)};
      S r[3];
      p2pResidual<S>(A.T[0], p, q, r);
      const S rr = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
      acc[0] += valid ? double(rr) : 0.0;
    }
  });
  blockReduceStore<1>(acc, A.partials + blockIdx.x);
}

// ---- reprojection (camera calibration), fp64, forward differences ------------------------------
__device__ __forceinline__ void reprojResidual(const double (&Mx)[12], const double (&P)[4],
                                               double u, double v, double (&r)[2]) {
  // as written, no fused multiply-adds: the CPU restatement evaluates the same four products and
  // three sums, and forward differences amplify a last-bit difference of a residual by eps / h_j
#pragma clang fp contract(off)
  double o[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    o[a] = ((Mx[a * 4 + 0] * P[0] + Mx[a * 4 + 1] * P[1]) + Mx[a * 4 + 2] * P[2]) +
           Mx[a * 4 + 3] * P[3];
  r[0] = u - (o[0] / o[2]);  // tst/camera_calibration.cpp:38
  r[1] = v - (o[1] / o[2]);  // :39
}

// Seven 3x4 projections at x and x + h_j e_j are 84 fp64 constants: as kernel arguments they asked
// for 180 scalar registers against ~100, and every reproj* linearize kernel spilled 128-148 of them
// (v_readlane / v_writelane around each use; rounds 1-3).  As in fd_kernels.hip the six perturbed
// projections live in LDS: 72 lanes copy them once per workgroup from where the arguments lie in
// memory (`in_memory`: the kernel-argument segment, or the resident forms' block in HBM), and each is
// read (same-address reads: broadcasts) while the one before it is being used.  The projection at x,
// the step reciprocals, the covariance and the loss stay in scalar registers (~50).  The tile's loads
// are issued before that copy, so the two latencies overlap.  Per element the arithmetic is the
// reference's: seven residuals with both divisions each, twelve quotients (linearization.h:101-107),
// contraction off.
//
// One element per lane, 256 per tile: the arithmetic of an element is one long dependent chain
// (≈ 400 fp64 instructions, 14 divisions), so what a sweep of BASELINE config 5 costs is that chain
// once per workgroup — with two elements per lane (tiles of 512, rounds 1-3) it ran twice, or
// interleaved in > 300 registers; measured in one process (scripts/probes/reproj_stamps.cpp,
// profiles/r4_reproj_forms.txt): 4.8 us per 40 k / 60 k elements against 5.7 (interleaved) and 6.1
// (one after the other) where an empty launch of the same grid takes 4.2, and 134 against 138 and
// 151 us at 4 M elements.
// block / num_blocks: this workgroup's place among those sweeping this cost (a launch may carry
// the workgroups of several costs: reprojResidentSetKernel); the cost's partial rows are num_blocks.
template <int COV, bool COST_ONLY>
__device__ __forceinline__ void reprojBody(const ReprojSweepArgs &A, int block, int num_blocks,
                                           const ReprojSweepArgs &in_memory) {
  constexpr int NACC = COST_ONLY ? 1 : ((COV == kCovGeneral) ? kAccFull : kAccSym);
  MOPT_STAMP(0);
  __shared__ double Mlds[kNumParams][12];
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;

  struct Element {
    double P[4], u, v;
  };
  auto loadElement = [&](int tile) {
    const unsigned char *tb = A.tiles + size_t(tile) * kReprojTileBytes;
    const double *planes = reinterpret_cast<const double *>(tb) + threadIdx.x;
    const int2 px = reinterpret_cast<const int2 *>(tb + size_t(4) * kReprojTilePoints * 8)[threadIdx.x];
    Element el;
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) el.P[pl] = planes[pl * kReprojTilePoints];
    el.u = double(px.x);
    el.v = double(px.y);
    return el;
  };

  // this workgroup's tiles: block, block + num_blocks, ...; the next one is loaded before the
  // arithmetic of the current one (unconditionally — past the end the last one again, an L2 hit:
  // a conditional prefetch makes the compiler wait for everything at the join, sweep_device.hpp)
  int tile = block;
  const int last = tile < A.num_tiles ? tile + ((A.num_tiles - 1 - tile) / num_blocks) * num_blocks : tile;
  Element el{};
  if (tile < A.num_tiles) el = loadElement(tile);
  if constexpr (!COST_ONLY) {
    // the one access indexed by lane goes to memory, not to a by-value copy (which would put the
    // whole struct into every lane's scratch)
    if (threadIdx.x < kNumParams * 12) (&Mlds[0][0])[threadIdx.x] = (&in_memory.M[1][0])[threadIdx.x];
    __syncthreads();
  }
  MOPT_STAMP(1);
  // `robust`: the loss kind is taken out of the element (a branch inside splits the basic block, and
  // the compiler then sinks the seven residuals below it, behind the LDS reads of all six projections)
  auto sweep = [&](auto robust) {
    for (; tile < A.num_tiles; tile += num_blocks) {
      const bool valid = (long long)tile * kReprojTilePoints + threadIdx.x < A.count;
      const Element nx = loadElement(tile + num_blocks <= last ? tile + num_blocks : last);
      double r[2];
      reprojResidual(A.M[0], el.P, el.u, el.v, r);
      const double rr = r[0] * r[0] + r[1] * r[1];
      MOPT_STAMP(2);
      if constexpr (COST_ONLY) {
        acc[0] += valid ? rr : 0.0;
      } else {
        double J[2][6];
        // one perturbed projection after the other (all seven residuals interleaved need > 256
        // registers), each read from LDS while the one before it is being used
        double Mj[2][12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Mj[0][k] = Mlds[0][k];
#pragma unroll
        for (int j = 0; j < kNumParams; ++j) {
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("" ::: "memory");  // read here, not hoisted into 144 registers
          if (j + 1 < kNumParams) {
#pragma unroll
            for (int k = 0; k < 12; ++k) Mj[(j + 1) & 1][k] = Mlds[j + 1][k];
          }
          double rp[2];
          reprojResidual(Mj[j & 1], el.P, el.u, el.v, rp);
          J[0][j] = (rp[0] - r[0]) * A.inv_h[j];
          J[1][j] = (rp[1] - r[1]) * A.inv_h[j];
        }
        __builtin_amdgcn_sched_barrier(0);
        MOPT_STAMP(3);
        // padded slots repeat the last element (relayoutReprojKernel): finite, left out by w = 0 —
        // a branch around the accumulation lets the compiler sink all seven residuals into it, behind
        // the LDS reads of all six projections (144 registers)
        double w = 1.0;
        if constexpr (decltype(robust)::value) w = lossWeight<double>(kLossGemanMcClure, A.loss_param, rr);
        accumulateDense<double, 2, 6, COV>(J, r, valid ? w : 0.0, valid ? rr : 0.0, A.cov, acc);
      }
      MOPT_STAMP(4);
      el = nx;
    }
  };
  if (!COST_ONLY && A.loss_kind == kLossGemanMcClure)
    sweep(std::true_type());
  else
    sweep(std::false_type());
  MOPT_STAMP(5);
  blockReduceStore<NACC>(acc, A.partials + size_t(block) * NACC);
  MOPT_STAMP(6);
}

template <int COV, bool COST_ONLY>
__global__ __launch_bounds__(kBlockThreads) void reprojKernel(const ReprojSweepArgs A) {
  reprojBody<COV, COST_ONLY>(A, blockIdx.x, gridDim.x, A);
}

template <int COV>
__global__ __launch_bounds__(kBlockThreads) void reprojResidentKernel(
    const ReprojSweepArgs *__restrict__ d_args, const LmControl *__restrict__ control) {
  if (control->done) return;
  const ReprojSweepArgs A = *d_args;
  reprojBody<COV, false>(A, blockIdx.x, gridDim.x, *d_args);
}

// The sweeps of several reprojection costs of one problem in one launch (device-resident LM):
// workgroups [first_block[k], first_block[k + 1]) sweep cost k.  Each cost alone fills part of the
// chip, behind one another they would also pay a launch boundary each.
template <int COV>
__global__ __launch_bounds__(kBlockThreads) void reprojResidentSetKernel(
    const ResidentSweepSet set, const LmControl *__restrict__ control) {
  if (control->done) return;
  const int k = costOfBlock(set);
  const ReprojSweepArgs *d_args = static_cast<const ReprojSweepArgs *>(set.args[k]);
  const ReprojSweepArgs A = *d_args;
  reprojBody<COV, false>(A, int(blockIdx.x) - set.first_block[k],
                         set.first_block[k + 1] - set.first_block[k], *d_args);
}

// ---- small parametric models over per-element scalar data ------------------------------------
// The other models the reference's tests run through the same cost classes (n != 6):
//   ExpCurve   y - exp(x0 t + x1)            tst/curve_fitting.cpp:81-98, multiple_objectives.cpp:81-98
//   Rational   y - x0 t / (x1 + t)           tst/test_models.h:7-20; Jacobian tst/differentiation.cpp:26-38
//   Powell     Powell's singular function    tst/powell.cpp:21-60 (4 outputs, one element)
// Same skeleton: per-element residual, analytic or forward-difference Jacobian
// (linearization.h:101-117 / :143-154), loss weight, dense accumulation, workgroup partial row.
// accept() is what IBaseModel::f / f_df return (model.h:32,43): false = "this index is not a residual",
// and the sweep skips it (linearization.h:102,144).  The *Marked forms of the models over observations
// (t, y) say so for an observation whose y is NaN — the marker the point2point sweeps use for a source
// without a correspondence — and replace that y by a harmless one, so that everything computed for the
// skipped index stays finite and a weight of zero is enough to leave it out (one select on the way
// in, not one per residual and Jacobian entry).  The check costs 5 % of a sweep that is bound by its
// arithmetic (10 M elements: 40.3 against 38.4 us), so data without markers run the forms without it.
template <typename S>
__device__ __forceinline__ bool acceptUnlessMarked(S (&d)[2]) {
  const bool ok = d[1] == d[1];
  d[1] = ok ? d[1] : S(0);
  return ok;
}

template <typename S>
struct ExpCurve {
  static constexpr int N = 2, M = 1, D = 2;
  static constexpr bool kHasJacobian = false;
  __device__ static bool accept(S (&)[D]) { return true; }
  __device__ static void residual(const S *x, const S *d, S (&r)[M]) {
#pragma clang fp contract(off)  // as written: the checker's arithmetic (forward differences amplify an ulp)
    r[0] = d[1] - exp(x[0] * d[0] + x[1]);
  }
  __device__ static void jacobian(const S *, const S *, S (&)[M][N]) {}
};
template <typename S>
struct ExpCurveMarked : ExpCurve<S> {
  __device__ static bool accept(S (&d)[2]) { return acceptUnlessMarked<S>(d); }
};

template <typename S>
struct Rational {
  static constexpr int N = 2, M = 1, D = 2;
  static constexpr bool kHasJacobian = true;
  __device__ static bool accept(S (&)[D]) { return true; }
  __device__ static void residual(const S *x, const S *d, S (&r)[M]) {
#pragma clang fp contract(off)  // as written: the checker's arithmetic (forward differences amplify an ulp)
    r[0] = d[1] - (x[0] * d[0]) / (x[1] + d[0]);
  }
  __device__ static void jacobian(const S *x, const S *d, S (&J)[M][N]) {
    const S denominator = x[1] + d[0];
    J[0][0] = -d[0] / denominator;
    J[0][1] = (x[0] * d[0]) / (denominator * denominator);
  }
};
template <typename S>
struct RationalMarked : Rational<S> {
  __device__ static bool accept(S (&d)[2]) { return acceptUnlessMarked<S>(d); }
};

template <typename S>
struct Powell {
  static constexpr int N = 4, M = 4, D = 0;
  static constexpr bool kHasJacobian = true;
  __device__ static bool accept(S (&)[1]) { return true; }
  __device__ static void residual(const S *x, const S *, S (&r)[M]) {
#pragma clang fp contract(off)  // as written: the checker's arithmetic (forward differences amplify an ulp)
    r[0] = x[0] + 10 * x[1];
    r[1] = sqrt(S(5)) * (x[2] - x[3]);
    r[2] = (x[1] - 2 * x[2]) * (x[1] - 2 * x[2]);
    r[3] = sqrt(S(10)) * (x[0] - x[3]) * (x[0] - x[3]);
  }
  // exactly the entries the reference's test model writes (tst/powell.cpp:31-57), including its
  // (x1 + 2 x2) in rows 2 — the test's own Jacobian, not the textbook one
  __device__ static void jacobian(const S *x, const S *, S (&J)[M][N]) {
    const S s5 = sqrt(S(5)), s10 = sqrt(S(10));
    J[0][0] = 1;  J[1][0] = 0;   J[2][0] = 0;                              J[3][0] = s10 * 2 * (x[0] - x[3]);
    J[0][1] = 10; J[1][1] = 0;   J[2][1] = 2 * (x[1] + 2 * x[2]);          J[3][1] = 0;
    J[0][2] = 0;  J[1][2] = s5;  J[2][2] = 2 * (x[1] + 2 * x[2]) * (-2);   J[3][2] = 0;
    J[0][3] = 0;  J[1][3] = -s5; J[2][3] = 0;                              J[3][3] = s10 * 2 * (x[0] - x[3]) * (-1);
  }
};

// The skeleton of the tiled sweeps (and of the run-time compiled twin, jit_model.cpp): a lane takes
// the V = 16 / sizeof(S) consecutive elements of one 16-byte pack per data plane and step, the next
// step's packs are requested before this one's arithmetic starts, the loss kind is taken out of the
// element, products go into the sums as fused multiply-adds (accumulateDense).  Rounds 1-3 loaded
// 8 bytes per lane and plane in a plain grid-stride loop: 52 us for the forward-difference sweep of
// the exp curve over 10 M elements against 37 us for the same model compiled at run time.
template <typename S, template <typename> class ModelT, int JAC, int COV, bool COST_ONLY>
__device__ __forceinline__ void scalarModelBody(const ScalarSweepArgs<S> &A, int block,
                                                int num_blocks) {
  using Model = ModelT<S>;
  constexpr int N = Model::N, M = Model::M, D = Model::D;
  constexpr int V = TileShape<S>::kVec;
  constexpr bool kNumeric = JAC == kJacNumeric || !Model::kHasJacobian;
  constexpr int NACC =
      COST_ONLY ? 1 : ((COV == kCovGeneral) ? N * N + N + 1 : N * (N + 1) / 2 + N + 1);
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  // (r+ - r) / h_j (linearization.h:105) as a product with 1 / h_j formed once per sweep, like the
  // hand-written point2point sweeps: an fp64 division per Jacobian entry and element otherwise
  S inv_h[N];
#pragma unroll
  for (int j = 0; j < N; ++j) inv_h[j] = S(1) / A.h[j];
  // `robust`: the loss kind is a property of the sweep (a branch inside the element splits its basic
  // block and lets the compiler sink one element's accumulation below the next one's residuals)
  auto sweep = [&](auto robust) {
    auto element = [&](S (&d)[D > 0 ? D : 1], bool valid) {
      // an index the model rejects is skipped like a slot past the end: weight zero (its data made
      // harmless by accept())
      valid = Model::accept(d) && valid;
      S r[M];
      Model::residual(A.x, d, r);
      S rr = 0;
#pragma unroll
      for (int a = 0; a < M; ++a) rr += r[a] * r[a];
      rr = valid ? rr : S(0);
      if constexpr (COST_ONLY) {
        acc[0] += double(rr);
      } else {
        S J[M][N];
        if constexpr (kNumeric) {
#pragma unroll
          for (int j = 0; j < N; ++j) {
            S xp[N];
#pragma unroll
            for (int k = 0; k < N; ++k) xp[k] = A.x[k];
            xp[j] += A.h[j];  // linearization.h:89
            S rp[M];
            Model::residual(xp, d, rp);
#pragma unroll
            for (int a = 0; a < M; ++a) J[a][j] = (rp[a] - r[a]) * inv_h[j];  // :105
          }
        } else {
          Model::jacobian(A.x, d, J);
        }
        S w = S(1);
        if constexpr (decltype(robust)::value) w = lossWeight<S>(kLossGemanMcClure, A.loss_param, rr);
        accumulateDense<S, M, N, COV>(J, r, valid ? w : S(0), rr, A.cov, acc);
      }
    };
    const long long step = (long long)num_blocks * kBlockThreads * V;
    long long i = ((long long)block * kBlockThreads + threadIdx.x) * V;
    Pack<S> cur[D > 0 ? D : 1], nxt[D > 0 ? D : 1];
    // (a run-time choice between these and non-temporal loads — one uniform branch per pack — cost
    // 6 us of the 38 at 10 M elements, whichever way it went: profiles/r4_jit_timing.txt)
    auto load = [&](const S *from) { return loadPack<S>(from); };
    if (i < A.count) {
#pragma unroll
      for (int p = 0; p < D; ++p) nxt[p] = load(A.data + p * A.stride + i);
    }
    for (; i < A.count; i += step) {
#pragma unroll
      for (int p = 0; p < D; ++p) cur[p] = nxt[p];
      // the next step's packs are requested before this one's arithmetic starts (past the end: this
      // step's again — an unconditional load, see sweepTiles)
      const long long ahead = i + step < A.count ? i + step : i;
#pragma unroll
      for (int p = 0; p < D; ++p) nxt[p] = load(A.data + p * A.stride + ahead);
      // a slot past the end (the zero-padded tail of the last pack) is evaluated on the pack's first
      // element, which is in range, and enters every sum with weight zero
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if constexpr (kNumeric && !COST_ONLY) __builtin_amdgcn_sched_barrier(0);  // one element after the other
        const bool valid = i + e < A.count;
        S d[D > 0 ? D : 1];
#pragma unroll
        for (int p = 0; p < D; ++p) d[p] = valid ? cur[p].v[e] : cur[p].v[0];
        element(d, valid);
      }
      if constexpr (kNumeric && !COST_ONLY) __builtin_amdgcn_sched_barrier(0);
    }
  };
  if (!COST_ONLY && A.loss_kind == kLossGemanMcClure)
    sweep(std::true_type());
  else
    sweep(std::false_type());
  blockReduceStore<NACC>(acc, A.partials + size_t(block) * NACC);
}

template <typename S, template <typename> class ModelT, int JAC, int COV, bool COST_ONLY>
__global__ __launch_bounds__(kBlockThreads) void scalarModelKernel(const ScalarSweepArgs<S> A) {
  scalarModelBody<S, ModelT, JAC, COV, COST_ONLY>(A, blockIdx.x, gridDim.x);
}

template <typename S, template <typename> class ModelT, int JAC, int COV>
__global__ __launch_bounds__(kBlockThreads) void scalarModelResidentKernel(
    const ScalarSweepArgs<S> *__restrict__ d_args, const LmControl *__restrict__ control) {
  if (control->done) return;
  const ScalarSweepArgs<S> A = *d_args;
  scalarModelBody<S, ModelT, JAC, COV, false>(A, blockIdx.x, gridDim.x);
}

// several costs over the same built-in model in one launch (tst/multiple_objectives.cpp:102-132
// splits the curve fit's 67 observations over two costs)
template <typename S, template <typename> class ModelT, int JAC, int COV>
__global__ __launch_bounds__(kBlockThreads) void scalarModelResidentSetKernel(
    const ResidentSweepSet set, const LmControl *__restrict__ control) {
  if (control->done) return;
  const int k = costOfBlock(set);
  const ScalarSweepArgs<S> A = *static_cast<const ScalarSweepArgs<S> *>(set.args[k]);
  scalarModelBody<S, ModelT, JAC, COV, false>(A, int(blockIdx.x) - set.first_block[k],
                                              set.first_block[k + 1] - set.first_block[k]);
}

}  // namespace

// ---- host-side launch wrappers -----------------------------------------------------------------
template <typename S>
hipError_t launchP2PLinearizeLiteral(const P2PSweepArgs<S> &args, int jac_mode, int cov_mode,
                                     int grid, const LaunchSite &site) {
  if (jac_mode == kJacNumeric) return launchForwardDiff<S>(args, cov_mode, grid, site);
  return withP2PAnalyticJac(jac_mode, [&](auto jac) {
    return withCov(cov_mode, [&](auto cov) {
      return dispatch::byBool(site.streaming, [&](auto streaming) {
        return launchBlocking(p2pLinearizeLiteralKernel<S, jac(), cov(), streaming()>, grid, site,
                              args.tiles, args.num_tiles, args);
      });
    });
  });
}
template hipError_t launchP2PLinearizeLiteral<float>(const P2PSweepArgs<float> &, int, int, int,
                                                     const LaunchSite &);
template hipError_t launchP2PLinearizeLiteral<double>(const P2PSweepArgs<double> &, int, int, int,
                                                      const LaunchSite &);

template <typename S>
hipError_t launchP2PMoments(const P2PSweepArgs<S> &args, int grid, const LaunchSite &site) {
  return dispatch::byBool(site.streaming, [&](auto streaming) {
    return launchBlocking(p2pMomentsKernel<S, streaming()>, grid, site, args.tiles, args.num_tiles, args);
  });
}
template hipError_t launchP2PMoments<float>(const P2PSweepArgs<float> &, int, const LaunchSite &);
template hipError_t launchP2PMoments<double>(const P2PSweepArgs<double> &, int,
                                             const LaunchSite &);

template <typename S>
hipError_t launchP2PCost(const P2PSweepArgs<S> &args, int grid, const LaunchSite &site) {
  return dispatch::byBool(site.streaming, [&](auto streaming) {
    return launchBlocking(p2pCostKernel<S, streaming()>, grid, site, args.tiles, args.num_tiles, args);
  });
}
template hipError_t launchP2PCost<float>(const P2PSweepArgs<float> &, int, const LaunchSite &);
template hipError_t launchP2PCost<double>(const P2PSweepArgs<double> &, int, const LaunchSite &);

hipError_t launchReprojLinearize(const ReprojSweepArgs &args, int cov_mode, int grid,
                                 const LaunchSite &site) {
  return withCov(cov_mode, [&](auto cov) {
    return launchBlocking(reprojKernel<cov(), false>, grid, site, args);
  });
}

hipError_t launchReprojCost(const ReprojSweepArgs &args, int grid, const LaunchSite &site) {
  return launchBlocking(reprojKernel<kCovIdentity, true>, grid, site, args);
}

namespace {
template <typename S, template <typename> class ModelT>
hipError_t launchScalarFor(ScalarModel<ModelT>, const ScalarSweepArgs<S> &args, bool cost_only,
                           int jac_mode, int cov_mode, int grid, const LaunchSite &site) {
  if (cost_only)
    return launchBlocking(scalarModelKernel<S, ModelT, kJacNumeric, kCovIdentity, true>, grid, site, args);
  return withCov(cov_mode, [&](auto cov) {
    return withModelJac(jac_mode, [&](auto jac) {
      return launchBlocking(scalarModelKernel<S, ModelT, jac(), cov(), false>, grid, site, args);
    });
  });
}
}  // namespace

template <typename S>
hipError_t launchScalarModel(const ScalarSweepArgs<S> &args, int model, bool cost_only,
                             int jac_mode, int cov_mode, int grid, const LaunchSite &site) {
  return withScalarModel(model, [&](auto kind) {
    return launchScalarFor<S>(kind, args, cost_only, jac_mode, cov_mode, grid, site);
  });
}
template hipError_t launchScalarModel<float>(const ScalarSweepArgs<float> &, int, bool, int, int,
                                             int, const LaunchSite &);
template hipError_t launchScalarModel<double>(const ScalarSweepArgs<double> &, int, bool, int, int,
                                              int, const LaunchSite &);

// ---- resident forms (device-resident LM) ---------------------------------------------------------
template <typename S>
hipError_t launchP2PMomentsResident(const S *tiles, int num_tiles, const P2PSweepArgs<S> *d_args,
                                    const LmControl *control, int grid, const LaunchSite &site) {
  return dispatch::byBool(site.streaming, [&](auto streaming) {
    return launchResident(p2pMomentsResidentKernel<S, streaming()>, grid, site.stream, tiles, num_tiles,
                          d_args, control);
  });
}
template hipError_t launchP2PMomentsResident<float>(const float *, int, const P2PSweepArgs<float> *,
                                                    const LmControl *, int, const LaunchSite &);
template hipError_t launchP2PMomentsResident<double>(const double *, int,
                                                     const P2PSweepArgs<double> *,
                                                     const LmControl *, int, const LaunchSite &);

template <typename S>
hipError_t launchP2PLiteralResident(const P2PSweepArgs<S> *d_args, const LmControl *control,
                                    int jac_mode, int cov_mode, int grid, const LaunchSite &site) {
  if (jac_mode == kJacNumeric)
    return launchForwardDiffResident<S>(d_args, control, cov_mode, grid, site);
  return withP2PAnalyticJac(jac_mode, [&](auto jac) {
    return withCov(cov_mode, [&](auto cov) {
      return launchResident(p2pLinearizeLiteralResidentKernel<S, jac(), cov()>, grid, site.stream,
                            d_args, control);
    });
  });
}
template hipError_t launchP2PLiteralResident<float>(const P2PSweepArgs<float> *, const LmControl *,
                                                    int, int, int, const LaunchSite &);
template hipError_t launchP2PLiteralResident<double>(const P2PSweepArgs<double> *,
                                                     const LmControl *, int, int, int,
                                                     const LaunchSite &);

template <typename S>
hipError_t launchP2PLiteralResidentSet(const ResidentSweepSet &set, const LmControl *control,
                                       int jac_mode, int cov_mode, const LaunchSite &site) {
  if (jac_mode == kJacNumeric) return launchForwardDiffResidentSet<S>(set, control, cov_mode, site);
  return withP2PAnalyticJac(jac_mode, [&](auto jac) {
    return withCov(cov_mode, [&](auto cov) {
      return launchResident(p2pLinearizeLiteralResidentSetKernel<S, jac(), cov()>,
                            set.first_block[set.num_costs], site.stream, set, control);
    });
  });
}
template hipError_t launchP2PLiteralResidentSet<float>(const ResidentSweepSet &, const LmControl *,
                                                       int, int, const LaunchSite &);
template hipError_t launchP2PLiteralResidentSet<double>(const ResidentSweepSet &, const LmControl *,
                                                        int, int, const LaunchSite &);

hipError_t launchReprojResident(const ReprojSweepArgs *d_args, const LmControl *control,
                                int cov_mode, int grid, const LaunchSite &site) {
  return withCov(cov_mode, [&](auto cov) {
    return launchResident(reprojResidentKernel<cov()>, grid, site.stream, d_args, control);
  });
}

hipError_t launchReprojResidentSet(const ResidentSweepSet &set, const LmControl *control,
                                   int cov_mode, const LaunchSite &site) {
  return withCov(cov_mode, [&](auto cov) {
    return launchResident(reprojResidentSetKernel<cov()>, set.first_block[set.num_costs], site.stream,
                          set, control);
  });
}

namespace {
template <typename S, template <typename> class ModelT>
hipError_t launchScalarResidentFor(ScalarModel<ModelT>, const ScalarSweepArgs<S> *d_args,
                                   const LmControl *control, int jac_mode, int cov_mode, int grid,
                                   hipStream_t stream) {
  return withCov(cov_mode, [&](auto cov) {
    return withModelJac(jac_mode, [&](auto jac) {
      return launchResident(scalarModelResidentKernel<S, ModelT, jac(), cov()>, grid, stream, d_args,
                            control);
    });
  });
}

template <typename S, template <typename> class ModelT>
hipError_t launchScalarResidentSetFor(ScalarModel<ModelT>, const ResidentSweepSet &set,
                                      const LmControl *control, int jac_mode, int cov_mode,
                                      hipStream_t stream) {
  return withCov(cov_mode, [&](auto cov) {
    return withModelJac(jac_mode, [&](auto jac) {
      return launchResident(scalarModelResidentSetKernel<S, ModelT, jac(), cov()>,
                            set.first_block[set.num_costs], stream, set, control);
    });
  });
}
}  // namespace

template <typename S>
hipError_t launchScalarModelResidentSet(const ResidentSweepSet &set, const LmControl *control,
                                        int model, int jac_mode, int cov_mode, hipStream_t stream) {
  return withScalarModel(model, [&](auto kind) {
    return launchScalarResidentSetFor<S>(kind, set, control, jac_mode, cov_mode, stream);
  });
}
template hipError_t launchScalarModelResidentSet<float>(const ResidentSweepSet &, const LmControl *,
                                                        int, int, int, hipStream_t);
template hipError_t launchScalarModelResidentSet<double>(const ResidentSweepSet &, const LmControl *,
                                                         int, int, int, hipStream_t);

template <typename S>
hipError_t launchScalarModelResident(const ScalarSweepArgs<S> *d_args, const LmControl *control,
                                     int model, int jac_mode, int cov_mode, int grid,
                                     hipStream_t stream) {
  return withScalarModel(model, [&](auto kind) {
    return launchScalarResidentFor<S>(kind, d_args, control, jac_mode, cov_mode, grid, stream);
  });
}
template hipError_t launchScalarModelResident<float>(const ScalarSweepArgs<float> *,
                                                     const LmControl *, int, int, int, int,
                                                     hipStream_t);
template hipError_t launchScalarModelResident<double>(const ScalarSweepArgs<double> *,
                                                      const LmControl *, int, int, int, int,
                                                      hipStream_t);

}  // namespace mopt
