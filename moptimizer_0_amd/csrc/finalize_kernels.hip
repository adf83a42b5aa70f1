// gfx950 kernels that turn the workgroup partials a sweep left into H | b | sum_sq and hand them
// over (publish_device.hpp): the blocking calls' finalize kernels, the resident forms that take the
// LM step in the same launch (lm_device.hpp), and the whole small minimisation in one launch — of one
// workgroup for a lone cost, of a workgroup per problem for a batch.
#include "sweep_device.hpp"
#include "fd_device.hpp"
#include "lm_device.hpp"
#include "publish_device.hpp"

namespace mopt {
namespace {

// ---- finalisation: workgroup partials -> H | b | sum_sq -----------------------------------------
// One workgroup of 1024 threads.  partials[grid][nacc] is read as a flat array with a stride that
// is a multiple of nacc, so each thread stays in one column and all of its (few) loads are
// independent and in flight together — the kernel costs about one memory round trip, not one
// per row.  Column totals are then formed in a fixed order (bitwise reproducible).
constexpr int kFinalThreads = 1024;
// The resident finalize kernels that run the LM step in the same launch: 512 threads, so that a
// lane has 256 VGPRs — under the 128 of a 1024-thread workgroup the step's register-held solve
// spilled 434 VGPRs to scratch on its one busy lane.  (The width of a one-workgroup kernel costs
// nothing measurable: scripts/probes/finalize_width_probe.cpp.)  At least n^2 + n + 1 = 273
// threads: one per published value of a 16-parameter problem.
constexpr int kStepThreads = 512;
constexpr int kMaxAccumulators = 288;  // n <= 16 (run-time compiled wide models): n*n + n + 1 <= 273

// K rows of one thread (t, t + stride, ...; zeros past the end) added up.  The K loads are issued
// together from clamped indices and fenced from the selects that zero the rows past the end: a load
// under a branch gets its own wait, and left alone the scheduler interleaves loads and selects
// (reusing vcc) — either way a batch became 3-4 dependent round trips.
template <int K>
__device__ __forceinline__ double columnBatch(const double *partials, int t, int stride,
                                              int total_elems) {
  int at[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int idx = t + k * stride;
    at[k] = idx < total_elems ? idx : 0;  // (row 0 exists whatever the grid)
  }
  __builtin_amdgcn_sched_barrier(0);
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = partials[at[k]];
  __builtin_amdgcn_sched_barrier(0);
  // (the comparisons again from a laundered copy of t: left to itself the compiler keeps the K lane
  // masks of the first round alive across the loads — 2 K scalar registers, spilled from K = 32 on)
  int t_again = t;
  asm volatile("" : "+v"(t_again));
  double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < K; ++k) s[k & 3] += (t_again + k * stride) < total_elems ? v[k] : 0.0;
  return (s[0] + s[1]) + (s[2] + s[3]);
}

struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};

// Column sums of the `grid` partial rows of `nacc` values -> total[0 .. nacc).  `parked` runs once
// per thread after the thread's rows have been requested and added and before the first barrier:
// the place where a resident kernel puts values it requested *before* this call (basis, LM state)
// into LDS, so that their round trip overlaps the rows'.
template <int T, typename Parked = NoHook>
__device__ __forceinline__ void columnTotals(const double *partials, int grid, int nacc,
                                             double (&scratch)[T],
                                             double (&total)[kMaxAccumulators],
                                             Parked parked = Parked()) {
  const int per_col = T / nacc;  // threads per column
  const int stride = per_col * nacc;
  const int total_elems = grid * nacc;
  const int t = threadIdx.x;
  // rows per thread, the same for all — 1024 threads: 256 rows x 23 values: 6; the two-workgroups-
  // per-CU sweeps, 512 rows x 28: 15, x 43: 23; 512 threads: 12, 29, 47 — each a single batch, one
  // memory round trip; larger grids continue in batches of four
  const int rows = (total_elems + stride - 1) / stride;
  constexpr bool kRoomy = T <= 512;  // 256 VGPRs a lane: batches of 32 and 48 fit
  double sum = 0.0;
  if (t < stride) {
    if (rows <= 6) {
      sum = columnBatch<6>(partials, t, stride, total_elems);
    } else if (rows <= 12) {
      sum = columnBatch<12>(partials, t, stride, total_elems);
    } else if (rows <= 16) {
      sum = columnBatch<16>(partials, t, stride, total_elems);
    } else if (rows <= 24) {
      sum = columnBatch<24>(partials, t, stride, total_elems);
    } else if (kRoomy && rows <= 32) {
      sum = columnBatch<kRoomy ? 32 : 4>(partials, t, stride, total_elems);
    } else if (kRoomy && rows <= 48) {
      sum = columnBatch<kRoomy ? 48 : 4>(partials, t, stride, total_elems);
    } else {
      sum = columnBatch<24>(partials, t, stride, total_elems);
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      int idx = t + 24 * stride;
      for (; idx + 3 * stride < total_elems; idx += 4 * stride) {
        const double a = partials[idx], b = partials[idx + stride], c = partials[idx + 2 * stride],
                     d = partials[idx + 3 * stride];
        s0 += a;
        s1 += b;
        s2 += c;
        s3 += d;
      }
      for (; idx < total_elems; idx += stride) s0 += partials[idx];
      sum += (s0 + s1) + (s2 + s3);
    }
  }
  parked();
  scratch[t] = sum;
  __syncthreads();
  if (t < nacc) {
    double v = 0.0;
    for (int g = 0; g < per_col; ++g) v += scratch[t + g * nacc];
    total[t] = v;
  }
  __syncthreads();
}

// rows of [upper triangle or full H | b | sum_sq] over n parameters -> H (n x n column-major) | b |
// sum_sq.  nacc tells the form: n(n+1)/2 + n + 1 (symmetric) or n*n + n + 1 (full).
template <int T, typename Parked = NoHook>
__device__ __forceinline__ unsigned long long finalizeDenseBody(const double *partials, int grid,
                                                                int nacc, int n, double *result,
                                                                const HostPublish &pub,
                                                                const PeerCombine &pc,
                                                                double *result_lds = nullptr,
                                                                Parked parked = Parked(),
                                                                unsigned long long sequence_add = 0) {
  static_assert(T >= kMaxWideParams * kMaxWideParams + kMaxWideParams + 1, "one thread per value");
  __shared__ double scratch[T];
  __shared__ double total[kMaxAccumulators];
  columnTotals<T>(partials, grid, nacc, scratch, total, parked);
  const int k = threadIdx.x;
  const int count = n * n + n + 1;
  double v = 0.0;
  if (k < count) {
    const bool full = (nacc == count);
    const int nh = full ? n * n : n * (n + 1) / 2;
    if (k < n * n) {
      const int i = k % n, j = k / n;  // column-major H(i, j)
      if (full) {
        v = total[j * n + i];
      } else {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        v = total[hi * (hi + 1) / 2 + lo];
      }
    } else {
      v = total[nh + (k - n * n)];  // b (n) then sum_sq
    }
  }
  unsigned long long status;
  v = peerCombine(pc, count, v, &status, sequence_add);
  if (k < count) {
    result[k] = v;
    if (result_lds) result_lds[k] = v;
  }
  publishToHost(pub, count, v, status);
  return status;
}

__global__ __launch_bounds__(kFinalThreads) void finalizeDenseKernel(const double *partials,
                                                                      int grid, int nacc, int n,
                                                                      double *result,
                                                                      const HostPublish pub,
                                                                      const PeerCombine pc) {
  finalizeDenseBody<kFinalThreads>(partials, grid, nacc, n, result, pub, pc);
}

// Resident forms (device-resident LM): nothing goes to the host, the peer-combine sequence number
// is the base the host assigned plus the number of trials the step kernel has counted.  STEP = 4 or
// 8: this cost is the last of its problem and the LM step (lm_device.hpp) runs right here, on the
// result still in LDS, as LevenbergMarquadtDynamic<float> or <double> — one launch and one memory
// round trip less per evaluated point; the stored LM state is requested before the finalize work so
// that its latency hides behind it.
template <int STEP>
struct StepScalar {
  using type = double;
};
template <>
struct StepScalar<4> {
  using type = float;
};

template <int STEP>
__global__ __launch_bounds__(kStepThreads) void finalizeDenseResidentKernel(
    const double *partials, int grid, int nacc, int n, double *result, LmControl *control,
    PeerCombine pc, const LmProblem P, int own_index) {
  if (control->done) return;
  using S = typename StepScalar<STEP>::type;
  LmStateWords state_words = {0u, 0u};
  if constexpr (STEP != 0) state_words = lmPrefetchState<S>(P);
  __shared__ double own[kSlotData];
  const unsigned long long status = finalizeDenseBody<kStepThreads>(
      partials, grid, nacc, n, result, HostPublish(), pc, own, NoHook(),
      (unsigned long long)control->trial);
  if (status && threadIdx.x == 0) control->pad[0] = int(status);  // a rank went missing
  if constexpr (STEP != 0) {
    __syncthreads();
    lmStepBody<S>(P, false, LmStart<S>(), own, own_index, true, state_words);
  }
}

// PEERS = false: no exchange between ranks, and no PeerCombine to read (a default-constructed one
// handed in by reference is a private array, i.e. scratch memory).
template <int T, typename Parked = NoHook, bool PEERS = true>
__device__ __forceinline__ unsigned long long finalizeMomentsBody(const double *partials, int grid,
                                                                  const AffineBasis &B,
                                                                  double *result,
                                                                  const HostPublish &pub,
                                                                  const PeerCombine &pc,
                                                                  double *result_lds = nullptr,
                                                                  Parked parked = Parked(),
                                                                  unsigned long long sequence_add = 0) {
  __shared__ double scratch[T];
  __shared__ double total[kMaxAccumulators];
  __shared__ double terms[36 * 16 + 6 * 4];
  columnTotals<T>(partials, grid, kAccMoments, scratch, total, parked);
  const int t = threadIdx.x;
  // 36 x 16 products for H, 6 x 4 for b: one per thread, in trips of T
  for (int item = t; item < 36 * 16 + 24; item += T) {
  if (item < 36 * 16) {
    const int o = item >> 4, ab = item & 15;
    const int i = o % 6, j = o / 6;
    int a = ab >> 2, b = ab & 3;
    double form = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double sj = 0.0;  // (S J_b)(r, j)
#pragma unroll
      for (int c = 0; c < 3; ++c) sj += B.cov[r * 3 + c] * B.J[b][c * 6 + j];
      form += B.J[a][r * 6 + i] * sj;
    }
    if (a > b) {
      const int tmp = a;
      a = b;
      b = tmp;
    }
    // (0,0)=0 (0,b)=b (1,1)=4 (1,2)=5 (1,3)=6 (2,2)=7 (2,3)=8 (3,3)=9
    const int wi = a == 0 ? b : (a == 1 ? 3 + b : (a == 2 ? 5 + b : 9));
    terms[item] = total[wi] * form;
  } else {
    const int u = item - 36 * 16;
    const int i = u >> 2, a = u & 3;
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double sv = 0.0;  // (S V(a, .))(r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        sv += B.cov[r * 3 + c] * (a == 0 ? total[10 + c] : total[13 + 3 * (a - 1) + c]);
      g += B.J[a][r * 6 + i] * sv;
    }
    terms[item] = g;
  }
  }
  __syncthreads();
  double v = 0.0;
  if (t < kResultDoubles) {
    if (t < 36) {
#pragma unroll
      for (int q = 0; q < 16; ++q) v += terms[t * 16 + q];
    } else if (t < 42) {
      const int i = t - 36;
      v = ((terms[576 + i * 4] + terms[576 + i * 4 + 1]) + terms[576 + i * 4 + 2]) +
          terms[576 + i * 4 + 3];
    } else {
      v = total[22];
    }
  }
  unsigned long long status = 0;
  if constexpr (PEERS) v = peerCombine(pc, kResultDoubles, v, &status, sequence_add);
  if (t < kResultDoubles) {
    result[t] = v;
    if (result_lds) result_lds[t] = v;
  }
  publishToHost(pub, kResultDoubles, v, status);
  return status;
}

__global__ __launch_bounds__(kFinalThreads) void finalizeMomentsKernel(const double *partials,
                                                                        int grid,
                                                                        const AffineBasis B,
                                                                        double *result,
                                                                        const HostPublish pub,
                                                                        const PeerCombine pc) {
  finalizeMomentsBody<kFinalThreads>(partials, grid, B, result, pub, pc);
}

template <int STEP>
__global__ __launch_bounds__(kStepThreads) void finalizeMomentsResidentKernel(
    const double *partials, int grid, const AffineBasis *__restrict__ d_basis, double *result,
    LmControl *control, const PeerCombine pc, const LmProblem P, int own_index) {
#ifdef MOPT_LM_TIMING
  const unsigned long long tick_entry = wall_clock64();
#endif
  if (control->done) return;
#ifdef MOPT_LM_TIMING
  const unsigned long long tick_control = wall_clock64();
#endif
  using S = typename StepScalar<STEP>::type;
  LmStateWords state_words = {0u, 0u};
  if constexpr (STEP != 0) state_words = lmPrefetchState<S>(P);
  // the basis is requested now and parked in LDS once the partial rows have been requested too
  // (columnTotals' hook): one round trip for state, basis and rows together
  constexpr int kBasisDoubles = int(sizeof(AffineBasis) / sizeof(double));
  const double basis_value = reinterpret_cast<const double *>(
      d_basis)[int(threadIdx.x) < kBasisDoubles ? int(threadIdx.x) : 0];  // unconditional: no wait
  __shared__ AffineBasis B;
  __shared__ double own[kSlotData];
  const auto park_basis = [&]() {
    if (int(threadIdx.x) < kBasisDoubles) reinterpret_cast<double *>(&B)[threadIdx.x] = basis_value;
  };
#ifdef MOPT_LM_TIMING
  const unsigned long long tick_basis = wall_clock64();
#endif
  const unsigned long long status = finalizeMomentsBody<kStepThreads>(
      partials, grid, B, result, HostPublish(), pc, own, park_basis,
      (unsigned long long)control->trial);
  if (status && threadIdx.x == 0) control->pad[0] = int(status);
#ifdef MOPT_LM_TIMING
  if (threadIdx.x == 0)
    printf("finalize: control word %llu, basis + state in LDS %llu, sums contracted %llu (x10 ns)\n",
           tick_control - tick_entry, tick_basis - tick_control, wall_clock64() - tick_basis);
#endif
  if constexpr (STEP != 0) {
    __syncthreads();
    // (rows of moments are a point2point cost's: the problem has its six parameters)
    lmStepBody<S, kNumParams>(P, false, LmStart<S>(), own, own_index, true, state_words);
  }
}

// A cost whose forward-difference sweep is chosen per evaluated point (sweep.hpp kLmGateMoments): the
// sweep left rows of moments (the word zero) or dense rows (non-zero); the word is rewritten only by the
// step at the end of this kernel, so it still says which.
template <int STEP>
__global__ __launch_bounds__(kStepThreads) void finalizeEitherResidentKernel(
    const double *partials, int grid_moments, int grid_literal, int nacc,
    const AffineBasis *__restrict__ d_basis, double *result, LmControl *control, const PeerCombine pc,
    const LmProblem P, int own_index) {
  const int gate = control[kLmGateMoments].done;  // (uniform: one scalar load)
  if (gate == kLmGateStopped) return;
  const bool literal = gate == kLmGateLiteralForm;
  using S = typename StepScalar<STEP>::type;
  LmStateWords state_words = {0u, 0u};
  if constexpr (STEP != 0) state_words = lmPrefetchState<S>(P);
  // the basis is requested whichever form ran (the literal one does not use it): with the state it is in
  // flight before the branch, and the rows are requested right behind — one round trip, as in the
  // single-purpose finalize kernels
  constexpr int kBasisDoubles = int(sizeof(AffineBasis) / sizeof(double));
  const double basis_value = reinterpret_cast<const double *>(
      d_basis)[int(threadIdx.x) < kBasisDoubles ? int(threadIdx.x) : 0];
  const unsigned long long trial = (unsigned long long)control->trial;
  __shared__ AffineBasis B;
  __shared__ double own[kSlotData];
  unsigned long long status;
  if (literal) {
    status = finalizeDenseBody<kStepThreads>(partials, grid_literal, nacc, kNumParams, result, HostPublish(),
                                             pc, own, NoHook(), trial);
  } else {
    const auto park_basis = [&]() {
      if (int(threadIdx.x) < kBasisDoubles) reinterpret_cast<double *>(&B)[threadIdx.x] = basis_value;
    };
    status = finalizeMomentsBody<kStepThreads>(partials, grid_moments, B, result, HostPublish(), pc, own,
                                               park_basis, trial);
  }
  if (status && threadIdx.x == 0) control->pad[0] = int(status);
  if constexpr (STEP != 0) {
    __syncthreads();
    lmStepBody<S, kNumParams>(P, false, LmStart<S>(), own, own_index, true, state_words);
  }
}

// ---- a whole minimisation in one launch ---------------------------------------------------------
// Small point2point problems (the reference's own test sizes: tst/point2point.cpp registers 1 k
// correspondences): under the launch-per-point loop an evaluated point costs two launches, 11-12 us,
// of which the sweep of a tile or two is a fraction.  Here one workgroup runs the loop of
// levenberg_marquadt_dyn.cpp:34-119 without leaving the kernel.  The correspondences — at most
// kSolveSmallTiles tiles — are loaded once and stay in registers for every evaluated point; per
// point the workgroup adds up their moments (momentsOfPack, the arithmetic of the resident sweep),
// reduces them to one row in LDS, contracts it as finalizeMomentsResidentKernel does and takes the
// LM step, whose state stays in LDS; the per-x constants and the Jacobian basis the step leaves for
// the next sweep stay in LDS too (through HBM they would come back through the scalar cache, which
// does not see this kernel's own stores).  The sums are those of the launch-per-point loop added in
// another order (one row instead of one per tile): the same iterates to rounding
// (tests/test_gpu_device_lm.py).  At most `max_points` evaluated points: the loop's own bound, which
// every thread reaches.
constexpr int kSolveSmallTiles = 4;

// FD_COV >= 0 (a covariance form): the kernel also holds the literal forward-difference form for that
// covariance (fd_device.hpp, over the packs held in registers, rotations re-read from LDS: registers are
// what this kernel is short of) and the step says per point which form runs — a cost that differentiates
// numerically under MOPT_KERNEL_AUTO / _MOMENTS (LmProblem::fd_per_iterate).  FD_COV = -1: moments only.
//
// The body of that kernel, shared by its two callers: p2pSolveSmallKernel (one problem, described by
// kernel arguments) and p2pSolveBatchKernel (a problem per workgroup, described by per-batch arrays).
// fill_problem(words): the caller's way of putting the problem's description into the LDS copy the loop
// reads (the barrier that makes it visible to every thread is the one behind the copies of the argument
// and basis blocks); `start` may lie in kernel arguments or in device memory.
static_assert(sizeof(LmProblem) % 4 == 0, "copied by words");
constexpr int kProblemWords = int(sizeof(LmProblem) / 4);

template <typename S, int FD_COV, typename FillProblem>
__device__ __forceinline__ void p2pSolveSmallBody(const S *tiles, int num_tiles,
                                                  const P2PSweepArgs<S> *__restrict__ d_args,
                                                  const AffineBasis *__restrict__ d_basis, double *result,
                                                  FillProblem &&fill_problem, const LmStart<S> &start,
                                                  int max_points) {
  constexpr bool kChooses = FD_COV >= 0;
  __shared__ int fd_choice;  // written by the step: the next point takes the literal form
  if (threadIdx.x == 0) fd_choice = 0;
  __shared__ P2PSweepArgs<S> A;
  __shared__ AffineBasis B;
  // the problem's description, read from LDS inside the loop: as kernel arguments its 1.2 KB are
  // loop invariants the compiler loads up front into scalar registers, of which there are 104 —
  // some 400 spills to vector lanes, read back one by one in every step
  __shared__ alignas(16) unsigned int problem_words[kProblemWords];
  fill_problem(problem_words);
  const LmProblem &P = *reinterpret_cast<const LmProblem *>(problem_words);
  __shared__ double row[kAccMoments];
  __shared__ double own[kSlotData];
  constexpr int V = TileShape<S>::kVec, TP = TileShape<S>::kPoints;
  Pack<S> held[kSolveSmallTiles][6];
#pragma unroll
  for (int t = 0; t < kSolveSmallTiles; ++t) {
    // (past the last tile: that tile again — an unconditional load; its values are never used)
    const S *base = tiles + size_t(t < num_tiles ? t : num_tiles - 1) * TileShape<S>::kP2PScalars +
                    threadIdx.x * V;
#pragma unroll
    for (int pl = 0; pl < 6; ++pl) held[t][pl] = loadPack<S>(base + pl * TP);
  }
  static_assert(sizeof(P2PSweepArgs<S>) % 4 == 0 && sizeof(AffineBasis) % 4 == 0, "copied by words");
  constexpr int kArgWords = int(sizeof(P2PSweepArgs<S>) / 4), kBasisWords = int(sizeof(AffineBasis) / 4);
  for (int i = threadIdx.x; i < kArgWords; i += kBlockThreads)
    reinterpret_cast<unsigned int *>(&A)[i] = reinterpret_cast<const unsigned int *>(d_args)[i];
  for (int i = threadIdx.x; i < kBasisWords; i += kBlockThreads)
    reinterpret_cast<unsigned int *>(&B)[i] = reinterpret_cast<const unsigned int *>(d_basis)[i];
  __syncthreads();
  // (one inlined copy of the step: its first run starts the minimisation, like lmStepKernel's `init`)
  for (int point = 0;; ++point) {
#ifdef MOPT_LM_TIMING
    const unsigned long long tick_step = wall_clock64();
#endif
    const bool finished = lmStepBodyFor<S, kMaxParams, true, kNumParams, kChooses>(
        P, point == 0, start, own, 0, false, LmStateWords(), &A, &B, &fd_choice);
    if (finished || point >= max_points) break;
#ifdef MOPT_LM_TIMING
    const unsigned long long tick_sweep = wall_clock64();
    unsigned long long tick_finalize = tick_sweep;
#endif
    bool literal = false;
    if constexpr (kChooses) literal = fd_choice != 0;  // (uniform; the step's barriers precede this read)
    if (literal) {
      if constexpr (kChooses) {
        constexpr int NACC = (FD_COV == kCovGeneral) ? kAccFull : kAccSym;
        __shared__ double dense_row[NACC];
        p2pForwardDiffRow<S, FD_COV, kFdRotationLds>(
            A, A,
            [&](auto &&body) {
#pragma unroll
              for (int t = 0; t < kSolveSmallTiles; ++t)
                if (t < num_tiles) body(held[t], (long long)t * TP + threadIdx.x * V);
            },
            dense_row);
        __syncthreads();
        // one row: nothing to add up — H (column-major) | b | sum_sq out of the row's layout, as
        // finalizeDenseBody lays them out
        const int k = threadIdx.x;
        constexpr int n = kNumParams, count = n * n + n + 1;
        if (k < count) {
          double v;
          if (k < n * n) {
            const int i = k % n, j = k / n;
            if (FD_COV == kCovGeneral) {
              v = dense_row[j * n + i];
            } else {
              const int lo = i < j ? i : j, hi = i < j ? j : i;
              v = dense_row[hi * (hi + 1) / 2 + lo];
            }
          } else {
            v = dense_row[(FD_COV == kCovGeneral ? n * n : n * (n + 1) / 2) + (k - n * n)];
          }
          result[k] = v;
          own[k] = v;
        }
        __syncthreads();
      }
    } else {
      double acc[kAccMoments];
#pragma unroll
      for (int k = 0; k < kAccMoments; ++k) acc[k] = 0.0;
#pragma unroll
      for (int t = 0; t < kSolveSmallTiles; ++t)
        if (t < num_tiles) momentsOfPack<S>(acc, held[t], (long long)t * TP + threadIdx.x * V, A);
      blockReduceStore<kAccMoments>(acc, row);
      __syncthreads();
#ifdef MOPT_LM_TIMING
      tick_finalize = wall_clock64();
#endif
      finalizeMomentsBody<kBlockThreads, NoHook, false>(row, 1, B, result, HostPublish(), PeerCombine(),
                                                        own);
      __syncthreads();
    }
#ifdef MOPT_LM_TIMING
    if (threadIdx.x == 0)
      printf("one launch, point %d: step %llu sweep of %d tiles %llu contraction %llu (x10 ns)\n", point,
             tick_sweep - tick_step, num_tiles, tick_finalize - tick_sweep, wall_clock64() - tick_finalize);
#endif
  }
}

template <typename S, int FD_COV>
__global__ __launch_bounds__(kBlockThreads) void p2pSolveSmallKernel(
    const S *tiles, int num_tiles, const P2PSweepArgs<S> *__restrict__ d_args,
    const AffineBasis *__restrict__ d_basis, double *result, const LmProblem problem,
    const LmStart<S> start, int max_points) {
  p2pSolveSmallBody<S, FD_COV>(
      tiles, num_tiles, d_args, d_basis, result,
      [&](unsigned int *words) {
        for (int i = threadIdx.x; i < kProblemWords; i += kBlockThreads)
          words[i] = reinterpret_cast<const unsigned int *>(&problem)[i];
      },
      start, max_points);
}

// B independent small problems, one per workgroup (mopt_batch, batch.cpp): workgroup b runs the body
// above over tiles [first_tile[b], first_tile[b + 1]) of the batch's tile array with its own argument,
// basis, result, control and report blocks and its own start pose.  One description of the problem
// serves the batch (options, Jacobian mode: device memory, written per call); each workgroup copies
// it into LDS and patches what is its own — the pointers and the bound of |p| its forward-difference
// choice is taken with — there, so that nothing per problem is held in registers across the loop.
// Nothing crosses workgroups.
static_assert(sizeof(LmStart<double>) == kMaxWideParams * sizeof(double) &&
                  sizeof(LmStart<float>) == kMaxWideParams * sizeof(float),
              "BatchSolveLaunch::starts is an array of these");
static_assert(kBatchResultStride >= kResultDoubles, "a problem's H | b | sum_sq");
template <typename S>
struct SolveBatchArgs {
  const S *tiles;
  const int *first_tile;             // [B + 1]
  const LmProblem *problem;          // the batch's one description (device memory)
  P2PSweepArgs<S> *args;             // [B]
  AffineBasis *basis;                // [B]
  double *results;                   // [B][kBatchResultStride]
  LmControl *controls;               // [B][kLmControlBlocks]
  LmReport *reports;                 // [B], mapped host memory
  const LmStart<S> *starts;          // [B]
  const double *source_bounds;       // [B]: |centre| + radius of each problem's sources
  int max_points;
};

template <typename S, int FD_COV>
__global__ __launch_bounds__(kBlockThreads) void p2pSolveBatchKernel(const SolveBatchArgs<S> batch) {
  const int b = blockIdx.x;
  const int first = batch.first_tile[b];
  p2pSolveSmallBody<S, FD_COV>(
      batch.tiles + size_t(first) * TileShape<S>::kP2PScalars, batch.first_tile[b + 1] - first,
      batch.args + b, batch.basis + b, batch.results + size_t(b) * kBatchResultStride,
      [&](unsigned int *words) {
        for (int i = threadIdx.x; i < kProblemWords; i += kBlockThreads)
          words[i] = reinterpret_cast<const unsigned int *>(batch.problem)[i];
        __syncthreads();
        if (threadIdx.x == 0) {
          LmProblem &P = *reinterpret_cast<LmProblem *>(words);
          P.control = batch.controls + size_t(b) * kLmControlBlocks;
          P.state = nullptr;  // (the state of a one-launch solve never leaves LDS)
          P.report = batch.reports + b;
          P.cost[0].args = batch.args + b;
          P.cost[0].basis = batch.basis + b;
          P.cost[0].result = batch.results + size_t(b) * kBatchResultStride;
          P.fd_source_bound = batch.source_bounds[b];
        }
      },
      batch.starts[b], batch.max_points);
}

__device__ __forceinline__ void finalizeCostBody(const double *partials, int grid, double *result,
                                                 const HostPublish &pub, const PeerCombine &pc) {
  __shared__ double lds[kFinalThreads / 64];
  double s = 0.0;
  for (int row = threadIdx.x; row < grid; row += kFinalThreads) s += partials[row];
  s = waveSum(s);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < kFinalThreads / 64; ++k) v += lds[k];
    lds[0] = v;
  }
  __syncthreads();
  unsigned long long status;
  const double v = peerCombine(pc, 1, lds[0], &status);
  if (threadIdx.x == 0) result[0] = v;
  publishToHost(pub, 1, v, status);
}

__global__ __launch_bounds__(kFinalThreads) void finalizeCostKernel(const double *partials,
                                                                     int grid, double *result,
                                                                     const HostPublish pub,
                                                                     const PeerCombine pc) {
  finalizeCostBody(partials, grid, result, pub, pc);
}

__global__ void publishKernel(const double *values, int count, const HostPublish pub) {
  const double v = int(threadIdx.x) < count ? values[threadIdx.x] : 0.0;
  publishToHost(pub, count, v);
}

}  // namespace

// ---- host-side launch wrappers -----------------------------------------------------------------
bool aqlFinalizersLoaded(const mopt_detail::AqlSite &site) {
  return site.queue &&
         mopt_detail::aqlLookup(site.device, reinterpret_cast<const void *>(finalizeDenseKernel)) &&
         mopt_detail::aqlLookup(site.device, reinterpret_cast<const void *>(finalizeMomentsKernel)) &&
         mopt_detail::aqlLookup(site.device, reinterpret_cast<const void *>(finalizeCostKernel));
}

namespace {
// A blocking call's finalize kernel (one workgroup; its last two parameters are the hand-over to the
// host and the sum over the ranks): to the queue its sweep went to, when that was the cost's own —
// the three kernels are looked up beforehand (aqlFinalizersLoaded), so that cannot fail over — else
// to the stream.
template <typename Kernel, typename... Args>
hipError_t launchFinalize(Kernel kernel, const HostPublish &pub, hipStream_t stream,
                          const PeerCombine *peers, const mopt_detail::AqlSite *aql,
                          const Args &...args) {
  const PeerCombine pc = peers ? *peers : PeerCombine();
  if (aql)
    return mopt_detail::aqlLaunch(*aql, kernel, 1u, uint32_t(kFinalThreads), args..., pub, pc)
               ? hipSuccess
               : hipErrorLaunchFailure;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(kFinalThreads), 0, stream, args..., pub, pc);
  return hipGetLastError();
}

bool isDenseRow(int nacc, int n) {
  return nacc == denseRowLength(n, kCovSymmetric) || nacc == denseRowLength(n, kCovGeneral);
}
}  // namespace

hipError_t launchFinalizeDense(const double *partials, int grid, int nacc, int n, double *result,
                               const HostPublish &pub, hipStream_t stream,
                               const PeerCombine *peers, const mopt_detail::AqlSite *aql) {
  if (n < 1 || n > kMaxWideParams || !isDenseRow(nacc, n)) return hipErrorInvalidValue;
  if (peers && peers->num_ranks > 0 && n * n + n + 1 > kSlotData) return hipErrorInvalidValue;
  return launchFinalize(finalizeDenseKernel, pub, stream, peers, aql, partials, grid, nacc, n, result);
}

hipError_t launchFinalizeMoments(const double *partials, int grid, const AffineBasis &basis,
                                 double *result, const HostPublish &pub, hipStream_t stream,
                                 const PeerCombine *peers, const mopt_detail::AqlSite *aql) {
  return launchFinalize(finalizeMomentsKernel, pub, stream, peers, aql, partials, grid, basis, result);
}

hipError_t launchFinalizeCost(const double *partials, int grid, double *result,
                              const HostPublish &pub, hipStream_t stream,
                              const PeerCombine *peers, const mopt_detail::AqlSite *aql) {
  return launchFinalize(finalizeCostKernel, pub, stream, peers, aql, partials, grid, result);
}

hipError_t launchPublish(const double *d_values, int count, const HostPublish &pub,
                         hipStream_t stream) {
  if (count < 0 || count > kMaxAccumulators) return hipErrorInvalidValue;
  hipLaunchKernelGGL(publishKernel, dim3(1), dim3((kMaxAccumulators + 63) / 64 * 64), 0, stream, d_values, count, pub);
  return hipGetLastError();
}

// ---- resident forms (device-resident LM) ---------------------------------------------------------
int solveSmallMaxTiles() { return kSolveSmallTiles; }

template <typename S>
hipError_t launchP2PSolveSmall(const S *tiles, int num_tiles, const P2PSweepArgs<S> *d_args,
                               const AffineBasis *d_basis, double *result, const LmProblem &problem,
                               const S *x0, int max_points, int fd_cov, hipStream_t stream) {
  if (num_tiles < 1 || num_tiles > kSolveSmallTiles || problem.num_costs != 1 ||
      problem.n != kNumParams || max_points < 1)
    return hipErrorInvalidValue;
  LmStart<S> start;
  for (int i = 0; i < kMaxWideParams; ++i) start.x[i] = i < problem.n ? x0[i] : S(0);
  // FD_COV: the covariance form of the literal forward-difference sweep the kernel holds next to the
  // moments where the step chooses per point (there it must be named); -1: the moments alone
  auto launch = [&](auto fd) {
    return launchResident(p2pSolveSmallKernel<S, fd()>, 1, stream, tiles, num_tiles, d_args, d_basis,
                          result, problem, start, max_points);
  };
  if (problem.fd_per_iterate)
    return dispatch::intOrFail<kCovIdentity, kCovSymmetric, kCovGeneral>(fd_cov, hipErrorInvalidValue,
                                                                         launch);
  return launch(dispatch::Int<-1>{});
}
template hipError_t launchP2PSolveSmall<float>(const float *, int, const P2PSweepArgs<float> *,
                                               const AffineBasis *, double *, const LmProblem &,
                                               const float *, int, int, hipStream_t);
template hipError_t launchP2PSolveSmall<double>(const double *, int, const P2PSweepArgs<double> *,
                                                const AffineBasis *, double *, const LmProblem &,
                                                const double *, int, int, hipStream_t);

template <typename S>
hipError_t launchP2PSolveBatch(const BatchSolveLaunch &launch, int fd_cov, hipStream_t stream) {
  if (launch.num_problems < 1 || launch.max_points < 1) return hipErrorInvalidValue;
  SolveBatchArgs<S> a;
  a.tiles = static_cast<const S *>(launch.tiles);
  a.first_tile = launch.first_tile;
  a.problem = launch.problem;
  a.args = static_cast<P2PSweepArgs<S> *>(launch.args);
  a.basis = launch.basis;
  a.results = launch.results;
  a.controls = launch.controls;
  a.reports = launch.reports;
  a.starts = static_cast<const LmStart<S> *>(launch.starts);
  a.source_bounds = launch.source_bounds;
  a.max_points = launch.max_points;
  auto go = [&](auto fd) {
    return launchResident(p2pSolveBatchKernel<S, fd()>, launch.num_problems, stream, a);
  };
  if (launch.fd_per_iterate)
    return dispatch::intOrFail<kCovIdentity, kCovSymmetric, kCovGeneral>(fd_cov, hipErrorInvalidValue, go);
  return go(dispatch::Int<-1>{});
}
template hipError_t launchP2PSolveBatch<float>(const BatchSolveLaunch &, int, hipStream_t);
template hipError_t launchP2PSolveBatch<double>(const BatchSolveLaunch &, int, hipStream_t);

namespace {
// A resident finalize kernel (one workgroup; its last three parameters are the sum over the ranks,
// the problem and this cost's slot in it): `pick(step)` names the kernel for a step scalar — 0 where no
// LM step is taken in this launch (`step` NULL), else LevenbergMarquadtDynamic<double | float> by
// `scalar_bytes`.
template <typename Pick, typename... Args>
hipError_t launchResidentFinalize(Pick pick, hipStream_t stream, const PeerCombine *peers,
                                  const LmProblem *step, int own_index, int scalar_bytes,
                                  const Args &...args) {
  const PeerCombine pc = peers ? *peers : PeerCombine();
  return withLmStepScalar(step != nullptr, scalar_bytes, [&](auto step_scalar) {
    hipLaunchKernelGGL(pick(step_scalar), dim3(1), dim3(kStepThreads), 0, stream, args..., pc,
                       step ? *step : LmProblem(), step ? own_index : 0);
    return hipGetLastError();
  });
}
}  // namespace

hipError_t launchFinalizeDenseResident(const double *partials, int grid, int nacc, int n,
                                       double *result, LmControl *control, hipStream_t stream,
                                       const PeerCombine *peers, const LmProblem *step,
                                       int own_index, int scalar_bytes) {
  if (n < 1 || n > kMaxWideParams || !isDenseRow(nacc, n)) return hipErrorInvalidValue;
  return launchResidentFinalize([](auto s) { return finalizeDenseResidentKernel<s()>; }, stream, peers,
                                step, own_index, scalar_bytes, partials, grid, nacc, n, result, control);
}

hipError_t launchFinalizeEitherResident(const double *partials, int grid_moments, int grid_literal,
                                        int nacc, const AffineBasis *d_basis, double *result,
                                        LmControl *control, hipStream_t stream,
                                        const PeerCombine *peers, const LmProblem *step,
                                        int own_index, int scalar_bytes) {
  if (nacc != kAccSym && nacc != kAccFull) return hipErrorInvalidValue;
  return launchResidentFinalize([](auto s) { return finalizeEitherResidentKernel<s()>; }, stream, peers,
                                step, own_index, scalar_bytes, partials, grid_moments, grid_literal,
                                nacc, d_basis, result, control);
}

hipError_t launchFinalizeMomentsResident(const double *partials, int grid,
                                         const AffineBasis *d_basis, double *result,
                                         LmControl *control, hipStream_t stream,
                                         const PeerCombine *peers, const LmProblem *step,
                                         int own_index, int scalar_bytes) {
  return launchResidentFinalize([](auto s) { return finalizeMomentsResidentKernel<s()>; }, stream, peers,
                                step, own_index, scalar_bytes, partials, grid, d_basis, result, control);
}

}  // namespace mopt
