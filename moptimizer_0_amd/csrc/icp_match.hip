// gfx950 kernels of the correspondence search (ICP update step) over the grid built with cell_order.hip,
// driven by icp.cpp: the search itself, the gather of the targets it found and the count of matched
// sources handed to the host.
#include "sweep_device.hpp"
#include "publish_device.hpp"

#include <cstdlib>
#include <limits>

namespace mopt {
namespace {

// ---- correspondence search (ICP update step) ---------------------------------------------------
// One thread per source point: warp it with the current pose, look through the grid cells around
// it — the 2 x 2 x 2 nearest first, the wave in lock step, then what of the (2 reach + 1)^3 block
// the best so far still admits —, keep the nearest target within the maximum distance, and write
// that target into the target planes of the point's slot (or the NaN marker).  The reference leaves
// this step to the user model's update(x) (model.h:24-26; "setup can be i.e nearest neighboor
// search", docs/Cost.puml:14-17) and ships no implementation, so semantics are defined here: exact
// nearest neighbour in the Euclidean metric, ties resolved to the first candidate in (cell z, y, x;
// original index) order.

// candidates per lane and trip of the first round (4, 6 and 8 measure the same; 2 is slower)
constexpr int kIcpTrip = 4;

template <typename S, int TRIP>
__device__ __forceinline__ void icpMatchBody(const IcpMatchArgs<S> &A, const S (&T)[12]) {
  constexpr int TP = TileShape<S>::kPoints;
  const long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= (long long)A.num_tiles * TP) return;  // (whole workgroups: TP is a multiple of their size)
  S *slot = A.tiles + (i / TP) * TileShape<S>::kP2PScalars + (i % TP);
  // No lane leaves before the end: the first round below runs in lock step over the wave, every
  // load from an address that exists whatever the lane holds (slots past the count are padding).
  const S p[3] = {slot[0 * TP], slot[1 * TP], slot[2 * TP]};
  S w[3], g[3];
  bool inside = i < A.count;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    w[a] = ((T[a * 4 + 0] * p[0] + T[a * 4 + 1] * p[1]) + T[a * 4 + 2] * p[2]) + T[a * 4 + 3];
    g[a] = floor((w[a] - A.origin[a]) * A.inv_cell);
    inside = inside && g[a] >= S(-A.reach) && g[a] <= S(A.dims[a] - 1 + A.reach);
  }
  const int c[3] = {inside ? int(g[0]) : 0, inside ? int(g[1]) : 0, inside ? int(g[2]) : 0};
  bool found = false;
  S best_d = A.max_dist2;
  // Ties go to the candidate stored first — (cell z, y, x; original index) order — whatever order
  // the cells are visited in, and however often: the position k is part of the comparison.
  int best_k = 0x7fffffff;
  // In the first round the winner's coordinates travel with it (reading them at the end would be
  // one more dependent round trip for every wave); the second round tracks distance and position
  // only and reads the coordinates of a winner it found once, at its end: six conditional moves
  // less per candidate where candidates are many.
  S best[3] = {S(0), S(0), S(0)};
  auto consider = [&](const S (&q)[3], int k, bool present, auto keep_coordinates) {
    const S d0 = w[0] - q[0], d1 = w[1] - q[1], d2 = w[2] - q[2];
    const S dist = d0 * d0 + d1 * d1 + d2 * d2;
    const bool better = present && dist <= A.max_dist2 &&
                        (!found || dist < best_d || (dist == best_d && k < best_k));
    found = found || better;
    best_d = better ? dist : best_d;
    best_k = better ? k : best_k;
    if constexpr (decltype(keep_coordinates)::value) {
#pragma unroll
      for (int a = 0; a < 3; ++a) best[a] = better ? q[a] : best[a];
    }
  };
  auto fetch = [&](int k, S (&q)[3]) {
    const Pack<S> *cand = reinterpret_cast<const Pack<S> *>(A.sorted + size_t(k) * 4);
    if (sizeof(S) == 8) {
      const Pack<S> lo = cand[0], hi = cand[1];
      q[0] = lo.v[0]; q[1] = lo.v[1]; q[2] = hi.v[0];
    } else {
      const Pack<S> all = cand[0];
      q[0] = all.v[0]; q[1] = all.v[1]; q[2] = all.v[2];
    }
  };
  // Offsets inside the own cell, [0, cell).  They are recomputed from the cell index and can
  // disagree with the binning's floor((w - origin) / cell) by a few ulps OF THE COORDINATE (not of
  // the offset): every gap to a face is shortened by that much before it is squared, in the scalar
  // type's own epsilon (targets were binned with floor()).
  constexpr S kUlps = S(16) * std::numeric_limits<S>::epsilon();
  const S fx = w[0] - (A.origin[0] + S(c[0]) * A.cell);
  const S fy = w[1] - (A.origin[1] + S(c[1]) * A.cell);
  const S fz = w[2] - (A.origin[2] + S(c[2]) * A.cell);
  const S ex = kUlps * (fabs(w[0]) + fabs(A.origin[0]) + A.cell);
  const S ey = kUlps * (fabs(w[1]) + fabs(A.origin[1]) + A.cell);
  const S ez = kUlps * (fabs(w[2]) + fabs(A.origin[2]) + A.cell);
  auto within = [&](S bound) {
    return bound * (S(1) - kUlps) <= (found ? best_d : A.max_dist2);
  };
  auto sq = [](S v) { return v > S(0) ? v * v : S(0); };

  // First round, the wave in lock step: the 2 x 2 x 2 cells nearest to the point (per axis the own
  // cell and the neighbour across the nearer face) hold every target closer than half a cell.
  // They are four runs of two consecutive cells: eight range bounds fetched together, then the
  // lane's candidates out of the four runs as ONE list, four per trip — every trip is eight (fp32:
  // four) loads in flight and one wait, and the wave makes as many trips as its longest list
  // needs.  Walking the rows one after the other instead, each lane under its own pruning, the
  // wave executed the union of its lanes' visits: ~116 vector loads per wave with an eighth of the
  // lanes active in each, ~20 dependent waits.
  const S half = S(0.5) * A.cell;
  const int sx = fx < half ? -1 : 0, sy = fy < half ? -1 : 0, sz = fz < half ? -1 : 0;
  int first[4], ends[4];
  {
    int xa = c[0] + sx, xb = xa + 1;
    xa = xa < 0 ? 0 : xa;
    xb = xb >= A.dims[0] ? A.dims[0] - 1 : xb;
    int at_a[4], at_b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = c[1] + sy + (r & 1), z = c[2] + sz + (r >> 1);
      const bool ok = inside && xa <= xb && y >= 0 && y < A.dims[1] && z >= 0 && z < A.dims[2];
      const int row = (z * A.dims[1] + y) * A.dims[0];  // the grid has at most 2^28 cells (icp.cpp)
      at_a[r] = ok ? row + xa : 0;  // (entry 0 twice: an empty run)
      at_b[r] = ok ? row + xb + 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      first[r] = A.cell_start[at_a[r]];
      ends[r] = A.cell_start[at_b[r]];
    }
  }
  const int n0 = ends[0] - first[0];
  const int n1 = n0 + (ends[1] - first[1]);
  const int n2 = n1 + (ends[2] - first[2]);
  const bool first_round = TRIP > 0;
  const int total = first_round ? n2 + (ends[3] - first[3]) : 0;
  constexpr int kSlots = TRIP > 0 ? TRIP : 1;
  for (int j = 0; __any(j < total); j += kSlots) {
    int k[kSlots];
    bool present[kSlots];
    S q[kSlots][3];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const int jj = j + u;
      present[u] = jj < total;
      // position jj of the four runs laid end to end (selects, no branches)
      int at = first[3] + (jj - n2);
      at = jj < n2 ? first[2] + (jj - n1) : at;
      at = jj < n1 ? first[1] + (jj - n0) : at;
      at = jj < n0 ? first[0] + jj : at;
      k[u] = present[u] ? at : 0;  // (a trip is only made when some lane has a candidate)
    }
#pragma unroll
    for (int u = 0; u < kSlots; ++u) fetch(k[u], q[u]);
#pragma unroll
    for (int u = 0; u < kSlots; ++u) consider(q[u], k[u], present[u], std::true_type());
  }

  // Everything else lies across a far face of that block: only a lane whose best so far (or the
  // maximum distance, while it has none) reaches the nearest of the three goes on — at about one
  // target per cell and a source within half a cell of its target, none.
  const S far_x = (sx < 0 ? A.cell - fx : fx) - ex;
  const S far_y = (sy < 0 ? A.cell - fy : fy) - ey;
  const S far_z = (sz < 0 ? A.cell - fz : fz) - ez;
  const bool go = inside && (!first_round || within(sq(fmin(far_x, fmin(far_y, far_z)))));
  const int first_round_k = best_k;
  // Second round, in lock step too (round 5; rounds 3-4 walked the rows one after the other, each
  // lane under its running bound: fewer candidates per lane, but two dependent waits of the whole
  // wave for every row ANY of its lanes visited).  The rows of the (2 reach + 1)^2 block around the
  // own one are taken nine (then eight) at a time: every lane that goes on lists, under the bound
  // it has now, the stretch of cells of each row it still has to see — a stretch is consecutive in
  // storage: one candidate range, two bounds —, the 18 bounds are fetched together, and the wave
  // walks the stretches laid end to end four candidates per trip like the first round: one wait
  // for the bounds and one per trip, every lane that has something active in every trip.  A cell is
  // listed only if its box can hold something at least as close as what has been found (or within
  // the maximum distance while nothing has); the bound is taken from the own cell's faces and
  // tightens from one group of rows to the next.
  const S gx[2] = {fx - ex, (A.cell - fx) - ex};
  const S gy[2] = {fy - ey, (A.cell - fy) - ey};
  const S gz[2] = {fz - ez, (A.cell - fz) - ez};
  const int R = A.reach;
  auto gapAlong = [&](const S (&gap)[2], int d) {  // to the slab of cells d steps away
    return d == 0 ? S(0) : gap[d < 0 ? 0 : 1] + S((d < 0 ? -d : d) - 1) * A.cell;
  };
  // rows(r, dy, dz) names row r < 9 of the group (the same for every lane of the wave) or says there
  // is none; skip_block: the rows of the 2 x 2 x 2 block have only their far cell left (reach 1)
  auto walkRows = [&](bool active, auto rows, auto skip_block) {
    int at_a[9], at_b[9];
    bool some = false;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      int dy = 0, dz = 0;
      const bool valid = rows(r, dy, dz);
      const int y = c[1] + dy, z = c[2] + dz;
      const S yz = sq(gapAlong(gy, dy)) + sq(gapAlong(gz, dz));
      int left = 0, right = 0;
      for (int step = 0; step < R; ++step) {
        left += (left == step && within(yz + sq(gx[0] + S(step) * A.cell))) ? 1 : 0;
        right += (right == step && within(yz + sq(gx[1] + S(step) * A.cell))) ? 1 : 0;
      }
      bool ok = valid && active && within(yz) && y >= 0 && y < A.dims[1] && z >= 0 && z < A.dims[2];
      int xa = c[0] - left, xb = c[0] + right;
      if constexpr (decltype(skip_block)::value) {
        // cells c0 + sx and c0 + sx + 1 of a row of the block were candidates of the first round
        const bool in_block = first_round && (dy == sy || dy == sy + 1) && (dz == sz || dz == sz + 1);
        xa = in_block ? (sx < 0 ? c[0] + 1 : c[0] - 1) : xa;
        xb = in_block ? xa : xb;
        ok = ok && (!in_block || (sx < 0 ? right > 0 : left > 0));
      }
      xa = xa < 0 ? 0 : xa;
      xb = xb >= A.dims[0] ? A.dims[0] - 1 : xb;
      ok = ok && xa <= xb;
      some = some || ok;
      const int row = (z * A.dims[1] + y) * A.dims[0];
      at_a[r] = ok ? row + xa : 0;  // (entry 0 twice: an empty stretch)
      at_b[r] = ok ? row + xb + 1 : 0;
    }
    if (!__any(some)) return;
    int lo[9], upto[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      lo[r] = A.cell_start[at_a[r]];
      upto[r] = A.cell_start[at_b[r]];
    }
    upto[0] -= lo[0];  // upto[r]: the list position one past row r's last candidate
#pragma unroll
    for (int r = 1; r < 9; ++r) upto[r] = upto[r - 1] + (upto[r] - lo[r]);
    const int listed = upto[8];
    for (int j = 0; __any(j < listed); j += kIcpTrip) {
      int k[kIcpTrip];
      bool present[kIcpTrip];
      S q[kIcpTrip][3];
#pragma unroll
      for (int u = 0; u < kIcpTrip; ++u) {
        const int jj = j + u;
        present[u] = jj < listed;
        int at = lo[8] + (jj - upto[7]);
#pragma unroll
        for (int r = 7; r >= 1; --r) at = jj < upto[r] ? lo[r] + (jj - upto[r - 1]) : at;
        at = jj < upto[0] ? lo[0] + jj : at;
        k[u] = present[u] ? at : 0;
      }
#pragma unroll
      for (int u = 0; u < kIcpTrip; ++u) fetch(k[u], q[u]);
      // (distance and position only: the coordinates of a winner found here are read once, at the end)
#pragma unroll
      for (int u = 0; u < kIcpTrip; ++u) consider(q[u], k[u], present[u], std::false_type());
    }
  };
  if (__any(go)) {
    // the own row and the ring of eight around it
    auto inner = [](int r, int &dy, int &dz) {
      dy = r % 3 - 1;
      dz = r / 3 - 1;
      return true;
    };
    if (R == 1) {
      walkRows(go, inner, std::true_type());
    } else {
      // Cells finer than the radius (icp.cpp picks them so where the targets are dense): after the
      // inner nine rows the rings further out, eight rows at a time, counter-clockwise from each
      // ring's (-ring, -ring) corner.  A lane is done once a ring's nearest face is out of its reach;
      // the walk ends when every lane is.  (Ring and row counters are the same for all lanes.)
      walkRows(go, inner, std::false_type());
      // (further out fewer and fewer lanes admit anything, and what they admit depends on what the
      // rows before have found: past ring A.lock_rings the rows are walked one after the other under
      // the running bound, the form of rounds 3-4 — a wave skips a row none of its lanes admits)
      auto visit = [&](int y, int z, int xa, int xb) {
        xa = xa < 0 ? 0 : xa;
        xb = xb >= A.dims[0] ? A.dims[0] - 1 : xb;
        if (z < 0 || z >= A.dims[2] || y < 0 || y >= A.dims[1] || xa > xb) return;
        const int row = (z * A.dims[1] + y) * A.dims[0];
        const int lo = A.cell_start[row + xa], hi = A.cell_start[row + xb + 1];
        for (int k = lo; k < hi; k += 2) {  // two candidates per step, both loads issued before either is used
          S qa[3], qb[3];
          const bool pair = k + 1 < hi;
          fetch(k, qa);
          fetch(pair ? k + 1 : k, qb);
          consider(qa, k, true, std::false_type());
          consider(qb, k + 1, pair, std::false_type());
        }
      };
      bool walking = go;
      for (int ring = 2; ring <= R; ++ring) {
        const S nearest = fmin(fmin(gapAlong(gy, -ring), gapAlong(gy, ring)),
                               fmin(gapAlong(gz, -ring), gapAlong(gz, ring)));
        walking = walking && within(sq(nearest));
        if (!__any(walking)) break;
        if (ring > A.lock_rings) {
          for (int u = 0; u < 8 * ring; ++u) {
            const int side = u / (2 * ring), along = u % (2 * ring);
            const int dy = side == 0 ? -ring + along : side == 1 ? ring : side == 2 ? ring - along : -ring;
            const int dz = side == 0 ? -ring : side == 1 ? -ring + along : side == 2 ? ring : ring - along;
            const S yz = sq(gapAlong(gy, dy)) + sq(gapAlong(gz, dz));
            if (!(walking && within(yz))) continue;
            int left = 0, right = 0;
            for (int step = 0; step < R; ++step) {
              left += (left == step && within(yz + sq(gx[0] + S(step) * A.cell))) ? 1 : 0;
              right += (right == step && within(yz + sq(gx[1] + S(step) * A.cell))) ? 1 : 0;
            }
            visit(c[1] + dy, c[2] + dz, c[0] - left, c[0] + right);
          }
          continue;
        }
        for (int base = 0; base < 8 * ring; base += 8) {
          auto outer = [&](int r, int &dy, int &dz) {
            const int u = base + r;
            const int side = u / (2 * ring), along = u % (2 * ring);
            dy = side == 0 ? -ring + along : side == 1 ? ring : side == 2 ? ring - along : -ring;
            dz = side == 0 ? -ring : side == 1 ? -ring + along : side == 2 ? ring : ring - along;
            return r < 8;
          };
          walkRows(walking, outer, std::false_type());
        }
      }
    }
  }
  if (go && best_k != first_round_k) fetch(best_k, best);
  const S nan = S(__builtin_nan(""));
  slot[3 * TP] = found ? best[0] : nan;
  slot[4 * TP] = found ? best[1] : nan;
  slot[5 * TP] = found ? best[2] : nan;
  // How many sources found a target: every wave leaves its count in a slot of its own and the
  // publishing kernel adds the slots — no atomics (15.6 k of them on one address, one per wave,
  // take 178 us at 1 M; one per workgroup behind a barrier made the search 57.6 us instead of 44.4).
  if (A.matched) {
    const unsigned long long in_wave = __ballot(found);
    if ((threadIdx.x & 63) == 0)
      A.matched[(size_t)blockIdx.x * (kBlockThreads / 64) + threadIdx.x / 64] =
          (unsigned int)__popcll(in_wave);
  }
}

template <typename S, int TRIP>
__global__ __launch_bounds__(kBlockThreads) void icpMatchKernel(const IcpMatchArgs<S> A) {
  icpMatchBody<S, TRIP>(A, A.T);
}

// Resident form for the device-resident LM: the pose comes from the cost's sweep constants in HBM
// (T at the point the step kernel has just proposed), and the search only runs when the step
// kernel asked for it — the model's update(x) at the top of an outer iteration
// (levenberg_marquadt_dyn.cpp:54) — or not at all once the loop has stopped.
template <typename S, int TRIP>
__global__ __launch_bounds__(kBlockThreads) void icpMatchResidentKernel(
    const IcpMatchArgs<S> A, const P2PSweepArgs<S> *__restrict__ d_args,
    const LmControl *__restrict__ control) {
  if (control->done || !control->pad[1]) return;
  S T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = d_args->T[0][k];
  icpMatchBody<S, TRIP>(A, T);
}

// the target of slot i as a packed triple: to position i, or to position order[i] (the caller's
// index of the source in that slot: an ICP cost keeps its sources in cell order)
template <typename S>
__global__ void gatherTargetsKernel(const S *__restrict__ tiles, long long count,
                                    const int *__restrict__ order, S *__restrict__ out_xyz) {
  constexpr int TP = TileShape<S>::kPoints;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const S *slot = tiles + (i / TP) * TileShape<S>::kP2PScalars + (i % TP);
  const long long to = order ? order[i] : i;
#pragma unroll
  for (int k = 0; k < 3; ++k) out_xyz[3 * to + k] = slot[(3 + k) * TP];
}

}  // namespace

// ---- host-side launch wrappers -----------------------------------------------------------------
// MOPT_ICP_FIRST_ROUND=0: the row-by-row search alone (measurements: scripts/icp_offsets_timing.py)
static bool icpFirstRound() {
  static const bool on = [] {
    const char *v = getenv("MOPT_ICP_FIRST_ROUND");
    return !(v && v[0] == '0');
  }();
  return on;
}

template <typename S>
hipError_t launchIcpMatch(const IcpMatchArgs<S> &args, hipStream_t stream) {
  const long long padded = (long long)args.num_tiles * TileShape<S>::kPoints;
  if (padded == 0) return hipSuccess;
  const unsigned blocks = unsigned((padded + kBlockThreads - 1) / kBlockThreads);
  if (icpFirstRound())
    hipLaunchKernelGGL((icpMatchKernel<S, kIcpTrip>), dim3(blocks), dim3(kBlockThreads), 0, stream, args);
  else
    hipLaunchKernelGGL((icpMatchKernel<S, 0>), dim3(blocks), dim3(kBlockThreads), 0, stream, args);
  return hipGetLastError();
}
template hipError_t launchIcpMatch<float>(const IcpMatchArgs<float> &, hipStream_t);
template hipError_t launchIcpMatch<double>(const IcpMatchArgs<double> &, hipStream_t);

template <typename S>
hipError_t launchIcpMatchResident(const IcpMatchArgs<S> &args, const P2PSweepArgs<S> *d_args,
                                  const LmControl *control, hipStream_t stream) {
  const long long padded = (long long)args.num_tiles * TileShape<S>::kPoints;
  if (padded == 0) return hipSuccess;
  const unsigned blocks = unsigned((padded + kBlockThreads - 1) / kBlockThreads);
  hipLaunchKernelGGL((icpMatchResidentKernel<S, kIcpTrip>), dim3(blocks), dim3(kBlockThreads), 0, stream, args,
                     d_args, control);
  return hipGetLastError();
}
template hipError_t launchIcpMatchResident<float>(const IcpMatchArgs<float> &,
                                                  const P2PSweepArgs<float> *, const LmControl *,
                                                  hipStream_t);
template hipError_t launchIcpMatchResident<double>(const IcpMatchArgs<double> &,
                                                   const P2PSweepArgs<double> *, const LmControl *,
                                                   hipStream_t);

template <typename S>
hipError_t launchGatherTargets(const S *tiles, long long count, const int *order, S *out_xyz,
                               hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const unsigned blocks = unsigned((count + 255) / 256);
  hipLaunchKernelGGL((gatherTargetsKernel<S>), dim3(blocks), dim3(256), 0, stream, tiles, count,
                     order, out_xyz);
  return hipGetLastError();
}
template hipError_t launchGatherTargets<float>(const float *, long long, const int *, float *,
                                               hipStream_t);
template hipError_t launchGatherTargets<double>(const double *, long long, const int *, double *,
                                                hipStream_t);

// matched sources of the correspondence search: the per-wave counts (icpMatchBody) added up and
// handed to mapped host memory as one double — no memset launch, no copy, no stream synchronisation
__global__ __launch_bounds__(1024) void publishCounterKernel(const unsigned int *wave_counts,
                                                             long long num_waves,
                                                             const HostPublish pub) {
  __shared__ unsigned long long per_wave[16];
  // (16-byte loads, all of a thread's requested before the first is added: 15.6 k counts of a
  // 1 M search are four loads per thread, one round trip)
  unsigned long long sum = 0;
  const long long quads = num_waves / 4;
  const uint4 *counts4 = reinterpret_cast<const uint4 *>(wave_counts);
  for (long long k = threadIdx.x; k < quads; k += 4 * blockDim.x) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long at = k + u * (long long)blockDim.x;
      v[u] = counts4[at < quads ? at : k];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k + u * (long long)blockDim.x < quads) sum += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  }
  if (threadIdx.x < num_waves - quads * 4) sum += wave_counts[quads * 4 + threadIdx.x];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
  if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x / 64] = sum;
  __syncthreads();
  double v = 0.0;
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int k = 0; k < int(blockDim.x) / 64; ++k) total += per_wave[k];
    v = double(total);
  }
  publishToHost(pub, 1, v);
}

hipError_t launchPublishCounter(const unsigned int *d_wave_counts, long long num_waves,
                                const HostPublish &pub, hipStream_t stream) {
  hipLaunchKernelGGL(publishCounterKernel, dim3(1), dim3(1024), 0, stream, d_wave_counts, num_waves,
                     pub);
  return hipGetLastError();
}

}  // namespace mopt
