// Voxel-grid downsampling (mopt_cloud_voxel_downsample, cloud.cpp): the device half that follows the
// sort of cell_order.hip.  The points arrive as a permutation in (voxel id, caller's index) order with
// their sorted keys; what is done here is the segmented reduction of that order into one centroid per
// occupied voxel:
//   voxelHeadFlagsKernel   flag[k] = key[k] != key[k-1]; after the exclusive scan (exclusiveScan)
//                          flag[k] is the number of voxels that begin before position k
//   voxelCentroidKernel    every wave walks 8 x 64 consecutive positions; per 64 a segmented Hillis-
//                          Steele scan over the lanes (six shuffle steps on x, y, z in fp64 and the count),
//                          the sum left open by lane 63 carried in registers into the next 64.  A voxel
//                          that begins and ends inside the wave's 512 positions is divided and stored by the
//                          lane that holds its last point.  The piece in front of the wave's first head and
//                          the piece behind its last one go to LDS, where one thread joins the four waves'
//                          pieces in wave order: a voxel closed inside the workgroup's 2048 positions is
//                          stored, the tile's own first and last open pieces go to its carry record
//   voxelFoldKernel        one thread per tile whose last piece is open: adds the first pieces of the
//                          tiles behind it, in tile order, up to the one that closes the voxel
// Every sum is taken in an order fixed by the positions alone (lane tree, then rounds, waves and tiles
// in ascending order): no atomics, so two calls give the same bits.  A voxel of any population costs
// the same per point; only the fold walks serially, one 64-byte record per 2048 points of the voxel.
// (The reference has no counterpart: model.h:24-26 leaves correspondences and all that precedes them to
// the user.)
#include <hip/hip_runtime.h>

#include "sweep.hpp"

namespace mopt {
namespace {

constexpr int kVoxelRounds = 8;                            // times 64 positions per wave
constexpr int kVoxelWaveSpan = 64 * kVoxelRounds;          // positions per wave
constexpr int kVoxelTile = kBlockThreads * kVoxelRounds;   // positions per workgroup
constexpr int kVoxelWaves = kBlockThreads / 64;

struct VoxelSum {
  double x, y, z;
  int n;
};

__device__ __forceinline__ VoxelSum voxelZero() { return VoxelSum{0.0, 0.0, 0.0, 0}; }
__device__ __forceinline__ VoxelSum voxelAdd(const VoxelSum &a, const VoxelSum &b) {
  return VoxelSum{a.x + b.x, a.y + b.y, a.z + b.z, a.n + b.n};
}
__device__ __forceinline__ VoxelSum voxelFromLane(const VoxelSum &v, int lane) {
  return VoxelSum{__shfl(v.x, lane, 64), __shfl(v.y, lane, 64), __shfl(v.z, lane, 64),
                  __shfl(v.n, lane, 64)};
}

// a tile's pieces of the voxels that cross its edges (64 bytes)
struct VoxelCarry {
  double first[3];          // sum in front of the tile's first head ...
  double last[3];           // ... and from its last head on, where that voxel is still open at the end
  int first_n, last_n;      // their populations; 0: no such piece
  int first_closed;         // the first piece's voxel ends inside this tile
  unsigned int last_voxel;  // output row of the last piece's voxel
};
static_assert(sizeof(VoxelCarry) == 64, "one record, one 64-byte line");

// what a wave leaves for the workgroup's join
struct VoxelWavePieces {
  VoxelSum first, last;
  int first_closed, seen_head;
  unsigned int last_voxel;
};

template <typename S>
__device__ __forceinline__ void voxelStore(S *out_xyz, int32_t *out_counts, unsigned int voxel,
                                           const VoxelSum &s) {
  const double n = double(s.n);
  out_xyz[3 * size_t(voxel) + 0] = S(s.x / n);  // (the one rounding to the scalar type)
  out_xyz[3 * size_t(voxel) + 1] = S(s.y / n);
  out_xyz[3 * size_t(voxel) + 2] = S(s.z / n);
  if (out_counts) out_counts[voxel] = s.n;
}

// flags[0 .. kept]: 1 where a voxel begins; flags[kept] = 0, so that the scan leaves the total there
__global__ __launch_bounds__(kBlockThreads) void voxelHeadFlagsKernel(const unsigned int *keys,
                                                                      long long kept,
                                                                      unsigned int *flags) {
  const long long k = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
  if (k > kept) return;
  flags[k] = (k < kept && (k == 0 || keys[k] != keys[k - 1])) ? 1u : 0u;
}

template <typename S>
__global__ __launch_bounds__(kBlockThreads) void voxelCentroidKernel(
    const S *__restrict__ xyz, const int *__restrict__ perm, const unsigned int *__restrict__ keys,
    const unsigned int *__restrict__ voxels_before, long long kept, S *__restrict__ out_xyz,
    int32_t *__restrict__ out_counts, VoxelCarry *__restrict__ carry) {
  __shared__ VoxelWavePieces pieces[kVoxelWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long wave_base = (long long)blockIdx.x * kVoxelTile + (long long)wave * kVoxelWaveSpan;
  // wave-uniform: the sum running into the next 64 positions, whether a head has been met, whether
  // the piece in front of the first head has been closed, the output row at the last position
  VoxelSum open = voxelZero();
  bool seen_head = false, first_closed = false;
  unsigned int last_voxel = 0;
  for (int r = 0; r < kVoxelRounds; ++r) {
    const long long k = wave_base + r * 64 + lane;
    const bool valid = k < kept;
    const unsigned int key = valid ? keys[k] : 0u;
    // (the position behind the last point is a head too: the zeros behind it form a piece of their
    // own, of population 0, which nothing stores)
    const bool head = valid ? (k == 0 || keys[k - 1] != key) : (k == kept);
    const bool tail = valid && (k + 1 >= kept || keys[k + 1] != key);
    VoxelSum v = voxelZero();
    unsigned int voxel = 0;
    if (valid) {
      const long long from = perm[k];
      v.x = double(xyz[3 * from + 0]);
      v.y = double(xyz[3 * from + 1]);
      v.z = double(xyz[3 * from + 2]);
      v.n = 1;
      voxel = voxels_before[k] + (head ? 1u : 0u) - 1u;
    }
    // inclusive segmented scan over the 64 lanes: v = sum from the lane's head (or lane 0) to the lane,
    // f = a head lies in [0, lane]
    int f = head ? 1 : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double ux = __shfl_up(v.x, off, 64), uy = __shfl_up(v.y, off, 64),
                   uz = __shfl_up(v.z, off, 64);
      const int un = __shfl_up(v.n, off, 64), uf = __shfl_up(f, off, 64);
      if (lane >= off) {
        if (!f) {
          v.x += ux;
          v.y += uy;
          v.z += uz;
          v.n += un;
        }
        f |= uf;
      }
    }
    const VoxelSum total = f ? v : voxelAdd(open, v);
    const bool closes_first = tail && !f && !seen_head;  // the voxel that ran into this wave ends here
    if (closes_first) {
      pieces[wave].first = total;
    } else if (tail) {
      voxelStore<S>(out_xyz, out_counts, voxel, total);
    }
    first_closed = first_closed || __any(closes_first ? 1 : 0);
    const bool tail63 = __shfl(tail ? 1 : 0, 63, 64) != 0;
    open = tail63 ? voxelZero() : voxelFromLane(total, 63);
    seen_head = seen_head || __shfl(f, 63, 64) != 0;
    last_voxel = __shfl(voxel, 63, 64);
  }
  if (lane == 0) {
    if (!first_closed) pieces[wave].first = seen_head ? voxelZero() : open;  // no head: all 512 positions
    pieces[wave].first_closed = first_closed ? 1 : 0;
    pieces[wave].seen_head = seen_head ? 1 : 0;
    pieces[wave].last = seen_head ? open : voxelZero();
    pieces[wave].last_voxel = last_voxel;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // the four waves' pieces in wave order
  VoxelSum tile_first = voxelZero(), run = voxelZero();
  bool in_first = true;  // still in front of the tile's first head
  int tile_first_closed = 0;
  unsigned int run_voxel = 0;
  for (int w = 0; w < kVoxelWaves; ++w) {
    const VoxelWavePieces p = pieces[w];
    if (p.first.n > 0) {
      if (in_first) tile_first = voxelAdd(tile_first, p.first);
      else run = voxelAdd(run, p.first);
      if (p.first_closed) {
        if (in_first) {
          tile_first_closed = 1;
          in_first = false;
        } else {
          voxelStore<S>(out_xyz, out_counts, run_voxel, run);
          run = voxelZero();
        }
      }
    }
    if (p.seen_head) in_first = false;
    if (p.last.n > 0) {
      run = p.last;
      run_voxel = p.last_voxel;
    }
  }
  VoxelCarry c;
  c.first[0] = tile_first.x, c.first[1] = tile_first.y, c.first[2] = tile_first.z;
  c.last[0] = run.x, c.last[1] = run.y, c.last[2] = run.z;
  c.first_n = tile_first.n;
  c.last_n = run.n;
  c.first_closed = tile_first_closed;
  c.last_voxel = run_voxel;
  carry[blockIdx.x] = c;
}

template <typename S>
__global__ __launch_bounds__(kBlockThreads) void voxelFoldKernel(const VoxelCarry *__restrict__ carry,
                                                                 int num_tiles, S *__restrict__ out_xyz,
                                                                 int32_t *__restrict__ out_counts) {
  const int t = blockIdx.x * kBlockThreads + threadIdx.x;
  if (t >= num_tiles || carry[t].last_n == 0) return;
  VoxelSum acc{carry[t].last[0], carry[t].last[1], carry[t].last[2], carry[t].last_n};
  for (int u = t + 1; u < num_tiles; ++u) {
    const VoxelCarry c = carry[u];
    acc = voxelAdd(acc, VoxelSum{c.first[0], c.first[1], c.first[2], c.first_n});
    if (c.first_closed) break;
  }
  voxelStore<S>(out_xyz, out_counts, carry[t].last_voxel, acc);
}

inline int voxelTiles(long long kept) { return int((kept + kVoxelTile - 1) / kVoxelTile); }

}  // namespace

hipError_t launchVoxelHeadFlags(const unsigned int *d_sorted_keys, long long kept,
                                unsigned int *d_flags, hipStream_t stream) {
  const unsigned blocks = unsigned((kept + 1 + kBlockThreads - 1) / kBlockThreads);
  hipLaunchKernelGGL(voxelHeadFlagsKernel, dim3(blocks), dim3(kBlockThreads), 0, stream, d_sorted_keys,
                     kept, d_flags);
  return hipGetLastError();
}

size_t voxelCarryBytes(long long kept) { return size_t(voxelTiles(kept)) * sizeof(VoxelCarry); }

template <typename S>
hipError_t launchVoxelCentroids(const S *d_xyz, const int *d_perm, const unsigned int *d_sorted_keys,
                                const unsigned int *d_voxels_before, long long kept, S *d_out_xyz,
                                int32_t *d_out_counts, void *d_carry, hipStream_t stream) {
  if (kept <= 0) return hipSuccess;
  const int tiles = voxelTiles(kept);
  hipLaunchKernelGGL(voxelCentroidKernel<S>, dim3(tiles), dim3(kBlockThreads), 0, stream, d_xyz, d_perm,
                     d_sorted_keys, d_voxels_before, kept, d_out_xyz, d_out_counts,
                     static_cast<VoxelCarry *>(d_carry));
  hipLaunchKernelGGL(voxelFoldKernel<S>, dim3((tiles + kBlockThreads - 1) / kBlockThreads),
                     dim3(kBlockThreads), 0, stream, static_cast<const VoxelCarry *>(d_carry), tiles,
                     d_out_xyz, d_out_counts);
  return hipGetLastError();
}

template hipError_t launchVoxelCentroids<double>(const double *, const int *, const unsigned int *,
                                                 const unsigned int *, long long, double *, int32_t *,
                                                 void *, hipStream_t);
template hipError_t launchVoxelCentroids<float>(const float *, const int *, const unsigned int *,
                                                const unsigned int *, long long, float *, int32_t *,
                                                void *, hipStream_t);

}  // namespace mopt
