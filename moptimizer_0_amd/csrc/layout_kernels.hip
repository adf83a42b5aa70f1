// gfx950 kernels that run once per data set, when a cost is constructed (cost.cpp): the caller's
// arrays into the tile layout the sweeps stream (sweep.hpp), and the bounding box of the sources.
#include "sweep.hpp"

namespace mopt {
namespace {

// ---- layout conversion (once per data set) -----------------------------------------------------
template <typename S>
__global__ void relayoutP2PKernel(const S *__restrict__ src, const S *__restrict__ tgt,
                                  long long count, S *__restrict__ tiles, long long padded) {
  constexpr int TP = TileShape<S>::kPoints;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= padded) return;
  const long long tile = i / TP;
  const int within = int(i % TP);
  S *dst = tiles + tile * TileShape<S>::kP2PScalars + within;
  const bool valid = i < count;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dst[k * TP] = valid ? src[3 * i + k] : S(0);
    dst[(3 + k) * TP] = valid ? tgt[3 * i + k] : S(0);
  }
}

// Bounding box of the sources, once per data set: the scale the choice between the moments and the
// literal evaluation depends on (sweep_choice.hpp leftBasisCancels, hasSmallForwardStep).  Every index is below
// `count`, so inside the tiles; a wavefront reduces with shuffles and its first lane takes the six
// atomics on ordered keys (sweep.hpp sourceBoxKey).
template <typename S>
__global__ __launch_bounds__(256) void sourceBoxKernel(const S *__restrict__ tiles, long long count,
                                                       unsigned long long *__restrict__ box) {
  constexpr int TP = TileShape<S>::kPoints;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const S *slot = tiles + (i / TP) * TileShape<S>::kP2PScalars + (i % TP);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = double(slot[k * TP]);
      lo[k] = fmin(lo[k], v);
      hi[k] = fmax(hi[k], v);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], off));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], off));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicMin(&box[k], sourceBoxKey(lo[k]));
      atomicMax(&box[3 + k], sourceBoxKey(hi[k]));
    }
  }
}

// ---- a batch of small problems (mopt_batch) ------------------------------------------------------
// The problem that owns `tile`: the last i with first_tile[i] <= tile (every problem has a tile).
__device__ __forceinline__ int problemOfTile(const int *__restrict__ first_tile, int num_problems, int tile) {
  int lo = 0, hi = num_problems - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first_tile[mid] <= tile) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One workgroup per tile of the batch: the tile's problem by bisection (uniform: scalar loads), then
// relayoutP2PKernel's copy with the slot index counted from the problem's first correspondence; the
// tail of each problem's last tile is zero-filled.
template <typename S>
__global__ __launch_bounds__(256) void relayoutP2PBatchKernel(const S *__restrict__ src, const S *__restrict__ tgt,
                                                              const long long *__restrict__ offsets,
                                                              const int *__restrict__ first_tile,
                                                              int num_problems, S *__restrict__ tiles) {
  constexpr int TP = TileShape<S>::kPoints;
  const int tile = blockIdx.x;
  const int problem = problemOfTile(first_tile, num_problems, tile);
  const long long begin = offsets[problem];
  const long long count = offsets[problem + 1] - begin;
  const long long tile_first = (long long)(tile - first_tile[problem]) * TP;
  S *dst_tile = tiles + size_t(tile) * TileShape<S>::kP2PScalars;
  for (int within = threadIdx.x; within < TP; within += blockDim.x) {
    const long long local = tile_first + within;
    const bool valid = local < count;
    const long long i = begin + (valid ? local : 0);  // (a problem is never empty)
    S *dst = dst_tile + within;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dst[k * TP] = valid ? src[3 * i + k] : S(0);
      dst[(3 + k) * TP] = valid ? tgt[3 * i + k] : S(0);
    }
  }
}

// One workgroup per problem (at most four tiles): the minima and maxima sourceBoxKernel finds for a
// cost, reduced within the workgroup and written as doubles — no atomics, nothing to initialise.
template <typename S>
__global__ __launch_bounds__(256) void sourceBoxBatchKernel(const S *__restrict__ tiles,
                                                            const long long *__restrict__ offsets,
                                                            const int *__restrict__ first_tile,
                                                            double *__restrict__ boxes) {
  constexpr int TP = TileShape<S>::kPoints;
  const int problem = blockIdx.x;
  const long long count = offsets[problem + 1] - offsets[problem];
  const S *base = tiles + size_t(first_tile[problem]) * TileShape<S>::kP2PScalars;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long i = threadIdx.x; i < count; i += blockDim.x) {
    const S *slot = base + (i / TP) * TileShape<S>::kP2PScalars + (i % TP);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = double(slot[k * TP]);
      lo[k] = fmin(lo[k], v);
      hi[k] = fmax(hi[k], v);
    }
  }
  __shared__ double wave_box[4][6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], off));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], off));
    }
    if ((threadIdx.x & 63) == 0) {
      wave_box[threadIdx.x >> 6][k] = lo[k];
      wave_box[threadIdx.x >> 6][3 + k] = hi[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    double v = wave_box[0][k];
    for (int w = 1; w < 4; ++w) v = k < 3 ? fmin(v, wave_box[w][k]) : fmax(v, wave_box[w][k]);
    boxes[size_t(problem) * 6 + k] = v;
  }
}

__global__ void relayoutReprojKernel(const double *__restrict__ pts, const int *__restrict__ pix,
                                     long long count, unsigned char *__restrict__ tiles,
                                     long long padded) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= padded) return;
  const long long tile = i / kReprojTilePoints;
  const int within = int(i % kReprojTilePoints);
  unsigned char *tb = tiles + tile * kReprojTileBytes;
  double *planes = reinterpret_cast<double *>(tb);
  int *pixels = reinterpret_cast<int *>(tb + size_t(4) * kReprojTilePoints * 8);
  // the tail of the last tile repeats the last element: whatever the sweep computes for a padded slot
  // is then as finite as for a real one, and a weight of zero is enough to leave it out (an all-zero
  // point projects to 0 / 0)
  const long long from = i < count ? i : count - 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) planes[k * kReprojTilePoints + within] = pts[4 * from + k];
  pixels[2 * within + 0] = pix[2 * from + 0];
  pixels[2 * within + 1] = pix[2 * from + 1];
}

}  // namespace

// ---- host-side launch wrappers -----------------------------------------------------------------
template <typename S>
hipError_t launchRelayoutP2P(const S *src_xyz, const S *tgt_xyz, long long count, S *tiles,
                             int num_tiles, hipStream_t stream) {
  const long long padded = (long long)num_tiles * TileShape<S>::kPoints;
  if (padded == 0) return hipSuccess;
  const unsigned blocks = unsigned((padded + 255) / 256);
  hipLaunchKernelGGL((relayoutP2PKernel<S>), dim3(blocks), dim3(256), 0, stream, src_xyz, tgt_xyz,
                     count, tiles, padded);
  return hipGetLastError();
}
template hipError_t launchRelayoutP2P<float>(const float *, const float *, long long, float *, int,
                                             hipStream_t);
template hipError_t launchRelayoutP2P<double>(const double *, const double *, long long, double *,
                                              int, hipStream_t);

template <typename S>
hipError_t launchRelayoutP2PBatch(const S *src_xyz, const S *tgt_xyz, const long long *offsets,
                                  const int *first_tile, int num_problems, int total_tiles, S *tiles,
                                  hipStream_t stream) {
  if (num_problems < 1 || total_tiles < num_problems) return hipErrorInvalidValue;
  hipLaunchKernelGGL((relayoutP2PBatchKernel<S>), dim3(total_tiles), dim3(256), 0, stream, src_xyz, tgt_xyz,
                     offsets, first_tile, num_problems, tiles);
  return hipGetLastError();
}
template hipError_t launchRelayoutP2PBatch<float>(const float *, const float *, const long long *,
                                                  const int *, int, int, float *, hipStream_t);
template hipError_t launchRelayoutP2PBatch<double>(const double *, const double *, const long long *,
                                                   const int *, int, int, double *, hipStream_t);

template <typename S>
hipError_t launchSourceBoxBatch(const S *tiles, const long long *offsets, const int *first_tile,
                                int num_problems, double *boxes, hipStream_t stream) {
  if (num_problems < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sourceBoxBatchKernel<S>), dim3(num_problems), dim3(256), 0, stream, tiles, offsets,
                     first_tile, boxes);
  return hipGetLastError();
}
template hipError_t launchSourceBoxBatch<float>(const float *, const long long *, const int *, int,
                                                double *, hipStream_t);
template hipError_t launchSourceBoxBatch<double>(const double *, const long long *, const int *, int,
                                                 double *, hipStream_t);

template <typename S>
hipError_t launchSourceBox(const S *tiles, long long count, unsigned long long *d_box, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(d_box, 0xff, 3 * sizeof(unsigned long long), stream);  // minima: the largest key
  if (e == hipSuccess) e = hipMemsetAsync(d_box + 3, 0, 3 * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  const long long wanted = (count + 255) / 256;
  const unsigned blocks = unsigned(wanted < 1024 ? wanted : 1024);
  hipLaunchKernelGGL((sourceBoxKernel<S>), dim3(blocks), dim3(256), 0, stream, tiles, count, d_box);
  return hipGetLastError();
}
template hipError_t launchSourceBox<float>(const float *, long long, unsigned long long *, hipStream_t);
template hipError_t launchSourceBox<double>(const double *, long long, unsigned long long *, hipStream_t);

hipError_t launchRelayoutReproj(const double *points_xyzw, const int32_t *pixels_uv,
                                long long count, unsigned char *tiles, int num_tiles,
                                hipStream_t stream) {
  const long long padded = (long long)num_tiles * kReprojTilePoints;
  if (padded == 0) return hipSuccess;
  const unsigned blocks = unsigned((padded + 255) / 256);
  hipLaunchKernelGGL(relayoutReprojKernel, dim3(blocks), dim3(256), 0, stream, points_xyzw,
                     pixels_uv, count, tiles, padded);
  return hipGetLastError();
}

}  // namespace mopt
