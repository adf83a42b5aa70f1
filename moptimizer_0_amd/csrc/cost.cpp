// Cost lifetime and configuration: the stream pool, what every create call shares, the wait for a
// cost's queued work, destruction, the staging of host inputs, the four mopt_*_create calls,
// mopt_point2point_set_data and the loss / covariance / kernel-variant setters.
#include "cost_state.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>

using namespace mopt_detail;

namespace mopt_detail {

namespace {
std::mutex g_stream_pool_mutex;
std::map<int, std::vector<hipStream_t>> g_stream_pool;
}  // namespace

hipError_t acquireStream(int device, hipStream_t *out) {
  {
    std::lock_guard<std::mutex> lock(g_stream_pool_mutex);
    auto &pool = g_stream_pool[device];
    if (!pool.empty()) {
      *out = pool.back();
      pool.pop_back();
      return hipSuccess;
    }
  }
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);  // current device == `device`
}

void releaseStream(int device, hipStream_t stream) {
  if (!stream) return;
  std::lock_guard<std::mutex> lock(g_stream_pool_mutex);
  g_stream_pool[device].push_back(stream);
}

void storeResult(const mopt_cost *c, const double *res, void *hessian, void *b, void *sum_sq) {
  const int n = c->n_params, nn = n * n;
  if (c->scalar_bytes == 8) {
    if (hessian) std::memcpy(hessian, res, nn * sizeof(double));
    if (b) std::memcpy(b, res + nn, n * sizeof(double));
    if (sum_sq) *static_cast<double *>(sum_sq) = res[nn + n];
  } else {
    if (hessian)
      for (int k = 0; k < nn; ++k) static_cast<float *>(hessian)[k] = float(res[k]);
    if (b)
      for (int k = 0; k < n; ++k) static_cast<float *>(b)[k] = float(res[nn + k]);
    if (sum_sq) *static_cast<float *>(sum_sq) = float(res[nn + n]);
  }
}

int selectDevice(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MOPT_ERR_NO_DEVICE, "no HIP device is visible to this process");
  if (device < 0 || device >= ndev)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "device index out of range");
  MOPT_HIP_TRY(hipSetDevice(device));
  return MOPT_OK;
}

int commonCreate(mopt_cost *c, int device) {
  if (const int rc = selectDevice(device)) return rc;
  c->device = device;
  hipDeviceProp_t prop;
  MOPT_HIP_TRY(hipGetDeviceProperties(&prop, device));
  c->num_cus = prop.multiProcessorCount;
  c->max_grid = c->num_cus * 16;
  MOPT_HIP_TRY(acquireStream(device, &c->stream));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&c->d_partials),
                         size_t(c->max_grid) * kPartialRowSlots * sizeof(double)));
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&c->d_result), kResultSlots * sizeof(double)));
  // results (43) + padding + flag word in one mapped, coherent host allocation
  MOPT_HIP_TRY(mappedHostAlloc(reinterpret_cast<void **>(&c->h_result),
                               (kResultSlots + 16) * sizeof(double)));
  std::memset(c->h_result, 0, (kResultSlots + 16) * sizeof(double));
  c->h_flag = reinterpret_cast<unsigned long long *>(c->h_result + kResultSlots);
  MOPT_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->h_result_dev), c->h_result, 0));
  c->h_flag_dev = reinterpret_cast<unsigned long long *>(c->h_result_dev + kResultSlots);
  // counted as a user of the device's direct-dispatch queues (aql.hpp; created when a cost first takes that path)
  c->aql_retained = mopt_detail::aqlRetain(device);
  return MOPT_OK;
}

hipError_t quiesceCost(mopt_cost *c) {
  hipError_t first = hipSuccess;
  if (c->aql_touched && c->aql_queue) {  // the finalize kernel of the last direct sweep may still be retiring
    (void)mopt_detail::aqlDrain(c->aql_queue);
    c->aql_touched = false;
  }
  if (c->aql_queue) mopt_detail::aqlForgetStamp(c->aql_queue, c);  // (a timed dispatch nobody collected)
  c->aql_timed = false;
  if (c->stream) first = hipStreamSynchronize(c->stream);
  c->hip_pending = false;
  c->own_async_pending = false;
  if (c->foreign_pending && c->foreign_done) {
    const hipError_t e = hipEventSynchronize(c->foreign_done);
    if (first == hipSuccess) first = e;
    c->foreign_pending = false;
  }
  return first;
}

void destroyCost(mopt_cost *c) {
  if (!c) return;
  for (mopt_cost *s : c->siblings)
    s->siblings.erase(std::remove(s->siblings.begin(), s->siblings.end(), c), s->siblings.end());
  c->siblings.clear();
  (void)hipSetDevice(c->device);
  (void)quiesceCost(c);
  if (c->foreign_done) (void)hipEventDestroy(c->foreign_done);
  for (auto &pr : c->pending_events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  for (auto e : c->free_events) (void)hipEventDestroy(e);
  if (c->comm) ncclCommDestroy(c->comm);
  c->comm = nullptr;
  releaseCombine(c);
  if (c->matcher) {
    deviceRelease(c->matcher->d_sorted);
    deviceRelease(c->matcher->d_cell_start);
    deviceRelease(c->matcher->d_matched);
    deviceRelease(c->matcher->d_order);
  }
  mopt::jitRelease(c->jit);
  releaseResident(c);
  deviceRelease(c->d_tiles);
  deviceRelease(c->d_partials);
  deviceRelease(c->d_result);
  mappedHostRelease(c->device, c->h_result, (kResultSlots + 16) * sizeof(double));
  releaseStream(c->device, c->stream);  // synchronised at the top of this function
  if (c->aql_retained) mopt_detail::aqlRelease(c->device);
  delete c;
}

namespace {
constexpr size_t kBounceBytes = size_t(8) << 20;
std::mutex g_bounce_mutex;
void *g_bounce = nullptr;  // pinned, allocated on first use, kept for the life of the process
}  // namespace

Staging::~Staging() {
  if (!block) return;
  (void)hipStreamSynchronize(stream);  // an early error return may leave a copy in flight
  deviceRelease(block);
}

int stageInputs(const void *ha, size_t bytes_a, const void *hb, size_t bytes_b, unsigned flags,
                hipStream_t s, Staging &st) {
  if (flags & MOPT_INPUT_DEVICE) {
    st.a = const_cast<void *>(ha);
    st.b = const_cast<void *>(hb);
    return MOPT_OK;
  }
  const size_t offset_b = (bytes_a + 255) & ~size_t(255);
  if (bytes_a + bytes_b == 0) return MOPT_OK;
  st.stream = s;
  MOPT_HIP_TRY(deviceAlloc(&st.block, offset_b + bytes_b));
  st.a = st.block;
  st.b = static_cast<char *>(st.block) + offset_b;
  // Small inputs go through a pinned bounce buffer owned by the library: a copy straight from
  // pageable memory makes the runtime pin the caller's pages first, which costs 4-8 ms for an
  // address range it has not seen before, whatever its size (measured: a 30 k-point cost took
  // 8 ms to construct, 1.4 MB of input).  Large inputs amortise that and skip the extra host copy.
  if (offset_b + bytes_b <= kBounceBytes) {
    std::lock_guard<std::mutex> lock(g_bounce_mutex);
    if (!g_bounce) MOPT_HIP_TRY(hipHostMalloc(&g_bounce, kBounceBytes, hipHostMallocPortable));
    if (bytes_a) std::memcpy(g_bounce, ha, bytes_a);
    if (bytes_b) std::memcpy(static_cast<char *>(g_bounce) + offset_b, hb, bytes_b);
    MOPT_HIP_TRY(hipMemcpyAsync(st.block, g_bounce, offset_b + bytes_b, hipMemcpyHostToDevice, s));
    MOPT_HIP_TRY(hipStreamSynchronize(s));  // the bounce buffer is free again
    return MOPT_OK;
  }
  if (bytes_a) MOPT_HIP_TRY(hipMemcpyAsync(st.a, ha, bytes_a, hipMemcpyHostToDevice, s));
  if (bytes_b) MOPT_HIP_TRY(hipMemcpyAsync(st.b, hb, bytes_b, hipMemcpyHostToDevice, s));
  return MOPT_OK;
}

template <typename S>
static void defaultReprojConstants(double K[12], double C[16]) {
  // tst/camera_calibration.cpp:22-30
  const double k[12] = {586.122314453125, 0, 638.8477694496105, 0, 0, 722.3973388671875,
                        323.031267074588, 0, 0, 0, 1, 0};
  std::memcpy(K, k, sizeof k);
  const double a = M_PI_2;
  const double rx[3][3] = {{1, 0, 0}, {0, std::cos(a), -std::sin(a)}, {0, std::sin(a), std::cos(a)}};
  const double rz[3][3] = {{std::cos(a), -std::sin(a), 0}, {std::sin(a), std::cos(a), 0}, {0, 0, 1}};
  for (int i = 0; i < 16; ++i) C[i] = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      C[r * 4 + c] = rx[r][0] * rz[0][c] + rx[r][1] * rz[1][c] + rx[r][2] * rz[2][c];
  C[15] = 1.0;
}

// ---- what the create calls share ----------------------------------------------------------------
using CostPtr = std::unique_ptr<mopt_cost, void (*)(mopt_cost *)>;

// a fresh cost that destroys itself unless released to the caller; null when host memory is out
static CostPtr newCost() { return CostPtr(new (std::nothrow) mopt_cost, destroyCost); }

// tiles of `tile_points` elements that hold `count` of them
static int tileCount(int64_t count, int tile_points, long long *tiles) {
  *tiles = (count + tile_points - 1) / tile_points;
  if (*tiles > std::numeric_limits<int>::max())
    return fail(MOPT_ERR_INVALID_ARGUMENT, "count too large");
  return MOPT_OK;
}

static int p2pTilePoints(int scalar_bytes) {
  return scalar_bytes == 8 ? mopt::TileShape<double>::kPoints : mopt::TileShape<float>::kPoints;
}

// plane stride padded to whole 16-byte packs (the sweep loads 16 bytes per lane and plane); the
// tail of the last pack is zero-filled and enters no sum
static long long paddedPlaneStride(int64_t count, int scalar_bytes) {
  const int vec = 16 / scalar_bytes;
  return (count + vec - 1) / vec * vec;
}

}  // namespace mopt_detail

extern "C" {

int mopt_point2point_create(mopt_cost **out, int device, int scalar_bytes, const void *src_xyz,
                            const void *tgt_xyz, int64_t count, unsigned flags) {
  if (!out) return fail(MOPT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 or 8");
  if (count < 0 || (count > 0 && (!src_xyz || !tgt_xyz)))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "bad point arrays / count");
  CostPtr c = newCost();
  if (!c) return fail(MOPT_ERR_HIP, "out of host memory");
  c->scalar_bytes = scalar_bytes;
  c->model = kModelPoint2Point;
  c->n_out = 3;
  c->count = count;
  long long tiles = 0;
  int rc = tileCount(count, p2pTilePoints(scalar_bytes), &tiles);
  if (rc != MOPT_OK) return rc;
  c->num_tiles = int(tiles);
  rc = commonCreate(c.get(), device);
  if (rc != MOPT_OK) return rc;
  if (!mopt_detail::g_creating_for_search) mopt_detail::aqlWarm(device);

  rc = mopt_point2point_set_data(c.get(), src_xyz, tgt_xyz, count, flags);
  if (rc != MOPT_OK) return rc;
  c->state_version = 0;
  *out = c.release();
  return MOPT_OK;
}

int mopt_point2point_set_data(mopt_cost *c, const void *src_xyz, const void *tgt_xyz,
                              int64_t count, unsigned flags) {
  if (!c || c->model != kModelPoint2Point)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "not a point2point cost");
  if (c->matcher)
    return fail(MOPT_ERR_UNSUPPORTED,
                "a cost made by mopt_icp_create owns its correspondences (mopt_icp_update)");
  if (count < 0 || (count > 0 && (!src_xyz || !tgt_xyz)))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "bad point arrays / count");
  MOPT_HIP_TRY(hipSetDevice(c->device));
  const int tile_points = p2pTilePoints(c->scalar_bytes);
  long long tiles = 0;
  const int tiles_rc = tileCount(count, tile_points, &tiles);
  if (tiles_rc != MOPT_OK) return tiles_rc;
  const size_t tile_bytes = size_t(tile_points) * 6 * c->scalar_bytes;
  MOPT_HIP_TRY(quiesceCost(c));
  if (tiles > c->capacity_tiles) {
    deviceRelease(c->d_tiles);  // nothing enqueued for this cost is still running
    c->d_tiles = nullptr;
    c->capacity_tiles = 0;
    MOPT_HIP_TRY(deviceAlloc(&c->d_tiles, tile_bytes * size_t(tiles)));
    c->capacity_tiles = tiles;
  }
  c->count = count;
  c->num_tiles = int(tiles);
  c->cache.valid = false;
  c->state_version += 1;
  if (tiles > 0) {
    Staging st;
    const size_t bytes = size_t(count) * 3 * c->scalar_bytes;
    const int rc = stageInputs(src_xyz, bytes, tgt_xyz, bytes, flags, c->stream, st);
    if (rc != MOPT_OK) return rc;
    MOPT_HIP_TRY(withScalar(c->scalar_bytes, [&](auto scalar) {
      using S = typename decltype(scalar)::type;
      return mopt::launchRelayoutP2P<S>(static_cast<const S *>(st.a), static_cast<const S *>(st.b), count,
                                        static_cast<S *>(c->d_tiles), c->num_tiles, c->stream);
    }));
    // the scale of the scene (leftBasisCancels, hasSmallForwardStep); d_result is idle: the cost was quiesced
    unsigned long long *d_box = reinterpret_cast<unsigned long long *>(c->d_result);
    unsigned long long box[6];
    MOPT_HIP_TRY(withScalar(c->scalar_bytes, [&](auto scalar) {
      using S = typename decltype(scalar)::type;
      return mopt::launchSourceBox<S>(static_cast<const S *>(c->d_tiles), count, d_box, c->stream);
    }));
    MOPT_HIP_TRY(hipMemcpyAsync(box, d_box, sizeof box, hipMemcpyDeviceToHost, c->stream));
    MOPT_HIP_TRY(hipStreamSynchronize(c->stream));
    double diag2 = 0.0, center2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double lo = mopt::sourceBoxValue(box[k]), hi = mopt::sourceBoxValue(box[3 + k]);
      c->src_center[k] = 0.5 * (lo + hi);
      diag2 += (hi - lo) * (hi - lo);
      center2 += c->src_center[k] * c->src_center[k];
    }
    c->src_radius = 0.5 * std::sqrt(diag2);
    c->src_bound = std::sqrt(center2) + c->src_radius;
  } else {
    c->src_center[0] = c->src_center[1] = c->src_center[2] = c->src_radius = c->src_bound = 0.0;
  }
  return MOPT_OK;
}


int mopt_reprojection_create(mopt_cost **out, int device, const double *points_xyzw,
                             const int32_t *pixels_uv, int64_t count, const double *camera_3x4,
                             const double *frame_4x4, unsigned flags) {
  if (!out) return fail(MOPT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (count <= 0 || !points_xyzw || !pixels_uv)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "Empty point / pixel list");
  CostPtr c = newCost();
  if (!c) return fail(MOPT_ERR_HIP, "out of host memory");
  c->scalar_bytes = 8;
  c->model = kModelReprojection;
  c->n_out = 2;
  c->count = count;
  defaultReprojConstants<double>(c->camera, c->frame);
  if (camera_3x4) std::memcpy(c->camera, camera_3x4, sizeof c->camera);
  if (frame_4x4) std::memcpy(c->frame, frame_4x4, sizeof c->frame);
  long long tiles = 0;
  int rc = tileCount(count, mopt::kReprojTilePoints, &tiles);
  if (rc != MOPT_OK) return rc;
  c->num_tiles = int(tiles);
  rc = commonCreate(c.get(), device);
  if (rc != MOPT_OK) return rc;
  mopt_detail::aqlWarm(device);
  MOPT_HIP_TRY(deviceAlloc(&c->d_tiles, size_t(mopt::kReprojTileBytes) * c->num_tiles));
  Staging st;
  rc = stageInputs(points_xyzw, size_t(count) * 32, pixels_uv, size_t(count) * 8, flags, c->stream,
                   st);
  if (rc != MOPT_OK) return rc;
  MOPT_HIP_TRY(mopt::launchRelayoutReproj(static_cast<const double *>(st.a),
                                          static_cast<const int32_t *>(st.b), count,
                                          static_cast<unsigned char *>(c->d_tiles), c->num_tiles,
                                          c->stream));
  MOPT_HIP_TRY(hipStreamSynchronize(c->stream));
  *out = c.release();
  return MOPT_OK;
}

int mopt_scalar_model_create(mopt_cost **out, int device, int scalar_bytes, int model_kind,
                             const void *t, const void *y, int64_t stride_scalars, int64_t count) {
  if (!out) return fail(MOPT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 or 8");
  int n = 0, m = 0, planes = 0;
  switch (model_kind) {
    case MOPT_MODEL_EXP_CURVE: n = 2; m = 1; planes = 2; break;
    case MOPT_MODEL_RATIONAL: n = 2; m = 1; planes = 2; break;
    case MOPT_MODEL_POWELL: n = 4; m = 4; planes = 0; break;
    default: return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown scalar model kind");
  }
  if (count < 1 || (planes > 0 && (!t || !y || stride_scalars < 1)))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "bad data arrays / count");
  CostPtr c = newCost();
  if (!c) return fail(MOPT_ERR_HIP, "out of host memory");
  c->scalar_bytes = scalar_bytes;
  c->model = kModelScalar;
  c->scalar_model = model_kind;
  c->n_params = n;
  c->n_out = m;
  c->count = count;
  c->num_tiles = 1;
  const long long padded = paddedPlaneStride(count, scalar_bytes);
  c->data_stride = padded;
  int rc = commonCreate(c.get(), device);
  if (rc != MOPT_OK) return rc;
  mopt_detail::aqlWarm(device);
  if (planes > 0) {
    // gather the (possibly interleaved) host arrays into contiguous planes t | y
    std::vector<unsigned char> staged(size_t(planes) * size_t(padded) * scalar_bytes, 0);
    const unsigned char *src[2] = {static_cast<const unsigned char *>(t),
                                   static_cast<const unsigned char *>(y)};
    for (int p = 0; p < planes; ++p)
      for (int64_t i = 0; i < count; ++i)
        std::memcpy(&staged[(size_t(p) * padded + size_t(i)) * scalar_bytes],
                    src[p] + size_t(i) * size_t(stride_scalars) * scalar_bytes, scalar_bytes);
    // an observation whose y is NaN is "not a residual" (f / f_df returning false: model.h:32,43):
    // data that carry the marker run the sweeps that look for it (sweep.hpp, ScalarModelKind)
    bool marked = false;
    for (int64_t i = 0; i < count && !marked; ++i) {
      const unsigned char *yi = &staged[(size_t(1) * padded + size_t(i)) * scalar_bytes];
      if (scalar_bytes == 8) {
        double v;
        std::memcpy(&v, yi, 8);
        marked = v != v;
      } else {
        float v;
        std::memcpy(&v, yi, 4);
        marked = v != v;
      }
    }
    if (marked)
      c->scalar_model = model_kind == MOPT_MODEL_EXP_CURVE ? int(mopt::kScalarExpCurveMarked)
                                                            : int(mopt::kScalarRationalMarked);
    MOPT_HIP_TRY(deviceAlloc(&c->d_tiles, staged.size()));
    MOPT_HIP_TRY(hipMemcpy(c->d_tiles, staged.data(), staged.size(), hipMemcpyHostToDevice));
  }
  mopt_cost_set_covariance(c.get(), nullptr);
  c->state_version = 0;
  *out = c.release();
  return MOPT_OK;
}

int mopt_jit_model_create(mopt_cost **out, int device, int scalar_bytes, int n_params,
                          int n_outputs, int n_planes, int n_aux, const char *setup_body,
                          const char *residual_body, const char *jacobian_body, const void *data,
                          int64_t plane_stride, int64_t count, unsigned flags) {
  if (!out) return fail(MOPT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 or 8");
  if (count < 1 || (n_planes > 0 && (!data || plane_stride < count)))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "bad data planes / count");
  CostPtr c = newCost();
  if (!c) return fail(MOPT_ERR_HIP, "out of host memory");
  c->scalar_bytes = scalar_bytes;
  c->model = kModelJit;
  c->n_params = n_params;
  c->n_out = n_outputs;
  c->count = count;
  c->num_tiles = 1;
  c->data_stride = count;
  int rc = commonCreate(c.get(), device);
  if (rc != MOPT_OK) return rc;
  if (!mopt::jitCreate(scalar_bytes, n_params, n_outputs, n_planes, n_aux, setup_body,
                       residual_body, jacobian_body, c->jit))
    return fail(MOPT_ERR_INVALID_ARGUMENT, mopt::jitLastError());
  if (n_planes > 0) {
    const long long padded = paddedPlaneStride(count, scalar_bytes);
    c->data_stride = padded;
    const size_t row = size_t(count) * scalar_bytes, pitch = size_t(padded) * scalar_bytes;
    MOPT_HIP_TRY(deviceAlloc(&c->d_tiles, pitch * n_planes));
    MOPT_HIP_TRY(hipMemset(c->d_tiles, 0, pitch * n_planes));
    MOPT_HIP_TRY(hipMemcpy2D(c->d_tiles, pitch, data, size_t(plane_stride) * scalar_bytes, row,
                             size_t(n_planes),
                             (flags & MOPT_INPUT_DEVICE) ? hipMemcpyDeviceToDevice
                                                         : hipMemcpyHostToDevice));
  }
  mopt_cost_set_covariance(c.get(), nullptr);
  c->state_version = 0;
  *out = c.release();
  return MOPT_OK;
}

int mopt_cost_destroy(mopt_cost *cost) {
  destroyCost(cost);
  return MOPT_OK;
}

int mopt_cost_set_covariance(mopt_cost *c, const void *cov_colmajor) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  const int m = c->n_out;
  constexpr int kCovSlots = mopt::kMaxWideOutputs * mopt::kMaxWideOutputs;
  if (m < 1 || m * m > kCovSlots) return fail(MOPT_ERR_INVALID_ARGUMENT, "output dimension out of range");
  double dense[kCovSlots];  // row-major m x m
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) {
      double v = (a == b) ? 1.0 : 0.0;
      if (cov_colmajor)
        v = c->scalar_bytes == 8 ? static_cast<const double *>(cov_colmajor)[b * m + a]
                                 : double(static_cast<const float *>(cov_colmajor)[b * m + a]);
      dense[a * m + b] = v;
    }
  double previous[kCovSlots];
  std::memcpy(previous, c->cov_m, sizeof previous);
  for (int k = 0; k < kCovSlots; ++k) c->cov_m[k] = 0.0;
  for (int k = 0; k < m * m; ++k) c->cov_m[k] = dense[k];
  for (int k = 0; k < 9; ++k) c->cov[k] = (k % 4 == 0) ? 1.0 : 0.0;
  if (m <= 3)
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) c->cov[a * 3 + b] = dense[a * m + b];
  bool identity = true, symmetric = true;
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) {
      if (dense[a * m + b] != (a == b ? 1.0 : 0.0)) identity = false;
      if (dense[a * m + b] != dense[b * m + a]) symmetric = false;
    }
  c->cov_mode = identity ? mopt::kCovIdentity
                         : (symmetric ? mopt::kCovSymmetric : mopt::kCovGeneral);
  if (std::memcmp(previous, c->cov_m, sizeof previous) != 0) c->state_version += 1;
  return MOPT_OK;
}

int mopt_cost_set_loss(mopt_cost *c, int loss_kind, double parameter) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  if (loss_kind != MOPT_LOSS_NONE && loss_kind != MOPT_LOSS_GEMAN_MCCLURE)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown loss_kind");
  if (c->loss_kind != loss_kind || c->loss_param != parameter) c->state_version += 1;
  c->loss_kind = loss_kind;
  c->loss_param = parameter;
  return MOPT_OK;
}

int mopt_cost_set_kernel_variant(mopt_cost *c, int variant) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  if (variant < MOPT_KERNEL_AUTO || variant > MOPT_KERNEL_MOMENTS_ALWAYS)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown kernel variant");
  if ((variant == MOPT_KERNEL_MOMENTS || variant == MOPT_KERNEL_MOMENTS_ALWAYS) &&
      c->model != kModelPoint2Point)
    return fail(MOPT_ERR_UNSUPPORTED, "only point2point Jacobians are affine in the data point");
  if (c->variant != variant) c->state_version += 1;
  c->variant = variant;
  return MOPT_OK;
}

}  // extern "C"
