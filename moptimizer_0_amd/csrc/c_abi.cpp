// The small entry points of libmoptimizer_hip.so's C ABI (declared in include/moptimizer_hip.h): the
// error string, version and device count, the SE(3) helpers, a cost's statistics, communicator, stream
// and profiling.  The rest of the ABI lives with its subject: cost.cpp (lifetime and configuration),
// blocking.cpp (the blocking and *_async sweeps), icp.cpp, group.cpp, combine.cpp, lm.cpp, batch.cpp.  There is no
// CPU implementation behind any entry point: when HIP cannot run the work the call returns an error code.
#include "cost_state.hpp"

#include <cstring>

#include "moptimizer_amd/so3.hpp"

using namespace mopt_detail;

namespace {
thread_local std::string g_last_error;
}  // namespace
namespace mopt_detail {
thread_local bool g_creating_for_search = false;
}

int mopt_detail::fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

namespace {
template <typename S>
void se3FromParams(const S *x, S *T, S *T_plus, S *h_out) {
  moptimizer::so3::convert6DOFParameterToMatrix<S>(x, T);
  if (!T_plus && !h_out) return;
  S h[kNumParams], xp[kNumParams][kNumParams];
  forwardSteps<S>(x, h, xp);
  for (int j = 0; j < kNumParams; ++j) {
    if (h_out) h_out[j] = h[j];
    if (T_plus) moptimizer::so3::convert6DOFParameterToMatrix<S>(xp[j], T_plus + 16 * j);
  }
}
}  // namespace

extern "C" {

const char *mopt_last_error(void) { return g_last_error.c_str(); }
const char *mopt_version(void) { return "moptimizer_hip 0.1 (gfx950)"; }

int mopt_device_count(int *count) {
  if (!count) return fail(MOPT_ERR_INVALID_ARGUMENT, "count is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return MOPT_OK;
}

int mopt_se3_from_params(int scalar_bytes, const void *x, void *T_out, void *T_plus_out,
                         void *h_out) {
  if (!x || !T_out) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  const bool known = mopt::dispatch::widthOrFail(scalar_bytes, false, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    se3FromParams<S>(static_cast<const S *>(x), static_cast<S *>(T_out), static_cast<S *>(T_plus_out),
                     static_cast<S *>(h_out));
    return true;
  });
  return known ? MOPT_OK : fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 or 8");
}

int mopt_se3_plus(int scalar_bytes, const void *x, const void *delta, void *x_out) {
  if (!x || !delta || !x_out) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  const bool known = mopt::dispatch::widthOrFail(scalar_bytes, false, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    moptimizer::so3::se3Plus<S>(static_cast<const S *>(x), static_cast<const S *>(delta),
                                static_cast<S *>(x_out));
    return true;
  });
  return known ? MOPT_OK : fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 or 8");
}

int mopt_se3_plus_right(int scalar_bytes, const void *x, const void *delta, void *x_out) {
  if (!x || !delta || !x_out) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  const bool known = mopt::dispatch::widthOrFail(scalar_bytes, false, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    moptimizer::so3::se3PlusRight<S>(static_cast<const S *>(x), static_cast<const S *>(delta),
                                     static_cast<S *>(x_out));
    return true;
  });
  return known ? MOPT_OK : fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 or 8");
}

int mopt_cost_info(const mopt_cost *c, int64_t *count, int *n, int *m, int *scalar_bytes,
                   int *device) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  if (count) *count = c->count;
  if (n) *n = c->n_params;
  if (m) *m = c->n_out;
  if (scalar_bytes) *scalar_bytes = c->scalar_bytes;
  if (device) *device = c->device;
  return MOPT_OK;
}

int mopt_cost_direct_dispatches(const mopt_cost *c, int64_t *sweeps) {
  if (!c || !sweeps) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  *sweeps = c->stat_direct_sweeps;
  return MOPT_OK;
}

int mopt_cost_lm_choice_stats(const mopt_cost *c, int64_t *points, int64_t *literal_points) {
  if (!c || !points || !literal_points) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  *points = c->stat_lm_choice_points;
  *literal_points = c->stat_lm_literal_points;
  return MOPT_OK;
}

int mopt_device_trim(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "no such device");
  if (!mopt_detail::aqlTrim(device))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "a cost of this process still lives on the device");
  return MOPT_OK;
}

int mopt_cost_stats(const mopt_cost *c, int64_t *sweeps, int64_t *cache_hits) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  if (sweeps) *sweeps = c->stat_sweeps;
  if (cache_hits) *cache_hits = c->stat_cache_hits;
  return MOPT_OK;
}

// ---- multi-process shard group: one rank per GPU, RCCL over xGMI ----------------------------
int mopt_comm_unique_id(void *id_out, int id_bytes) {
  if (!id_out || id_bytes < int(sizeof(ncclUniqueId)))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "id buffer must hold MOPT_COMM_ID_BYTES bytes");
  ncclUniqueId id;
  MOPT_NCCL_TRY(ncclGetUniqueId(&id));
  std::memset(id_out, 0, size_t(id_bytes));
  std::memcpy(id_out, &id, sizeof id);
  return MOPT_OK;
}

int mopt_cost_comm_init_rank(mopt_cost *c, const void *id, int rank, int num_ranks) {
  if (!c || !id || num_ranks < 1 || rank < 0 || rank >= num_ranks)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "bad communicator arguments");
  if (c->comm) return fail(MOPT_ERR_INVALID_ARGUMENT, "a communicator is already attached");
  MOPT_HIP_TRY(hipSetDevice(c->device));
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof uid);
  const ShardCombine &sc = c->combine;
  if ((sc.host_block || sc.peer_attached) && (sc.rank != rank || sc.num_ranks != num_ranks))
    return fail(MOPT_ERR_INVALID_ARGUMENT,
                "rank / num_ranks differ from the transport already attached to this cost");
  MOPT_NCCL_TRY(ncclCommInitRank(&c->comm, num_ranks, uid, rank));
  c->comm_size = num_ranks;
  c->combine.rank = rank;
  c->combine.num_ranks = num_ranks;
  c->combine.mode = MOPT_COMBINE_RCCL;
  c->cache.valid = false;
  return MOPT_OK;
}

int mopt_cost_comm_info(const mopt_cost *c, int *num_ranks, int *rank) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  int count = 0, user_rank = -1;
  if (c->comm) {
    MOPT_NCCL_TRY(ncclCommCount(c->comm, &count));
    MOPT_NCCL_TRY(ncclCommUserRank(c->comm, &user_rank));
  }
  if (num_ranks) *num_ranks = count;
  if (rank) *rank = user_rank;
  return MOPT_OK;
}

int mopt_cost_stream(mopt_cost *c, void **hip_stream) {
  if (!c || !hip_stream) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  *hip_stream = c->stream;
  return MOPT_OK;
}

int mopt_cost_synchronize(mopt_cost *c) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  MOPT_HIP_TRY(hipSetDevice(c->device));
  if (c->aql_touched && c->aql_queue) {  // whatever went through the direct path (aql.hpp) as well
    (void)mopt_detail::aqlDrain(c->aql_queue);
    c->aql_touched = false;
  }
  MOPT_HIP_TRY(hipStreamSynchronize(c->stream));
  c->own_async_pending = false;
  c->hip_pending = false;
  return MOPT_OK;
}

int mopt_cost_set_profiling(mopt_cost *c, int enabled) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  MOPT_HIP_TRY(hipSetDevice(c->device));
  const int rc = resolvePendingEvents(c);
  if (rc != MOPT_OK) return rc;
  c->profiling = enabled > 0 ? enabled : 0;
  c->profiling_tick = 0;
  c->sweep_ms_total = 0.0;
  c->sweep_launches = 0;
  return MOPT_OK;
}

int mopt_cost_profile(mopt_cost *c, double *sweep_ms_total, int64_t *sweep_launches) {
  if (!c) return fail(MOPT_ERR_INVALID_ARGUMENT, "cost is NULL");
  MOPT_HIP_TRY(hipSetDevice(c->device));
  const int rc = resolvePendingEvents(c);
  if (rc != MOPT_OK) return rc;
  if (sweep_ms_total) *sweep_ms_total = c->sweep_ms_total;
  if (sweep_launches) *sweep_launches = c->sweep_launches;
  return MOPT_OK;
}

}  // extern "C"
