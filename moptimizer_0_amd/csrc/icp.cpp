// Correspondence search entry points (mopt_icp_*): the step upstream of the sweep, i.e. what a
// registration model's update(x) does before every linearization (model.h:24-26,
// levenberg_marquadt_dyn.cpp:54).  Grid construction and search run on the GPU (cell_order.hip,
// icpMatchKernel in icp_match.hip); this file is their host side.
#include "cell_order.hpp"
#include "cost_state.hpp"

#include <cmath>
#include <cstring>
#include <limits>

#include "moptimizer_amd/so3.hpp"

using namespace mopt_detail;

namespace {
// Grid over the targets and cell-ordered copy of the sources, built on the device (cell_order.hip);
// the host only chooses the resolution.  On return `d_src_sorted` holds the n sources in cell
// order (packed xyz) and matcher->d_order (device memory) the original index of each.
template <typename S>
int buildIcpGrid(const S *src, long long n, const S *tgt, long long m, double max_distance,
                 unsigned flags, hipStream_t s, std::unique_ptr<IcpMatcher> &out_matcher,
                 DeviceScratch &d_src_sorted) {
  auto mt = std::make_unique<IcpMatcher>();
  mt->max_dist = max_distance;
  mt->num_targets = m;
  DeviceScratch d_tgt(s), d_src(s), d_perm_t(s), d_perm_s(s);
  MOPT_HIP_TRY(d_tgt.alloc(size_t(m) * 3 * sizeof(S)));
  MOPT_HIP_TRY(d_src.alloc(size_t(n) * 3 * sizeof(S)));
  // (clouds already in device memory are copied too: 24 B a point at HBM speed, and the caller's
  // arrays are free again when this returns, as with host arrays)
  const hipMemcpyKind kind = (flags & MOPT_INPUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (m > 0) MOPT_HIP_TRY(hipMemcpyAsync(d_tgt.p, tgt, size_t(m) * 3 * sizeof(S), kind, s));
  if (n > 0) MOPT_HIP_TRY(hipMemcpyAsync(d_src.p, src, size_t(n) * 3 * sizeof(S), kind, s));
  double lo[3], hi[3];
  MOPT_HIP_TRY(mopt::cloudBoundingBox<S>(d_tgt.as<S>(), m, lo, hi, s));
  // The resolution (cell_lattice.hpp has the rules): `reach` cells to the search radius, first by the
  // box's volume, then by the cells the targets occupy.
  // 2^26 cells (a 256 MB offset table at most) since round 5: a scanned surface fills a thin sheet of
  // its bounding box, and with 2^24 a million-point scan searched within 4 point spacings stayed at one
  // cell to the radius, ~12 targets per occupied cell — whole ICP solves 1 M x 1 M, radius 2 / 4 / 8
  // spacings: 1.29 / 2.16 / 1.90 ms -> 1.21 / 1.30 / 1.46 (profiles/r5_icp_cells_cap.txt; 2^28 gains
  // nothing more: finer cells speed the first round up and slow the second down)
  static const int cells_log2 = envInt("MOPT_ICP_MAX_CELLS_LOG2", mopt::kMostCellsLog2);
  static const int forced_reach = envInt("MOPT_ICP_REACH", 0);  // tests and measurements
  const mopt::SearchBox box(lo, hi, max_distance, mopt::searchCellCap(cells_log2));
  int reach = box.firstReach(m, forced_reach);
  out_matcher = std::move(mt);  // from here on the caller frees the matcher's device arrays
  IcpMatcher &g = *out_matcher;
  MOPT_HIP_TRY(d_perm_t.alloc(size_t(m) * sizeof(int)));
  // the targets binned at `reach`, and again while refineReach asks for another resolution
  int reach_before = 0;
  double per_cell_before = 0.0;
  bool settled = false;
  for (int attempt = 0;; ++attempt) {
    g.reach = reach;
    g.lattice = box.latticeAt(reach);
    const long long ncells = g.lattice.cells();
    if (g.d_cell_start) deviceRelease(g.d_cell_start);
    g.d_cell_start = nullptr;
    MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&g.d_cell_start), size_t(ncells + 1) * sizeof(int)));
    mopt::CellOrder targets;
    targets.d_perm = d_perm_t.as<int>();
    targets.d_cell_start = g.d_cell_start;
    MOPT_HIP_TRY(mopt::sortByCell<S>(d_tgt.as<S>(), m, g.lattice, targets, s));
    if (settled || !mopt::refinementPossible(reach, reach_before, forced_reach, m)) break;
    long long occupied = 0;
    MOPT_HIP_TRY(mopt::countOccupiedCells(g.d_cell_start, ncells, &occupied, s));
    const double per_cell = double(m) / double(occupied > 0 ? occupied : 1);
    const mopt::Refinement next = mopt::refineReach(reach, reach_before, per_cell_before, attempt, per_cell);
    if (next.what == mopt::Refinement::kStop) break;
    if (next.what == mopt::Refinement::kStepBack) {
      reach = next.reach;
      settled = true;
      continue;
    }
    const int finer = box.mostReach(next.reach);
    if (finer <= reach) break;
    reach_before = reach;
    per_cell_before = per_cell;
    reach = finer;
  }
  // (one matched count per wave of the search: whole tiles of sources, 64 to a wave)
  constexpr long long kTile = mopt::TileShape<S>::kPoints;
  if (m > 0) {
    MOPT_HIP_TRY(deviceAlloc(&g.d_sorted, size_t(m) * 4 * sizeof(S)));
    MOPT_HIP_TRY(mopt::gatherByOrder<S>(d_tgt.as<S>(), d_perm_t.as<int>(), m, static_cast<S *>(g.d_sorted),
                                        true, s));
  }
  // the sources in the cell order of their un-warped position; those with a NaN or infinite
  // coordinate sort behind the others and are left out of the cost (they can have no target, and
  // their arithmetic would turn every sum into NaN): the cost holds the first `kept` of the order
  MOPT_HIP_TRY(d_perm_s.alloc(size_t(n) * sizeof(int)));
  mopt::CellOrder sources;
  sources.d_perm = d_perm_s.as<int>();
  sources.park_non_finite = true;
  MOPT_HIP_TRY(mopt::sortByCell<S>(d_src.as<S>(), n, g.lattice, sources, s));
  const long long kept = n - sources.parked;
  g.num_sources = n;
  g.num_waves = (kept + kTile - 1) / kTile * kTile / 64;
  MOPT_HIP_TRY(deviceAlloc(reinterpret_cast<void **>(&g.d_matched),
                           size_t(g.num_waves > 0 ? g.num_waves : 1) * sizeof(unsigned int)));
  MOPT_HIP_TRY(d_src_sorted.alloc(size_t(kept) * 3 * sizeof(S)));
  MOPT_HIP_TRY(mopt::gatherByOrder<S>(d_src.as<S>(), d_perm_s.as<int>(), kept, d_src_sorted.as<S>(), false,
                                      s));
  MOPT_HIP_TRY(hipStreamSynchronize(s));
  g.d_order = d_perm_s.as<int>();  // the matcher keeps the order (its first `kept` entries) on the device
  d_perm_s.p = nullptr;
  g.kept = kept;
  return MOPT_OK;
}

}  // namespace

namespace mopt_detail {
// everything of a search that does not depend on the pose
template <typename S>
void fillIcpArgs(const mopt_cost *c, mopt::IcpMatchArgs<S> &a) {
  const IcpMatcher &mt = *c->matcher;
  a.tiles = static_cast<S *>(c->d_tiles);
  a.count = c->count;
  a.num_tiles = c->num_tiles;
  a.sorted = static_cast<const S *>(mt.d_sorted);
  a.cell_start = mt.d_cell_start;
  for (int k = 0; k < 3; ++k) {
    a.origin[k] = S(mt.lattice.origin[k]);
    a.dims[k] = mt.lattice.dims[k];
  }
  a.inv_cell = S(1.0 / mt.lattice.edge);
  a.cell = S(mt.lattice.edge);
  a.reach = mt.reach;
  a.max_dist2 = S(mt.max_dist * mt.max_dist);
  for (int k = 0; k < 12; ++k) a.T[k] = S(k % 5 == 0 ? 1 : 0);
  a.matched = nullptr;
  // The inner nine rows in lock step, the rings beyond row by row under the running bound: with every
  // ring in lock step (MOPT_ICP_LOCK_RINGS=8) reach 3 took 0.154 / 0.178 / 0.229 ms per 1 M at 0.4 / 0.7 /
  // 1.5 radii apart against 0.139 / 0.163 / 0.214, reach 8 on a surface 1.09 against 0.97, reach 2 the
  // same (profiles/r5_icp_lock_rings.txt)
  static const int lock_rings = envInt("MOPT_ICP_LOCK_RINGS", 1);
  a.lock_rings = lock_rings;
}
template void fillIcpArgs<float>(const mopt_cost *, mopt::IcpMatchArgs<float> &);
template void fillIcpArgs<double>(const mopt_cost *, mopt::IcpMatchArgs<double> &);
}  // namespace mopt_detail

namespace {
template <typename S>
int icpUpdate(mopt_cost *c, const S *x, int64_t *num_matched) {
  const IcpMatcher &mt = *c->matcher;
  mopt::IcpMatchArgs<S> a;
  fillIcpArgs<S>(c, a);
  const auto T = moptimizer::so3::rigidFrom6DOF<S>(x);
  std::memcpy(a.T, T.m, sizeof T.m);
  a.matched = num_matched ? mt.d_matched : nullptr;
  MOPT_HIP_TRY(mopt::launchIcpMatch<S>(a, c->stream));
  c->cache.valid = false;
  c->state_version += 1;
  if (num_matched) {
    // the count comes back like a sweep result: a one-wave kernel stores it into mapped host
    // memory and releases a sequence word — no memset, no copy, no stream synchronisation
    const int slot = mopt_detail::kResultSlots - 1;  // beyond any n*n + n + 1 <= 73
    const mopt::HostPublish pub = nextPublish(c, slot);
    MOPT_HIP_TRY(mopt::launchPublishCounter(mt.d_matched, mt.num_waves, pub, c->stream));
    const int rc = waitPublished(c, pub.sequence);
    if (rc != MOPT_OK) return rc;
    *num_matched = int64_t(c->h_result[slot]);
  }
  return MOPT_OK;
}
}  // namespace

extern "C" {

int mopt_icp_create(mopt_cost **out, int device, int scalar_bytes, const void *src_xyz,
                    int64_t num_src, const void *tgt_xyz, int64_t num_tgt, double max_distance) {
  return mopt_icp_create_from(out, device, scalar_bytes, src_xyz, num_src, tgt_xyz, num_tgt,
                              max_distance, MOPT_INPUT_HOST);
}

int mopt_icp_create_from(mopt_cost **out, int device, int scalar_bytes, const void *src_xyz,
                         int64_t num_src, const void *tgt_xyz, int64_t num_tgt, double max_distance,
                         unsigned flags) {
  if (!out) return fail(MOPT_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (num_src < 0 || num_tgt < 0 || (num_src > 0 && !src_xyz) || (num_tgt > 0 && !tgt_xyz) ||
      num_tgt > std::numeric_limits<int>::max() || num_src > std::numeric_limits<int>::max())
    return fail(MOPT_ERR_INVALID_ARGUMENT, "bad clouds");
  if (!(max_distance > 0.0)) return fail(MOPT_ERR_INVALID_ARGUMENT, "max_distance must be > 0");
  // (before any copy is sized by it: a 2-byte scalar type would be read as fp32, past the caller's buffer)
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(MOPT_ERR_INVALID_ARGUMENT, "scalar_bytes must be 4 (float) or 8 (double)");
  if (flags & ~unsigned(MOPT_INPUT_DEVICE))
    return fail(MOPT_ERR_INVALID_ARGUMENT, "unknown flag bits (MOPT_INPUT_HOST or MOPT_INPUT_DEVICE)");
  if (const int rc = selectDevice(device)) return rc;
  std::unique_ptr<IcpMatcher> matcher;
  auto freeMatcher = [&]() {
    if (!matcher) return;
    deviceRelease(matcher->d_sorted);
    deviceRelease(matcher->d_cell_start);
    deviceRelease(matcher->d_matched);
    deviceRelease(matcher->d_order);
  };
  hipStream_t build_stream = nullptr;
  MOPT_HIP_TRY(acquireStream(device, &build_stream));
  DeviceScratch d_src_sorted(build_stream);  // (read once more by the cost's own stream, which the create call synchronises)
  int rc = withScalar(scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    return buildIcpGrid<S>(static_cast<const S *>(src_xyz), num_src, static_cast<const S *>(tgt_xyz), num_tgt,
                           max_distance, flags, build_stream, matcher, d_src_sorted);
  });
  (void)hipStreamSynchronize(build_stream);
  releaseStream(device, build_stream);
  // the sources go into the resident tiles in cell order; the target planes are filled by the
  // first search
  mopt_cost *raw = nullptr;
  if (rc == MOPT_OK) {
    g_creating_for_search = true;  // (its update(x) is queued on the stream: never on the direct path)
    rc = mopt_point2point_create(&raw, device, scalar_bytes, d_src_sorted.p, d_src_sorted.p,
                                 int64_t(matcher->kept), MOPT_INPUT_DEVICE);
    g_creating_for_search = false;
  }
  if (rc != MOPT_OK) {
    freeMatcher();
    return rc;
  }
  std::unique_ptr<mopt_cost, void (*)(mopt_cost *)> c(raw, destroyCost);
  c->matcher = std::move(matcher);
  const double zero8[6] = {0, 0, 0, 0, 0, 0};
  const float zero4[6] = {0, 0, 0, 0, 0, 0};
  rc = mopt_icp_update(c.get(), scalar_bytes == 8 ? static_cast<const void *>(zero8)
                                                   : static_cast<const void *>(zero4), nullptr);
  if (rc != MOPT_OK) return rc;
  *out = c.release();
  return MOPT_OK;
}

int mopt_icp_update(mopt_cost *c, const void *x, int64_t *num_matched) {
  if (!c || !x) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  if (!c->matcher) return fail(MOPT_ERR_INVALID_ARGUMENT, "not a cost made by mopt_icp_create");
  MOPT_HIP_TRY(hipSetDevice(c->device));
  return withScalar(c->scalar_bytes, [&](auto scalar) {
    using S = typename decltype(scalar)::type;
    return icpUpdate<S>(c, static_cast<const S *>(x), num_matched);
  });
}

int mopt_icp_grid(const mopt_cost *c, double *cell_edge, int *reach, int dims[3], double origin[3]) {
  if (!c || !c->matcher) return fail(MOPT_ERR_INVALID_ARGUMENT, "not an ICP cost");
  const IcpMatcher &mt = *c->matcher;
  if (cell_edge) *cell_edge = mt.lattice.edge;
  if (reach) *reach = mt.reach;
  for (int a = 0; a < 3; ++a) {
    if (dims) dims[a] = mt.lattice.dims[a];
    if (origin) origin[a] = mt.lattice.origin[a];
  }
  return MOPT_OK;
}

int mopt_icp_get_matches(mopt_cost *c, void *tgt_out_xyz) {
  if (!c || !tgt_out_xyz) return fail(MOPT_ERR_INVALID_ARGUMENT, "NULL argument");
  if (c->model != kModelPoint2Point) return fail(MOPT_ERR_INVALID_ARGUMENT, "not a point2point cost");
  MOPT_HIP_TRY(hipSetDevice(c->device));
  // An ICP cost keeps its sources in cell order and leaves out those with non-finite coordinates:
  // the triples go to the caller's positions on the device (NaN — all bits set — where nothing is
  // written), then one copy.
  const int *order = c->matcher ? c->matcher->d_order : nullptr;
  const long long rows = c->matcher ? c->matcher->num_sources : c->count;
  if (rows == 0) return MOPT_OK;
  const size_t bytes = size_t(rows) * 3 * c->scalar_bytes;
  void *d_tmp = nullptr;
  MOPT_HIP_TRY(deviceAlloc(&d_tmp, bytes));
  hipError_t e = order ? hipMemsetAsync(d_tmp, 0xff, bytes, c->stream) : hipSuccess;
  if (e == hipSuccess)
    e = withScalar(c->scalar_bytes, [&](auto scalar) {
      using S = typename decltype(scalar)::type;
      return mopt::launchGatherTargets<S>(static_cast<const S *>(c->d_tiles), c->count, order,
                                          static_cast<S *>(d_tmp), c->stream);
    });
  if (e == hipSuccess) e = hipMemcpyAsync(tgt_out_xyz, d_tmp, bytes, hipMemcpyDeviceToHost, c->stream);
  const hipError_t synced = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = synced;
  deviceRelease(d_tmp);
  if (e != hipSuccess) return fail(MOPT_ERR_HIP, std::string("gather: ") + hipGetErrorString(e));
  return MOPT_OK;
}

}  // extern "C"
