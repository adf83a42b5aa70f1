// Device-unit program: the device functions of the Levenberg-Marquardt step (csrc/lm_device.hpp),
// called unchanged from thin test kernels, one case per lane (or per workgroup), on raw arrays.
// Links nothing of the product library.  tests/test_gpu_device_units.py drives it and judges the
// results against long-double references (tests/device_units_reference.py).
//
//   device_units <op> <scalar_bytes> <n> <count> <in.bin> <out.bin>
//
// scalar_bytes: 4 (float) or 8 (double).  Both files are raw little-endian arrays of that scalar,
// `count` records one after the other.  H is column-major n x n, as the step holds it.
//
//   op            n          input record                          output record
//   positive      2, 4, 6    H[n*n] b[n] lambda sentinel           delta[n] flag
//                 solveDampedPositive<S, n>, one system per lane.  delta is pre-filled with the
//                 sentinel; flag is 1 or 0 (what the function returned).
//   pivoted8      1 .. 8     H[n*n] b[n] lambda sentinel           device delta[n] host delta[n]
//   pivoted16     1 .. 16    (the same)
//                 solveDamped<S, kMaxParams / kMaxWideParams>, one system per workgroup, lane 0,
//                 SolveScratch in LDS (its delta pre-filled with the sentinel).  The host half is
//                 dense::PivotedLDLT<S> of tests/support/moptimizer_caller/ldlt.hpp on the same
//                 damped matrix (m_ii += lambda * H_ii), compiled with contraction off.
//   host_pivoted  1 .. 16    (the same)                            host delta[n]
//                 the host half alone: no HIP call is made, runs without a device.
//   se3plus       6          x[6] delta[6]                         out[6]
//   se3plusright  6          x[6] delta[6]                         out[6]
//   rigid         6          x[6]                                  T[12] (row-major 3x4)
//   fstep         1          x                                     forwardStep(x)
//   rcp           1          d                                     fastReciprocal(d)
//
// Any HIP error prints the error and exits with status 2 before anything further is launched; a
// malformed command line or file exits with status 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lm_device.hpp"
#include "moptimizer_caller/ldlt.hpp"

#define HIP_CHECK(call)                                                                         \
  do {                                                                                          \
    const hipError_t err_ = (call);                                                             \
    if (err_ != hipSuccess) {                                                                   \
      std::fprintf(stderr, "device_units: %s: %s (%s:%d)\n", #call, hipGetErrorString(err_),     \
                   __FILE__, __LINE__);                                                         \
      std::exit(2);                                                                             \
    }                                                                                           \
  } while (0)

namespace {

constexpr int kLanes = 64;

template <typename S, int N>
__global__ void positiveKernel(const S *in, S *out, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const S *rec = in + size_t(i) * (N * N + N + 2);
  S H[N * N], b[N], delta[N];
  for (int q = 0; q < N * N; ++q) H[q] = rec[q];
  for (int q = 0; q < N; ++q) b[q] = rec[N * N + q];
  const S lambda = rec[N * N + N], sentinel = rec[N * N + N + 1];
  for (int q = 0; q < N; ++q) delta[q] = sentinel;
  const bool ok = mopt::solveDampedPositive<S, N>(H, b, lambda, delta);
  S *o = out + size_t(i) * (N + 1);
  for (int q = 0; q < N; ++q) o[q] = delta[q];
  o[N] = ok ? S(1) : S(0);
}

// H and b in LDS, where the step holds them (LmState / the sums over the costs)
template <typename S, int NMAX>
__global__ void pivotedKernel(const S *in, S *out, int n) {
  __shared__ S H[NMAX * NMAX];
  __shared__ S b[NMAX];
  __shared__ mopt::SolveScratch<S, NMAX> scratch;
  const S *rec = in + size_t(blockIdx.x) * (n * n + n + 2);
  const int tid = threadIdx.x;
  for (int q = tid; q < n * n; q += blockDim.x) H[q] = rec[q];
  if (tid < n) b[tid] = rec[n * n + tid];
  if (tid < NMAX) scratch.delta[tid] = rec[n * n + n + 1];
  __syncthreads();
  if (tid == 0) mopt::solveDamped<S, NMAX>(H, b, rec[n * n + n], n, scratch);
  __syncthreads();
  if (tid < n) out[size_t(blockIdx.x) * (2 * n) + tid] = scratch.delta[tid];
}

template <typename S, int OP>
__global__ void se3Kernel(const S *in, S *out, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  S x[6], d[6], r[6];
  for (int q = 0; q < 6; ++q) {
    x[q] = in[size_t(i) * 12 + q];
    d[q] = in[size_t(i) * 12 + 6 + q];
  }
  if (OP == 0)
    mopt::se3Plus<S>(x, d, r);
  else
    mopt::se3PlusRight<S>(x, d, r);
  for (int q = 0; q < 6; ++q) out[size_t(i) * 6 + q] = r[q];
}

template <typename S>
__global__ void rigidKernel(const S *in, S *out, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  S x[6], T[12];
  for (int q = 0; q < 6; ++q) x[q] = in[size_t(i) * 6 + q];
  mopt::rigidFrom6DOF<S>(x, T);
  for (int q = 0; q < 12; ++q) out[size_t(i) * 12 + q] = T[q];
}

template <typename S, int OP>
__global__ void scalarKernel(const S *in, S *out, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  out[i] = OP == 0 ? mopt::forwardStep<S>(in[i]) : mopt::fastReciprocal(in[i]);
}

// The host statement on the damped matrix, formed as solveDamped forms it.  (The whole host half
// of this unit is compiled with contraction off, see the Makefile; the pragma says so here too.)
template <typename S>
void hostPivoted(const S *rec, int n, S *delta) {
#pragma clang fp contract(off)
  using moptimizer::dense::Matrix;
  Matrix<S> a(n, n), rhs(n, 1);
  for (int c = 0; c < n; ++c)
    for (int r = 0; r < n; ++r) a(r, c) = rec[c * n + r];
  const S lambda = rec[n * n + n];
  for (int i = 0; i < n; ++i) {
    a(i, i) += lambda * rec[i * n + i];
    rhs[i] = -rec[n * n + i];
  }
  const Matrix<S> x = moptimizer::dense::PivotedLDLT<S>(a).solve(rhs);
  for (int i = 0; i < n; ++i) delta[i] = x[i];
}

[[noreturn]] void usage(const char *why) {
  std::fprintf(stderr, "device_units: %s\nusage: device_units <op> <scalar_bytes> <n> <count> <in.bin> <out.bin>\n",
               why);
  std::exit(1);
}

template <typename S>
int run(const std::string &op, int n, int count, const char *in_path, const char *out_path) {
  size_t in_rec = 0, out_rec = 0;
  const bool positive = op == "positive";
  const bool pivoted = op == "pivoted8" || op == "pivoted16" || op == "host_pivoted";
  if (positive) {
    if (n != 2 && n != 4 && n != 6) usage("positive takes n = 2, 4 or 6");
    in_rec = size_t(n) * n + n + 2, out_rec = n + 1;
  } else if (pivoted) {
    const int nmax = op == "pivoted8" ? mopt::kMaxParams : mopt::kMaxWideParams;
    if (n < 1 || n > nmax) usage("n outside 1 .. NMAX");
    in_rec = size_t(n) * n + n + 2, out_rec = op == "host_pivoted" ? n : 2 * n;
  } else if (op == "se3plus" || op == "se3plusright") {
    in_rec = 12, out_rec = 6;
  } else if (op == "rigid") {
    in_rec = 6, out_rec = 12;
  } else if (op == "fstep" || op == "rcp") {
    in_rec = 1, out_rec = 1;
  } else {
    usage("unknown op");
  }
  if (count < 1 || count > (1 << 20)) usage("count outside 1 .. 2^20");

  std::vector<S> in(in_rec * count), out(out_rec * count, S(0));
  std::FILE *f = std::fopen(in_path, "rb");
  if (!f) usage("cannot open the input file");
  const size_t got = std::fread(in.data(), sizeof(S), in.size(), f);
  const bool more = std::fgetc(f) != EOF;
  std::fclose(f);
  if (got != in.size() || more) usage("the input file does not hold count records");

  if (op != "host_pivoted") {
    S *din = nullptr, *dout = nullptr;
    HIP_CHECK(hipMalloc(&din, in.size() * sizeof(S)));
    HIP_CHECK(hipMalloc(&dout, out.size() * sizeof(S)));
    HIP_CHECK(hipMemcpy(din, in.data(), in.size() * sizeof(S), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dout, 0, out.size() * sizeof(S)));
    const dim3 block(kLanes), grid_lanes((count + kLanes - 1) / kLanes), grid_systems(count);
    if (positive) {
      if (n == 2) positiveKernel<S, 2><<<grid_lanes, block>>>(din, dout, count);
      if (n == 4) positiveKernel<S, 4><<<grid_lanes, block>>>(din, dout, count);
      if (n == 6) positiveKernel<S, 6><<<grid_lanes, block>>>(din, dout, count);
    } else if (op == "pivoted8") {
      pivotedKernel<S, mopt::kMaxParams><<<grid_systems, block>>>(din, dout, n);
    } else if (op == "pivoted16") {
      pivotedKernel<S, mopt::kMaxWideParams><<<grid_systems, block>>>(din, dout, n);
    } else if (op == "se3plus") {
      se3Kernel<S, 0><<<grid_lanes, block>>>(din, dout, count);
    } else if (op == "se3plusright") {
      se3Kernel<S, 1><<<grid_lanes, block>>>(din, dout, count);
    } else if (op == "rigid") {
      rigidKernel<S><<<grid_lanes, block>>>(din, dout, count);
    } else if (op == "fstep") {
      scalarKernel<S, 0><<<grid_lanes, block>>>(din, dout, count);
    } else {
      scalarKernel<S, 1><<<grid_lanes, block>>>(din, dout, count);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out.data(), dout, out.size() * sizeof(S), hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(din));
    HIP_CHECK(hipFree(dout));
  }
  if (pivoted) {
    const size_t at = op == "host_pivoted" ? 0 : n;
    for (int i = 0; i < count; ++i) hostPivoted<S>(&in[in_rec * i], n, &out[out_rec * i + at]);
  }

  f = std::fopen(out_path, "wb");
  if (!f) usage("cannot open the output file");
  const size_t put = std::fwrite(out.data(), sizeof(S), out.size(), f);
  if (std::fclose(f) != 0 || put != out.size()) usage("cannot write the output file");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 7) usage("six arguments");
  const std::string op = argv[1];
  const int bytes = std::atoi(argv[2]), n = std::atoi(argv[3]), count = std::atoi(argv[4]);
  if (bytes == 8) return run<double>(op, n, count, argv[5], argv[6]);
  if (bytes == 4) return run<float>(op, n, count, argv[5], argv[6]);
  usage("scalar_bytes is 4 or 8");
}
