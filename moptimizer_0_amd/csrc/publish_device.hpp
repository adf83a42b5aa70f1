// The device side of the hand-over protocol (sweep.hpp, HostPublish and PeerCombine), shared by the
// kernels that publish a result (finalize_kernels.hip, icp_match.hip): write-through payload, drain,
// barrier, then the sequence word.  Everything is in an anonymous namespace of the including
// translation unit.
#pragma once

#include "sweep.hpp"

namespace mopt {
namespace {

// Write-through store at system scope (sc0 sc1): straight to mapped host memory, nothing left
// dirty in L2, so publishing needs no L2 write-back (a system-scope release fence costs two).
__device__ __forceinline__ void storeSystem(double *p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long *>(p),
                     static_cast<unsigned long long>(__double_as_longlong(v)), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}

// Called by every thread of the (single) finalize workgroup; threads k < count hold result k in
// `v`.  Payload goes out write-through, every storing wave drains it (s_waitcnt vmcnt(0)), the
// workgroup meets at a barrier, then one lane stores the sequence word — the payload is complete
// before the flag is issued (cdna_hip_programming.md Guideline 16, form R1, at system scope).
__device__ __forceinline__ void publishToHost(const HostPublish &pub, int count, double v,
                                              unsigned long long status = 0) {
  if (pub.host_flag == nullptr) return;
  if (int(threadIdx.x) < count && pub.host_result) storeSystem(pub.host_result + threadIdx.x, v);
  if (threadIdx.x == 0 && pub.host_status)
    __hip_atomic_store(pub.host_status, status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_store(pub.host_flag, pub.sequence, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ double loadSystem(const double *p) {
  return __longlong_as_double(static_cast<long long>(
      __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_SYSTEM)));
}

// Sum of `v` over the ranks (sweep.hpp, PeerCombine), by the single finalize workgroup; threads
// k < count hold value k.  Same producer form as publishToHost (write-through payload, every
// storing wave drained, barrier, then the sequence word), here into every rank's slot block;
// the consumer side polls the G flags of the own block with system-scope loads from one lane
// each, sleeps between polls, gives up after timeout_ticks (the wait must end on every path: a
// peer that never arrives turns into kStatusPeerTimeout and NaN sums, not into a hung GPU), and
// then adds the G slots in rank order.
// (`sequence_add`: the resident kernels' trial count on top of pc.sequence — a separate argument,
// because a modified copy of `pc` is a private array indexed by lane: scratch for every launch)
__device__ __forceinline__ double peerCombine(const PeerCombine &pc, int count, double v,
                                              unsigned long long *status,
                                              unsigned long long sequence_add = 0) {
  *status = 0;
  if (pc.num_ranks <= 0) return v;
  const unsigned long long sequence = pc.sequence + sequence_add;
  __shared__ double *peer_block[kMaxPeers];
  __shared__ int timed_out;
  const int tid = threadIdx.x;
  const int G = pc.num_ranks;
  if (tid < kMaxPeers) peer_block[tid] = pc.blocks[tid < G ? tid : 0];
  if (tid == 0) timed_out = 0;
  __syncthreads();
  const size_t mine = slotIndex(sequence, G, pc.rank);
  if (tid < count)
    for (int p = 0; p < G; ++p) storeSystem(peer_block[p] + mine + pc.offset + tid, v);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  double *own = peer_block[pc.rank];
  if (tid < G) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(peer_block[tid] + mine + kSlotFlag),
                       sequence, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long *flag = reinterpret_cast<const unsigned long long *>(
        own + slotIndex(sequence, G, tid) + kSlotFlag);
    const unsigned long long started = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < sequence) {
      if (wall_clock64() - started > pc.timeout_ticks) {
        timed_out = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
  }
  __syncthreads();
  double total = 0.0;
  if (tid < count)
    for (int k = 0; k < G; ++k)
      total += loadSystem(own + slotIndex(sequence, G, k) + pc.offset + tid);
  if (timed_out) {
    *status = kStatusPeerTimeout;
    total = __builtin_nan("");
  }
  return total;
}

}  // namespace
}  // namespace mopt
