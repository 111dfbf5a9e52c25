// Sum of one fp32 value per thread over a whole launch of 256-thread workgroups, added to a device float in ONE fp32
// addition (the ticket scheme of the BatchNormalization statistics in dj_igemm.h): wave shuffle in fp32, the four wave sums
// of a workgroup in fp64 into one of DJ_SUMSQ_REPLICAS accumulators of a slot, a ticket, and the workgroup that takes the
// last ticket adds the fp64 total to out[0] and clears the slot.  An fp32 atomic per workgroup on out[0] itself would round
// the running total once per workgroup: 0.7e-6 .. 2e-6 of the sum at a million elements, different from run to run.  The
// workgroups spread their sums over the replicas, each on a 128-byte line of its own like the ticket, so that no line takes
// more atomics than out[0] would.  Launches that may be in flight together must not share a slot: the launcher hands them
// out in turn.
#pragma once
#include "dj_common.h"

#define DJ_SUMSQ_SLOTS 64
#define DJ_SUMSQ_REPLICAS 8

struct DjSumsqSlot {
  struct {
    double v;
    double pad[15];
  } acc[DJ_SUMSQ_REPLICAS];
  unsigned ticket;
  unsigned pad[31];
};

// Called by EVERY thread of every workgroup (it holds a __syncthreads), blockDim.x == 256.
__device__ __forceinline__ void dj_sumsq_finish(float acc, DjSumsqSlot* s, float* out) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&s->acc[blockIdx.x % DJ_SUMSQ_REPLICAS].v,
              ((double)red[0] + (double)red[1]) + ((double)red[2] + (double)red[3]));
    // the ticket after the sum has been performed: device-scope atomics are complete when vmcnt reaches zero
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (atomicAdd(&s->ticket, 1u) == gridDim.x - 1u) {
      double total = 0.0;
      for (int r = 0; r < DJ_SUMSQ_REPLICAS; ++r) {
        total += __hip_atomic_load(&s->acc[r].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&s->acc[r].v, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __hip_atomic_store(&s->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicAdd(out, (float)total);
    }
  }
}
