// age.hip — the flow-aging sweep and the age-aware harvest (contract: age.h).
//
// Both stream the table once: a lane owns one slot per pass of a capped grid (age_grid), 64-bit
// index arithmetic (n up to 2^32 - 1 slots), no LDS, no scratch, and no workgroup ever waits for
// another.
//   age_sweep_kernel    one 16-B row load per lane; a wave whose ballot of armed rows is empty does
//                       nothing more.  Only armed lanes load their 8-B counter, as a relaxed
//                       agent-scope load (served by L2, where the packet kernels' atomics land): a
//                       value as fresh as the sweep's launch is enough, since a later increment is
//                       caught by the next sweep.  A row is stored (one 16-B store) only where it
//                       changed.  Expired slots are compacted per wave: one ballot, mbcnt for the
//                       lane's rank, one global atomic add per wave that has any, and a lane writes
//                       its slot only if its index is below cap.
//   harvest_age_kernel  harvest_kernel's exchange, plus the row's touched flag / seen reset.
// Kept apart from kernels.hip so that file's register allocation does not move.
#include <hip/hip_runtime.h>

#include "age.h"
#include "host.h"

namespace nfdp {
namespace {

using u64 = unsigned long long;

__device__ __forceinline__ AgeRow load_row(const AgeRow* rows, uint64_t i) {
  const uint4 q = *reinterpret_cast<const uint4*>(rows + i);
  AgeRow r;
  r.seen = (uint64_t)q.x | ((uint64_t)q.y << 32);
  r.last = q.z;
  r.tmo = q.w;
  return r;
}
__device__ __forceinline__ void store_row(AgeRow* rows, uint64_t i, const AgeRow& r) {
  *reinterpret_cast<uint4*>(rows + i) = make_uint4((uint32_t)r.seen, (uint32_t)(r.seen >> 32), r.last, r.tmo);
}

}  // namespace

__global__ __launch_bounds__(256) void age_sweep_kernel(const u64* __restrict__ ctr, AgeRow* __restrict__ rows,
                                                        uint64_t n, uint32_t now, uint32_t* __restrict__ out,
                                                        uint32_t cap, uint32_t* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kAgeBlock;
  // (wave-uniform trips: `base` is the wave's first slot, so the ballots see whole waves)
  for (uint64_t base = (uint64_t)blockIdx.x * kAgeBlock + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint64_t i = base + lane;
    AgeRow r{0, 0, 0};
    if (i < n) r = load_row(rows, i);
    const bool armed = (r.tmo & kAgeTmoMask) != 0;
    if (!__ballot(armed)) continue;
    bool expired = false;
    if (armed) {
      const u64 c = __hip_atomic_load(ctr + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const AgeVerdict v = age_step(r, c, now);
      if (v == kAgeRefresh) store_row(rows, i, r);
      expired = v == kAgeExpired;
    }
    const u64 ex = __ballot(expired);
    if (!ex) continue;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ex >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ex, 0u));
    uint32_t first = 0;
    if (lane == (uint32_t)__builtin_ctzll(ex)) first = atomicAdd(count, (uint32_t)__popcll(ex));
    first = __shfl(first, __builtin_ctzll(ex));
    // (count <= n < 2^32: the sum never wraps)
    const uint64_t at = (uint64_t)first + rank;
    if (expired && at < cap) out[at] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(256) void harvest_age_kernel(u64* __restrict__ ctr, AgeRow* __restrict__ rows,
                                                          u64* __restrict__ out, uint64_t n) {
  const uint64_t stride = (uint64_t)gridDim.x * kAgeBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kAgeBlock + threadIdx.x; i < n; i += stride) {
    AgeRow r = load_row(rows, i);
    const u64 v = atomicExch(ctr + i, 0ull);
    out[i] = v;
    if (age_harvest_step(r, v)) store_row(rows, i, r);
  }
}

hipError_t launch_age_sweep(const unsigned long long* ctr, AgeRow* rows, uint64_t n, uint32_t now_tick, uint32_t* out,
                            uint32_t cap, uint32_t* count, hipStream_t s) {
  if (!count || n > 0xFFFFFFFFull || (n && (!ctr || !rows)) || (cap && !out)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), s);
  if (e != hipSuccess || n == 0) return e;
  uint32_t groups, per_pass;
  age_grid(n, groups, per_pass);
  hipLaunchKernelGGL(age_sweep_kernel, dim3(groups), dim3(kAgeBlock), 0, s, ctr, rows, n, now_tick, out, cap, count);
  return hipGetLastError();
}

hipError_t launch_harvest_age(unsigned long long* ctr, AgeRow* rows, unsigned long long* out, uint64_t n,
                              hipStream_t s) {
  if (n > 0xFFFFFFFFull || (n && (!ctr || !rows || !out))) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  uint32_t groups, per_pass;
  age_grid(n, groups, per_pass);
  hipLaunchKernelGGL(harvest_age_kernel, dim3(groups), dim3(kAgeBlock), 0, s, ctr, rows, out, n);
  return hipGetLastError();
}

}  // namespace nfdp
