// police.hip — the token-bucket policer passes around the fused kernel (contract: police.h).
//
// The verdict of frame i depends on every earlier frame of its meter in the batch: a keyed,
// ordered prefix sum over the whole batch.  Three phases, ordered by the stream alone (no
// workgroup ever waits for another: no look-back, no spin, no grid barrier).  Each of G <= 1024
// workgroups owns one contiguous slot range (police_ranges):
//   police_sum    per-range, per-meter byte sums (LDS tallies) -> row g of the [G][kMaxMeters] workspace
//   police_scan   refill every configured meter at now_ns, allow = tokens / 1e9, an exclusive scan
//                 down the G rows (row g becomes range g's base), green sums zeroed; 16 workgroups,
//                 each alone with 16 meters' columns
//   police_apply  each workgroup re-reads its range in trips of 256 slots, forms the ordered
//                 per-meter inclusive prefix (a wave-level keyed scan over the distinct meters in
//                 the wave, the waves of a trip ordered through per-wave LDS rows), adds its base,
//                 compares with allow, marks red in-metas, tallies the meter counters in LDS (one
//                 global atomic per meter per workgroup) and each meter's green bytes
//   police_commit tokens -= green * 1e9
// and, after the fused kernel, police_fix restores the red slots' in-metas, rewrites their out
// metas and moves their drop count from bad_port to overflow.
// Everything is integer arithmetic: the result does not depend on the order of the atomics.
// Kept apart from kernels.hip so that file's register allocation does not move.
#include "host.h"
#include "police.h"

namespace nfdp {
namespace {

using u64 = unsigned long long;

// Inclusive add scan over the 64 lanes in DPP moves (every lane active): shifts by 1, 2, 4, 8 inside
// each row of 16 lanes, then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3 -
// the sequence LLVM's atomic optimizer emits for gfx9.  A lane with no source adds 0 (`old`).
// (As 6 dependent __shfl_up steps, an LDS-crossbar round trip each, the keyed scan of
// police_apply took 98 us per 4M slots of 8 meters; see docs/DATAPLANE.md "Policer".)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
#define NFDP_DPP_ADD(ctrl, rows) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xF, false)
  NFDP_DPP_ADD(0x111, 0xF);   // row_shr:1
  NFDP_DPP_ADD(0x112, 0xF);   // row_shr:2
  NFDP_DPP_ADD(0x114, 0xF);   // row_shr:4
  NFDP_DPP_ADD(0x118, 0xF);   // row_shr:8
  NFDP_DPP_ADD(0x142, 0xA);   // row_bcast:15 into rows 1, 3
  NFDP_DPP_ADD(0x143, 0xC);   // row_bcast:31 into rows 2, 3
#undef NFDP_DPP_ADD
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void police_sum_kernel(const uint32_t* inmeta, uint32_t n, uint32_t range,
                                                         const uint16_t* port_meter, u64* ws) {
  __shared__ u64 tally[kMaxMeters];
  tally[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t lo = blockIdx.x * range;
  const uint32_t hi = n - lo < range ? n : lo + range;
  for (uint32_t base = lo; base < hi; base += 256) {   // block-uniform trips
    const uint32_t i = base + threadIdx.x;
    int m = -1;
    uint32_t len = 0;
    if (i < hi) {
      const uint32_t im = inmeta[i];
      m = police_meter_of(port_meter, im);
      len = im >> 16;
    }
    // a wave whose metered frames all sit on one meter (the usual case) adds one sum: 64 lanes
    // on one LDS word serialise
    const u64 act = __ballot(m >= 0);
    if (act) {
      const int lead = __builtin_ctzll(act);
      const int m0 = __shfl(m, lead);
      if (!__ballot(m >= 0 && m != m0)) {
        uint32_t s = m >= 0 ? len : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((int)lane == lead) atomicAdd(&tally[m0], (u64)s);
      } else if (m >= 0) {
        atomicAdd(&tally[m], (u64)len);
      }
    }
  }
  __syncthreads();
  ws[(size_t)blockIdx.x * kMaxMeters + threadIdx.x] = tally[threadIdx.x];   // zeros too: no clear pass
}

// The meters' columns of the G rows are independent: workgroup j scans the 16 meters 16j .. 16j+15
// (one 128-B line per row), thread (q, c) a run of rows of meter 16j + c, the 64 runs chained
// through LDS.  (One workgroup over all 256 columns, 2 MB through one CU: 93 us per 4M slots.)
constexpr uint32_t kScanCols = 16, kScanRuns = 1024 / kScanCols;
__global__ __launch_bounds__(1024) void police_scan_kernel(PoliceArgs a, uint32_t groups) {
  __shared__ u64 part[kScanRuns][kScanCols];
  const uint32_t c = threadIdx.x % kScanCols, q = threadIdx.x / kScanCols;
  const uint32_t m = blockIdx.x * kScanCols + c;
  const uint32_t per = (groups + kScanRuns - 1) / kScanRuns;
  const uint32_t g0 = q * per < groups ? q * per : groups;
  const uint32_t g1 = g0 + per < groups ? g0 + per : groups;
  u64* col = a.ws + m;
  u64 sum = 0;
#pragma unroll 8
  for (uint32_t g = g0; g < g1; ++g) sum += col[(size_t)g * kMaxMeters];
  part[q][c] = sum;
  __syncthreads();
  u64 run = 0;
  for (uint32_t k = 0; k < q; ++k) run += part[k][c];
#pragma unroll 8
  for (uint32_t g = g0; g < g1; ++g) {
    const u64 v = col[(size_t)g * kMaxMeters];
    col[(size_t)g * kMaxMeters] = run;
    run += v;
  }
  if (q == 0) {
    const MeterCfg cfg = a.cfg[m];
    u64 allow = 0;
    if (cfg.rate_Bps) {
      MeterState st = a.state[m];
      meter_refill(cfg, st, a.now_ns);
      a.state[m] = st;
      allow = meter_allow(st);
    }
    a.ws[(size_t)kPoliceMaxGroups * kMaxMeters + m] = allow;
    a.ws[(size_t)(kPoliceMaxGroups + 1) * kMaxMeters + m] = 0;   // green bytes of this batch
  }
}

__global__ __launch_bounds__(256) void police_apply_kernel(uint32_t* inmeta, uint32_t n, uint32_t range,
                                                           PoliceArgs a) {
  __shared__ u64 run[kMaxMeters];        // meter's byte prefix before the current trip
  __shared__ u64 allow[kMaxMeters];
  __shared__ uint32_t wtot[4][kMaxMeters];   // this trip: bytes of the meter in each wave (0: none)
  __shared__ uint32_t gp[kMaxMeters], rp[kMaxMeters];
  __shared__ u64 gb[kMaxMeters], rb[kMaxMeters];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  run[t] = a.ws[(size_t)blockIdx.x * kMaxMeters + t];
  allow[t] = a.ws[(size_t)kPoliceMaxGroups * kMaxMeters + t];
#pragma unroll
  for (int w = 0; w < 4; ++w) wtot[w][t] = 0;
  gp[t] = 0; rp[t] = 0; gb[t] = 0; rb[t] = 0;
  __syncthreads();
  const uint32_t lo = blockIdx.x * range;
  const uint32_t hi = n - lo < range ? n : lo + range;
  auto fetch = [&](uint32_t base, uint32_t& im, int& m) {
    const uint32_t i = base + t;
    im = 0; m = -1;
    if (i < hi) { im = inmeta[i]; m = police_meter_of(a.port_meter, im); }
  };
  uint32_t im, nim;
  int m, nm;
  fetch(lo, im, m);
  for (uint32_t base = lo; base < hi; base += 256) {   // block-uniform trips, in slot order
    const uint32_t i = base + t;
    fetch(base + 256, nim, nm);   // the next trip's slots are in flight while this one is judged
    const uint32_t len = im >> 16;
    // keyed inclusive scan inside the wave: one round per distinct meter present
    uint32_t incl = 0;
    u64 kmask = 0;   // the lanes of this lane's meter
    u64 pend = __ballot(m >= 0);
    while (pend) {   // wave-uniform
      const int k = __shfl(m, __builtin_ctzll(pend));
      const bool mine = m == k;
      const u64 mk = __ballot(mine);
      if (__popcll(mk) == 1) {
        if (mine) { incl = len; kmask = mk; }
      } else {
        const uint32_t s = wave_incl_scan(mine ? len : 0u);
        if (mine) { incl = s; kmask = mk; }
      }
      pend &= ~mk;
    }
    const bool lead = m >= 0 && (int)lane == __builtin_ctzll(kmask);   // one lane per (wave, meter)
    const uint32_t tot = __shfl(incl, m >= 0 ? 63 - __builtin_clzll(kmask) : (int)lane);
    if (lead) wtot[wv][m] = tot;
    __syncthreads();
    bool green = false;
    if (m >= 0) {
      u64 pre = run[m] + incl;
      for (uint32_t w = 0; w < wv; ++w) pre += wtot[w][m];
      green = pre <= allow[m];
      if (!green) inmeta[i] = police_mark(im);
    }
    // per (wave, meter): a meter's green frames are a prefix of its frames, so its green bytes in
    // the wave are the inclusive sum at its last green lane
    const u64 gmask = __ballot(green) & kmask;
    const uint32_t gsum = __shfl(incl, gmask ? 63 - __builtin_clzll(gmask) : (int)lane);
    const uint32_t gby = gmask ? gsum : 0u;
    __syncthreads();   // every read of run / wtot of this trip is done
    if (lead) {
      const uint32_t gpk = (uint32_t)__popcll(gmask);
      atomicAdd(&run[m], (u64)tot);
      wtot[wv][m] = 0;
      if (gpk) { atomicAdd(&gp[m], gpk); atomicAdd(&gb[m], (u64)gby); }
      if ((uint32_t)__popcll(kmask) != gpk) {
        atomicAdd(&rp[m], (uint32_t)__popcll(kmask) - gpk);
        atomicAdd(&rb[m], (u64)(tot - gby));
      }
    }
    im = nim; m = nm;
    // (no third barrier: the next trip's first one orders these updates before its reads, and a
    // wave rewrites only its own wtot row)
  }
  __syncthreads();
  if (gb[t]) atomicAdd(a.ws + (size_t)(kPoliceMaxGroups + 1) * kMaxMeters + t, gb[t]);
  if (a.count && a.meter_ctr) {
    u64* c = a.meter_ctr + 4 * t;
    if (gp[t]) { atomicAdd(c, (u64)gp[t]); atomicAdd(c + 1, gb[t]); }
    if (rp[t]) { atomicAdd(c + 2, (u64)rp[t]); atomicAdd(c + 3, rb[t]); }
  }
}

__global__ __launch_bounds__(256) void police_commit_kernel(PoliceArgs a) {
  const uint32_t m = threadIdx.x;
  const u64 green = a.ws[(size_t)(kPoliceMaxGroups + 1) * kMaxMeters + m];
  if (a.cfg[m].rate_Bps && green) {
    MeterState st = a.state[m];
    meter_charge(st, green);
    a.state[m].tokens = st.tokens;
  }
}

// After the fused kernel: red slots' in-metas restored, their out metas -> overflow drops, their
// bad_port count (in-meta port >= kMaxPorts) moved to overflow.
__global__ __launch_bounds__(256) void police_fix_kernel(uint32_t* inmeta, uint32_t* out_meta, uint32_t n,
                                                         u64* drop_ctr, uint32_t count) {
  __shared__ uint32_t c;
  if (threadIdx.x == 0) c = 0;
  __syncthreads();
  uint32_t mine = 0;
  // (n < 2^31 and the stride is at most 2^18: i never wraps)
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t im = inmeta[i];
    if (!police_marked(im)) continue;
    inmeta[i] = police_unmark(im);
    out_meta[i] = make_meta(kPortNone, im >> 16, kOverflow);
    ++mine;
  }
  if (mine) atomicAdd(&c, mine);
  __syncthreads();
  if (threadIdx.x == 0 && c && count) {
    atomicAdd(drop_ctr + kBadPort, 0ull - (u64)c);
    atomicAdd(drop_ctr + kOverflow, (u64)c);
  }
}

hipError_t launch_police(uint32_t* inmeta, uint32_t n, const PoliceArgs& a, hipStream_t s, uint32_t phases) {
  if (!a.port_meter || !a.cfg || !a.state || !a.ws || (n && !inmeta)) return hipErrorInvalidValue;
  if (n > 0x7FFFFFFFu) return hipErrorInvalidValue;
  uint32_t groups = 0, range = kPoliceRangeAlign;
  if (n) police_ranges(n, groups, range);
  if (groups && (phases & 1u))
    hipLaunchKernelGGL(police_sum_kernel, dim3(groups), dim3(256), 0, s, inmeta, n, range, a.port_meter, a.ws);
  if (phases & 2u)
    hipLaunchKernelGGL(police_scan_kernel, dim3(kMaxMeters / kScanCols), dim3(1024), 0, s, a, groups);
  if (groups && (phases & 4u))
    hipLaunchKernelGGL(police_apply_kernel, dim3(groups), dim3(256), 0, s, inmeta, n, range, a);
  if (groups && (phases & 8u)) hipLaunchKernelGGL(police_commit_kernel, dim3(1), dim3(kMaxMeters), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_police_fix(uint32_t* inmeta, uint32_t* out_meta, uint32_t n, unsigned long long* drop_ctr,
                             bool count, hipStream_t s) {
  if (!inmeta || !out_meta || !drop_ctr) return hipErrorInvalidValue;
  if (n > 0x7FFFFFFFu) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const uint32_t g = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(police_fix_kernel, dim3(g), dim3(256), 0, s, inmeta, out_meta, n, drop_ctr, count ? 1u : 0u);
  return hipGetLastError();
}

}  // namespace nfdp
