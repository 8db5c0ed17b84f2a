// age.h — per-flow idle timeout: a device-side aging sweep over the flow table's packed counters.
// The silicon the reference offloads flows to ages them itself (OvS max-idle / revalidation on the
// OvS-DPDK data path, the flow AGE action with an aged-flow query on DPU NICs); here the "silicon"
// is our kernels (age.hip), so the sweep decides expiry in HBM and the host gets only the list of
// expired slots, instead of a copy of every counter (DataPlane.harvest: 8 B per slot).
//
// Contract (shared by the oracle in host.cpp, the kernels in age.hip and the tests):
//   * one AgeRow {u64 seen; u32 last; u32 tmo} per flow slot, nbuckets * 4 rows, in a buffer of
//     their own (FlowSlot, FlowAction, TablesView and the packet kernels do not know it).
//     tmo bits 0..29: the idle timeout in ticks (0: the slot is not aged), bit 31 kAgeNew: armed,
//     not yet seen by a sweep, bit 30 kAgeTouched: a harvest saw traffic since the last sweep.
//   * time is a u32 tick count (the host: (now_ns - epoch_ns) / tick_ns); every comparison is
//     u32 and wrap-safe: (now - last) >= tmo.
//   * sweep, per slot, c = flow_ctr[slot]:
//       1. timeout 0: skipped (row not written, counter not read);
//       2. kAgeNew: last = now, seen = c, both flags cleared; never expires in this sweep;
//       3. c != seen or kAgeTouched: last = now, seen = c, flag cleared;
//       4. else, now - last >= tmo: EXPIRED (equality expires); the slot index goes to the list,
//          the row is NOT modified (so a sweep whose list overflowed finds it again).
//     Outputs: count = all expired slots (may exceed cap), list = the first min(count, cap) slots
//     claimed, in no particular order (the oracle: slot order).
//   * age-aware harvest (in place of harvest_kernel while aging is on), per slot:
//       v = exchange(ctr, 0); out = v; armed and v != seen: kAgeTouched set; seen = 0.
//     So a harvest between two sweeps neither hides traffic nor fakes it.
//   * granularity: activity is dated to the sweep that observed it.  A flow lives at least its
//     timeout and less than its timeout plus two sweep intervals.
#pragma once
#include <cstdint>

#include "nfdp.h"

namespace nfdp {

constexpr uint32_t kAgeNew = 0x80000000u;
constexpr uint32_t kAgeTouched = 0x40000000u;
constexpr uint32_t kAgeTmoMask = 0x3FFFFFFFu;   // timeouts: 1 .. 2^30 - 1 ticks
constexpr uint32_t kAgeBlock = 256;             // threads of a sweep workgroup, one slot each per pass
constexpr uint32_t kAgeMaxGroups = 2048;        // grid cap: 8 workgroups of 4 waves on each of 256 CUs

struct AgeRow {
  uint64_t seen;   // the packed counter as the last sweep (or harvest: 0) left it
  uint32_t last;   // tick of the last sweep that saw activity
  uint32_t tmo;    // timeout ticks | kAgeNew | kAgeTouched
};
static_assert(sizeof(AgeRow) == 16, "age row layout");

enum AgeVerdict : int { kAgeSkip = 0, kAgeKeep = 1, kAgeRefresh = 2, kAgeExpired = 3 };

// One slot's sweep step (rules 1 - 4): kAgeRefresh means `r` changed and is to be stored.
NFDP_HD AgeVerdict age_step(AgeRow& r, uint64_t c, uint32_t now) {
  const uint32_t tmo = r.tmo & kAgeTmoMask;
  if (!tmo) return kAgeSkip;
  if ((r.tmo & (kAgeNew | kAgeTouched)) || c != r.seen) {
    r.last = now; r.seen = c; r.tmo = tmo;
    return kAgeRefresh;
  }
  return (uint32_t)(now - r.last) >= tmo ? kAgeExpired : kAgeKeep;
}

// One slot's harvest step on the counter value `v` just exchanged out: true when `r` changed.
NFDP_HD bool age_harvest_step(AgeRow& r, uint64_t v) {
  const AgeRow o = r;
  if ((r.tmo & kAgeTmoMask) && v != r.seen) r.tmo |= kAgeTouched;
  r.seen = 0;
  return r.tmo != o.tmo || r.seen != o.seen;
}

// Launch geometry of a sweep / age-aware harvest over n slots: `groups` workgroups of kAgeBlock
// threads; a thread takes slots i, i + per_pass, ... (per_pass = groups * kAgeBlock).
inline void age_grid(uint64_t n, uint32_t& groups, uint32_t& per_pass) {
  const uint64_t g = (n + kAgeBlock - 1) / kAgeBlock;
  groups = (uint32_t)(g < kAgeMaxGroups ? (g ? g : 1) : kAgeMaxGroups);
  per_pass = groups * kAgeBlock;
}

}  // namespace nfdp
