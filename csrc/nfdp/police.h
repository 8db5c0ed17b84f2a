// police.h — per-vport max_tx_rate: a single-rate, two-colour, byte-based token-bucket policer on
// ingress vports (what a VF transmits enters the switch on its vport).  The reference leaves
// `ip link set … vf N max_tx_rate` to the NIC (dpu-cni/pkgs/sriov/sriov.go LinkSetVfRate); here the
// "VF" is a GPU vport, so the limit is enforced by passes around the fused kernel (police.hip),
// the way pair_kernel / pair_fix_kernel resolve wide header pairs around it.
//
// Contract (shared by the oracle in host.cpp, the kernels in police.hip and the tests):
//   * kMaxMeters meters; port_meter[kMaxPorts] (u16): 0 = unmetered, else meter id + 1.  Ports may
//     share a meter.  A meter with rate_Bps == 0 is not configured (the host binds no port to it).
//   * state per meter: tokens in 1e-9 byte, last_ns.  A new / re-configured meter starts full
//     (tokens = burst * 1e9, last_ns = 0).
//   * a batch has ONE arrival time now_ns.  Refill: elapsed = max(0, now - last), clamped to
//     full_ns = ceil(burst * 1e9 / rate) (so nothing overflows: every intermediate < 2^63 for
//     rate <= 5e10 B/s, burst < 2^31), tokens = min(burst * 1e9, tokens + elapsed * rate),
//     last = max(last, now).
//   * allow = tokens / 1e9 (whole bytes).  In slot order a frame of meter m is green iff the
//     inclusive sum of the in-meta lengths of it and of all earlier frames of m in the batch (red
//     ones too) is <= allow: the green set is the maximal prefix that fits.  Then
//     tokens -= green_bytes * 1e9 (the sub-byte remainder carries over).
//   * slots whose in-meta port is >= kMaxPorts (kPortCont too) or unmetered are not judged.
//   * a red frame's in-meta port becomes kPoliceMark | port: the fused kernel and the oracle drop
//     it as bad_port unchanged; the fix pass restores the in-meta, rewrites the out meta to
//     make_meta(kPortNone, len, kOverflow) and moves the count from bad_port to overflow.  In-meta
//     ports 0xE000..0xEFFF are therefore reserved while a port is bound to a meter.
//   * meter_ctr[m] = {green_pkts, green_bytes, red_pkts, red_bytes} (u64 each).
#pragma once
#include "nfdp.h"

namespace nfdp {

constexpr int kMaxMeters = 256;
constexpr uint64_t kNano = 1000000000ull;          // token unit: 1e-9 byte
constexpr uint32_t kPoliceMark = 0xE000u;          // in-meta port of a red frame: kPoliceMark | port
constexpr uint32_t kPoliceMaxGroups = 1024;        // workgroups of a police launch (one slot range each)
constexpr uint32_t kPoliceRangeAlign = 256;        // a range is a multiple of the workgroup's 256 slots
constexpr uint64_t kMeterMaxRate = 50000000000ull; // 400 Gbit/s in bytes per second
constexpr uint64_t kMeterMaxBurst = 0x7FFFFFFFull;

struct MeterCfg {
  uint64_t rate_Bps;     // 0: not configured
  uint64_t burst_bytes;
  uint64_t full_ns;      // ceil(burst_bytes * 1e9 / rate_Bps): an empty bucket is full after this long
  uint64_t pad;
};
struct MeterState {
  uint64_t tokens;       // 1e-9 byte
  uint64_t last_ns;
};
static_assert(sizeof(MeterCfg) == 32 && sizeof(MeterState) == 16, "meter table layout");

// One batch's police arguments (device or host pointers).
struct PoliceArgs {
  const uint16_t* port_meter;        // kMaxPorts
  const MeterCfg* cfg;               // kMaxMeters
  MeterState* state;                 // kMaxMeters
  unsigned long long* meter_ctr;     // kMaxMeters * 4 (null or count == 0: not counted)
  unsigned long long* ws;            // police_ws_words() u64 (GPU only)
  unsigned long long now_ns;
  uint32_t count;
};

NFDP_HD void meter_refill(const MeterCfg& c, MeterState& s, uint64_t now_ns) {
  uint64_t el = now_ns > s.last_ns ? now_ns - s.last_ns : 0ull;
  if (el > c.full_ns) el = c.full_ns;
  const uint64_t cap = c.burst_bytes * kNano;
  const uint64_t t = s.tokens + el * c.rate_Bps;   // < 2 * cap + rate < 2^63
  s.tokens = t < cap ? t : cap;
  if (now_ns > s.last_ns) s.last_ns = now_ns;
}
NFDP_HD uint64_t meter_allow(const MeterState& s) { return s.tokens / kNano; }
NFDP_HD void meter_charge(MeterState& s, uint64_t green_bytes) { s.tokens -= green_bytes * kNano; }

// The meter a slot is charged to (-1: not judged).
NFDP_HD int police_meter_of(const uint16_t* port_meter, uint32_t inmeta) {
  const uint32_t port = inmeta & 0xFFFFu;
  if (port >= (uint32_t)kMaxPorts) return -1;
  const int m = (int)port_meter[port] - 1;
  return m < kMaxMeters ? m : -1;
}
NFDP_HD uint32_t police_mark(uint32_t inmeta) { return (inmeta & 0xFFFF0FFFu) | kPoliceMark; }
NFDP_HD bool police_marked(uint32_t inmeta) { return (inmeta & 0xF000u) == kPoliceMark; }
NFDP_HD uint32_t police_unmark(uint32_t inmeta) { return inmeta & 0xFFFF0FFFu; }

// Slot ranges of a launch over n slots: `groups` workgroups of `range` slots each (the last one
// ragged).  range is a multiple of kPoliceRangeAlign, groups <= kPoliceMaxGroups.
inline void police_ranges(uint32_t n, uint32_t& groups, uint32_t& range) {
  const uint64_t per = ((uint64_t)n + kPoliceMaxGroups - 1) / kPoliceMaxGroups;
  uint64_t r = (per + kPoliceRangeAlign - 1) / kPoliceRangeAlign * kPoliceRangeAlign;
  if (r == 0) r = kPoliceRangeAlign;
  range = (uint32_t)r;
  groups = (uint32_t)(((uint64_t)n + r - 1) / r);
}
// workspace words (u64): [kPoliceMaxGroups][kMaxMeters] range sums / bases, allow[], green[]
constexpr size_t police_ws_words() { return (size_t)(kPoliceMaxGroups + 2) * kMaxMeters; }

}  // namespace nfdp
