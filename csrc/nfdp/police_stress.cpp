// police_stress.cpp — stand-alone driver of the policer's CPU oracle (host.cpp oracle_police /
// oracle_police_fix) for the host-only sanitizer build (native/build.py build_sanitized, target
// "police"): random batches over exactly sized heap buffers (so an out-of-bounds access is caught),
// extreme rates, bursts and arrival times (so an overflow in the refill is caught by UBSan's
// checks and by the invariants below), checked against a naive re-statement of the contract.
// Usage: police_stress [batches]   -> prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "host.h"

using namespace nfdp;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "police_stress: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  const int batches = argc > 1 ? std::atoi(argv[1]) : 200;
  std::mt19937_64 rng(7);
  std::vector<uint16_t> port_meter(kMaxPorts, 0);
  std::vector<MeterCfg> cfg(kMaxMeters);
  std::vector<MeterState> st(kMaxMeters);
  std::vector<unsigned long long> ctr(4 * kMaxMeters, 0);
  std::vector<uint64_t> drop(kNumReasons, 0);
  const uint64_t rates[] = {125000ull, 100000000ull, kMeterMaxRate};
  const uint64_t bursts[] = {1ull, 6000ull, 2 * kMaxFrame, kMeterMaxBurst};
  for (int m = 0; m < kMaxMeters; ++m) {
    if (m % 5 == 4) { cfg[m] = MeterCfg{}; st[m] = MeterState{}; continue; }   // not configured
    const uint64_t r = rates[rng() % 3], b = bursts[rng() % 4];
    cfg[m] = MeterCfg{r, b, (b * kNano + r - 1) / r, 0};
    st[m] = MeterState{b * kNano, 0};
  }
  for (int p = 0; p < kMaxPorts; ++p)
    if (rng() % 3) port_meter[p] = (uint16_t)(1 + rng() % kMaxMeters);
  for (int m = 4; m < kMaxMeters; m += 5)     // (the host binds no port to a meter that is not configured)
    for (int p = 0; p < kMaxPorts; ++p)
      if (port_meter[p] == m + 1) port_meter[p] = 0;
  const unsigned long long times[] = {0ull, 1ull, 1000ull, 1000000ull, 999ull, 1ull << 40, 1ull << 63, ~0ull, 5ull};
  uint64_t judged = 0;
  for (int it = 0; it < batches; ++it) {
    const uint32_t n = it % 7 == 0 ? 0u : (uint32_t)(1 + rng() % 3000);
    std::vector<uint32_t> im(n), out_meta(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t k = (uint32_t)(rng() % 16);
      const uint32_t port = k == 0 ? kPortCont : k == 1 ? (uint32_t)kMaxPorts + (uint32_t)(rng() % 8) : k == 2 ? 0xFFFFu
                                                        : (uint32_t)(rng() % (k < 8 ? 16 : kMaxPorts));
      im[i] = port | ((uint32_t)(rng() % 65536) << 16);
    }
    const std::vector<uint32_t> im0 = im;
    const std::vector<MeterState> before = st;
    PoliceArgs a{port_meter.data(), cfg.data(), st.data(), ctr.data(), nullptr, times[it % 9], 1u};
    oracle_police(im.data(), n, a);
    // the contract, restated slot by slot
    std::vector<uint64_t> used(kMaxMeters, 0), green(kMaxMeters, 0);
    uint64_t red = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t port = im0[i] & 0xFFFFu;
      const int m = port < (uint32_t)kMaxPorts ? (int)port_meter[port] - 1 : -1;
      if (m < 0) { REQUIRE(im[i] == im0[i]); continue; }
      MeterState s = before[m];
      meter_refill(cfg[m], s, a.now_ns);
      REQUIRE(s.tokens <= cfg[m].burst_bytes * kNano);
      used[m] += im0[i] >> 16;
      const bool ok = used[m] <= s.tokens / kNano;
      REQUIRE(police_marked(im[i]) == !ok);
      REQUIRE(police_unmark(im[i]) == im0[i]);
      if (ok) green[m] += im0[i] >> 16; else ++red;
      ++judged;
    }
    for (int m = 0; m < kMaxMeters; ++m) {
      if (!cfg[m].rate_Bps) { REQUIRE(st[m].tokens == 0 && st[m].last_ns == 0); continue; }
      MeterState s = before[m];
      meter_refill(cfg[m], s, a.now_ns);
      REQUIRE(st[m].tokens == s.tokens - green[m] * kNano && st[m].last_ns == s.last_ns);
      REQUIRE(st[m].last_ns >= before[m].last_ns);
    }
    drop[kBadPort] += red;   // what the pipeline would have counted for the marked slots
    oracle_police_fix(im.data(), out_meta.data(), n, drop.data(), true);
    REQUIRE(im == im0);
    for (uint32_t i = 0; i < n; ++i)
      if (out_meta[i]) REQUIRE(meta_reason(out_meta[i]) == kOverflow && meta_port(out_meta[i]) == kPortNone);
    REQUIRE(drop[kBadPort] == 0);
  }
  uint64_t counted = 0;
  for (int m = 0; m < kMaxMeters; ++m) counted += ctr[4 * m] + ctr[4 * m + 2];
  REQUIRE(counted == judged && judged > 0);
  std::printf("ok\n");
  return 0;
}
