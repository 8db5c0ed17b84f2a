// age_stress.cpp — stand-alone driver of the flow-aging CPU oracles (host.cpp oracle_age_sweep /
// oracle_harvest_age) for the host-only sanitizer build (native/build.py build_sanitized, target
// "age"): random tables over exactly sized heap buffers (so an out-of-bounds access is caught),
// ticks on both sides of the u32 wrap, cap of 0, 1 and n, sweeps interleaved with traffic and
// harvests, checked against a re-statement of the contract (age.h) slot by slot.
// Usage: age_stress [rounds]   -> prints "ok".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "host.h"

using namespace nfdp;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "age_stress: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 300;
  std::mt19937_64 rng(11);
  uint64_t expired_seen = 0, refreshed_seen = 0, touched_seen = 0;
  for (int it = 0; it < rounds; ++it) {
    const uint64_t n = it % 9 == 0 ? 0 : 1 + rng() % 700;
    const uint32_t cap = it % 3 == 0 ? 0u : it % 3 == 1 ? 1u : (uint32_t)n;
    // exactly sized heap buffers (no vector slack)
    std::unique_ptr<uint64_t[]> ctr(new uint64_t[n]), hv(new uint64_t[n]);
    std::unique_ptr<AgeRow[]> rows(new AgeRow[n]);
    std::unique_ptr<uint32_t[]> out(new uint32_t[cap]);
    uint32_t now = it % 4 == 0 ? 0xFFFFFFF0u + (uint32_t)(rng() % 16) : (uint32_t)rng();   // near / across the wrap
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t k = (uint32_t)(rng() % 8);
      const uint32_t tmo = k == 0 ? 0u : k == 1 ? kAgeTmoMask : 1u + (uint32_t)(rng() % 40);
      const uint32_t fl = k == 0 ? 0u : (rng() % 4 == 0 ? kAgeNew : 0u) | (rng() % 5 == 0 ? kAgeTouched : 0u);
      ctr[i] = rng() % 3 ? (rng() % 4) << 40 | (rng() % 9000) : 0;
      rows[i] = AgeRow{rng() % 2 ? ctr[i] : rng() % 5, now - (uint32_t)(rng() % 48), tmo | fl};
    }
    for (int step = 0; step < 6; ++step) {
      std::vector<AgeRow> before(rows.get(), rows.get() + n);
      std::vector<uint64_t> c0(ctr.get(), ctr.get() + n);
      if (step % 3 == 2) {
        oracle_harvest_age(ctr.get(), rows.get(), hv.get(), n);
        for (uint64_t i = 0; i < n; ++i) {
          REQUIRE(hv[i] == c0[i] && ctr[i] == 0 && rows[i].seen == 0 && rows[i].last == before[i].last);
          const bool armed = before[i].tmo & kAgeTmoMask;
          const uint32_t want = before[i].tmo | (armed && c0[i] != before[i].seen ? kAgeTouched : 0u);
          REQUIRE(rows[i].tmo == want);
          touched_seen += want != before[i].tmo;
        }
      } else {
        uint32_t count = 0xDEADBEEFu;
        oracle_age_sweep(ctr.get(), rows.get(), n, now, out.get(), cap, &count);
        uint32_t want = 0;
        for (uint64_t i = 0; i < n; ++i) {
          const AgeRow b = before[i];
          const uint32_t tmo = b.tmo & kAgeTmoMask;
          if (!tmo) { REQUIRE(!std::memcmp(&rows[i], &b, sizeof b)); continue; }
          if ((b.tmo & kAgeNew) || (b.tmo & kAgeTouched) || c0[i] != b.seen) {
            REQUIRE(rows[i].last == now && rows[i].seen == c0[i] && rows[i].tmo == tmo);
            ++refreshed_seen;
            continue;
          }
          REQUIRE(!std::memcmp(&rows[i], &b, sizeof b));   // kept or expired: the row is not modified
          if ((uint32_t)(now - b.last) >= tmo) {
            if (want < cap) REQUIRE(out[want] == (uint32_t)i);   // slot order
            ++want;
          }
        }
        REQUIRE(count == want);
        expired_seen += want;
        for (uint64_t i = 0; i < n; ++i) REQUIRE(ctr[i] == c0[i]);
      }
      // traffic on some slots, time moves on (sometimes over the wrap)
      for (uint64_t i = 0; i < n; ++i)
        if (rng() % 4 == 0) ctr[i] += (1ull << 40) | 64;
      now += (uint32_t)(rng() % 24);
    }
  }
  REQUIRE(expired_seen > 0 && refreshed_seen > 0 && touched_seen > 0);
  std::printf("ok\n");
  return 0;
}
