"""Flow aging on the CPU (csrc/nfdp/age.h): the sweep / harvest oracles category by category, and
DataPlane("cpu") against an independent model (flow_aging_common.Model: a dict key -> timeout, last
observed tick) through schedules of traffic, inserts, erases, timeout changes, harvests and sweeps."""
import numpy as np
import pytest

import flow_aging_common as C
from dpu_operator_amd.dataplane import scenario as S
from dpu_operator_amd.dataplane import tables as T
from dpu_operator_amd.dataplane.engine import DataPlane

NEW, TOUCHED = T.AGE_NEW, T.AGE_TOUCHED


def _sweep(nf, rows, ctr, now, cap=None):
    rows = np.array(rows, T.AGE_ROW_DTYPE)
    ctr = np.array(ctr, np.uint64)
    cap = len(rows) if cap is None else cap
    out = np.full(max(cap, 1), 0xFFFFFFFF, np.uint32)
    cnt = np.zeros(1, np.uint32)
    nf.oracle_age_sweep(ctr.ctypes.data, rows.ctypes.data, len(rows), now, out.ctypes.data, cap, cnt.ctypes.data)
    return rows, int(cnt[0]), out[: min(int(cnt[0]), cap)].tolist()


def _row(r):
    return (int(r["seen"]), int(r["last"]), int(r["tmo"]))


def test_constants_match_the_header(nf):
    assert (nf.AGE_NEW, nf.AGE_TOUCHED, nf.AGE_TMO_MASK) == (T.AGE_NEW, T.AGE_TOUCHED, T.AGE_TMO_MASK)
    assert nf.age_grid(1) == (1, 256) and nf.age_grid(257) == (2, 512)
    g, per = nf.age_grid(1 << 30)
    assert per == g * 256 and nf.age_grid(per + 1) == (g, per)   # capped: a second pass from per + 1 on


def test_sweep_unarmed_row_is_not_touched(nf):
    rows, cnt, lst = _sweep(nf, [(7, 3, 0), (9, 1, TOUCHED), (9, 1, NEW)], [5, 5, 5], 1000)
    assert [_row(r) for r in rows] == [(7, 3, 0), (9, 1, TOUCHED), (9, 1, NEW)] and cnt == 0 and lst == []


def test_sweep_new_row_is_dated_and_never_expires(nf):
    rows, cnt, _ = _sweep(nf, [(0, 0, 5 | NEW), (0, 0, 5 | NEW | TOUCHED)], [42, 0], 1000)
    assert [_row(r) for r in rows] == [(42, 1000, 5), (0, 1000, 5)] and cnt == 0


def test_sweep_touched_row_is_active(nf):
    rows, cnt, _ = _sweep(nf, [(0, 10, 5 | TOUCHED)], [0], 1000)   # c == seen, but a harvest saw traffic
    assert _row(rows[0]) == (0, 1000, 5) and cnt == 0


def test_sweep_counter_moved_is_active(nf):
    rows, cnt, _ = _sweep(nf, [(41, 10, 5)], [42], 1000)
    assert _row(rows[0]) == (42, 1000, 5) and cnt == 0


def test_sweep_idle_one_tick_short_is_kept_and_equality_expires(nf):
    rows, cnt, lst = _sweep(nf, [(42, 996, 5), (42, 995, 5), (42, 0, 5)], [42, 42, 42], 1000)
    assert cnt == 2 and lst == [1, 2]
    # kept and expired rows alike are bit-identical after the sweep
    assert [_row(r) for r in rows] == [(42, 996, 5), (42, 995, 5), (42, 0, 5)]


def test_sweep_is_wrap_safe(nf):
    last = 0xFFFFFFFE
    rows, cnt, lst = _sweep(nf, [(1, last, 5), (1, last, 6), (1, last, T.AGE_TMO_MASK)], [1, 1, 1], 3)   # now - last = 5
    assert cnt == 1 and lst == [0]
    rows, cnt, _ = _sweep(nf, [(1, 3, 5 | TOUCHED)], [1], 0xFFFFFFFF)
    assert _row(rows[0]) == (1, 0xFFFFFFFF, 5) and cnt == 0


def test_sweep_cap_smaller_than_count(nf):
    before = [(9, 0, 1)] * 10
    rows, cnt, lst = _sweep(nf, before, [9] * 10, 50, cap=3)
    assert cnt == 10 and lst == [0, 1, 2]
    assert [_row(r) for r in rows] == before                      # the next sweep finds them all again
    _, cnt, lst = _sweep(nf, rows, [9] * 10, 51, cap=0)
    assert cnt == 10 and lst == []


def test_harvest_oracle(nf):
    rows = np.array([(5, 7, 3), (5, 7, 3), (0, 7, 3 | NEW), (4, 7, 0), (0, 0, 0)], T.AGE_ROW_DTYPE)
    ctr = np.array([5, 6, 9, 8, 2], np.uint64)
    out = np.zeros(5, np.uint64)
    nf.oracle_harvest_age(ctr.ctypes.data, rows.ctypes.data, out.ctypes.data, 5)
    assert out.tolist() == [5, 6, 9, 8, 2] and not ctr.any()
    assert [_row(r) for r in rows] == [(0, 7, 3), (0, 7, 3 | TOUCHED), (0, 7, 3 | NEW | TOUCHED), (0, 7, 0), (0, 0, 0)]


# ---------------------------------------------------------------------------------- DataPlane
def _planes(installed=200, max_expired=65536):
    dp, sc = C.make_plane("cpu", 1 << 10, 256, installed, max_expired=max_expired)
    ref_all, _ = C.make_plane("cpu", 1 << 10, 256, 256, aging=False)
    ref_none, _ = C.make_plane("cpu", 1 << 10, 256, 0, aging=False)
    return dp, sc, ref_all, ref_none


def test_schedule_against_the_model():
    dp, sc, ref_all, ref_none = _planes()
    r = C.Runner(dp, sc, 200, ref_all, ref_none)
    sets = C.model_schedule(r, 200)
    assert sum(len(s) for s in sets) == 113
    st = dp.flow_age_stats()
    assert st["expired_total"] == 113 and st["sweeps"] == len(sets) and st["armed"] == 0
    assert len(dp.flows) == 220 - 113


def test_harvest_between_traffic_and_sweep_keeps_the_flow_and_the_counters():
    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200)
    twin, _ = C.make_plane("cpu", 1 << 10, 256, 200, aging=False)
    r = C.Runner(dp, sc, 200)
    r.arm(np.arange(0, 10), 0.5)
    r.sweep(0.0)
    pk, im = S.traffic(sc, 64, seed=5, flows=np.arange(0, 5))
    dp.run(pk, im.copy())
    twin.run(pk, im.copy())
    for i in range(5):
        r.model.hit(C.key_of(sc, i))
    for i in range(10):
        assert dp.flow_counters(sc.keys[i]) == twin.flow_counters(sc.keys[i])     # (each call harvests)
    assert dp.flow_counters(sc.keys[0])[0] > 0
    assert r.sweep(0.5) == {C.key_of(sc, i) for i in range(5, 10)}               # 0..4 count as active
    dp.run(pk, im.copy())
    twin.run(pk, im.copy())
    dp.harvest()
    twin.harvest()
    assert np.array_equal(dp.flow_totals, twin.flow_totals)
    for i in range(5):
        r.model.hit(C.key_of(sc, i))
    assert not r.sweep(0.9)
    assert len(r.sweep(1.4)) == 5


def test_rows_follow_cuckoo_moves():
    dp, sc = C.make_plane("cpu", 16, 64, 0, seed=1)
    r = C.Runner(dp, sc, 0)
    peak = C.moves_schedule(r)                 # expiry by key equals the model at every sweep
    assert peak >= 55                          # past 85 % of 64 slots
    assert dp.flow_age_stats()["relocated"] > 0
    assert not dp.age_rows()["tmo"].any()


def test_moved_row_keeps_its_clock_exactly():
    dp, sc = C.make_plane("cpu", 16, 64, 0, seed=1)
    dp.flows.insert_many(sc.keys[:30], sc.actions[:30])
    dp.set_flow_timeout(sc.keys[:30], np.arange(30) * 0.1 + 1.0)
    dp.age_flows(C.BASE_NS)
    before = {C.key_of(sc, i): dp.age_rows()[dp.flows.find(sc.keys[i])].copy() for i in range(30)}
    pk, im = S.traffic(sc, 64, seed=4, flows=np.arange(0, 30))
    dp.run(pk, im.copy())                      # counters stand when the inserts move entries
    for n in range(30, 58):
        dp.flows.insert(sc.keys[n], sc.actions[n])
    dp.commit()
    assert dp.flow_age_stats()["relocated"] > 0
    rows = dp.age_rows()
    for i in range(30):
        row = rows[dp.flows.find(sc.keys[i])]
        assert (row["last"], row["tmo"] & T.AGE_TMO_MASK) == (before[C.key_of(sc, i)]["last"], 10 + i)
        assert row["seen"] == 0                # the age-aware harvest ran before the move
    armed = np.nonzero(rows["tmo"])[0]
    assert sorted(armed) == sorted(dp.flows.find(sc.keys[i]) for i in range(30))   # nothing left behind
    assert np.array_equal(dp.flow_timeouts(sc.keys[:30]), 10 + np.arange(30))


def test_erase_and_reinsert_gives_a_fresh_clock_and_zero_disarms():
    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200)
    r = C.Runner(dp, sc, 200)
    r.arm(np.arange(0, 4), 0.5)
    r.sweep(0.0)
    r.erase([0])
    r.insert([0])                              # same key, same commit: the row is cleared, unarmed
    r.erase([1])
    r.insert([1])
    r.arm([1], 0.5)                            # armed again: dated by the next sweep
    r.arm([2], 0)
    assert r.sweep(0.5) == {C.key_of(sc, 3)}
    assert dp.flow_age_stats()["armed"] == 1
    assert not r.sweep(0.9)
    assert r.sweep(1.0) == {C.key_of(sc, 1)}
    assert dp.flows.find(sc.keys[0]) >= 0 and dp.flows.find(sc.keys[2]) >= 0
    assert not dp.age_rows()["tmo"].any()


def test_list_smaller_than_the_expired_set_drains_over_calls():
    dp, sc, ref_all, ref_none = _planes(max_expired=7)
    r = C.Runner(dp, sc, 200, ref_all, ref_none)
    r.arm(np.arange(0, 40), 0.5)
    r.sweep(0.0)
    now = C.BASE_NS + 5 * C.TICK_NS
    first = dp.age_flows(now)
    assert len(first) == 7 and dp.flow_age_stats()["armed"] == 33
    for k in first:
        r.model.erase(tuple(int(x) for x in k))
        r.installed.discard(int(np.nonzero((sc.keys == k).all(axis=1))[0][0]))
    rest = r.sweep(0.5, drain=True)            # no duplicates, the union is the model's set
    assert len(rest) == 33 and not rest & {tuple(int(x) for x in k) for k in first}
    assert dp.flow_age_stats()["sweeps"] == 1 + 1 + 5 + 1
    r.traffic(np.arange(0, 60))                # the 40 miss, the others forward as before


def test_expired_ipv6_flow_leaves_the_side_table():
    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200)
    act = T.flow_action(chain_id=sc.chain_id, out_port=1)[0]
    dp.add_flow6("fd00::1", "fd00::2", 1000, 2000, 17, sc.bridge, act)
    dp.add_flow6("fd00::3", "fd00::4", 1000, 2000, 17, sc.bridge, act)
    k1, _ = T.flow_key6("fd00::1", "fd00::2", 1000, 2000, 17, sc.bridge)
    k2, _ = T.flow_key6("fd00::3", "fd00::4", 1000, 2000, 17, sc.bridge)
    assert dp.set_flow_timeout(k1, 0.3) == 1
    assert len(dp.age_flows(C.BASE_NS)) == 0
    got = dp.age_flows(C.BASE_NS + 3 * C.TICK_NS)
    assert [tuple(int(x) for x in k) for k in got] == [tuple(int(x) for x in k1)]
    assert tuple(int(x) for x in k1) not in dp.flows6 and tuple(int(x) for x in k2) in dp.flows6
    assert dp.flows.find(k1) < 0 and dp.flows.find(k2) >= 0


class _Spy:
    def __init__(self, nf):
        self._nf, self.calls = nf, []

    def __getattr__(self, name):
        if "age" in name or "harvest" in name:
            self.calls.append(name)
        return getattr(self._nf, name)


def test_off_means_off():
    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200, aging=False)
    twin, _ = C.make_plane("cpu", 1 << 10, 256, 200, aging=False)
    dp.nf = _Spy(dp.nf)
    pk, im = S.traffic(sc, 300, seed=9)
    a, b = dp.run(pk, im.copy()), twin.run(pk, im.copy())
    assert np.array_equal(a.out, b.out) and np.array_equal(a.meta, b.meta)
    dp.flows.erase(sc.keys[0])
    twin.flows.erase(sc.keys[0])
    assert dp.commit() == twin.commit()
    dp.harvest()
    twin.harvest()
    assert np.array_equal(dp.flow_totals, twin.flow_totals)
    assert dp.nf.calls == []                                       # the CPU harvest is a plain copy
    assert not [k for k in dp._dev if k.startswith("age")] and dp.flows.age is None
    for call in (lambda: dp.set_flow_timeout(sc.keys[:1], 1.0), dp.age_flows, dp.flow_age_stats):
        with pytest.raises(RuntimeError):
            call()
    dp.enable_flow_aging()
    assert sorted(k for k in dp._dev if k.startswith("age")) == ["age_cnt", "age_list", "age_rows"]
    dp.harvest()
    assert dp.nf.calls == ["oracle_harvest_age"]


def test_needs_the_flow_counters():
    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200, aging=False)
    dp.count_flows = False
    with pytest.raises(ValueError):
        dp.enable_flow_aging()
    dp.count_flows = True
    dp.enable_flow_aging()
    dp.count_flows = False
    pk, im = S.traffic(sc, 8, seed=9)
    with pytest.raises(ValueError):
        dp.run(pk, im)
    with pytest.raises(ValueError):
        dp.age_flows()


def test_timeouts_round_up_and_are_bounded():
    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200)
    assert dp.set_flow_timeout(sc.keys[0], 0.01) == 1              # one key, rounded up to one tick
    assert dp.set_flow_timeout(sc.keys[1:4], [0.1, 0.11, 1.0]) == 3
    dp.commit()
    assert dp.flow_timeouts(sc.keys[:5]).tolist() == [1, 1, 2, 10, 0]
    rows = dp.age_rows()
    assert rows["tmo"][dp.flows.find(sc.keys[2])] == 2 | NEW
    for bad in (-1.0, (T.AGE_TMO_MASK + 10) * 0.1, float("nan")):
        with pytest.raises(ValueError):
            dp.set_flow_timeout(sc.keys[0], bad)
    assert dp.set_flow_timeout(sc.keys[0], (T.AGE_TMO_MASK - 10) * 0.1) == 1      # (float seconds: a few ticks of slack at 3.4 years)


def test_reset_counters_rearms():
    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200)
    dp.set_flow_timeout(sc.keys[:3], 0.5)
    assert len(dp.age_flows(C.BASE_NS)) == 0
    pk, im = S.traffic(sc, 32, seed=5, flows=np.arange(0, 3))
    dp.run(pk, im.copy())
    dp.reset_counters()
    rows = dp.age_rows()
    for i in range(3):
        assert _row(rows[dp.flows.find(sc.keys[i])]) == (0, 0, 5 | NEW)
    assert len(dp.age_flows(C.BASE_NS + 9 * C.TICK_NS)) == 0       # new again: dated, not expired
    assert len(dp.age_flows(C.BASE_NS + 14 * C.TICK_NS)) == 3


def test_multi_gpu_planes_refuse():
    from dpu_operator_amd.dataplane.multi import MultiDataPlane

    mdp = MultiDataPlane(["cpu", "cpu"], flow_buckets=1 << 10)
    with pytest.raises(NotImplementedError):
        mdp.enable_flow_aging()


def test_snapshot_round_trip(tmp_path):
    from dpu_operator_amd.dataplane import snapshot

    dp, sc = C.make_plane("cpu", 1 << 10, 256, 200)
    dp.set_flow_timeout(sc.keys[:10], 0.5)
    dp.set_flow_timeout(sc.keys[10:20], 2.0)
    dp.age_flows(C.BASE_NS)
    dp.set_flow_timeout(sc.keys[20:22], 1.0)                       # still pending at the save
    path = str(tmp_path / "snap.npz")
    snapshot.save(dp, path)
    with np.load(path) as z:
        assert int(z["age_tick_ns"]) == C.TICK_NS and len(z["flow_idle_ticks"]) == len(z["flow_keys"]) == 200
        assert int(np.count_nonzero(z["flow_idle_ticks"])) == 22
    new = DataPlane(device="cpu", flow_buckets=1 << 10)
    snapshot.load(new, path)
    assert new.flow_age_stats()["armed"] == 22 and new.flows.age.tick_ns == C.TICK_NS
    assert np.array_equal(new.flow_timeouts(sc.keys[:24]), [5] * 10 + [20] * 10 + [10, 10, 0, 0])
    # a fresh idle clock: dated by the first sweep, whatever its time
    assert len(new.age_flows(C.BASE_NS + 100 * C.TICK_NS)) == 0
    got = new.age_flows(C.BASE_NS + 105 * C.TICK_NS)
    assert {tuple(int(x) for x in k) for k in got} == {C.key_of(sc, i) for i in range(10)}
    # a snapshot without the arrays loads as before
    plain, _ = C.make_plane("cpu", 1 << 10, 256, 200, aging=False)
    snapshot.save(plain, path)
    with np.load(path) as z:
        assert "flow_idle_ticks" not in z.files
    old = DataPlane(device="cpu", flow_buckets=1 << 10)
    snapshot.load(old, path)
    assert old._age_stats is None and len(old.flows) == 200


def test_oracles_under_address_and_ub_sanitizers(tmp_path):
    """The oracles in a stand-alone program (csrc/nfdp/age_stress.cpp: exactly sized heap buffers,
    wrap-around ticks, cap of 0, 1 and n, the contract restated slot by slot), built host-only with
    -fsanitize=address,undefined and run as a process of its own."""
    import os
    import shutil
    import subprocess

    from dpu_operator_amd.native.build import SANITIZERS, build_sanitized

    # skipped only where the toolchain cannot link and run a sanitized program at all (a trivial
    # main decides that); a failure to build the real target is a failure of this test
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    cxx = shutil.which("g++") or "g++"
    try:
        ok = subprocess.run([cxx, *SANITIZERS["asan"], str(probe), "-o", str(tmp_path / "probe")],
                            capture_output=True, timeout=120).returncode == 0
        ok = ok and subprocess.run([str(tmp_path / "probe")], capture_output=True, timeout=60).returncode == 0
    except OSError:
        ok = False
    if not ok:
        pytest.skip("no C++ toolchain with the address / undefined-behaviour sanitizer runtimes")
    exe = build_sanitized("asan", target="age")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "200"], capture_output=True, text=True, timeout=180, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip().endswith("ok")
