"""The token-bucket policer's CPU oracle (csrc/nfdp/host.cpp oracle_police / oracle_police_fix,
contract in csrc/nfdp/police.h) against an independent model: a plain Python loop over Python ints
that shares no code with police.h.  Verdicts, meter state (exactly), meter / port / drop counters
and the restored in-meta are compared; an unmetered twin plane fed only the model's green frames
is the reference for everything the pipeline does with them."""
import numpy as np
import pytest

from dpu_operator_amd.dataplane import scenario as S
from dpu_operator_amd.dataplane import tables as T
from dpu_operator_amd.dataplane.engine import DataPlane

OVERFLOW = 11
NANO = 10 ** 9


class Model:
    """Sequential policer over Python ints."""

    def __init__(self):
        self.cfg = {}      # meter -> (rate_Bps, burst)
        self.state = {}    # meter -> [tokens, last_ns]
        self.ctr = {}      # meter -> [green_pkts, green_bytes, red_pkts, red_bytes]
        self.port_meter = {}

    def set(self, m, mbps, burst):
        self.cfg[m] = (mbps * 125000, burst)
        self.state[m] = [burst * NANO, 0]
        self.ctr.setdefault(m, [0, 0, 0, 0])

    def run(self, ports, lens, now):
        allow, used = {}, {}
        for m, (rate, burst) in self.cfg.items():
            tok, last = self.state[m]
            tok = min(burst * NANO, tok + max(0, now - last) * rate)
            self.state[m] = [tok, max(last, now)]
            allow[m], used[m] = tok // NANO, 0
        red = np.zeros(len(ports), bool)
        for i, (p, ln) in enumerate(zip(ports.tolist(), lens.tolist())):
            m = self.port_meter.get(p) if p < 4094 else None
            if m is None:
                continue
            used[m] += ln
            ok = used[m] <= allow[m]
            red[i] = not ok
            c = self.ctr[m]
            c[0 if ok else 2] += 1
            c[1 if ok else 3] += ln
            if ok:
                self.state[m][0] -= ln * NANO
        return red

    def state_array(self):
        a = np.zeros((T.MAX_METERS, 2), np.uint64)
        for m, (tok, last) in self.state.items():
            a[m] = (tok, last)
        return a

    def ctr_array(self):
        a = np.zeros((T.MAX_METERS, 4), np.uint64)
        for m, c in self.ctr.items():
            a[m] = c
        return a


def _plane():
    dp = DataPlane(device="cpu", flow_buckets=1 << 10)
    sc = S.build_sfc(dp, n_pods=4, n_flows=512, n_acl=8, seed=2)
    dp.commit(full=True)
    return dp, sc


@pytest.fixture()
def planes():
    dp, sc = _plane()
    ref, _ = _plane()     # never sees a meter: the pipeline's reference for the green frames
    return dp, ref, sc, Model()


def _set(dp, model, m, mbps, burst, ports=()):
    dp.meters.set(m, mbps, burst)
    model.set(m, mbps, burst)
    for p in ports:
        dp.meters.bind(p, m)
        model.port_meter[p] = m
    dp.commit()


def _check(dp, ref, model, pk, im, now):
    """One batch through the metered plane, the model and (green frames only) the twin."""
    im0 = im.copy()
    ports, lens = (im0 & 0xFFFF).astype(np.int64), (im0 >> 16).astype(np.int64)
    red = model.run(ports, lens, now)
    r = dp.run(pk, im, now_ns=now)
    assert np.array_equal(im, im0)                       # restored byte for byte
    reason = (r.meta >> 26) & 0xF
    assert np.array_equal(reason == OVERFLOW, red)
    assert np.array_equal(r.meta[red], (0xFFF | ((lens[red] & 0x3FFF) << 12) | (OVERFLOW << 26)).astype(np.uint32))
    g = ~red
    rr = ref.run(np.ascontiguousarray(pk[g]), np.ascontiguousarray(im0[g]))
    assert np.array_equal(r.meta[g], rr.meta) and np.array_equal(r.out[g], rr.out)
    assert np.array_equal(dp.meter_state(), model.state_array())
    assert np.array_equal(dp.meter_counters(), model.ctr_array())
    assert np.array_equal(dp.port_counters(), ref.port_counters())   # red frames: no rx count
    d, dref = dp.drop_counters(), ref.drop_counters()
    assert d.pop("overflow", 0) == int(model.ctr_array()[:, 2].sum())
    assert d == dref
    return red


def _from_port(sc, pod, n, frame_len=56, seed=1):   # tagged: 60 B in memory
    return S.traffic(sc, n, seed=seed, src_pods=np.array([pod]), frame_len=frame_len)


def test_basic_burst_and_refill(planes):
    dp, ref, sc, model = planes
    _set(dp, model, 0, 800, 6000, [int(sc.pod_port[1])])          # 1e8 B/s, 6000 B
    pk, im = _from_port(sc, 1, 1000)
    red = _check(dp, ref, model, pk, im, 1_000_000)
    assert not red[:100].any() and red[100:].all()                # frame 100's prefix == 6000: green
    red = _check(dp, ref, model, pk, im, 1_000_000 + 30_000)      # +30 us: 3000 B
    assert not red[:50].any() and red[50:].all()
    assert dp.drop_counters()["overflow"] == 900 + 950


def test_sub_byte_carry(planes):
    dp, ref, sc, model = planes
    _set(dp, model, 3, 800, 6000, [int(sc.pod_port[0])])
    pk, im = _from_port(sc, 0, 200)
    now = 5_000
    _check(dp, ref, model, pk, im, now)                           # drains the bucket
    greens = []
    for _ in range(8):                                            # +305 ns: 30.5 B per batch
        now += 305
        greens.append(int((~_check(dp, ref, model, pk[:3], im[:3], now)).sum()))
    # 30.5 B a batch and 60-B frames: a frame fits every other batch only because halves carry over
    assert sum(greens) == 4 and dp.meter_state()[3, 0] % NANO in (0, NANO // 2)


def test_time_going_backwards(planes):
    dp, ref, sc, model = planes
    _set(dp, model, 1, 800, 6000, [int(sc.pod_port[2])])
    pk, im = _from_port(sc, 2, 150)
    _check(dp, ref, model, pk, im, 10_000_000)
    red = _check(dp, ref, model, pk, im, 9_000_000)               # elapsed 0: nothing refilled
    assert red.all() and dp.meter_state()[1, 1] == 10_000_000


def test_large_elapsed_clamps_to_full(planes):
    dp, ref, sc, model = planes
    _set(dp, model, 255, 400000, (1 << 31) - 1, [int(sc.pod_port[2])])   # the largest rate and burst
    _set(dp, model, 7, 1, 1, [int(sc.pod_port[3])])                       # the smallest
    pk, im = S.traffic(sc, 400, seed=5)
    _check(dp, ref, model, pk, im, 1)
    _check(dp, ref, model, pk, im, 1 << 63)
    _check(dp, ref, model, pk, im, (1 << 64) - 1)
    st = dp.meter_state()
    assert st[255, 0] <= ((1 << 31) - 1) * NANO and st[7, 0] == 1 * NANO


def test_shared_meter(planes):
    dp, ref, sc, model = planes
    _set(dp, model, 9, 800, 3000, [int(sc.pod_port[0]), int(sc.pod_port[3])])
    pk, im = S.traffic(sc, 300, seed=6, src_pods=np.array([0, 3]), frame_len=56)
    assert len(set((im & 0xFFFF).tolist())) == 2
    red = _check(dp, ref, model, pk, im, 77)
    assert not red[:50].any() and red[50:].all()                  # one prefix over both ports, slot order


def test_unmetered_invalid_and_continuation_slots(planes):
    dp, ref, sc, model = planes
    _set(dp, model, 4, 800, 1200, [int(sc.pod_port[1])])
    pk, im = S.traffic(sc, 400, seed=8)
    im[3::7] = (im[3::7] & 0xFFFF0000) | 0xFFFD                   # continuation slots
    im[5::11] = (im[5::11] & 0xFFFF0000) | 4094                   # >= kMaxPorts
    im[6::13] = (im[6::13] & 0xFFFF0000) | 0xFFFF
    red = _check(dp, ref, model, pk, im, 123)
    ports = im & 0xFFFF
    assert not red[ports != int(sc.pod_port[1])].any() and red.any()
    assert int(dp.meter_counters()[4, [0, 2]].sum()) == int((ports == int(sc.pod_port[1])).sum())


def test_config_change_resets_only_that_meter(planes):
    dp, ref, sc, model = planes
    _set(dp, model, 0, 800, 6000, [int(sc.pod_port[0])])
    _set(dp, model, 1, 800, 6000, [int(sc.pod_port[1])])
    pk, im = S.traffic(sc, 600, seed=9, src_pods=np.array([0, 1]))
    _check(dp, ref, model, pk, im, 1000)                          # both drained
    before = dp.meter_state()
    dp.meters.set(1, 800, 6000)                                   # unchanged config: nothing resets
    dp.commit()
    assert np.array_equal(dp.meter_state(), before)
    _set(dp, model, 1, 800, 9000)                                 # changed: meter 1 starts full
    st = dp.meter_state()
    assert st[1, 0] == 9000 * NANO and st[1, 1] == 0 and np.array_equal(st[0], before[0])
    _check(dp, ref, model, pk, im, 1000)
    dp.reset_counters()                                           # counters, not state
    assert not dp.meter_counters().any() and np.array_equal(dp.meter_state(), model.state_array())


def test_default_burst_and_ranges():
    mt = T.MeterTable()
    mt.set(0, 100)                                                # 10 ms at 12.5 MB/s
    assert tuple(int(x) for x in mt.a[0])[:3] == (12_500_000, 125_000, 10_000_000)
    mt.set(1, 1)                                                  # 1250 B in 10 ms: two maximum frames instead
    assert int(mt.a[1]["burst_bytes"]) == 2 * 9600
    mt.set(2, 400000)
    assert int(mt.a[2]["burst_bytes"]) == 500_000_000
    mt.set(3, 7, 1000)
    assert int(mt.a[3]["full_ns"]) == -(-1000 * NANO // 875000)
    for bad in ((0, 0), (0, 400001), (256, 10), (-1, 10)):
        with pytest.raises(ValueError):
            mt.set(*bad)
    with pytest.raises(ValueError):
        mt.set(0, 10, 1 << 31)
    with pytest.raises(ValueError):
        mt.bind(5, 200)                                           # not configured
    mt.bind(5, 3)
    mt.bind(6, 3)
    assert mt.active() and mt.meter_of(5) == 3
    mt.clear(3)
    assert not mt.active() and mt.meter_of(6) is None


class _Spy:
    def __init__(self, nf):
        self._nf, self.calls = nf, []

    def __getattr__(self, name):
        if name.startswith(("oracle_police", "launch_police")):
            self.calls.append(name)
        return getattr(self._nf, name)


def test_no_meter_bound_is_the_plain_path(planes):
    dp, ref, sc, _ = planes
    dp.meters.set(0, 100)                                         # configured, no port bound
    dp.commit()
    dp.nf = _Spy(dp.nf)
    pk, im = S.traffic(sc, 500, seed=10)
    im[7] = (im[7] & 0xFFFF0000) | 0xE001                         # an in-meta port in the mark's range
    im0 = im.copy()
    r, rr = dp.run(pk, im), ref.run(pk, im0.copy())
    assert dp.nf.calls == []
    assert np.array_equal(r.meta, rr.meta) and np.array_equal(r.out, rr.out) and np.array_equal(im, im0)
    assert np.array_equal(dp.port_counters(), ref.port_counters()) and dp.drop_counters() == ref.drop_counters()
    assert not dp.meter_counters().any()
    dp.meters.bind(int(sc.pod_port[0]), 0)
    dp.commit()
    dp.run(pk, im, now_ns=1)
    assert dp.nf.calls == ["oracle_police", "oracle_police_fix"]


def test_oracle_under_address_and_ub_sanitizers(tmp_path):
    """The oracle in a stand-alone program (csrc/nfdp/police_stress.cpp: exactly sized heap buffers,
    extreme rates / bursts / arrival times, the contract restated slot by slot), built host-only
    with -fsanitize=address,undefined and run as a process of its own."""
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
    exe = build_sanitized("asan", target="police")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "120"], capture_output=True, text=True, timeout=180, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout.strip().endswith("ok")


def test_multi_gpu_planes_refuse_meters():
    """Not enforced there yet: refused rather than silently ignored."""
    from dpu_operator_amd.dataplane.multi import MultiDataPlane

    mdp = MultiDataPlane(["cpu", "cpu"], flow_buckets=1 << 10)
    sc = S.build_sfc(mdp, n_pods=4, n_flows=64, n_acl=4, seed=2)
    mdp.commit(full=True)
    mdp.meters.set(0, 100)
    mdp.commit()                                                  # configured, not bound: fine
    mdp.meters.bind(int(sc.pod_port[0]), 0)
    with pytest.raises(NotImplementedError):
        mdp.commit()
    pk, im = S.traffic(sc, 16, seed=1)
    with pytest.raises(NotImplementedError):
        mdp.run(pk, im)


def test_uncounted_batch_charges_state_not_counters(planes):
    """run(flags=1): the meters are charged and the frames judged as ever, the meter counters stay."""
    dp, ref, sc, model = planes
    _set(dp, model, 0, 800, 6000, [int(sc.pod_port[1])])
    pk, im = _from_port(sc, 1, 150)
    im0 = im.copy()
    red = model.run((im & 0xFFFF).astype(np.int64), (im >> 16).astype(np.int64), 1000)
    r = dp.run(pk, im, now_ns=1000, flags=1)
    assert np.array_equal(((r.meta >> 26) & 0xF) == OVERFLOW, red) and np.array_equal(im, im0)
    assert np.array_equal(dp.meter_state(), model.state_array())
    assert not dp.meter_counters().any()
    assert dp.drop_counters() == {"overflow": 50}        # (the oracle pipeline always counts its drops)
