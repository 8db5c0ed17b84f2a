"""GPU tests of the token-bucket policer passes (csrc/nfdp/police.hip) against the C++ oracle
(host.cpp oracle_police / oracle_police_fix): three consecutive batches with rising arrival times,
so the meters' state carries from one to the next; meta, out, the restored in-meta, meter state,
meter / port / drop counters must be identical.  Shapes are the smallest at which the passes can
go wrong: around one wave, several workgroup ranges of one 256-slot trip each with a ragged tail
(from the range size the launcher exports), and - the smallest batch that has them - 1024 ranges
of two trips each, where the scan also walks more than one row per thread."""
import numpy as np
import pytest

from dpu_operator_amd.dataplane import scenario as S
from dpu_operator_amd.dataplane import tables as T
from dpu_operator_amd.dataplane.engine import DataPlane
from dpu_operator_amd.native import nfdp

pytestmark = pytest.mark.gpu

OVERFLOW, CONT = 11, 15
EXTRA = 200              # 64 more valid ports: more distinct meters in a wave than the 16 pods give
ONLY_LAST = 300          # a port whose frames lie only in the last range


def _torch():
    import torch

    return torch


def _build(device):
    dp = DataPlane(device=device, flow_buckets=1 << 12)
    sc = S.build_sfc(dp, n_pods=16, n_flows=1 << 12, n_acl=40, seed=0)
    for p in list(range(EXTRA, EXTRA + 64)) + [ONLY_LAST]:
        dp.ports.set(p, flags=T.PORT_VALID, bridge_id=sc.bridge, mac=S.pod_mac(p))
    vx = S.install_vxlan(dp, sc)
    dp.commit(full=True)
    return dp, sc, vx


@pytest.fixture(scope="module")
def planes():
    g, sc, vx = _build("cuda")
    c, _, _ = _build("cpu")
    return g, c, sc, vx


RANGE = None


def _range():
    global RANGE
    if RANGE is None:
        RANGE = int(nfdp().police_ranges(1)[1])
    return RANGE


def _n_ranges():
    """Three full workgroup ranges and a ragged tail that is no multiple of 64."""
    n = 3 * _range() + 37
    assert tuple(nfdp().police_ranges(n)) == (4, _range())
    return n


def _batch(sc, n, seed):
    sizes = np.random.default_rng(seed).integers(60, 1515, n)       # frames of 60..1514 B in memory
    pk, im, _, lens = S.traffic_frames(sc, n, sizes, seed=seed)
    assert lens.min() >= 60 and lens.max() <= 1514
    return pk, im


def _prefix(im, k):
    return int((im[:k + 1] >> 16).sum())


def _layout(name, sc, pk, im):
    """-> (in-meta, {meter: (mbps, burst)}, {port: meter}) of a meter layout over the batch."""
    n, pods = len(im), [int(p) for p in sc.pod_port]
    im = im.copy()
    if name == "one_meter_out_mid_wave":
        # every lane on the same key; allow == the prefix at slot 30 (equality: green), red from 31
        k = min(30, max(n - 2, 0))
        return im, {5: (800, _prefix(im, k))}, {p: 5 for p in pods}
    if name == "distinct64":
        # 64 distinct meters inside every wave; small buckets: most run out in the batch
        im = (im & 0xFFFF0000) | (EXTRA + np.arange(n) % 64).astype(np.uint32)
        return im, {10 + k: (100 + k, 1 + 150 * k) for k in range(64)}, {EXTRA + k: 10 + k for k in range(64)}
    if name == "interleaved":
        # metered pods (own meter, or one shared by two) between unmetered ones
        cfg = {k: (400, 4000 + 1000 * k) for k in range(0, 16, 2)}
        bind = {pods[k]: k for k in range(0, 16, 2)}
        bind[pods[3]] = 2
        return im, cfg, bind
    if name == "out_on_range_boundary":
        # allow == the prefix at the last slot of range 0
        return im, {255: (800, _prefix(im, _range() - 1))}, {p: 255 for p in pods}
    if name == "only_last_range":
        lo = 3 * _range()
        im[lo::2] = (im[lo::2] & 0xFFFF0000) | ONLY_LAST
        return im, {0: (800, 3000), 1: (800, 100_000)}, {ONLY_LAST: 0, pods[0]: 1}
    raise KeyError(name)


def _configure(dp, cfg, bind):
    for m in range(T.MAX_METERS):          # every case starts from full buckets
        if dp.meters.configured(m):
            dp.meters.clear(m)
    for m, (mbps, burst) in cfg.items():
        dp.meters.set(m, mbps, burst)
    for p, m in bind.items():
        dp.meters.bind(p, m)
    dp.commit()
    dp.reset_counters()


REASONS = []   # the last _compare's meta reasons, one array per batch


def _compare(g, c, pk, im, times, heads=None):
    torch = _torch()
    reds = []
    REASONS.clear()
    for now in times:
        tpk = torch.from_numpy(pk).to(g.tdev)     # (fresh: the pair pass rewrites terminated heads in place)
        tim = torch.from_numpy(im.view(np.int32).copy()).to(g.tdev)
        cim = im.copy()
        r = g.run(tpk, tim, now_ns=now)
        rc = c.run(pk, cim, now_ns=now)
        torch.cuda.synchronize()
        meta = r.meta.cpu().numpy().view(np.uint32)
        assert np.array_equal(meta, rc.meta)
        assert np.array_equal(r.out.cpu().numpy(), rc.out)
        back = tim.cpu().numpy().view(np.uint32)
        red = ((meta >> 26) & 0xF) == OVERFLOW
        # (wide pairs: the pair pass rewrites terminated heads and continuations in place on the
        # GPU, policer or not; what the policer marked must be back)
        sel = slice(None) if heads is None else heads[red[heads]]
        assert np.array_equal(back[sel], im[sel]) and np.array_equal(cim, im)
        assert np.array_equal(g.meter_state(), c.meter_state())
        assert np.array_equal(g.meter_counters(), c.meter_counters())
        assert np.array_equal(g.port_counters(), c.port_counters())
        assert g.drop_counters() == c.drop_counters()
        REASONS.append((meta >> 26) & 0xF)
        reds.append(REASONS[-1] == OVERFLOW)
    return reds


TIMES = (1_000_000, 1_020_000, 1_055_000)   # +20 us, +35 us: partial refills (2000 B, 3500 B at 800 Mbit/s)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("layout", ["one_meter_out_mid_wave", "distinct64", "interleaved"])
def test_small_batches_match_oracle(planes, layout, n):
    g, c, sc, _ = planes
    pk, im = _batch(sc, n, seed=100 + n)
    im, cfg, bind = _layout(layout, sc, pk, im)
    for dp in (g, c):
        _configure(dp, cfg, bind)
    reds = _compare(g, c, pk, im, TIMES)
    if layout == "one_meter_out_mid_wave" and n > 32:
        assert not reds[0][:31].any() and reds[0][31:].all()


@pytest.mark.parametrize("layout", ["one_meter_out_mid_wave", "distinct64", "interleaved", "out_on_range_boundary",
                                    "only_last_range"])
def test_several_ranges_match_oracle(planes, layout):
    g, c, sc, _ = planes
    n = _n_ranges()
    pk, im = _batch(sc, n, seed=7)
    im, cfg, bind = _layout(layout, sc, pk, im)
    for dp in (g, c):
        _configure(dp, cfg, bind)
    reds = _compare(g, c, pk, im, TIMES)
    if layout == "out_on_range_boundary":
        assert not reds[0][:_range()].any() and reds[0][_range():].all()
    if layout == "only_last_range":
        on = (im & 0xFFFF) == ONLY_LAST
        assert not on[:3 * _range()].any() and reds[0][on].any() and not reds[0][on].all()
    assert all(r.any() for r in reds[:2])


def test_vxlan_pairs_with_a_metered_vtep(planes):
    """Wide header pairs on a metered VTEP port: the police pass runs before the pair pass, so a
    policed head is not terminated and its continuation stays kCont."""
    g, c, sc, vx = planes
    pk, im, _ = S.traffic_vxlan(sc, vx, 200, seed=4)
    heads = np.arange(0, len(im), 2)
    assert ((im[heads] & 0xFFFF) == vx["vtep"]).all() and ((im[heads + 1] & 0xFFFF) == 0xFFFD).all()
    burst = int((im[heads][:90] >> 16).sum())
    for dp in (g, c):
        _configure(dp, {8: (800, burst)}, {vx["vtep"]: 8})
    reds = _compare(g, c, pk, im, TIMES, heads=heads)
    assert not reds[0][heads][:90].any() and reds[0][heads][90:].all()
    for red, reason in zip(reds, REASONS):
        assert red[heads].any() and (reason[heads + 1] == CONT).all()


def test_graph_capture_refuses_meters(planes):
    g, c, sc, _ = planes
    for dp in (g, c):
        _configure(dp, {0: (100, None)}, {int(sc.pod_port[0]): 0})
    with pytest.raises(NotImplementedError):
        g.capture(64)
    for dp in (g, c):
        _configure(dp, {}, {})
    assert not g._police_on


# ---- more than one trip per workgroup, more than one row per scan thread ----
# 1024 ranges of 512 slots (two trips of 256 each, the last range ragged): the carry of the
# per-meter prefix from trip to trip, the per-wave rows' clearing, the next trip's prefetch, and
# the scan's 16 rows per thread chained through LDS - what runs at the headline shape.
DEEP_N = 1024 * 512 - 219


@pytest.fixture(scope="module")
def deep_batch(planes):
    _, _, sc, _ = planes
    assert tuple(nfdp().police_ranges(DEEP_N)) == (1024, 512)
    pk, im = S.traffic(sc, DEEP_N, seed=31)
    sizes = np.random.default_rng(32).integers(60, 1515, DEEP_N)    # frames of 60..1514 B in memory
    return S.with_sizes(pk, im, sizes)


def _deep_layout(name, sc, im):
    pods = [int(p) for p in sc.pod_port]
    if name == "out_in_second_trip":       # allow == the prefix at slot 100 of range 700's second trip
        return {7: (800, _prefix(im, 700 * 512 + 256 + 100))}, {p: 7 for p in pods}
    if name == "out_on_trip_boundary":     # ... at the last slot of range 333's first trip
        return {7: (800, _prefix(im, 333 * 512 + 255))}, {p: 7 for p in pods}
    if name == "many_meters":
        # a meter per pod (two pods share one), each running out at another depth of the batch;
        # odd pods 5.. unmetered in between
        lens, ports = (im >> 16).astype(np.int64), im & 0xFFFF
        cfg, bind = {}, {}
        for k in (0, 1, 2, 3, 4, 6, 8, 10, 12, 14):
            total = int(lens[ports == pods[k]].sum())
            cfg[20 + k] = (800, max(1, total * (k + 1) // 17))
            bind[pods[k]] = 20 + k
        bind[pods[15]] = 20 + 14
        return cfg, bind
    raise KeyError(name)


@pytest.mark.parametrize("layout", ["out_in_second_trip", "out_on_trip_boundary", "many_meters"])
def test_two_trips_per_range_match_oracle(planes, deep_batch, layout):
    g, c, sc, _ = planes
    pk, im = deep_batch
    cfg, bind = _deep_layout(layout, sc, im)
    for dp in (g, c):
        _configure(dp, cfg, bind)
    reds = _compare(g, c, pk, im, TIMES)
    if layout == "out_in_second_trip":
        k = 700 * 512 + 256 + 100
        assert not reds[0][:k + 1].any() and reds[0][k + 1:].all()
    if layout == "out_on_trip_boundary":
        k = 333 * 512 + 255
        assert not reds[0][:k + 1].any() and reds[0][k + 1:].all()
    if layout == "many_meters":
        first_red = [int(np.argmax(reds[0] & ((im & 0xFFFF) == int(sc.pod_port[k])))) for k in (0, 4, 8, 12)]
        assert first_red == sorted(first_red) and first_red[0] > 512
        assert len({f // 512 for f in first_red}) == 4          # in four different ranges
    assert all(r.any() for r in reds)


def test_uncounted_batches_still_charge_the_meters(planes):
    """Launch flag 1 (no counters): verdicts and meter state as ever, the meter counters untouched,
    on the GPU as in the oracle path.  (The oracle pipeline itself takes no flags and counts its
    port / drop counters regardless, so those are not compared here.)"""
    torch = _torch()
    g, c, sc, _ = planes
    pk, im = _batch(sc, 257, seed=9)
    im, cfg, bind = _layout("interleaved", sc, pk, im)
    for dp in (g, c):
        _configure(dp, cfg, bind)
    for now in TIMES[:2]:
        tim = torch.from_numpy(im.view(np.int32).copy()).to(g.tdev)
        r = g.run(torch.from_numpy(pk).to(g.tdev), tim, now_ns=now, flags=1)
        rc = c.run(pk, im.copy(), now_ns=now, flags=1)
        torch.cuda.synchronize()
        meta = r.meta.cpu().numpy().view(np.uint32)
        assert np.array_equal(meta, rc.meta) and (((meta >> 26) & 0xF) == OVERFLOW).any()
        assert np.array_equal(tim.cpu().numpy().view(np.uint32), im)
        assert np.array_equal(g.meter_state(), c.meter_state())
        assert not g.meter_counters().any() and not c.meter_counters().any()
        assert g.drop_counters() == {}
