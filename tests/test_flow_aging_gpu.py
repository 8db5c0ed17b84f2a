"""Flow aging on the GPU (csrc/nfdp/age.hip): age_sweep_kernel and harvest_age_kernel against their
sequential oracles, bit for bit, from one slot up to the first size at which a thread of the capped
grid takes a second slot; then DataPlane("cuda") against DataPlane("cpu") and the independent model
through the schedules of tests/flow_aging_common.py."""
import numpy as np
import pytest

import flow_aging_common as C
from dpu_operator_amd.dataplane import tables as T

pytestmark = pytest.mark.gpu

NOW = 3          # the ticks wrapped a moment ago: every `last` below lies before the wrap
NEW, TOUCHED = T.AGE_NEW, T.AGE_TOUCHED


def _sizes(nf):
    _, per_pass = nf.age_grid(1 << 31)        # the capped grid's slots per pass
    return [1, 63, 64, 65, 255, 256, 257, per_pass + 37]


def _table(n, seed=0):
    """Rows / counters of n slots: every category in every wave (unarmed, new, touched, counter
    moved, idle one tick short, idle for exactly the timeout, idle for long), but wave 1 all
    expired and wave 2 all unarmed (where there are that many slots)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    cat = (i * 5 + i // 64) % 7
    wave = i // 64
    cat = np.where(wave == 1, 5 + (i % 2), cat)
    cat = np.where(wave == 2, 0, cat)
    tmo = rng.integers(1, 50, n).astype(np.uint32)
    tmo[i % 97 == 0] = T.AGE_TMO_MASK
    idle = np.where(cat == 4, tmo - 1, np.where(cat == 5, tmo, np.minimum(tmo.astype(np.int64) + 1000, T.AGE_TMO_MASK)))
    rows = np.zeros(n, T.AGE_ROW_DTYPE)
    ctr = (rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(40)) | rng.integers(0, 1 << 30, n).astype(np.uint64)
    rows["seen"] = np.where(cat == 3, ctr ^ np.uint64(1 << 40), ctr)
    rows["last"] = ((NOW - idle.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)
    rows["tmo"] = np.where(cat == 0, 0, tmo | np.where(cat == 1, NEW, 0).astype(np.uint32)
                           | np.where(cat == 2, TOUCHED, 0).astype(np.uint32)).astype(np.uint32)
    rows["seen"][cat == 0] = 0
    rows["last"][cat == 0] = 0
    return rows, ctr


def _oracle_sweep(nf, rows, ctr, cap):
    rows, ctr = rows.copy(), ctr.copy()
    out = np.zeros(max(cap, 1), np.uint32)
    cnt = np.zeros(1, np.uint32)
    nf.oracle_age_sweep(ctr.ctypes.data, rows.ctypes.data, len(rows), NOW, out.ctypes.data, cap, cnt.ctypes.data)
    return rows, int(cnt[0]), out[: min(int(cnt[0]), cap)]


def _gpu_sweep(nf, rows, ctr, cap):
    import torch

    dev = torch.device("cuda")
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
    d_ctr = torch.from_numpy(ctr.view(np.int64).copy()).to(dev)
    d_out = torch.full((max(cap, 1),), -1, dtype=torch.int32, device=dev)
    d_cnt = torch.full((1,), 12345, dtype=torch.int32, device=dev)      # the launcher zeroes it
    s = torch.cuda.current_stream()
    nf.launch_age_sweep(d_ctr.data_ptr(), d_rows.data_ptr(), len(rows), NOW, d_out.data_ptr(), cap, d_cnt.data_ptr(),
                        s.cuda_stream)
    s.synchronize()
    cnt = int(d_cnt.cpu().numpy().view(np.uint32)[0])
    assert np.array_equal(d_ctr.cpu().numpy().view(np.uint64), ctr)     # the sweep only reads the counters
    return d_rows.cpu().numpy().view(T.AGE_ROW_DTYPE), cnt, d_out.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def cases(nf):
    """Per size: the table and the oracle's verdict with room for every expired slot (computed once)."""
    out = {}
    for n in _sizes(nf):
        rows, ctr = _table(n, seed=n)
        out[n] = (rows, ctr, _oracle_sweep(nf, rows, ctr, n))
    return out


@pytest.mark.parametrize("k", range(8))
def test_sweep_kernel_matches_the_oracle(nf, cases, k):
    n = _sizes(nf)[k]
    rows, ctr, (o_rows, o_cnt, o_list) = cases[n]
    if n >= 65:
        assert o_cnt > 0 and o_cnt < n
    g_rows, g_cnt, g_out = _gpu_sweep(nf, rows, ctr, n)
    assert g_cnt == o_cnt
    assert g_rows.tobytes() == o_rows.tobytes()
    assert np.array_equal(np.sort(g_out[:g_cnt]), o_list)          # (the oracle lists in slot order)
    if g_cnt < n:
        assert np.all(g_out[g_cnt:] == 0xFFFFFFFF)                  # nothing written past the count


@pytest.mark.parametrize("k", range(3, 8))
def test_sweep_list_smaller_than_the_expired_set(nf, cases, k):
    n = _sizes(nf)[k]
    rows, ctr, (o_rows, o_cnt, o_list) = cases[n]
    cap = o_cnt // 2
    assert 1 <= cap < o_cnt
    g_rows, g_cnt, g_out = _gpu_sweep(nf, rows, ctr, cap)
    assert g_cnt == o_cnt                                           # exact, beyond the list's end too
    assert len(g_out) == cap and len(np.unique(g_out)) == cap and np.isin(g_out, o_list).all()
    assert g_rows.tobytes() == o_rows.tobytes()                     # expired rows stay as they are
    g_rows, g_cnt, _ = _gpu_sweep(nf, rows, ctr, 0)
    assert g_cnt == o_cnt and g_rows.tobytes() == o_rows.tobytes()


@pytest.mark.parametrize("k", range(8))
def test_harvest_kernel_matches_the_oracle(nf, cases, k):
    import torch

    n = _sizes(nf)[k]
    rows, ctr, _ = cases[n]
    o_rows, o_ctr, o_out = rows.copy(), ctr.copy(), np.zeros(n, np.uint64)
    nf.oracle_harvest_age(o_ctr.ctypes.data, o_rows.ctypes.data, o_out.ctypes.data, n)
    assert np.array_equal(o_out, ctr) and not o_ctr.any()
    if n >= 65:
        assert np.any(o_rows["tmo"] != rows["tmo"])                 # some rows became touched
    dev = torch.device("cuda")
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
    d_ctr = torch.from_numpy(ctr.view(np.int64).copy()).to(dev)
    d_out = torch.zeros(n, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream()
    nf.launch_harvest_age(d_ctr.data_ptr(), d_rows.data_ptr(), d_out.data_ptr(), n, s.cuda_stream)
    s.synchronize()
    assert not d_ctr.any().item()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), o_out)
    assert d_rows.cpu().numpy().tobytes() == o_rows.tobytes()


def test_planes_on_gpu_and_cpu_agree_with_the_model():
    runs = []
    for device in ("cuda", "cpu"):
        dp, sc = C.make_plane(device, 4096, 256, 200)
        r = C.Runner(dp, sc, 200)
        C.model_schedule(r, 200)              # every sweep's expired keys equal the model's
        runs.append(r)
    g, c = runs
    assert g.expired_sets == c.expired_sets and sum(len(s) for s in g.expired_sets) == 113
    assert len(g.batches) == len(c.batches)
    for (go, gm), (co, cm) in zip(g.batches, c.batches):
        assert np.array_equal(gm, cm) and np.array_equal(go, co)
    # (the rows' `last` ticks count from each plane's own epoch: compared through the model only)
    for key in g.sc.keys[:220]:
        assert g.dp.flows.find(key) == c.dp.flows.find(key)


def test_rows_follow_cuckoo_moves_on_the_gpu():
    dp, sc = C.make_plane("cuda", 16, 64, 0, seed=1)
    r = C.Runner(dp, sc, 0)
    assert C.moves_schedule(r) >= 55
    assert dp.flow_age_stats()["relocated"] > 0
    assert not dp.age_rows()["tmo"].any()
