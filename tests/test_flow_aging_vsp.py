"""Flow idle timeouts through the GPU VSP (vsp/gpu.py install_flows / remove_flows / expire_flows
over DataPlane.age_flows, csrc/nfdp/age.h): the control path, its persistence across restarts, the
metrics and the sweeper thread."""
import logging
import time

import numpy as np

from dpu_operator_amd.dataplane import tables as T
from dpu_operator_amd.vsp.gpu import GpuVsp, _enc

T0 = 50_000_000_000
S = 1_000_000_000


def _vsp(**kw):
    vsp = GpuVsp(device="cpu", flow_buckets=1 << 10, **kw)
    vsp.init(True, "dpu0")
    vsp.set_num_vfs(3)
    return vsp


def _flows(lo, n):
    i = np.arange(lo, lo + n)
    keys = T.flow_key(0x0A000002 + (i % 3), 0x0A800000 + i, 1000 + i, 53, 17, 1)
    return keys, T.flow_action(chain_id=0, out_port=1 + (i % 2), flow_id=i)


def _installed(vsp, keys):
    return [vsp.dp.flows.find(k) >= 0 for k in keys]


def test_install_with_timeout_expire_and_remove():
    vsp = _vsp()
    ka, aa = _flows(0, 10)
    kb, ab = _flows(10, 10)
    kc, ac = _flows(20, 5)
    assert vsp.expire_flows(T0) == 0                     # nothing aged yet: no sweep, no buffers
    assert not vsp._aging()
    vsp.install_flows(kc, ac)
    vsp.install_flows(ka, aa, idle_timeout_s=0.5)
    vsp.install_flows(kb, ab, idle_timeout_s=5)
    assert vsp.dp.flow_timeouts(np.concatenate([ka, kb, kc])).tolist() == [5] * 10 + [50] * 10 + [0] * 5
    assert vsp.expire_flows(T0) == 0
    assert vsp.expire_flows(T0 + S // 2) == 10
    assert _installed(vsp, np.concatenate([ka, kb, kc])) == [False] * 10 + [True] * 15
    assert vsp.remove_flows(np.concatenate([kb[:4], ka[:2]])) == 4
    assert _installed(vsp, kb) == [False] * 4 + [True] * 6
    assert vsp.dp.flow_age_stats()["armed"] == 6
    vsp.install_flows(kb[4:6], ab[4:6])                  # installed again without a timeout: not aged
    assert vsp.expire_flows(T0 + 6 * S) == 4
    assert _installed(vsp, kb) == [False] * 4 + [True] * 2 + [False] * 4 and all(_installed(vsp, kc))
    try:
        vsp.install_flows(ka, aa, idle_timeout_s=-1)
    except ValueError:
        pass
    else:
        raise AssertionError("negative timeout accepted")


def test_restart_keeps_survivors_and_their_timeouts(tmp_path):
    vsp = _vsp(state_dir=str(tmp_path))
    for name, fn, args in (("Init", vsp.init, (True, "dpu0")), ("SetNumVfs", vsp.set_num_vfs, (3,))):
        vsp._call(name, fn, *args)
    ka, aa = _flows(0, 10)
    kb, ab = _flows(10, 10)
    kc, ac = _flows(20, 5)
    vsp.install_flows(ka, aa, idle_timeout_s=0.5)
    vsp.install_flows(kb, ab, idle_timeout_s=5)
    vsp.install_flows(kc, ac)
    assert vsp.expire_flows(T0) == 0 and vsp.expire_flows(T0 + S) == 10
    vsp.remove_flows(kc[:1])
    everything = np.concatenate([ka, kb, kc])
    want = [False] * 10 + [True] * 10 + [False] + [True] * 4
    # crash: a new VSP on the same directory replays the journal (install, install, install, remove, remove)
    again = GpuVsp(device="cpu", flow_buckets=1 << 10, state_dir=str(tmp_path))
    assert _installed(again, everything) == want
    assert again.dp.flow_timeouts(everything).tolist() == [0] * 10 + [50] * 10 + [0] * 5
    # ... and from a snapshot: the timeouts travel in it, the idle clock starts anew
    again.checkpoint()
    third = GpuVsp(device="cpu", flow_buckets=1 << 10, state_dir=str(tmp_path))
    assert third.restored == 0 and _installed(third, everything) == want
    assert third.dp.flow_timeouts(everything).tolist() == [0] * 10 + [50] * 10 + [0] * 5
    assert third.expire_flows(T0 + 100 * S) == 0 and third.expire_flows(T0 + 105 * S) == 10
    fourth = GpuVsp(device="cpu", flow_buckets=1 << 10, state_dir=str(tmp_path))
    assert _installed(fourth, everything) == [False] * 21 + [True] * 4


def test_bulk_expiry_takes_a_checkpoint(tmp_path, monkeypatch):
    import dpu_operator_amd.vsp.gpu as G

    monkeypatch.setattr(G, "JOURNAL_FLOWS_MAX", 8)
    vsp = _vsp(state_dir=str(tmp_path))
    for name, fn, args in (("Init", vsp.init, (True, "dpu0")), ("SetNumVfs", vsp.set_num_vfs, (3,))):
        vsp._call(name, fn, *args)
    k, a = _flows(0, 20)
    vsp.install_flows(k, a, idle_timeout_s=1)            # > 8: a checkpoint, not a record
    assert vsp.expire_flows(T0) == 0 and vsp.expire_flows(T0 + S) == 20
    again = GpuVsp(device="cpu", flow_buckets=1 << 10, state_dir=str(tmp_path))
    assert again.restored == 0 and not any(_installed(again, k))


def test_old_install_record_replays(tmp_path):
    vsp = _vsp(state_dir=str(tmp_path))
    for name, fn, args in (("Init", vsp.init, (True, "dpu0")), ("SetNumVfs", vsp.set_num_vfs, (3,))):
        vsp._call(name, fn, *args)
    k, a = _flows(0, 6)
    vsp.journal.append({"rpc": "InstallFlows", "args": _enc([k.tobytes(), a.tobytes()])})   # as written before
    again = GpuVsp(device="cpu", flow_buckets=1 << 10, state_dir=str(tmp_path))
    assert all(_installed(again, k)) and not again._aging()


def test_metrics_families_appear():
    from prometheus_client import CollectorRegistry, generate_latest

    from dpu_operator_amd.utils.metrics import register_dataplane

    vsp = _vsp()
    reg = CollectorRegistry()
    register_dataplane(lambda: vsp.dp, "gpu0", reg)
    assert b"dpu_flows_aged" not in generate_latest(reg)
    k, a = _flows(0, 6)
    vsp.install_flows(k, a, idle_timeout_s=1)
    vsp.install_flows(*_flows(6, 2), idle_timeout_s=9)
    assert vsp.expire_flows(T0) == 0 and vsp.expire_flows(T0 + S) == 6
    text = generate_latest(reg).decode()
    assert 'dpu_flows_expired_total{dataplane="gpu0"} 6.0' in text
    assert 'dpu_flows_aged{dataplane="gpu0"} 2.0' in text
    assert 'dpu_flow_sweep_seconds{dataplane="gpu0"}' in text


def test_sweeper_thread_expires_and_stops_with_the_vsp(caplog):
    vsp = _vsp()
    k, a = _flows(0, 4)
    vsp.install_flows(k, a, idle_timeout_s=0.1)
    vsp.install_flows(*_flows(4, 2))
    vsp.start_flow_sweeper(0.05)
    thread = vsp._sweeper[0]
    deadline = time.monotonic() + 10.0
    while any(_installed(vsp, k)) and time.monotonic() < deadline:
        time.sleep(0.01)
    assert not any(_installed(vsp, k)) and len(vsp.dp.flows) == 2
    # a failing sweep is logged and the thread goes on
    boom = {"n": 0}

    def fail(now_ns=None):
        boom["n"] += 1
        raise RuntimeError("boom")

    vsp.dp.age_flows = fail
    with caplog.at_level(logging.ERROR, logger="dpu.vsp.gpu"):
        while boom["n"] < 2 and time.monotonic() < deadline:
            time.sleep(0.01)
    assert boom["n"] >= 2 and thread.is_alive()
    assert any("flow sweep failed" in r.message for r in caplog.records)
    vsp.stop()
    assert not thread.is_alive() and vsp._sweeper is None


def test_several_gpus_store_the_timeout_and_warn_once(caplog):
    vsp = GpuVsp(device="cpu", flow_buckets=1 << 10, gpus=2)
    vsp.init(True, "dpu0")
    k, a = _flows(0, 4)
    with caplog.at_level(logging.WARNING, logger="dpu.vsp.gpu"):
        vsp.install_flows(k[:2], a[:2], idle_timeout_s=2)
        vsp.install_flows(k[2:], a[2:], idle_timeout_s=3)
    assert sum("idle timeouts are stored but not enforced" in r.message for r in caplog.records) == 1
    assert vsp.flow_idle_s[k[0].tobytes()] == 2 and vsp.flow_idle_s[k[3].tobytes()] == 3
    assert vsp.expire_flows() == 0
    vsp.remove_flows(k[:1])
    assert k[0].tobytes() not in vsp.flow_idle_s


def test_command_line_flag():
    from dpu_operator_amd.cmd.vsp import parse_args

    assert parse_args([]).flow_sweep_interval == 0.0
    assert parse_args(["--flow-sweep-interval", "2.5"]).flow_sweep_interval == 2.5
