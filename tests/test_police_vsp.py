"""max_tx_rate on GPU vports (vsp/gpu.py set_vf_rate -> a token-bucket meter on the VF port,
csrc/nfdp/police.h): the control path, its persistence, the netlink pick-up, the engines that do
not enforce it yet, and one end-to-end case through the live path's batch engine."""
import collections
import logging
import os

from dpu_operator_amd.cni.netlink import FakeNetlink, Link
from dpu_operator_amd.dataplane import tables as T
from dpu_operator_amd.dataplane.engine import DataPlane
from dpu_operator_amd.ops import packets as P
from dpu_operator_amd.vsp.gpu import GpuVsp

OVERFLOW = 11
MACS = ["00:11:22:33:44:%02x" % (0x50 + i) for i in range(3)]


def _vsp(**kw):
    vsp = GpuVsp(device="cpu", flow_buckets=1 << 10, **kw)
    vsp.init(True, "dpu0")
    vsp.set_num_vfs(3)
    return vsp


def _bridge_ports(vsp):
    for i, mac in enumerate(MACS):
        vsp.create_bridge_port(f"host0-{i}", bytes.fromhex(mac.replace(":", "")), 1, [str(2 + i)])


def _burst(vsp, vf, n):
    """n 60-B frames from VF `vf` to the wire -> reasons."""
    frames, _ = P.craft(n, dmac="02:00:00:00:ff:01", smac=MACS[vf], src_ip=0x0A000002 + vf, dst_ip=0x08080808,
                        sport=1234, dport=53)
    _, meta = vsp.process(frames, [vf] * n)
    return P.meta_fields(meta)[2]


def test_set_vf_rate_polices_that_vf_only():
    vsp = _vsp()
    _bridge_ports(vsp)
    vsp.set_vf_rate(0, 100, burst_bytes=6000)          # 100 frames of 60 B
    assert vsp.dp.meters.meter_of(0) == 0 and tuple(int(x) for x in vsp.dp.meters.a[0])[:2] == (12_500_000, 6000)
    reasons = _burst(vsp, 0, 400)
    # (the bucket refills while the batch is prepared only in later batches: the first one starts full)
    assert (reasons[:100] == 0).all() and (reasons[100:] == OVERFLOW).all()
    assert vsp.dp.drop_counters().get("overflow") == 300
    assert (_burst(vsp, 1, 400) == 0).all() and (_burst(vsp, 2, 400) == 0).all()
    ctr = vsp.dp.meter_counters()
    assert tuple(int(x) for x in ctr[0]) == (100, 6000, 300, 300 * 60) and not ctr[1:].any()
    # rate 0 removes the meter, as `ip link set ... vf 0 max_tx_rate 0`
    vsp.set_vf_rate(0, 0)
    assert not vsp.dp.meters.active() and not vsp.dp.meters.configured(0)
    assert (_burst(vsp, 0, 400) == 0).all()
    # the default bucket: 10 ms at the rate
    vsp.set_vf_rate(2, 1000)
    assert int(vsp.dp.meters.a[2]["burst_bytes"]) == 1_250_000
    for bad in ((7, 10), (0, -1), (0, T.METER_MAX_MBPS + 1)):
        try:
            vsp.set_vf_rate(*bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_rate_survives_journal_restore_and_checkpoint(tmp_path):
    vsp = _vsp(state_dir=str(tmp_path))
    for name, fn, args in (("Init", vsp.init, (True, "dpu0")), ("SetNumVfs", vsp.set_num_vfs, (3,))):
        vsp._call(name, fn, *args)
    for i, mac in enumerate(MACS):
        vsp._call("CreateBridgePort", vsp.create_bridge_port, f"host0-{i}", bytes.fromhex(mac.replace(":", "")), 1,
                  [str(2 + i)])
    vsp.set_vf_rate(1, 100, burst_bytes=6000)
    salt = vsp._salt
    # crash: a new VSP on the same directory replays the journal
    again = GpuVsp(device="cpu", flow_buckets=1 << 10, state_dir=str(tmp_path))
    assert again._salt == salt and again.vports[1]["max_tx_rate"] == 100
    assert again.dp.meters.meter_of(1) == 1 and int(again.dp.meters.a[1]["burst_bytes"]) == 6000
    reasons = _burst(again, 1, 150)
    assert (reasons[:100] == 0).all() and (reasons[100:] == OVERFLOW).all()
    # ... and restores it from a snapshot
    again.checkpoint()
    third = GpuVsp(device="cpu", flow_buckets=1 << 10, state_dir=str(tmp_path))
    assert third.vports[1]["max_tx_rate"] == 100 and third.dp.meters.meter_of(1) == 1
    reasons = _burst(third, 1, 150)
    assert (reasons[:100] != OVERFLOW).all() and (reasons[100:] == OVERFLOW).all()


def test_bridge_port_picks_up_the_rate_from_netlink():
    """The colocated case: the CNI's link_set_vf went to the netlink manager the VSP holds."""
    nl = FakeNetlink()
    nl.add_link(Link(name="ens1f0", kind="device"))
    nl.link_set_vf("ens1f0", 1, mac=MACS[1], max_tx_rate=200, min_tx_rate=50)
    nl.link_set_vf("ens1f0", 2, mac=MACS[2])
    vsp = _vsp(nl=nl)
    _bridge_ports(vsp)
    assert vsp.vports[1]["max_tx_rate"] == 200 and vsp.dp.meters.meter_of(1) == 1
    assert int(vsp.dp.meters.a[1]["rate_Bps"]) == 25_000_000
    assert vsp.dp.meters.meter_of(0) is None and vsp.dp.meters.meter_of(2) is None   # no record / no rate
    vsp.create_bridge_port("host3-0", bytes.fromhex(MACS[0].replace(":", "")), 1, ["2"])   # a PF unknown there
    assert vsp.dp.meters.meter_of(0) is None


def test_a_pods_rate_leaves_with_the_pod(caplog):
    """The next pod on a VF does not inherit the previous tenant's limit: a rate taken from netlink
    goes with delete_bridge_port, and a netlink rate of 0 clears it; a rate an operator set with
    set_vf_rate stays.  The PF is found by the VF's MAC, whatever its position among the links."""
    nl = FakeNetlink()
    nl.add_link(Link(name="ens9f0", kind="device"))          # another PF, lower ifindex, same VF numbers
    nl.link_set_vf("ens9f0", 1, mac="00:aa:00:00:00:01", max_tx_rate=999)
    nl.add_link(Link(name="ens1f0", kind="device"))
    nl.link_set_vf("ens1f0", 1, mac=MACS[1], max_tx_rate=200)
    vsp = _vsp(nl=nl)
    mac1 = bytes.fromhex(MACS[1].replace(":", ""))
    vsp.create_bridge_port("host1-1", mac1, 1, ["3"])
    assert vsp.vports[1]["max_tx_rate"] == 200               # ens1f0's record (by MAC), not ens9f0's
    assert int(vsp.dp.meters.a[1]["rate_Bps"]) == 25_000_000
    vsp.delete_bridge_port("host1-1")
    assert vsp.vports[1]["max_tx_rate"] == 0 and not vsp.dp.meters.active() and not vsp.dp.meters.configured(1)
    # the CNI put the VF back to no limit; the next pod is unmetered
    nl.link_set_vf("ens1f0", 1, max_tx_rate=0)
    vsp.create_bridge_port("host1-1", mac1, 1, ["3"])
    assert vsp.dp.meters.meter_of(1) is None
    # a pod's rate, then the same pod re-added with rate 0 in netlink
    nl.link_set_vf("ens1f0", 1, max_tx_rate=300)
    vsp.create_bridge_port("host1-1", mac1, 1, ["3"])
    assert vsp.vports[1]["max_tx_rate"] == 300
    nl.link_set_vf("ens1f0", 1, max_tx_rate=0)
    vsp.create_bridge_port("host1-1", mac1, 1, ["3"])
    assert vsp.vports[1]["max_tx_rate"] == 0 and vsp.dp.meters.meter_of(1) is None
    # an operator's rate is not the pod's: it survives both
    vsp.set_vf_rate(1, 50)
    vsp.create_bridge_port("host1-1", mac1, 1, ["3"])
    vsp.delete_bridge_port("host1-1")
    assert vsp.vports[1]["max_tx_rate"] == 50 and vsp.dp.meters.meter_of(1) == 1
    # a rate netlink holds that no meter can realise is logged, not applied
    nl.link_set_vf("ens1f0", 2, mac=MACS[2], max_tx_rate=T.METER_MAX_MBPS + 1)
    with caplog.at_level(logging.WARNING, logger="dpu.vsp.gpu"):
        caplog.clear()
        vsp.create_bridge_port("host1-2", bytes.fromhex(MACS[2].replace(":", "")), 1, ["4"])
    assert vsp.dp.meters.meter_of(2) is None
    assert any("not applied" in r.getMessage() for r in caplog.records)


def test_ring_and_native_engines_store_and_warn(caplog):
    for engine in ("ring", "native"):
        vsp = GpuVsp(device="cpu", flow_buckets=1 << 10, live=True, live_engine=engine)
        vsp._ensure_dp()
        vsp.vports[0] = {"name": "v0", "mac": MACS[0], "role": "free", "vlan": 0, "pod_mac": MACS[0], "bridge": 1}
        with caplog.at_level(logging.WARNING, logger="dpu.vsp.gpu"):
            caplog.clear()
            vsp.set_vf_rate(0, 100)
            vsp.set_vf_rate(0, 200)
        assert vsp.vports[0]["max_tx_rate"] == 200
        assert not vsp.dp.meters.active() and not vsp.dp.meters.configured(0)
        warned = [r for r in caplog.records if "not enforced" in r.getMessage()]
        assert len(warned) == 1                          # once


class QueuePort:
    """A vport for the live path without a netdev: frames in through inject(), out into `sent`."""

    def __init__(self):
        self.fd, self._w = os.pipe()
        os.set_blocking(self.fd, False)
        self.inq, self.sent = collections.deque(), []

    def inject(self, frame: bytes) -> None:
        self.inq.append(frame)
        os.write(self._w, b"x")

    def read(self):
        if not self.inq:
            return None
        os.read(self.fd, 1)
        return self.inq.popleft()

    def write(self, frame) -> bool:
        self.sent.append(bytes(frame))
        return True

    def close(self) -> None:
        os.close(self.fd)
        os.close(self._w)


def test_livepath_batch_engine_enforces_the_rate():
    """A pod bursts past its bucket through netio.LivePath (batch engine, the oracle): the peer
    receives only the green prefix and the meter's counters account for every frame sent."""
    from dpu_operator_amd.dataplane.netio import LivePath

    dp = DataPlane(device="cpu", flow_buckets=1 << 10, mac_slots=1 << 10)
    for i in range(2):
        dp.ports.set(i, flags=T.PORT_VALID, bridge_id=7, mac=MACS[i])
        dp.macs.insert(7, MACS[i], i)
    dp.meters.set(0, 100, 50_000)                        # 50 frames of 1000 B
    dp.meters.bind(0, 0)
    dp.commit(full=True)
    ports = {0: QueuePort(), 1: QueuePort()}
    live = LivePath(dp, ports, burst=512)
    try:
        hdr = bytes.fromhex(MACS[1].replace(":", "")) + bytes.fromhex(MACS[0].replace(":", "")) + b"\x88\xb5"
        sent = [hdr + i.to_bytes(2, "big") + bytes(1000 - 16) for i in range(120)]
        for f in sent:
            ports[0].inject(f)
        assert live.poll_once(0.5) > 0 and live.error is None
        assert ports[1].sent == sent[:50]                # the green prefix, in order, whole frames
        assert ports[0].sent == []
        ctr = dp.meter_counters()[0]
        assert tuple(int(x) for x in ctr) == (50, 50_000, 70, 70_000)
        assert dp.drop_counters().get("overflow") == 70 and live.stats["drop"] == 70
        assert int(dp.port_counters()[0, 0]) == 50       # red frames are not rx-counted
        # the peer is unmetered: its reply burst all arrives
        back = [bytes.fromhex(MACS[0].replace(":", "")) + bytes.fromhex(MACS[1].replace(":", "")) + b"\x88\xb5" +
                bytes(1000 - 14)] * 80
        for f in back:
            ports[1].inject(f)
        live.poll_once(0.5)
        assert ports[0].sent == back
    finally:
        for p in ports.values():
            p.close()
