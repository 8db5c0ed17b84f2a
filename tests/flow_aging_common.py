"""Shared by the flow-aging tests (CPU and GPU): an independent model of the idle timeouts (a dict
key -> [timeout ticks, last observed tick]; it shares no code with the oracle or the kernels) and a
runner that plays one schedule of traffic, inserts, erases, timeout changes, harvests and sweeps on
a DataPlane and checks every step against the model and two never-aged reference planes."""
import numpy as np

from dpu_operator_amd.dataplane import scenario as S
from dpu_operator_amd.dataplane.engine import DataPlane

TICK_NS = 100_000_000
BASE_NS = 1_000 * TICK_NS     # schedule time 0 (every time is a whole number of ticks)


class Model:
    def __init__(self):
        self.flows = {}        # key -> [timeout ticks, last observed tick (None: not yet swept)]
        self.active = set()    # keys hit since the last sweep

    def arm(self, key, ticks):
        if ticks:
            self.flows[key] = [ticks, None]
        else:
            self.flows.pop(key, None)

    def erase(self, key):
        self.flows.pop(key, None)
        self.active.discard(key)

    def hit(self, key):
        self.active.add(key)

    def sweep(self, now):
        out = set()
        for k, st in self.flows.items():
            if st[1] is None or k in self.active:
                st[1] = now
            elif now - st[1] >= st[0]:
                out.add(k)
        for k in out:
            del self.flows[k]
        self.active.clear()
        return out


def key_of(sc, i):
    return tuple(int(x) for x in sc.keys[i])


def make_plane(device, buckets, n_flows, installed, seed=3, aging=True, max_expired=65536):
    """A plane with the SFC scenario, the first `installed` of its flows in the table."""
    dp = DataPlane(device=device, flow_buckets=buckets)
    sc = S.build_sfc(dp, n_pods=4, n_flows=n_flows, n_acl=8, seed=seed, install_flows=False)
    if installed:
        dp.flows.insert_many(sc.keys[:installed], sc.actions[:installed])
    dp.commit(full=True)
    if aging:
        dp.enable_flow_aging(tick_ns=TICK_NS, max_expired=max_expired)
    return dp, sc


def to_dev(dp, pk, im):
    if not dp.gpu:
        return pk, im
    import torch

    return (torch.from_numpy(pk).to(dp.tdev), torch.from_numpy(im.view(np.int32)).to(dp.tdev))


def to_host(dp, r):
    if not dp.gpu:
        return np.asarray(r.out), np.asarray(r.meta, np.uint32)
    return r.out.cpu().numpy(), r.meta.cpu().numpy().view(np.uint32)


class Runner:
    """Plays ops on `dp`; `ref_all` has every scenario flow installed, `ref_none` none, neither ages:
    a frame of an installed flow must come out as from ref_all, any other as from ref_none."""

    def __init__(self, dp, sc, installed, ref_all=None, ref_none=None):
        self.dp, self.sc, self.model = dp, sc, Model()
        self.installed = set(range(installed))
        self.ref_all, self.ref_none = ref_all, ref_none
        self.expired_sets = []     # per sweep: the set of expired keys (as returned)
        self.batches = []          # per traffic batch: (out, meta)
        self.seed = 100

    def insert(self, idx):
        for i in idx:
            self.dp.flows.insert(self.sc.keys[i], self.sc.actions[i])
            self.installed.add(int(i))

    def erase(self, idx):
        for i in idx:
            assert self.dp.flows.erase(self.sc.keys[i])
            self.installed.discard(int(i))
            self.model.erase(key_of(self.sc, i))

    def arm(self, idx, idle_s):
        idx = np.asarray(idx)
        n = self.dp.set_flow_timeout(self.sc.keys[idx], idle_s)
        here = [int(i) for i in idx if int(i) in self.installed]
        assert n == len(here)
        for i in here:
            self.model.arm(key_of(self.sc, i), int(round(idle_s * 1e9)) // TICK_NS)

    def traffic(self, idx, per_flow=2):
        idx = np.asarray(idx)
        self.seed += 1
        pk, im, f = S.traffic(self.sc, per_flow * len(idx), seed=self.seed, flows=idx, return_flows=True)
        while True:   # (the generator draws flows at random: top up until every flow of idx has a frame)
            missing = np.setdiff1d(idx, f)
            if not len(missing):
                break
            self.seed += 1
            p2, i2, f2 = S.traffic(self.sc, per_flow * len(missing), seed=self.seed, flows=missing, return_flows=True)
            pk, im, f = np.concatenate([pk, p2]), np.concatenate([im, i2]), np.concatenate([f, f2])
        out, meta = to_host(self.dp, self.dp.run(*to_dev(self.dp, pk, im.copy())))
        for i in set(int(x) for x in f):
            if i in self.installed:
                self.model.hit(key_of(self.sc, i))
        if self.ref_all is not None:
            oa, ma = to_host(self.ref_all, self.ref_all.run(pk, im.copy()))
            on, mn = to_host(self.ref_none, self.ref_none.run(pk, im.copy()))
            inst = np.isin(f, np.fromiter(self.installed, np.int64, len(self.installed)))
            assert np.array_equal(meta, np.where(inst, ma, mn))
            assert np.array_equal(out, np.where(inst[:, None], oa, on))
            assert np.any(ma != mn)    # (a hit and a miss do differ: the check above is not vacuous)
        self.batches.append((out, meta))

    def harvest(self, idx):
        """flow_counters() of some flows: each call harvests."""
        return [self.dp.flow_counters(self.sc.keys[i]) for i in idx]

    def sweep(self, t_s, drain=False):
        """One age_flows at schedule time t_s (seconds, a multiple of the tick); `drain`: repeated
        while it returns anything (a list smaller than the expired set)."""
        now_ns = BASE_NS + int(round(t_s * 1e9))
        want = self.model.sweep(now_ns // TICK_NS)
        got = []
        while True:
            keys = self.dp.age_flows(now_ns)
            got += [tuple(int(x) for x in k) for k in keys]
            if not drain or not len(keys):
                break
        assert len(got) == len(set(got))           # no duplicates
        assert set(got) == want, (t_s, len(got), len(want))
        for k in got:
            assert self.dp.flows.find(k) < 0
        by_key = {key_of(self.sc, i): i for i in self.installed}
        for k in got:
            self.installed.discard(by_key[k])
        self.expired_sets.append(set(got))
        return set(got)


def model_schedule(r: Runner, n_installed: int):
    """The schedule of the model test and of the CPU / GPU twin test: needs >= 200 flows
    installed of 256 in the scenario.  Returns the per-sweep expired sets."""
    assert n_installed == 200
    A, B, C = np.arange(0, 40), np.arange(40, 80), np.arange(80, 100)
    rest = np.arange(100, 200)
    r.arm(A, 1.0)
    r.arm(B, 0.5)
    r.arm(C, 2.0)
    assert not r.sweep(0.0)                        # armed rows are new: dated by this sweep
    r.traffic(np.concatenate([A[:20], rest[:30]]))
    assert not r.sweep(0.4)
    assert len(r.sweep(0.5)) == 40                 # B: idle for exactly its timeout
    r.traffic(np.concatenate([B[:5], A[20:30], rest]))   # B is gone: its frames miss
    r.harvest(A[20:22])                            # a harvest between traffic and sweep hides nothing
    assert len(r.sweep(1.0)) == 10                 # A[30:40] (A[:20] seen at 0.4, A[20:30] just now)
    r.erase(C[:5])
    r.insert(C[:5])                                # back, unarmed
    r.arm(C[5:10], 0.3)                            # a changed timeout re-arms
    r.arm(C[10:12], 0)                             # disarmed
    r.arm(np.array([250]), 1.0)                    # not installed: ignored
    assert len(r.sweep(1.4)) == 20                 # A[:20]
    r.traffic(np.concatenate([C[:12], rest[:10]]))
    assert not r.sweep(1.6)                        # C[5:10] were hit
    r.insert(np.arange(200, 220))
    r.arm(np.arange(200, 220), 0.2)
    assert len(r.sweep(1.9)) == 5                  # C[5:10]: 0.3 after 1.6
    assert len(r.sweep(2.0)) == 18                 # C[12:20] (since 0.0) and A[20:30] (since 1.0)
    r.traffic(np.arange(200, 210))
    assert len(r.sweep(2.1)) == 10                 # 210..219: dated 1.9, idle for 0.2
    r.traffic(np.concatenate([A, B, C, np.arange(200, 220)]))   # mostly gone: misses
    assert not r.sweep(2.3)                        # 200..209 were hit
    assert len(r.sweep(2.5)) == 10                 # 200..209
    assert not r.model.flows
    return r.expired_sets


def moves_schedule(r: Runner):
    """A 16-bucket (64-slot) table filled past 85 % in rounds, with traffic and sweeps between the
    rounds, then left to expire: the late inserts relocate armed entries.  Returns the peak fill."""
    t, n, peak = 0.0, 0, 0
    for rnd in range(6):
        k = 10 if rnd < 5 else 8
        idx = np.arange(n, n + k)
        n += k
        r.insert(idx)
        r.arm(idx[: k // 2], 1.5 + 0.1 * rnd)
        r.arm(idx[k // 2:], 4.0)
        r.sweep(t)
        peak = max(peak, len(r.dp.flows))
        r.traffic(np.arange(rnd % 3, n, 3))
        r.sweep(t + 0.2)
        t += 0.4
    while t < 7.5:
        r.sweep(t)
        t += 0.5
    assert not r.model.flows and len(r.dp.flows) == 0
    return peak
