"""What the token-bucket policer (csrc/nfdp/police.hip) costs on the headline scenario.

The headline shape (4M slots, 1M flows, ACL 256 -> SNAT -> L2, 8 pods) through DataPlane.run:
  * once with no meter: the path of every batch before the policer existed (nothing else launched);
  * once with every pod port bound to a meter of its own, at a rate and bucket that pass about half
    of each batch's bytes (the batches' arrival times advance by --dt-us per step).
The two are timed alternately, `--runs` times `--steps` steps each after a warm-up (device events
around the steps); then each police kernel alone (sum, scan, apply, commit, fix; events around
single launches, one sample per run).  Medians are reported.  Prints one JSON line and writes it
to --out.  A measurement needs the GPU: there is no CPU fall-back.

Usage: python tools/police_bench.py [--batch 4194304] [--flows 1048576] [--runs 7] [--steps 10] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = (("police_sum", 1), ("police_scan", 2), ("police_apply", 4), ("police_commit", 8))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 22)
    ap.add_argument("--flows", type=int, default=1 << 20)
    ap.add_argument("--acl", type=int, default=256)
    ap.add_argument("--pods", type=int, default=8)
    ap.add_argument("--hash", default="lds")
    ap.add_argument("--rotate", type=int, default=2, help="distinct traffic batches")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=7, help="timed runs per variant (>= 5)")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed run")
    ap.add_argument("--dt-us", type=float, default=1000.0, help="arrival-time step between batches")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("police_bench measures on the GPU: none visible")
    from dpu_operator_amd.dataplane import scenario as S
    from dpu_operator_amd.dataplane.engine import DataPlane

    dev = torch.device("cuda", 0)
    buckets = 1 << max(10, int(math.ceil(math.log2(a.flows / 2))))
    dp = DataPlane(device=str(dev), flow_buckets=buckets, hash_mode=a.hash, acl_mode="mfma")
    sc = S.build_sfc(dp, n_pods=a.pods, n_flows=a.flows, n_acl=a.acl, seed=0)
    dp.commit(full=True)
    n = a.batch
    batches, pod_bytes = [], None
    for r in range(a.rotate):
        pk, im = S.traffic(sc, n, seed=r + 1)
        if pod_bytes is None:
            pod_bytes = np.bincount((im & 0xFFFF).astype(np.int64), weights=(im >> 16).astype(np.float64),
                                    minlength=a.pods)[: a.pods]
        batches.append((torch.from_numpy(pk).to(dev), torch.from_numpy(im.view(np.int32)).to(dev)))
        del pk, im
    out, meta, lat = dp.alloc_batch(n)
    # a bucket of half a batch's bytes per pod, refilled by as much per step: about half is dropped
    dt_ns = int(a.dt_us * 1000)
    half = int(pod_bytes.mean() / 2)
    mbps = max(1, min(400000, round(half / (dt_ns * 1e-9) * 8 / 1e6)))
    ports = [int(p) for p in sc.pod_port]

    def bind(on: bool) -> None:
        for k, p in enumerate(ports):
            if on:
                dp.meters.set(k, mbps, half)
            dp.meters.bind(p, k if on else None)
        dp.commit()

    clock = [1_000_000_000]

    def steps(k: int) -> float:
        """k steps -> microseconds per step (device events; ends in a synchronise)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(k):
            pk, im = batches[j % a.rotate]
            clock[0] += dt_ns
            dp.run(pk, im, out, meta, lat, now_ns=clock[0])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k

    def check(metered: bool) -> None:
        """The benchmark measures what it says: in-metas restored, about half dropped (or none)."""
        torch.cuda.synchronize()
        assert int((batches[0][1].view(torch.int32) & 0xF000).ne(0).sum()) == 0, "an in-meta was left marked"
        of = int(((meta.view(torch.int32) >> 26) & 0xF).eq(11).sum())
        assert (of > 0) == metered, (of, metered)

    res = {"unmetered": [], "metered": []}
    for metered in (False, True):     # warm up both shapes
        bind(metered)
        steps(a.warmup)
        check(metered)
    dp.reset_counters()
    for _ in range(max(a.runs, 5)):   # alternating: both variants see the same machine state
        for metered in (False, True):
            bind(metered)
            steps(1)
            res["metered" if metered else "unmetered"].append(steps(a.steps))
    ctr = dp.meter_counters()[: a.pods].astype(np.float64)
    drop_frac = float(ctr[:, 3].sum() / max(ctr[:, 1].sum() + ctr[:, 3].sum(), 1))

    # each police kernel alone: one launch between two events, the fix after the fused pass
    bind(True)
    nf, s = dp.nf, torch.cuda.current_stream(dev).cuda_stream
    per = {name: [] for name, _ in PHASES}
    per["police_fix"], per["fused_and_rest"] = [], []
    for r in range(max(a.runs, 5)):
        pk, im = batches[r % a.rotate]
        clock[0] += dt_ns
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 4)]
        ev[0].record()
        for j, (_, bit) in enumerate(PHASES):
            nf.launch_police(dp._meter_ptrs(), im.data_ptr(), n, clock[0], True, s, phases=bit)
            ev[j + 1].record()
        dp._police_on = False          # the fused pass alone over the marked batch
        dp.run(pk, im, out, meta, lat)
        dp._police_on = True
        ev[5].record()
        nf.launch_police_fix(im.data_ptr(), meta.data_ptr(), n, dp._ptr("drop_ctr"), True, s)
        ev[6].record()
        ev[6].synchronize()
        for j, (name, _) in enumerate(PHASES):
            per[name].append(ev[j].elapsed_time(ev[j + 1]) * 1e3)
        per["fused_and_rest"].append(ev[4].elapsed_time(ev[5]) * 1e3)
        per["police_fix"].append(ev[5].elapsed_time(ev[6]) * 1e3)
    check(True)

    med = statistics.median
    kern = {k: round(med(v), 2) for k, v in per.items()}
    police = sum(kern[k] for k, _ in PHASES) + kern["police_fix"]
    r = {
        "tool": "police_bench", "box": torch.cuda.get_device_name(dev), "batch": n, "flows": a.flows, "acl": a.acl,
        "pods": a.pods, "meters": a.pods, "mbps": mbps, "burst_bytes": half, "dt_us": a.dt_us,
        "red_byte_fraction": round(drop_frac, 4), "runs": len(res["metered"]), "steps_per_run": a.steps,
        "unmetered_step_us": round(med(res["unmetered"]), 2), "metered_step_us": round(med(res["metered"]), 2),
        "unmetered_runs_us": [round(x, 1) for x in res["unmetered"]],
        "metered_runs_us": [round(x, 1) for x in res["metered"]],
        "kernel_us": kern, "police_kernels_us": round(police, 2),
        "police_ranges": list(nf.police_ranges(n)),
    }
    r["police_over_unmetered"] = round(r["metered_step_us"] / r["unmetered_step_us"] - 1, 4)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r, indent=1) + "\n")


if __name__ == "__main__":
    main()
