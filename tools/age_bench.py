"""What the flow-aging sweep (csrc/nfdp/age.hip) costs, against the only way to find idle flows
without it: DataPlane.harvest(), which copies every packed counter to the host.

For each table size (the headline table: 1M flows in 2^21 slots; and a large one, --large-log2 slots):
  * age_sweep_kernel over a table with every slot armed, with no slot / 1 % / every slot expired
    (a sweep leaves kept and expired rows as they are, so every launch does the same work);
  * harvest_age_kernel against the plain harvest_kernel;
  * the sweep end to end as DataPlane.age_flows pays for it (launch, synchronise, count and list
    read back) with 1 % expired, and DataPlane.harvest() end to end (kernel, the device-to-host
    copy of 8 B per slot, the unpack and accumulate in numpy), aging off and on.
Kernel times: device events around --launches back-to-back launches, the variants alternating,
--runs runs after a warm-up, medians reported.  End-to-end times: a host clock around calls that end
in a synchronise.  Bytes per sweep are counted from the shapes (16-B row + 8-B counter per armed slot,
4 B per listed slot) and put against the HBM bandwidth measured for an in-order sweep.  Prints one
JSON line and writes it to --out.  A measurement needs the GPU: there is no CPU fall-back.

Usage: python tools/age_bench.py [--large-log2 27] [--runs 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SWEEP_TBPS = 6.0      # measured in-order HBM table sweep on an MI355X (8 TB/s spec)
NOW = 1000


def bench_table(nf, torch, dev, n, runs, launches, cap):
    from dpu_operator_amd.dataplane.engine import DataPlane

    s = torch.cuda.current_stream(dev).cuda_stream
    med = statistics.median
    ctr = torch.full((n,), (3 << 40) | 192, dtype=torch.int64, device=dev)
    out = torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    hv = torch.empty(n, dtype=torch.int64, device=dev)

    def rows_for(frac_expired):
        """Every slot armed (timeout 50 ticks), seen == counter; the expired ones idle for 60."""
        w = torch.empty((n, 2), dtype=torch.int64, device=dev)
        w[:, 0] = (3 << 40) | 192
        i = torch.arange(n, device=dev)
        exp = (i % 100 == 0) if frac_expired == 0.01 else torch.full((n,), bool(frac_expired), device=dev)
        last = torch.where(exp, torch.tensor(NOW - 60, device=dev), torch.tensor(NOW - 10, device=dev))
        w[:, 1] = last | (50 << 32)
        return w

    variants = {"none": rows_for(0.0), "one_percent": rows_for(0.01), "all": rows_for(1.0)}
    hrows = rows_for(0.0)                 # the harvests' own rows (they reset `seen`)

    def sweep(rows, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            nf.launch_age_sweep(ctr.data_ptr(), rows.data_ptr(), n, NOW, out.data_ptr(), cap, cnt.data_ptr(), s)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k

    def harvest(aged, k):
        rows = hrows
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            if aged:
                nf.launch_harvest_age(ctr.data_ptr(), rows.data_ptr(), hv.data_ptr(), n, s)
            else:
                nf.launch_harvest(ctr.data_ptr(), hv.data_ptr(), n, s)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k

    def sweep_e2e(rows):
        t0 = time.perf_counter()
        nf.launch_age_sweep(ctr.data_ptr(), rows.data_ptr(), n, NOW, out.data_ptr(), cap, cnt.data_ptr(), s)
        torch.cuda.current_stream(dev).synchronize()
        c = int(cnt.cpu().numpy().view(np.uint32)[0])
        lst = out[: min(c, cap)].cpu().numpy()
        return (time.perf_counter() - t0) * 1e6, c, len(lst)

    t = {f"sweep_{k}": [] for k in variants}
    t.update(harvest_plain=[], harvest_age=[], sweep_e2e=[])
    counts = {}
    for k, rows in variants.items():      # warm-up; the counts say the tables are what they claim
        sweep(rows, 2)
        counts[k] = int(cnt.cpu().numpy().view(np.uint32)[0])
    assert counts == {"none": 0, "one_percent": (n + 99) // 100, "all": n}, counts
    ctr_before = ctr.clone()
    harvest(True, 1)
    harvest(False, 1)
    ctr.copy_(ctr_before)                  # (the harvests zero the counters; their timing does not depend on it)
    for _ in range(runs):
        for k, rows in variants.items():
            t[f"sweep_{k}"].append(sweep(rows, launches))
        t["sweep_e2e"].append(sweep_e2e(variants["one_percent"])[0])
    ctr.copy_(ctr_before)
    for _ in range(runs):
        t["harvest_plain"].append(harvest(False, launches))
        t["harvest_age"].append(harvest(True, launches))
    ctr.copy_(ctr_before)
    del variants, hrows, hv
    torch.cuda.empty_cache()

    # DataPlane.harvest() end to end on a plane of this size (no flows needed: the harvest reads
    # every slot's counter whatever the table holds), aging off, then on
    e2e = {"off": [], "on": []}
    dp = DataPlane(device=str(dev), flow_buckets=n // 4)
    reps = max(3, min(runs, 5))
    for mode in ("off", "on"):
        if mode == "on":
            dp.enable_flow_aging()
        dp.harvest()
        for _ in range(reps):
            t0 = time.perf_counter()
            dp.harvest()
            e2e[mode].append((time.perf_counter() - t0) * 1e6)
    del dp
    torch.cuda.empty_cache()

    r = {"slots": n, "cap": cap, "launches_per_run": launches, "runs": runs}
    for k, v in t.items():
        r[k + "_us"] = round(med(v), 2)
    r["sweep_runs_us"] = {k: [round(x, 1) for x in t[f"sweep_{k}"]] for k in ("none", "one_percent", "all")}
    r["harvest_e2e_us"] = {m: round(med(v), 1) for m, v in e2e.items()}
    r["harvest_e2e_runs_us"] = {m: [round(x) for x in v] for m, v in e2e.items()}
    r["expired_counts"] = counts
    for k in ("none", "one_percent", "all"):
        listed = min(counts[k], cap)
        b = 24 * n + 4 * listed
        r[f"sweep_{k}_bytes"] = b
        tbps = b / (r[f"sweep_{k}_us"] * 1e-6) / 1e12
        r[f"sweep_{k}_TBps"] = round(tbps, 3)
        r[f"sweep_{k}_of_hbm_sweep"] = round(tbps / HBM_SWEEP_TBPS, 3)
    r["harvest_e2e_over_sweep_e2e"] = round(r["harvest_e2e_us"]["off"] / r["sweep_e2e_us"], 1)
    r["harvest_copy_bytes"] = 8 * n
    return r


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--headline-log2", type=int, default=21, help="slots of the headline table (1M flows: 2^21)")
    ap.add_argument("--large-log2", type=int, default=27, help="slots of the large table")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--cap", type=int, default=65536, help="expired-list entries (DataPlane max_expired)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("age_bench measures on the GPU: none visible")
    from dpu_operator_amd.native import nfdp

    nf = nfdp()
    dev = torch.device("cuda", 0)
    res = {"tool": "age_bench", "box": torch.cuda.get_device_name(dev), "hbm_sweep_TBps_reference": HBM_SWEEP_TBPS,
           "age_grid": {}, "tables": {}}
    for name, lg, launches in (("headline", a.headline_log2, 50), ("large", a.large_log2, 5)):
        n = 1 << lg
        res["age_grid"][name] = list(nf.age_grid(n))
        res["tables"][name] = bench_table(nf, torch, dev, n, max(a.runs, 5), launches, a.cap)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
