"""bench.py's plain run and `--dump-outputs`: the plain line carries the headline alone (what
`--full` adds stays null), and the dumped arrays are the last timed step's egress slots and
metadata - checked against the C++ oracle on that step's batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("p50_latency_us_64k_batch", "small_batch_host_rtt", "p50_latency_us_ring", "ring", "exchange", "unsteered",
             "variants", "imix", "value_mixed", "hop_pipeline", "live", "live_veth", "p50_latency_us_pod")


def test_dump_outputs_sample_is_fixed_and_exact(tmp_path):
    import bench

    n = bench.DUMP_ROWS + 12345
    rng = np.random.default_rng(5)
    out = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    meta = np.arange(n, dtype=np.int32)   # every word its own row number: the dump shows which rows were kept
    small = np.array([-1, -2**31, 7], np.int32)   # the GPU path holds the 32-bit words as int32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"out": out, "meta": meta, "small": small}, suffix=".rank1" if d == "b" else "")
    o, m = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "a" / "meta.npy")
    assert o.dtype == np.float32 and m.dtype == np.float64
    assert o.shape == (bench.DUMP_ROWS, 64) and m.shape == (bench.DUMP_ROWS,)
    assert o.nbytes + m.nbytes <= 64 << 20
    # the same rows of every array, ascending, values exact
    idx = m.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(o, out[idx].astype(np.float32))
    # a second dump keeps the same rows; a small array is written whole, its words as unsigned
    assert np.array_equal(np.load(tmp_path / "b" / "out.rank1.npy"), o)
    assert np.array_equal(np.load(tmp_path / "b" / "meta.rank1.npy"), m)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), np.array([2**32 - 1, 2**31, 7], np.float64))
    # tensors (what the fused path hands over: the sample is gathered on their device) give the same files
    import torch

    bench.dump_outputs(str(tmp_path / "t"), {"out": torch.from_numpy(out), "meta": torch.from_numpy(meta),
                                             "small": torch.from_numpy(small)})
    assert np.array_equal(np.load(tmp_path / "t" / "out.npy"), o) and np.load(tmp_path / "t" / "out.npy").dtype == o.dtype
    assert np.array_equal(np.load(tmp_path / "t" / "meta.npy"), m) and np.load(tmp_path / "t" / "meta.npy").dtype == m.dtype
    assert np.array_equal(np.load(tmp_path / "t" / "small.npy"), np.load(tmp_path / "a" / "small.npy"))


@pytest.mark.gpu
def test_plain_bench_run_dumps_last_step(tmp_path):
    from dpu_operator_amd.dataplane import scenario as S
    from dpu_operator_amd.dataplane.engine import DataPlane

    # warmup 2 + 4 timed steps over a rotation of 4: the last step runs batch 1, the first ran batch 0
    steps, warmup, batch, flows, rotate = 4, 2, 1 << 16, 1 << 16, 4
    assert (warmup + steps - 1) % rotate != 0
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", str(batch),
           "--flows", str(flows), "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["unit"] == "Mpps" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["forwarded_fraction"] == 1.0
    assert abs(line["value"] - batch / line["ms_per_step"] / 1e3) <= 0.01 * line["value"]
    assert all(line[k] is None for k in FULL_ONLY)
    # the oracle on the batch the last timed step ran (bench.py: seed r + 1 for batch r of the rotation)
    buckets = 1 << max(10, int(np.ceil(np.log2(flows / 2))))
    cpu = DataPlane(device="cpu", flow_buckets=buckets)
    sc = S.build_sfc(cpu, n_pods=8, n_flows=flows, n_acl=256, seed=0, pod_gpu=np.zeros(8, np.int64))
    cpu.commit(full=True)
    pk, im = S.traffic(sc, batch, seed=(warmup + steps - 1) % rotate + 1, src_pods=np.arange(8))
    rc = cpu.run(pk, im)
    out, meta = np.load(tmp_path / "dump" / "out.npy"), np.load(tmp_path / "dump" / "meta.npy")
    assert sorted(os.listdir(tmp_path / "dump")) == ["meta.npy", "out.npy"]
    assert out.dtype == np.float32 and meta.dtype == np.float64
    assert np.array_equal(meta, rc.meta.astype(np.float64))
    assert np.array_equal(out, rc.out.astype(np.float32))
