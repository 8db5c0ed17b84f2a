"""The flow-aging kernels (csrc/nfdp/age.hip) use no scratch memory, spill nothing and keep the full
occupancy (CPU: reads the compiler's resource remarks the build records in dpu_operator_amd/native/
_nfdp.resources.json; without a current record they are produced here, a few seconds)."""
import json
import subprocess
from pathlib import Path

import pytest

from dpu_operator_amd.native.build import parse_resource_remarks

REPO = Path(__file__).resolve().parent.parent
SRC = REPO / "csrc" / "nfdp"
RECORD = REPO / "dpu_operator_amd" / "native" / "_nfdp.resources.json"
KERNELS = ["age_sweep_kernel", "harvest_age_kernel"]


@pytest.fixture(scope="module")
def rows():
    newest = max(p.stat().st_mtime for p in list(SRC.glob("*.h")) + [SRC / "age.hip"])
    if RECORD.exists() and RECORD.stat().st_mtime >= newest:
        rec = json.loads(RECORD.read_text())
        if not rec.get("flags") and "age.hip" in rec["sources"]:
            return rec["sources"]["age.hip"]
    cmd = ["/opt/rocm/lib/llvm/bin/clang++", "--offload-arch=gfx950", "-x", "hip", "-munsafe-fp-atomics", "-O3",
           "-std=c++17", "-I", str(SRC), "--cuda-device-only", "-c", str(SRC / "age.hip"), "-o", "/dev/null",
           "-Rpass-analysis=kernel-resource-usage"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired) as e:
        pytest.skip(f"no gfx950 compiler here: {e}")
    assert r.returncode == 0, r.stderr[-2000:]
    return parse_resource_remarks(r.stderr)


@pytest.mark.parametrize("kernel", KERNELS)
def test_age_kernels_use_no_scratch_and_keep_occupancy(rows, kernel):
    hits = [r for r in rows if kernel in r["name"]]
    assert len(hits) == 1, (kernel, [r["name"] for r in rows])
    r = hits[0]
    assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r
    assert r.get("SGPRs Spill", 0) == 0, r
    assert r.get("LDS Size [bytes/block]", 0) == 0, r
    # streaming passes: nothing below the full 8 waves per SIMD
    assert r.get("Occupancy [waves/SIMD]", 0) == 8, r
