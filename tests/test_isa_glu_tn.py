"""Build-time invariants of glu_tn_kernel's tile loop (csrc/glu.hip), checked on the device assembly (no GPU), as
tests/test_isa_loop_waits.py does for glu_xa_kernel: register prefetch one tile ahead, two tiles per trip, so no wait inside the
loop may be a full `s_waitcnt vmcnt(0)` -- every wait leaves at least the next tile's four loads in flight -- and the kernel
keeps its accumulators, fragments and both register sets without scratch at four waves per SIMD."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_glu_tn_tile_loop_keeps_its_prefetch_in_flight_and_spills_nothing(tmp_path):
    sys.path.insert(0, ROOT)
    from unsloth_amd import _build
    import isa_loop_waits
    out = tmp_path / "glu.s"
    cmd = [HIPCC] + _build._flags("glu.hip") + ["--cuda-device-only", "-S", os.path.join(ROOT, "unsloth_amd", "csrc", "glu.hip"),
                                                "-o", str(out)]
    subprocess.run([c for c in cmd if c != "-fPIC"], check=True, capture_output=True)
    asm = out.read_text()
    kernels = {k: v for k, v in isa_loop_waits.loops_of(str(out)).items() if re.search(r"\d+glu_tn_kernelI", k)}
    assert len(kernels) == 2, sorted(kernels)                   # bf16, fp16
    for k, ls in kernels.items():
        lab, n, nld, nst, waits, drains = max(ls, key=lambda l: l[1])      # the tile loop is the longest loop of the kernel
        assert nld == 8 and nst == 6, (k, nld, nst)             # two tiles per trip: dw, e, g, P loads; df, de, row-product stores
        assert not drains, f"{k}: full vmcnt(0) inside the tile loop at body offsets {drains} (waits {waits})"
        assert all(int(w) >= 4 for w in waits), (k, waits)      # the next tile's loads are never waited for
        assert int(re.search(re.escape(k) + r"\.private_seg_size, (\d+)", asm).group(1)) == 0, k
        assert int(re.search(re.escape(k) + r"\.num_vgpr, (\d+)", asm).group(1)) <= 128, k
