"""CPU: the host side of decoding 17 .. 64 sequences -- no instance of the rows kernel (csrc/decode.hip gemv_rows_kernel, the
MT = 2 | 4 token-tile instances of uamd_gemv_rows64 among them) uses scratch, and `unsloth_fast_generate` sends a call of 48 rows
to an engine of batch 48 and still builds an engine for 80."""
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from tests._decode_batched import Recorder, StubEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_instance_of_the_rows_kernel_uses_scratch(tmp_path):
    """The widest instances hold 64 accumulator and 64 token-fragment registers beside two stages of weights: they take one
    workgroup per CU rather than spill. Kernel metadata of every gemv_rows_kernel instance: no private segment, no spilled
    register; and every (NF4 | dense, RT, MT) instance the launchers name is there, for both 16-bit types."""
    import sys
    sys.path.insert(0, ROOT)
    from unsloth_amd import _build
    out = tmp_path / "decode.s"
    cmd = [HIPCC] + _build._flags("decode.hip") + ["--cuda-device-only", "-S",
           os.path.join(ROOT, "unsloth_amd", "csrc", "decode.hip"), "-o", str(out)]
    subprocess.run([c for c in cmd if c != "-fPIC"], check=True, capture_output=True)
    lines = out.read_text().split("\n")
    seen = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s+\.name:\s+(_ZN\S*gemv_rows_kernelI(DF16b|DF16_)Lb([01])ELi(\d)ELi(\d)E\S*)$", l)
        if not m:
            continue
        meta = {}
        for k in lines[i - 12:i + 12]:                                # the fields of this kernel's metadata entry
            mm = re.match(r"\s+\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", k)
            if mm:
                meta.setdefault(mm.group(1), int(mm.group(2)))
        key = (m.group(2), bool(int(m.group(3))), int(m.group(4)), int(m.group(5)))
        seen[key] = meta
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (key, meta)
        assert meta["vgpr_count"] <= 256, (key, meta)
    want = {(t, nf4, rt, mt) for t in ("DF16b", "DF16_") for mt in (1, 2, 4)
            for nf4, rts in ((True, (1, 2, 4)), (False, (1, 2))) for rt in rts}
    assert set(seen) == want, set(seen) ^ want
    assert any(mt > 1 for _, _, _, mt in seen)


def _model(B, S):
    m = SimpleNamespace(generation_config=None, model=None)
    m._uamd_decode_engine = StubEngine(B, S)
    m._old_generate = Recorder(ret="hf")
    return m


def test_routing_of_48_and_80_rows(monkeypatch):
    from unsloth_amd.kernels import decode as D
    from unsloth_amd.models import decode as MD
    assert (D.MAX_ROWS, D.MAX_ROWS_WIDE) == (16, 64)
    built = []

    def make(model, max_seq_len=None, batch=1, **kw):
        built.append(batch)
        return StubEngine(batch, max_seq_len)
    monkeypatch.setattr(MD, "DecodeEngine", make)
    kw = dict(max_new_tokens=3, do_sample=True, temperature=2.0)
    m = _model(48, 64)                                               # the engine of an earlier call of 48 rows serves this one
    out = MD.unsloth_fast_generate(m, torch.zeros(6, 4, dtype=torch.long), num_return_sequences=8, **kw)
    assert out.shape == (48, 7) and not built and not m._old_generate.calls
    assert m._uamd_decode_engine.B == 48 and m._uamd_decode_engine.calls[-1]["num_return_sequences"] == 8
    m = _model(6, 64)                                                # another batch: an engine of 48 rows is built
    out = MD.unsloth_fast_generate(m, torch.zeros(6, 4, dtype=torch.long), num_return_sequences=8, **kw)
    assert out.shape == (48, 7) and built == [48] and m._uamd_decode_engine.B == 48 and not m._old_generate.calls
    out = MD.unsloth_fast_generate(m, torch.zeros(10, 4, dtype=torch.long), num_return_sequences=8, **kw)
    assert out.shape == (80, 7) and built == [48, 80] and m._uamd_decode_engine.B == 80 and not m._old_generate.calls
