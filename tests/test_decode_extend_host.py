"""Host side of chunked prefill: `prefill_chunk_size` reaches the engine; without it a call is routed as before."""
from types import SimpleNamespace

import torch

from tests._decode_batched import Recorder, StubEngine


def test_prefill_chunk_size_reaches_the_engine():
    from unsloth_amd.models.decode import route_generate, unsloth_fast_generate
    ids = torch.zeros(2, 40, dtype=torch.long)
    m = SimpleNamespace(generation_config=None, model=None, _uamd_decode_engine=StubEngine(2, 64), _old_generate=Recorder(ret="hf"))
    unsloth_fast_generate(m, ids, max_new_tokens=3)
    plain = m._uamd_decode_engine.calls[-1]
    assert "prefill_chunk_size" not in plain and "append" not in plain
    unsloth_fast_generate(m, ids, max_new_tokens=3, prefill_chunk_size=16)
    assert m._uamd_decode_engine.calls[-1] == dict(plain, prefill_chunk_size=16) and not m._old_generate.calls
    where, what = route_generate(m, ids, 3, dict(prefill_chunk_size=16))
    assert where == "engine" and what["prefill_chunk_size"] == 16
    assert "prefill_chunk_size" not in route_generate(m, ids, 3, {})[1]
    # the model's record (for_inference(model, prefill_chunk_size=N)); the call's keyword wins, 0 switches it off
    m._uamd_prefill_chunk_size = 8
    unsloth_fast_generate(m, ids, max_new_tokens=3)
    assert m._uamd_decode_engine.calls[-1]["prefill_chunk_size"] == 8
    unsloth_fast_generate(m, ids, max_new_tokens=3, prefill_chunk_size=0)
    assert m._uamd_decode_engine.calls[-1] == plain
    # a call HF's generate takes keeps going there, without the engine's keyword
    assert unsloth_fast_generate(m, ids, max_new_tokens=3, prefill_chunk_size=16, repetition_penalty=1.3) == "hf"
    assert "prefill_chunk_size" not in m._old_generate.calls[-1][1]
