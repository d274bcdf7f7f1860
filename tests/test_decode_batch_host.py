"""CPU: the host side of batched decode (models/decode.py) -- the left-padding classifier, where `unsloth_fast_generate` sends
a call (`num_return_sequences`, `generation_config=`, padded masks) checked with a stub engine, and the new C symbol."""
from types import SimpleNamespace

import pytest
import torch

from tests._decode_batched import Recorder, StubEngine


def test_left_padded_masks_give_lengths_everything_else_is_refused():
    from unsloth_amd.models.decode import left_pad_lengths
    assert left_pad_lengths(torch.tensor([[0, 0, 1], [1, 1, 1], [0, 1, 1]])).tolist() == [1, 3, 2]
    assert left_pad_lengths(torch.ones(2, 5, dtype=torch.long)).tolist() == [5, 5]
    assert left_pad_lengths(torch.tensor([[0, 0, 0, 7]])).tolist() == [1]            # any non-zero is a real token
    assert left_pad_lengths(torch.tensor([[1, 1, 0], [1, 1, 1]])) is None            # right padding
    assert left_pad_lengths(torch.tensor([[0, 1, 0, 1]])) is None                    # a hole
    assert left_pad_lengths(torch.tensor([[0, 1, 1, 0]])) is None                    # padded on both sides
    assert left_pad_lengths(torch.tensor([[0, 0], [1, 1]])) is None                  # an empty row


def _model(B, S):
    m = SimpleNamespace(generation_config=None, model=None)
    m._uamd_decode_engine = StubEngine(B, S)
    m._old_generate = Recorder(ret="hf")
    return m


def test_routing_of_num_return_sequences():
    from unsloth_amd.models.decode import unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(6, 64)
    out = unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, do_sample=True, temperature=2.0)
    assert out.shape == (6, 7) and not m._old_generate.calls
    kw = m._uamd_decode_engine.calls[-1]
    assert kw["num_return_sequences"] == 3 and kw["do_sample"] and kw["temperature"] == 2.0 and kw["max_new_tokens"] == 3
    with pytest.raises(ValueError):                                                  # greedy: one sequence per prompt, as in HF
        unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3)
    assert len(m._uamd_decode_engine.calls) == 1 and not m._old_generate.calls
    m = _model(2, 64)
    unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=1)
    assert m._uamd_decode_engine.calls[-1]["num_return_sequences"] == 1


def test_routing_of_generation_config():
    from transformers import GenerationConfig
    from unsloth_amd.models.decode import route_generate, unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(2, 64)
    gc = GenerationConfig(do_sample=True, temperature=0.7, top_p=0.9, max_new_tokens=5)
    out = unsloth_fast_generate(m, ids, generation_config=gc)
    assert out.shape == (2, 9) and not m._old_generate.calls
    kw = m._uamd_decode_engine.calls[-1]
    assert kw["do_sample"] and kw["temperature"] == pytest.approx(0.7) and kw["top_p"] == pytest.approx(0.9)
    # explicit keywords stand above the object, the object above the model's own generation config
    m.generation_config = GenerationConfig(do_sample=True, temperature=0.3, top_p=0.5, max_new_tokens=11)
    unsloth_fast_generate(m, ids, generation_config=gc, temperature=1.5, max_new_tokens=2)
    kw = m._uamd_decode_engine.calls[-1]
    assert kw["temperature"] == 1.5 and kw["top_p"] == pytest.approx(0.9) and kw["max_new_tokens"] == 2
    unsloth_fast_generate(m, ids)
    kw = m._uamd_decode_engine.calls[-1]
    assert kw["temperature"] == pytest.approx(0.3) and kw["max_new_tokens"] == 11
    # num_return_sequences may come from the object
    m6 = _model(6, 64)
    unsloth_fast_generate(m6, ids, generation_config=GenerationConfig(do_sample=True, num_return_sequences=3, max_new_tokens=2))
    assert m6._uamd_decode_engine.calls[-1]["num_return_sequences"] == 3
    # a field the engine does not implement, set to something that matters: HF's generate
    n = len(m._uamd_decode_engine.calls)
    bad = GenerationConfig(do_sample=True, repetition_penalty=1.1, max_new_tokens=5)
    assert unsloth_fast_generate(m, ids, generation_config=bad) == "hf"
    assert len(m._old_generate.calls) == 1 and m._old_generate.calls[-1][1]["generation_config"] is bad
    assert len(m._uamd_decode_engine.calls) == n
    assert route_generate(m, ids, None, dict(generation_config=GenerationConfig(num_beams=4)))[0] == "old"
    assert route_generate(m, ids, None, dict(generation_config=GenerationConfig(repetition_penalty=1.0)))[0] == "engine"
    # still unsupported, as before
    assert route_generate(m, ids, 3, dict(return_dict_in_generate=True))[0] == "old"
    assert route_generate(m, ids, 3, dict(output_scores=True))[0] == "old"


def test_routing_of_padded_masks():
    from unsloth_amd.models.decode import unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(2, 64)
    left = torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1]])
    unsloth_fast_generate(m, ids, max_new_tokens=3, attention_mask=left)
    assert not m._old_generate.calls and m._uamd_decode_engine.calls[-1]["attention_mask"] is left
    unsloth_fast_generate(m, ids, max_new_tokens=3, attention_mask=torch.ones_like(ids))
    assert not m._old_generate.calls and m._uamd_decode_engine.calls[-1]["attention_mask"] is None
    # the pad token, where one is known (keyword, generation_config= or the model's config), is what the zeros must hide
    ids7 = torch.tensor([[7, 7, 3, 4], [1, 2, 3, 4]])
    unsloth_fast_generate(m, ids7, max_new_tokens=3, attention_mask=left, pad_token_id=7)
    assert not m._old_generate.calls and m._uamd_decode_engine.calls[-1]["attention_mask"] is left
    m.generation_config = SimpleNamespace(pad_token_id=7, eos_token_id=None, max_new_tokens=None)
    unsloth_fast_generate(m, ids7, max_new_tokens=3, attention_mask=left)
    assert not m._old_generate.calls and len(m._uamd_decode_engine.calls) == 4
    assert unsloth_fast_generate(m, ids, max_new_tokens=3, attention_mask=left) == "hf"          # zeros hide token 0, pad is 7
    assert len(m._old_generate.calls) == 1 and m._old_generate.calls[-1][1]["attention_mask"] is left
    assert unsloth_fast_generate(m, ids7, max_new_tokens=3, attention_mask=left, pad_token_id=9) == "hf"
    assert len(m._old_generate.calls) == 2 and len(m._uamd_decode_engine.calls) == 4
    m.generation_config = None
    for refused in (torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1]]), torch.tensor([[1, 0, 1, 1], [1, 1, 1, 1]]),
                    torch.tensor([[0, 0, 0, 0], [1, 1, 1, 1]])):
        n = len(m._old_generate.calls)
        assert unsloth_fast_generate(m, ids, max_new_tokens=3, attention_mask=refused) == "hf"
        assert len(m._old_generate.calls) == n + 1 and m._old_generate.calls[-1][1]["attention_mask"] is refused
    del m._old_generate
    with pytest.raises(NotImplementedError):
        unsloth_fast_generate(m, ids, max_new_tokens=3, attention_mask=torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1]]))


def test_the_rows_kernel_is_part_of_the_abi():
    import ctypes
    from unsloth_amd import _lib
    assert "uamd_gemv_rows" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["uamd_gemv_rows"]
    assert res is ctypes.c_int and len(args) == 12 and args[4] == ctypes.POINTER(_lib.GemvGroup)
