"""CPU: the host side of prompt-lookup decoding -- the draft and accept rules of tests/_lookup_ref.py on hand-written cases
(tests/test_gpu_decode_lookup.py runs the same cases through uamd_ngram_draft / uamd_accept_greedy), where
`unsloth_fast_generate` sends a call with HF's two keywords, and the new C symbols."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests import _lookup_ref as ref
from tests._decode_batched import Recorder, StubEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("uamd_rope_kv_append_span", "uamd_attn_decode_span", "uamd_ngram_draft", "uamd_accept_greedy")


@pytest.mark.parametrize("case", ref.DRAFT_CASES, ids=[c[0] for c in ref.DRAFT_CASES])
def test_draft_rule(case):
    _, hist, K, n_max, tok, nd = case
    assert ref.draft(hist, K, n_max) == (tok, nd)


@pytest.mark.parametrize("case", ref.ACCEPT_CASES, ids=[c[0] for c in ref.ACCEPT_CASES])
def test_accept_rule(case):
    _, tok, a, eos, remaining, m, done = case
    assert ref.accept(tok, a, eos, remaining) == (m, done)


def test_replay_of_a_periodic_text():
    # period 4 after a prompt of 6: the first step sees one period and a half, from then on every step yields K + 1 tokens
    seq = [1, 2, 3, 4, 1, 2] + [3, 4, 1, 2] * 5
    stats, per_step, new = ref.replay(seq, 6, 3, 2)
    assert new == 20 and sum(per_step) == 19 and per_step[:-1] == [4] * 4 and stats["tokens"] == 19
    assert stats["accepted"] == 19 - stats["steps"] and stats["drafted"] >= stats["accepted"]
    # an eos in the middle of a draft ends the text there; max_new_tokens cuts the last step
    stats, per_step, new = ref.replay(seq[:6 + 3], 6, 3, 2, eos=[1])           # drafts 4 1 2 after the first token 3
    assert seq[6:9] == [3, 4, 1] and new == 3 and per_step == [2] and stats["drafted"] == 3 and stats["accepted"] == 1
    stats, per_step, new = ref.replay(seq[:6 + 6], 6, 3, 2, max_new_tokens=6)
    assert new == 6 and per_step == [4, 1]


def _model(B, S):
    m = SimpleNamespace(generation_config=None, model=None)
    m._uamd_decode_engine = StubEngine(B, S)
    m._old_generate = Recorder(ret="hf")
    return m


def test_routing_of_prompt_lookup(monkeypatch):
    from transformers import GenerationConfig
    from unsloth_amd.models.decode import route_generate, unsloth_fast_generate
    ids = torch.zeros(1, 4, dtype=torch.long)
    m = _model(1, 64)
    out = unsloth_fast_generate(m, ids, max_new_tokens=5, prompt_lookup_num_tokens=4)
    assert out.shape == (1, 9) and not m._old_generate.calls
    kw = m._uamd_decode_engine.calls[-1]
    assert kw["prompt_lookup_num_tokens"] == 4 and kw["max_matching_ngram_size"] == 2 and not kw["do_sample"]
    where, what = route_generate(m, ids, 5, dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=3))
    assert where == "engine" and what["need"] == 4 + 5 + 4 and what["batch"] == 1 and what["max_matching_ngram_size"] == 3
    # the same two fields of a generation_config= object; keywords stand above it
    gc = GenerationConfig(prompt_lookup_num_tokens=6, max_matching_ngram_size=4, max_new_tokens=3)
    where, what = route_generate(m, ids, None, dict(generation_config=gc))
    assert where == "engine" and what["prompt_lookup_num_tokens"] == 6 and what["max_matching_ngram_size"] == 4
    assert what["need"] == 4 + 3 + 6
    where, what = route_generate(m, ids, None, dict(generation_config=gc, prompt_lookup_num_tokens=2))
    assert what["prompt_lookup_num_tokens"] == 2 and what["need"] == 4 + 3 + 2
    # None / 0: neutral -- the settings of a call without the keyword
    plain = route_generate(m, ids, 5, {})
    for off in (None, 0):
        assert route_generate(m, ids, 5, dict(prompt_lookup_num_tokens=off)) == plain
    assert "prompt_lookup_num_tokens" not in plain[1] and plain[1]["need"] == 9
    # an engine too small for the K draft slots is replaced by one that holds them: 4 + 5 + 3 fits 12 slots, 4 + 5 + 4 does not
    from unsloth_amd.models import decode as MD
    m = _model(1, 12)
    small, built = m._uamd_decode_engine, []
    monkeypatch.setattr(MD, "DecodeEngine", lambda model, **kw: built.append(kw) or StubEngine(kw["batch"], kw["max_seq_len"]))
    unsloth_fast_generate(m, ids, max_new_tokens=5, prompt_lookup_num_tokens=3)
    assert len(small.calls) == 1 and not built
    unsloth_fast_generate(m, ids, max_new_tokens=5, prompt_lookup_num_tokens=4)
    assert len(small.calls) == 1 and built == [dict(max_seq_len=13, batch=1)]
    assert m._uamd_decode_engine.calls[-1]["prompt_lookup_num_tokens"] == 4


def test_prompt_lookup_outside_one_greedy_sequence_stays_with_hf():
    from unsloth_amd.models.decode import route_generate, unsloth_fast_generate
    m = _model(2, 64)
    one, two = torch.zeros(1, 4, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long)
    assert route_generate(m, one, 5, dict(prompt_lookup_num_tokens=4, do_sample=True))[0] == "old"
    assert route_generate(m, two, 5, dict(prompt_lookup_num_tokens=4))[0] == "old"
    assert route_generate(m, one, 5, dict(prompt_lookup_num_tokens=4, do_sample=True, num_return_sequences=2))[0] == "old"
    assert unsloth_fast_generate(m, two, max_new_tokens=5, prompt_lookup_num_tokens=4) == "hf"
    assert len(m._old_generate.calls) == 1 and m._old_generate.calls[-1][1]["prompt_lookup_num_tokens"] == 4
    assert not m._uamd_decode_engine.calls


def test_symbols_are_declared_and_bound():
    from unsloth_amd import _lib
    header = open(os.path.join(ROOT, "include", "unsloth_amd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_engine_generate_takes_the_keywords():
    import inspect
    from unsloth_amd.models.decode import DecodeEngine
    p = inspect.signature(DecodeEngine.generate).parameters
    assert p["prompt_lookup_num_tokens"].default is None and p["max_matching_ngram_size"].default == 2
