"""-m gpu: DecodeEngine.extend, prefill(chunk=N) and generate(append=True) against the training-path forward. The bound on
logits is the one tests/test_gpu_decode_shared.py holds engines to, err < 4e-2 x max |logits| per row; generated tokens follow
tests/test_gpu_decode_lookup.py's rule for near-ties: the reference logit of every emitted token within 2 x that of the best."""
import pytest
import torch

from tests._decode_batched import DEV, full_logits, g, left_padded, tiny

pytestmark = pytest.mark.gpu
BOUND = 4e-2


def _check(model, logits, seqs, what):
    for b, seq in enumerate(seqs):
        ref = full_logits(model, seq.view(1, -1).to(DEV))[0]
        err, scale = (logits[b] - ref).abs().max().item(), ref.abs().max().item()
        assert err < BOUND * scale, (what, b, err, scale)


@pytest.mark.parametrize("lengths", [(9,), (9, 5, 7)], ids=["one-sequence", "three-left-padded"])
def test_extend_then_replayed_steps_match_the_training_path(lengths):
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    B = len(lengths)
    ids, mask, rows = left_padded(lengths, 9, seed=40)
    eng = DecodeEngine(model, max_seq_len=64, batch=B)
    _check(model, eng.prefill(ids, mask), rows, "prefill")
    more = torch.randint(1, 1000, (B, 20), generator=g(41))
    rows = [torch.cat([r, m]) for r, m in zip(rows, more)]
    _check(model, eng.extend(more), rows, "extend")
    assert eng.kv_len.tolist() == [L + 20 for L in lengths]
    for i in range(4):                                           # the captured step reads kv_len from the device
        tok = torch.randint(1, 1000, (B,), generator=g(50 + i))
        rows = [torch.cat([r, t.view(1)]) for r, t in zip(rows, tok)]
        _check(model, eng.step(tok.to(DEV)), rows, f"step {i}")
    assert eng._graph is not None and eng.kv_len.tolist() == [L + 24 for L in lengths]


def test_chunked_prefill_matches_the_one_shot_prefill():
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    ids, mask, rows = left_padded((13, 11), 13, seed=60)
    one, eng = DecodeEngine(model, max_seq_len=64, batch=2), DecodeEngine(model, max_seq_len=64, batch=2)
    one.prefill(ids, mask)
    logits = eng.prefill(ids, mask, chunk=4)
    assert eng.kv_len.tolist() == one.kv_len.tolist() == [13, 11]
    _check(model, logits, rows, "prefill(chunk=4)")
    with pytest.raises(ValueError, match="cover the longest padding"):
        eng.prefill(ids, mask, chunk=2)


def test_generate_append_continues_the_conversation():
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    eng = DecodeEngine(model, max_seq_len=64, batch=1)
    first = eng.generate(torch.randint(1, 1000, (1, 7), generator=g(70)), max_new_tokens=5)
    # the cache holds everything but the last emitted token: the next turn starts with it
    turn = torch.cat([first[:, -1:].cpu(), torch.randint(1, 1000, (1, 6), generator=g(71))], dim=1)
    out = eng.generate(turn, max_new_tokens=5, append=True)
    assert out.shape == (1, 7 + 5) and torch.equal(out[:, :7].cpu(), turn)
    conv = torch.cat([first[:, :-1], out], dim=1)
    for i in range(conv.shape[1] - 5, conv.shape[1]):
        ref = full_logits(model, conv[:, :i])[0]
        assert ref.max() - ref[conv[0, i]] <= 2 * BOUND * ref.abs().max(), i
    eng.generate(turn[:, :3], max_new_tokens=2, append=True, prompt_lookup_num_tokens=3)
    assert eng.lookup_stats["fallback"] == "append=True"


def test_out_of_scope_engines_and_chunks_past_capacity_are_refused():
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    ids = torch.randint(1, 1000, (2, 9), generator=g(80))
    for kw in (dict(kv_cache_dtype="fp8"), dict(share_prompt=2)):
        eng = DecodeEngine(model, max_seq_len=64, batch=2, **kw)
        for call in (lambda: eng.extend(ids), lambda: eng.prefill(ids, chunk=4), lambda: eng.generate(ids, append=True)):
            with pytest.raises(NotImplementedError):
                call()
    eng = DecodeEngine(model, max_seq_len=128, batch=2)
    eng.prefill(ids)
    with pytest.raises(ValueError, match="exceed"):
        eng.extend(torch.ones(2, 120, dtype=torch.long))
    assert eng.kv_len.tolist() == [9, 9]
