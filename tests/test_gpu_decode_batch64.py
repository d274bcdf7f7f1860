"""-m gpu: batched decode of 17 .. 64 sequences (models/decode.py on uamd_gemv_rows64) -- the token step against the
training-path forward, eager against hipGraph replay, left-padded prompts, num_return_sequences, the shared prompt cache and
the FP8 cache at these sizes; 65 rows stay on the previous route. The tiny model and the helpers of tests/_decode_batched.py."""
import pytest
import torch

from tests._decode_batched import DEV, Recorder, full_logits, g, left_padded, tiny

pytestmark = pytest.mark.gpu


def _record(monkeypatch):
    from unsloth_amd import _lib
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("load_in_4bit", [True, False])
def test_batch_24_matches_training_path_and_graph_equals_eager(load_in_4bit, monkeypatch):
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = tiny(load_in_4bit)
    B = 24
    ids = torch.randint(0, 1000, (B, 21), generator=g(12)).to(DEV)
    eng = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=True)
    eng_e = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=False)
    assert eng.rows and eng.use_graph and not eng_e.use_graph
    lg, lg_e = eng.prefill(ids), eng_e.prefill(ids)
    assert torch.equal(lg, lg_e)
    names = _record(monkeypatch)
    seq = ids
    for step in range(6):
        full = full_logits(model, seq)
        for b in range(B):
            scale = full[b].abs().max().item()
            err = (lg[b] - full[b]).abs().max().item()
            assert err < 4e-2 * scale, (step, b, err, scale)
        nxt = torch.argmax(lg, dim=-1)
        seq = torch.cat([seq, nxt.view(B, 1)], dim=1)
        names.clear()
        lg_e = eng_e.step(nxt).clone()
        assert "uamd_gemv_rows64" in names and not any(n.startswith("uamd_gemm") for n in names), names
        lg = eng.step(nxt).clone()
        assert torch.equal(lg, lg_e), f"graph replay differs from the eager step at step {step}"
    assert eng._graph is not None and eng.kv_len.tolist() == [27] * B
    # the sampled step is a capture of its own and agrees with the eager one too
    outs = [e.generate(ids, max_new_tokens=5, do_sample=True, temperature=1.3, top_k=50,
                       generator=torch.Generator(DEV).manual_seed(5)) for e in (eng, eng_e)]
    assert eng._graph_s is not None and torch.equal(outs[0], outs[1])


def test_batch_64(monkeypatch):
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = tiny(True)
    B = 64
    ids = torch.randint(0, 1000, (B, 8), generator=g(13)).to(DEV)
    eng = DecodeEngine(model, max_seq_len=128, batch=B, use_graph=True)
    eng_e = DecodeEngine(model, max_seq_len=128, batch=B, use_graph=False)
    assert eng.rows and eng.use_graph
    lg, lg_e = eng.prefill(ids), eng_e.prefill(ids)
    assert torch.equal(lg, lg_e)
    seq = ids
    watch = [0, 31, 63]
    for step in range(4):                                            # prefill + three steps
        full = full_logits(model, seq[watch])
        for i, b in enumerate(watch):
            scale = full[i].abs().max().item()
            err = (lg[b] - full[i]).abs().max().item()
            assert err < 4e-2 * scale, (step, b, err, scale)
        if step == 3:
            break
        nxt = torch.argmax(lg, dim=-1)
        seq = torch.cat([seq, nxt.view(B, 1)], dim=1)
        lg_e = eng_e.step(nxt).clone()
        lg = eng.step(nxt).clone()
        assert torch.equal(lg, lg_e), f"graph replay differs from the eager step at step {step}"
    assert eng._graph is not None and eng.kv_len.tolist() == [11] * B


def test_left_padded_batch_of_20():
    """Lengths cycling through (1, 5, 13, 21): kv_len, and rows 1 and 19 bit-equal between two engines whose other rows hold
    other prompts, over prefill + 4 steps."""
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    B, T = 20, 21
    lengths = [(1, 5, 13, 21)[b % 4] for b in range(B)]
    ids, mask, _ = left_padded(lengths, T, seed=40)
    ids2, _, _ = left_padded(lengths, T, seed=190)
    ids2[1], ids2[19] = ids[1], ids[19]
    eng = DecodeEngine(model, max_seq_len=256, batch=B)
    eng2 = DecodeEngine(model, max_seq_len=256, batch=B)
    assert eng.rows and eng.use_graph
    lg = eng.prefill(ids.to(DEV), mask.to(DEV)).clone()
    lg2 = eng2.prefill(ids2.to(DEV), mask.to(DEV)).clone()
    assert eng.kv_len.tolist() == lengths
    for step in range(5):
        assert torch.equal(lg[1], lg2[1]) and torch.equal(lg[19], lg2[19]), f"a row depends on its companions at step {step}"
        assert not torch.equal(lg[0], lg2[0])
        if step == 4:
            break
        nxt, nxt2 = torch.argmax(lg, dim=-1), torch.argmax(lg2, dim=-1)
        lg, lg2 = eng.step(nxt).clone(), eng2.step(nxt2).clone()
    assert eng.kv_len.tolist() == [L + 4 for L in lengths]


def test_generate_3_prompts_times_8_return_sequences():
    from unsloth_amd import FastLanguageModel
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True, fresh=True)
    FastLanguageModel.for_inference(model)
    rec = Recorder(ret="hf")
    model._old_generate = rec
    ids = torch.randint(0, 1000, (3, 9), generator=g(23)).to(DEV)
    gen = lambda: torch.Generator(DEV).manual_seed(7)
    kw = dict(max_new_tokens=5, do_sample=True, temperature=2.0, top_k=0)
    out = model.generate(input_ids=ids, num_return_sequences=8, generator=gen(), **kw)
    assert out.shape == (24, 14) and not rec.calls
    eng = model._uamd_decode_engine
    assert eng.B == 24 and eng.rows and eng.use_graph
    assert torch.equal(out[:, :9], ids.repeat_interleave(8, 0))
    want = DecodeEngine(model, max_seq_len=128, batch=24).generate(ids.repeat_interleave(8, 0), generator=gen(), **kw)
    assert torch.equal(out, want)
    for b in range(3):                                               # replicas draw differently
        assert len({tuple(r.tolist()) for r in out[8 * b:8 * b + 8, 9:]}) > 1


def test_shared_prompt_cache_2_prompts_times_12(monkeypatch):
    """tests/test_gpu_decode_shared.py's engine case at P = 2, n = 12 (24 rows): the shared engine against the replicated one
    (bits, where the code is the same) and against the training-path forward."""
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = tiny(True)
    P, n = 2, 12
    B = P * n
    ids = torch.randint(1, 1000, (P, 9), generator=g(31)).to(DEV)
    rows = [ids[p] for p in range(P)]
    lens = [9] * P
    rep = DecodeEngine(model, max_seq_len=256, batch=B)
    sh = DecodeEngine(model, max_seq_len=256, batch=B, share_prompt=n, max_new_tokens=128)
    sh_e = DecodeEngine(model, max_seq_len=256, batch=B, share_prompt=n, max_new_tokens=128, use_graph=False)
    assert sh.use_graph and sh.rows and sh.share_prompt == n and (sh.S, sh.S_n) == (256, 128)
    Hk, D = sh.Hk, sh.D
    assert all(t.shape == (P, Hk, 256, D) for t in sh.pk + sh.pv)
    assert all(t.shape == (B, Hk, 128, D) for t in sh.k_cache + sh.v_cache)
    lg_r = rep.prefill(ids, None, repeat=n).clone()
    lg = sh.prefill(ids, None, repeat=n).clone()
    lg_e = sh_e.prefill(ids, None, repeat=n).clone()
    assert torch.equal(lg, lg_r) and torch.equal(lg_e, lg_r)
    assert sh.prompt_len.tolist() == lens and sh.kv_len.tolist() == [9] * B and sh.new_len.tolist() == [0] * B
    for p, L in enumerate(lens):
        assert torch.equal(sh.pk[0][p, :, :L], rep.k_cache[0][p * n, :, :L])
        assert torch.equal(sh.pv[0][p, :, :L], rep.v_cache[0][p * n, :, :L])
        assert float(sh.pk[0][p, :, L:].float().abs().sum()) == 0.0
    assert all(float(t.float().abs().sum()) == 0.0 for t in sh.k_cache + sh.v_cache)
    names = _record(monkeypatch)
    seqs = [rows[r // n].view(1, -1) for r in range(B)]
    shift = torch.arange(B, device=DEV)
    for step in range(7):                                            # prefill + six steps
        for p in range(P):
            full = full_logits(model, torch.cat(seqs[p * n:(p + 1) * n], dim=0))
            for i in range(n):
                scale = full[i].abs().max().item()
                err = (lg[p * n + i] - full[i]).abs().max().item()
                assert err < 4e-2 * scale, (step, p, i, err, scale)
        if step == 6:
            break
        nxt = (torch.argmax(lg, dim=-1) + shift) % 1000              # every row its own token: the rows of a group differ
        seqs = [torch.cat([s, nxt[r].view(1, 1)], dim=1) for r, s in enumerate(seqs)]
        names.clear()
        lg_e = sh_e.step(nxt).clone()
        assert "uamd_attn_decode_shared" in names and "uamd_attn_decode" not in names, names
        assert "uamd_gemv_rows64" in names and not any(nm.startswith("uamd_gemm") for nm in names), names
        lg = sh.step(nxt).clone()
        assert torch.equal(lg, lg_e), f"graph replay differs from the eager step at step {step}"
        if step == 0:                                                # layer 0's K / V do not depend on attention
            rep.step(nxt)
            for r in range(B):
                assert torch.equal(sh.k_cache[0][r, :, 0], rep.k_cache[0][r, :, 9])
                assert torch.equal(sh.v_cache[0][r, :, 0], rep.v_cache[0][r, :, 9])
    assert sh._graph is not None
    for e in (sh, sh_e):
        assert e.kv_len.tolist() == [15] * B and e.new_len.tolist() == [6] * B and e.prompt_len.tolist() == lens
    outs = [e.generate(ids, max_new_tokens=5, do_sample=True, temperature=1.3, top_k=50,
                       num_return_sequences=n, generator=torch.Generator(DEV).manual_seed(5)) for e in (sh, sh_e)]
    assert sh._graph_s is not None and torch.equal(outs[0], outs[1])


def test_fp8_cache_graph_replay_equals_the_eager_step_at_24(monkeypatch):
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    B = 24
    ids = torch.randint(1, 1000, (B, 13), generator=g(63 + B)).to(DEV)
    eg = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=True, kv_cache_dtype="fp8")
    ee = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=False, kv_cache_dtype="fp8")
    assert eg.rows and eg.use_graph and not ee.use_graph
    lg, le = eg.prefill(ids), ee.prefill(ids)
    assert torch.equal(lg, le)
    names = _record(monkeypatch)
    for step in range(4):
        nxt = torch.argmax(lg, dim=-1)
        names.clear()
        le = ee.step(nxt).clone()
        assert "uamd_rope_kv_append_fp8" in names and "uamd_attn_decode_fp8" in names and "uamd_gemv_rows64" in names, names
        assert not {"uamd_rope_kv_append", "uamd_attn_decode", "uamd_attn_decode_fused"} & set(names), names
        lg = eg.step(nxt).clone()
        assert torch.equal(lg, le), f"graph replay differs from the eager step at step {step}"
    assert eg._graph is not None and eg.kv_len.tolist() == [17] * B
    for li in range(len(eg.k_cache)):
        assert torch.equal(eg.k_cache[li], ee.k_cache[li]) and torch.equal(eg.v_scale[li], ee.v_scale[li])


def test_batch_65_stays_on_the_previous_route():
    from unsloth_amd.models.decode import DecodeEngine
    eng = DecodeEngine(tiny(True), max_seq_len=128, batch=65, use_graph=True)
    assert not eng.rows and not eng.use_graph
