"""-m gpu: a tiny Qwen3 (2 layers, hidden 256, 4 / 2 heads, head_dim 128 != hidden / heads, non-unit q_norm / k_norm weights) on
the hand-kernel path. Training: `distance` = the worst relative error over the loss and every LoRA gradient against transformers'
Qwen3ForCausalLM in fp32; ours may be 1.5 x that of stock HF run in bf16 on the same inputs, measured here (the margin: two bf16
sums in different orders). Decode: tests/test_gpu_decode_batched.py's rule, logits within 4e-2 x max |logits| of the training path."""
import functools

import pytest
import torch
from transformers import Qwen3Config

from tests._decode_batched import DEV, full_logits, g, left_padded, tiny

pytestmark = pytest.mark.gpu
T = 33


@functools.lru_cache(maxsize=None)
def qwen3():
    from unsloth_amd import FastLanguageModel
    cfg = Qwen3Config(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      head_dim=128, vocab_size=1000, rms_norm_eps=1e-6, max_position_embeddings=256, tie_word_embeddings=False,
                      rope_parameters={"rope_type": "default", "rope_theta": 1e6})
    model, _ = FastLanguageModel.from_pretrained(config=cfg, max_seq_length=128, load_in_4bit=True, device=DEV,
                                                 use_gradient_checkpointing=False)
    model = FastLanguageModel.get_peft_model(model, r=8, lora_alpha=16, use_gradient_checkpointing=False)
    gg = g(3)
    for n, p in model.named_parameters():
        if "lora_B" in n:
            p.data.copy_((torch.randn(p.shape, generator=gg) * 0.05).to(DEV))
        if "q_norm" in n or "k_norm" in n:
            p.data.copy_((torch.rand(p.shape, generator=gg) * 1.5 + 0.25).to(DEV))
    return model


def _hf(model, ids, labels, dtype):
    """(loss, LoRA gradients) of stock HF: oracle/ref_model.py places a Llama's weights; q_norm / k_norm are copied here and its loss redone."""
    from oracle.ref_model import NAMES, hf_reference_loss_and_lora_grads
    _, _, ref = hf_reference_loss_and_lora_grads(model, ids, labels, device=DEV, dtype=dtype, return_model=True)
    where = []
    for li, (layer, rl) in enumerate(zip(model.get_base_model().model.layers, ref.model.layers)):
        for n in ("q_norm", "k_norm"):
            getattr(rl.self_attn, n).weight.data.copy_(getattr(layer.self_attn, n).weight.data)
        where += [(f"layers.{li}.{p}.{n}", getattr(getattr(rl, p), n).weight, getattr(getattr(layer, p), n)) for p, n in NAMES]
    logits = ref(input_ids=ids.to(DEV), use_cache=False).logits.float()
    loss = torch.nn.functional.cross_entropy(logits[:, :-1].flatten(0, 1), labels[:, 1:].flatten().to(DEV), ignore_index=-100)
    grads = {}
    for (key, _, proj), dW in zip(where, torch.autograd.grad(loss, [w for _, w, _ in where])):
        (A, B), s = [m[proj.active_adapters[0]].weight.detach().float() for m in (proj.lora_A, proj.lora_B)], proj.scaling[proj.active_adapters[0]]
        grads[key + ".lora_A"], grads[key + ".lora_B"] = s * B.t() @ dW.float(), s * dW.float() @ A.t()
    return float(loss.detach()), grads


def _distance(got, oracle):
    (loss, grads), (ref_loss, ref_grads) = got, oracle
    return max([abs(loss - ref_loss) / abs(ref_loss)] + [float((grads[k].float() - w).norm() / w.norm()) for k, w in ref_grads.items()])


@functools.lru_cache(maxsize=None)
def _case():
    ids = torch.randint(0, 1000, (2, T), generator=g(1))
    labels = ids.masked_fill(torch.arange(T) < 5, -100)
    oracle = _hf(qwen3(), ids, labels, torch.float32)
    return ids, labels, oracle, _distance(_hf(qwen3(), ids, labels, torch.bfloat16), oracle)


@pytest.mark.parametrize("gc", [False, "unsloth", "unsloth:min"])
def test_training_matches_hf_qwen3(gc):
    from unsloth_amd import FastLanguageModel
    model, (ids, labels, oracle, yardstick) = qwen3(), _case()
    FastLanguageModel.for_training(model, gc)
    model.zero_grad(set_to_none=True)
    out = model(input_ids=ids.to(DEV), labels=labels.to(DEV))
    out.loss.backward()
    grads = {"layers." + n.split(".layers.", 1)[1].replace(".default.weight", ""): p.grad
             for n, p in model.named_parameters() if p.requires_grad}
    assert set(grads) == set(oracle[1]) and len(grads) == 28
    ours = _distance((float(out.loss.detach()), grads), oracle)
    print(f"gc={gc}: distance to the fp32 oracle {ours:.3e}, stock HF in bf16 {yardstick:.3e}")
    assert ours <= 1.5 * yardstick


def test_decode_matches_training_path(monkeypatch):
    from unsloth_amd import FastLanguageModel
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = FastLanguageModel.for_inference(qwen3())
    for lengths in ((T,), (4, T, 17)):
        ids, mask, rows = left_padded(lengths, T, seed=50)
        eng = DecodeEngine(model, max_seq_len=128, batch=len(lengths))
        assert eng.qk_norm and eng.use_graph
        lg = eng.prefill(ids.to(DEV), mask.to(DEV)).clone()
        seqs = [r.view(1, -1).to(DEV) for r in rows]
        for step in range(7):                                        # prefill + six steps
            for b, seq in enumerate(seqs):
                full = full_logits(model, seq)[0]
                err, scale = (lg[b] - full).abs().max().item(), full.abs().max().item()
                assert err < 4e-2 * scale, (lengths, step, b, err, scale)
            nxt = torch.argmax(lg, dim=-1)
            seqs = [torch.cat([s, nxt[b].view(1, 1)], dim=1) for b, s in enumerate(seqs)]
            lg = eng.step(nxt).clone()
    ids, mask = ids.to(DEV), mask.to(DEV)
    out = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=4)
    assert out.shape == (3, T + 4) and torch.equal(out[:, :T], ids)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=4, do_sample=True, temperature=1.5, top_k=50)
    a, b = (model.generate(generator=torch.Generator(DEV).manual_seed(5), **kw) for _ in range(2))
    assert a.shape == (3, T + 4) and torch.equal(a, b) and int(a.max()) < 1000


def test_refused_combinations_raise_before_any_launch(monkeypatch):
    from unsloth_amd import FastLanguageModel, _lib
    from unsloth_amd.models import decode
    model = FastLanguageModel.for_inference(qwen3())
    ids = torch.randint(0, 1000, (1, 9), generator=g(2)).to(DEV)
    eng = decode.DecodeEngine(model, max_seq_len=64, batch=1)
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    new = lambda **kw: decode.DecodeEngine(model, max_seq_len=64, **kw)
    gen = lambda **kw: model.generate(input_ids=ids, max_new_tokens=2, **kw)
    for refused in (lambda: new(batch=1, kv_cache_dtype="fp8"), lambda: new(batch=2, share_prompt=2), eng._step_body_fused,
                    lambda: eng.extend(ids), lambda: eng.prefill(ids, chunk=4), lambda: eng.generate(ids, append=True),
                    lambda: eng.generate(ids, prompt_lookup_num_tokens=3), lambda: gen(prompt_lookup_num_tokens=3),
                    lambda: gen(kv_cache_dtype="fp8"), lambda: gen(prefill_chunk_size=4),
                    lambda: gen(do_sample=True, num_return_sequences=2, share_prompt_cache=True),
                    lambda: FastLanguageModel.from_pretrained(config=Qwen3Config(), full_finetuning=True, device=DEV)):
        with pytest.raises(NotImplementedError):
            refused()
    assert names == []
    # a Llama model still decodes one sequence with the single-launch step
    monkeypatch.setattr(decode, "FUSED_STEP", True)                  # (the module's default, whatever an earlier test left)
    llama = decode.DecodeEngine(tiny(True), max_seq_len=64, batch=1)
    assert llama.B == 1 and llama.kv_cache_dtype is None and llama.use_graph
    llama.step(torch.argmax(llama.prefill(ids), dim=-1))
    assert "uamd_attn_decode_fused" in names and "uamd_rope_kv_append" not in names
