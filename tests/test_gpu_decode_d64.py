"""-m gpu: the decode path at head_dim 64 (TinyLlama-1.1B, Qwen2.5-0.5B, Llama-3.2-1B). A key is 8 lanes x 16 B there, a
wave-load covers 8 keys and a block-load 32 (csrc/decode.hip DecGeo<64>), so the lengths, window starts and split sizes below
sit on and around multiples of 32 where tests/test_gpu_decode.py has them around multiples of 16. The error bounds are that
file's for the same comparisons: they come from the rounding of the 16-bit output and of the chunk-wise fp32 accumulation,
neither of which depends on the head dim."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64


def g(seed):
    return torch.Generator().manual_seed(seed)


def _rope_tables(S, dtype):
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(S).float()[:, None] * inv[None, :]
    cos = torch.cat([ang.cos(), ang.cos()], dim=1).to(dtype).to(DEV)
    sin = torch.cat([ang.sin(), ang.sin()], dim=1).to(dtype).to(DEV)
    return cos, sin


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,Hq,Hk", [(1, 8, 2), (3, 4, 4)])
def test_rope_kv_append_d64_matches_training_rope(dtype, B, Hq, Hk):
    """The q|k|v row and the cache rows at kv_len are bit-equal to fast_rope_embedding at positions kv_len; nothing else in either
    cache is written. (rope_append_kernel takes D at run time: the guard for the kernel the other tests lean on.)"""
    from unsloth_amd.kernels import decode as Dk
    from unsloth_amd.kernels.rope_embedding import fast_rope_embedding
    S = 256
    qkv = torch.randn(B, (Hq + 2 * Hk) * D, generator=g(7)).to(dtype).to(DEV)
    cos, sin = _rope_tables(S, dtype)
    kv_len = torch.tensor([5, 17, 200][:B], dtype=torch.int32, device=DEV)
    kc = torch.zeros(B, Hk, S, D, dtype=dtype, device=DEV)
    vc = torch.zeros_like(kc)
    ref = qkv.clone()
    Qr = ref[:, :Hq * D].view(B, 1, Hq, D).transpose(1, 2)
    Kr = ref[:, Hq * D:(Hq + Hk) * D].view(B, 1, Hk, D).transpose(1, 2)
    fast_rope_embedding(Qr, Kr, cos, sin, kv_len.clone())                  # in place on `ref`, positions = kv_len
    Dk.rope_kv_append(qkv, cos, sin, kv_len, kc, vc, Hq, Hk, D)
    assert torch.equal(qkv, ref)
    for b in range(B):
        L = int(kv_len[b])
        assert torch.equal(kc[b, :, L], qkv[b, Hq * D:(Hq + Hk) * D].view(Hk, D))
        assert torch.equal(vc[b, :, L], qkv[b, (Hq + Hk) * D:].view(Hk, D))
        for c in (kc, vc):
            assert float(c[b, :, :L].float().abs().sum()) == 0 and float(c[b, :, L + 1:].float().abs().sum()) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Hq,Hk", [(4, 4), (8, 2), (8, 1), (7, 1), (32, 4)])
@pytest.mark.parametrize("lens,window", [((1,), 0), ((31, 32, 33), 0), ((16, 129), 0), ((1000, 37, 512), 0), ((700,), 256),
                                         ((100,), 96)])
def test_attn_decode_d64_matches_fp64_softmax(dtype, Hq, Hk, lens, window):
    """uamd_attn_decode at D = 64 against an fp64 softmax on the CPU over the same rounded inputs. 31 / 32 / 33 straddle one
    32-key block-load; 700 - 256 = 444 and 100 - 96 = 4 are window starts that are no multiples of 32; (32, 4) is TinyLlama's
    own layout (G = 8)."""
    from unsloth_amd.kernels import decode as Dk
    S, B = 1024, len(lens)
    G = Hq // Hk
    q = torch.randn(B, Hq * D, generator=g(8)).to(dtype)
    kc = torch.randn(B, Hk, S, D, generator=g(9)).to(dtype)
    vc = torch.randn(B, Hk, S, D, generator=g(10)).to(dtype)
    kv_len = torch.tensor([l - 1 for l in lens], dtype=torch.int32)        # len_add = 1: the new token is already appended
    part = torch.empty(B, Hq, S // 128, D + 2, dtype=torch.float32, device=DEV)
    out = torch.full((B, Hq * D), float("nan"), dtype=dtype, device=DEV)
    Dk.attn_decode(q.to(DEV), kc.to(DEV), vc.to(DEV), kv_len.to(DEV), out, part, 128, 1.0 / math.sqrt(D), len_add=1,
                   window=window)
    got = out.double().cpu().view(B, Hq, D)
    worst = 0.0
    for b, L in enumerate(lens):
        first = L - window if (window and L > window) else 0
        k = kc[b, :, first:L].double().repeat_interleave(G, dim=0)         # [Hq, n, D]
        v = vc[b, :, first:L].double().repeat_interleave(G, dim=0)
        s = torch.einsum("hnd,hd->hn", k, q[b].double().view(Hq, D)) / math.sqrt(D)
        want = torch.einsum("hn,hnd->hd", torch.softmax(s, dim=1), v)
        worst = max(worst, (got[b] - want).abs().max().item())
    print(f"attn_decode D=64 {dtype} Hq={Hq} Hk={Hk} lens={lens} window={window}: max abs err {worst:.3e}")
    assert worst < (1.2e-2 if dtype == torch.bfloat16 else 2e-3)           # NaN (an unwritten output) fails this too


def _fused_against_three_launches(dtype, Hq, Hk, lens, window, S, split_keys, steps, cos, sin):
    """Both paths over `steps` consecutive tokens; asserts what tests/test_gpu_decode.py asserts for D = 128."""
    from unsloth_amd.kernels import decode as Dk
    B = len(lens)
    kc1 = torch.randn(B, Hk, S, D, generator=g(9)).to(dtype).to(DEV)
    vc1 = torch.randn(B, Hk, S, D, generator=g(10)).to(dtype).to(DEV)
    kc2, vc2 = kc1.clone(), vc1.clone()
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    part1 = torch.empty(B, Hq, S // split_keys, D + 2, dtype=torch.float32, device=DEV)
    part2, cnt = Dk.fused_attn_workspace(B, Hq, Hk, S, D, split_keys, DEV)
    scale = 1.0 / math.sqrt(D)
    for step in range(steps):
        if max(lens) + step >= S:                 # the cache is full (lens 511 of 512: one token into its last slot, then stop)
            break
        raw = torch.randn(B, (Hq + 2 * Hk) * D, generator=g(20 + step)).to(dtype).to(DEV)
        q1 = raw.clone()
        out1 = torch.empty(B, Hq * D, dtype=dtype, device=DEV)
        Dk.rope_kv_append(q1, cos, sin, kv_len, kc1, vc1, Hq, Hk, D)
        Dk.attn_decode(q1[:, :Hq * D], kc1, vc1, kv_len, out1, part1, split_keys, scale, len_add=1, window=window)
        keep = raw.clone()
        out2 = torch.full((B, Hq * D), float("nan"), dtype=dtype, device=DEV)
        Dk.attn_decode_fused(raw, cos, sin, kv_len, kc2, vc2, out2, part2, cnt, split_keys, scale, Hq, window=window)
        assert torch.equal(raw, keep)                                      # the raw row is left untouched
        err = (out2.float() - out1.float()).abs().max().item()
        mag = max(out1.float().abs().max().item(), 1e-3)
        print(f"fused D=64 {dtype} Hq={Hq} Hk={Hk} lens={lens} window={window} split={split_keys} step {step}: "
              f"err {err:.3e} of max {mag:.3e}")
        assert err <= (1.6e-2 if dtype == torch.bfloat16 else 2e-3) * mag, (step, err)
        assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1)
        assert int(cnt.abs().sum()) == 0                      # arrival counters (large launches) back at zero
        kv_len += 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Hq,Hk", [(4, 4), (8, 2), (32, 4), (7, 1), (32, 8)])
@pytest.mark.parametrize("lens,window,S", [((0,), 0, 512), ((1, 127, 128), 0, 512), ((31, 32), 0, 512), ((255, 300, 511), 0, 512),
                                           ((129, 400), 96, 512), ((1500, 100, 2046), 0, 2048)])
def test_attn_decode_fused_d64_is_the_three_launches(dtype, Hq, Hk, lens, window, S):
    """uamd_attn_decode_fused at D = 64 against uamd_rope_kv_append -> uamd_attn_decode over three consecutive tokens: raw row
    untouched, caches bit-equal, counters back at zero, output within the rounding of the output dtype. lens = tokens already in
    the cache: 31 / 32 put the new key last in a block-load / first in the next, 127 / 128 the same for a split. The S = 2048 case
    with 8 KV heads is 16 x 8 x 3 = 384 workgroups, more than one per CU: the arrival-counter combine; the rest combine through
    {value, tag} granules."""
    cos, sin = _rope_tables(S, dtype)
    _fused_against_three_launches(dtype, Hq, Hk, lens, window, S, 128, 3, cos, sin)


@pytest.mark.parametrize("split_keys,lens", [(256, (700, 255, 256)), (512, (1000,)), (64, (130, 64)), (32, (40,))])
def test_attn_decode_fused_d64_with_other_split_sizes(split_keys, lens):
    """Splits of several 128-key trips per workgroup, and the 64- and 32-key ones where a trip is half / three quarters empty
    (32 = one block-load at D = 64, the smallest split the kernels take)."""
    dtype, S = torch.bfloat16, 1024
    cos = torch.randn(S, D, generator=g(1)).clamp(-1, 1).to(dtype).to(DEV)
    sin = torch.randn(S, D, generator=g(2)).clamp(-1, 1).to(dtype).to(DEV)
    _fused_against_three_launches(dtype, 8, 2, lens, 0, S, split_keys, 1, cos, sin)


def test_split_keys_below_a_block_load_is_an_argument_error_at_d64():
    """split_keys = 16 is a whole block-load at D = 128 and half of one at D = 64: both entry points refuse it before launching
    (outputs and caches keep what they held)."""
    from unsloth_amd.kernels import decode as Dk
    dtype, S, Hq, Hk, B = torch.bfloat16, 1024, 8, 2, 1
    assert Dk.block_keys(64) == 32 and Dk.block_keys(128) == 16
    cos, sin = _rope_tables(S, dtype)
    kc = torch.randn(B, Hk, S, D, generator=g(9)).to(dtype).to(DEV)
    vc = torch.randn(B, Hk, S, D, generator=g(10)).to(dtype).to(DEV)
    kc0, vc0 = kc.clone(), vc.clone()
    kv_len = torch.tensor([40], dtype=torch.int32, device=DEV)
    raw = torch.randn(B, (Hq + 2 * Hk) * D, generator=g(3)).to(dtype).to(DEV)
    part1 = torch.empty(B, Hq, S // 16, D + 2, dtype=torch.float32, device=DEV)
    part2, cnt = Dk.fused_attn_workspace(B, Hq, Hk, S, D, 16, DEV)
    out = torch.full((B, Hq * D), float("nan"), dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError, match="uamd_attn_decode_fused"):
        Dk.attn_decode_fused(raw, cos, sin, kv_len, kc, vc, out, part2, cnt, 16, 1.0 / math.sqrt(D), Hq)
    with pytest.raises(RuntimeError, match="uamd_attn_decode"):
        Dk.attn_decode(raw[:, :Hq * D], kc, vc, kv_len, out, part1, 16, 1.0 / math.sqrt(D), len_add=1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and torch.equal(kc, kc0) and torch.equal(vc, vc0)
    assert int(part2.ws.abs().sum()) == 0 and int(cnt.abs().sum()) == 0


def _config(Hk, head_dim=64):
    from transformers import LlamaConfig
    return LlamaConfig(hidden_size=512, intermediate_size=1408, num_hidden_layers=2, num_attention_heads=8,
                       num_key_value_heads=Hk, head_dim=head_dim, vocab_size=1000, rms_norm_eps=1e-5, max_position_embeddings=512,
                       rope_parameters={"rope_type": "default", "rope_theta": 5e5}, tie_word_embeddings=False)


def _build_tiny64(Hk, load_in_4bit, r=8):
    from unsloth_amd import FastLanguageModel
    model, _ = FastLanguageModel.from_pretrained(config=_config(Hk), max_seq_length=256, load_in_4bit=load_in_4bit, device=DEV,
                                                 random_state=3407, use_gradient_checkpointing=False)
    model = FastLanguageModel.get_peft_model(model, r=r, lora_alpha=2 * r, use_gradient_checkpointing=False, random_state=3407)
    gg = torch.Generator().manual_seed(11)
    for n, p in model.named_parameters():
        if "lora_B" in n:
            p.data.copy_((torch.randn(p.shape, generator=gg) * 0.05).to(DEV))
    model.eval()
    return model


@functools.lru_cache(maxsize=None)
def _tiny64(Hk, load_in_4bit):
    """One model per (KV heads, NF4), shared by the engine tests and never modified by them."""
    return _build_tiny64(Hk, load_in_4bit)


@pytest.mark.parametrize("load_in_4bit", [True, False])
@pytest.mark.parametrize("Hk", [2, 1])
def test_engine_d64_logits_match_training_path_forward(Hk, load_in_4bit, monkeypatch):
    """Prefill of 21 tokens + 6 steps of the batch-1 fused step at head_dim 64: every step's logits are within 4e-2 x max|logits|
    of the training-path forward's last position over the same prefix, the graph-replayed and the eager engine agree bit for
    bit, and greedy generate is the argmax chain."""
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = _tiny64(Hk, load_in_4bit)
    ids = torch.randint(0, 1000, (1, 21), generator=g(12)).to(DEV)
    eng = DecodeEngine(model, max_seq_len=256, batch=1, use_graph=True)
    eng_e = DecodeEngine(model, max_seq_len=256, batch=1, use_graph=False)
    assert eng.D == 64 and eng.fsplit % 32 == 0
    lg, lg_e = eng.prefill(ids), eng_e.prefill(ids)
    assert torch.equal(lg, lg_e)
    seq = ids
    for step in range(6):
        with torch.no_grad():
            full = model(input_ids=seq).logits[:, -1].float()
        scale = full.abs().max().item()
        err = (lg - full).abs().max().item()
        print(f"engine D=64 Hk={Hk} nf4={load_in_4bit} step {step}: err {err:.3e} of max {scale:.3e}")
        assert err < 4e-2 * scale, (step, err, scale)
        nxt = torch.argmax(lg, dim=-1)
        seq = torch.cat([seq, nxt.view(1, 1)], dim=1)
        lg, lg_e = eng.step(nxt).clone(), eng_e.step(nxt).clone()
        assert torch.equal(lg, lg_e), f"graph replay differs from the eager step at step {step}"
    assert int(eng.kv_len[0]) == 27
    out = DecodeEngine(model, max_seq_len=256).generate(ids, max_new_tokens=6)
    assert torch.equal(out[:, :27], seq[:, :27])


@pytest.mark.parametrize("load_in_4bit", [True, False])
@pytest.mark.parametrize("Hk", [2, 1])
def test_engine_d64_batch_2_matches_training_path_forward(Hk, load_in_4bit, monkeypatch):
    """The batch > 1 step (rope_kv_append -> attn_decode -> combine, small-M GEMMs) on two different prompts of equal length."""
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = _tiny64(Hk, load_in_4bit)
    ids = torch.randint(0, 1000, (2, 21), generator=g(14)).to(DEV)
    assert not torch.equal(ids[0], ids[1])
    eng = DecodeEngine(model, max_seq_len=256, batch=2)
    lg = eng.prefill(ids)
    seq = ids
    for step in range(6):
        with torch.no_grad():
            full = model(input_ids=seq).logits[:, -1].float()
        scale = full.abs().max().item()
        err = (lg - full).abs().max().item()
        print(f"engine D=64 batch 2 Hk={Hk} nf4={load_in_4bit} step {step}: err {err:.3e} of max {scale:.3e}")
        assert err < 4e-2 * scale, (step, err, scale)
        nxt = torch.argmax(lg, dim=-1)
        seq = torch.cat([seq, nxt.view(2, 1)], dim=1)
        lg = eng.step(nxt).clone()
    assert eng.kv_len.tolist() == [27, 27]


def test_for_inference_generate_at_head_dim_64_is_the_decode_engine():
    """FastLanguageModel.for_inference on a head_dim-64 model: model.generate is the decode engine's greedy chain and never
    reaches HF's generate. Any head dim the kernels are not instantiated for is refused by name."""
    from unsloth_amd import FastLanguageModel
    from unsloth_amd.models.decode import DecodeEngine
    model = _build_tiny64(2, True)                                         # its own model: for_inference rebinds generate
    FastLanguageModel.for_inference(model)
    assert not model.training and hasattr(model, "_old_generate")

    def no_hf_generate(*a, **k):
        raise AssertionError("generate went to HF's generate")
    model._old_generate = no_hf_generate
    ids = torch.randint(0, 1000, (1, 9), generator=g(13)).to(DEV)
    out = model.generate(input_ids=ids, max_new_tokens=5)
    want = DecodeEngine(model, max_seq_len=128).generate(ids, max_new_tokens=5)
    assert out.shape == (1, 14) and torch.equal(out, want)
    assert model._uamd_decode_engine.D == 64


def test_decode_engine_names_the_supported_head_dims():
    from unsloth_amd import FastLanguageModel
    from unsloth_amd.models.decode import DecodeEngine
    model, _ = FastLanguageModel.from_pretrained(config=_config(2, head_dim=96), max_seq_length=128, load_in_4bit=False,
                                                 device=DEV, random_state=3407, use_gradient_checkpointing=False)
    with pytest.raises(NotImplementedError) as e:
        DecodeEngine(model, max_seq_len=128)
    assert "64" in str(e.value) and "128" in str(e.value)
