"""-m gpu: prompt-lookup decoding -- uamd_rope_kv_append_span, uamd_attn_decode_span, uamd_ngram_draft, uamd_accept_greedy
(csrc/decode.hip) and DecodeEngine.generate(prompt_lookup_num_tokens=K).

The span attention is judged row by row against an fp64 reference over each row's own key range (tests/_decode_edges.ref64_ranges)
with the softmax mass placed on the row's first and last key and on the keys just outside (tests/_lookup_ref.span_inputs); the
bound is BOUND_FACTOR x the error of the host restatement of the documented roundings (tests/_decode_shared.rounding_model: P
rounded once, the sum over the rounded P, one rounding at the store), as in tests/test_gpu_decode_shared.py. The measured ratios
go to decode_lookup_edge_report.json in the directory UAMD_REPORT_DIR names (default: test_reports/ in the repository root,
git-ignored); profiles/decode_lookup_edge_report.json is a committed copy of one MI355X run.

The engine is held to the training-path forward: every generated token's reference logit is within 2 b of its row's maximum, b =
4e-2 x max |logits| being the bound tests/test_gpu_decode.py::test_engine_logits_match_training_path_forward puts on the engine's
logits against that forward (the engine takes the arg-max of logits within b of the reference, so the token it picks cannot lie
more than 2 b below the reference's best). The step counters must equal the python rules replayed over the emitted text."""
import json
import math
import os

import pytest
import torch

from tests import _lookup_ref as ref
from tests._decode_batched import DEV, g, tiny
from tests._decode_edges import BOUND_FACTOR, DTYPES, ref64_ranges, row_err
from tests._decode_shared import rounding_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
LOGIT_BOUND = 4e-2              # b / max |logits|: tests/test_gpu_decode.py::test_engine_logits_match_training_path_forward


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_lookup_edge_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _rope_tables(S, D, dtype):
    inv = 1.0 / (5e5 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(S).float()[:, None] * inv[None, :]
    return ang.cos().to(dtype).to(DEV), ang.sin().to(dtype).to(DEV)


# ---- the span append ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("R", [1, 2, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_span_append_is_r_single_appends(D, R, dtype_name):
    from unsloth_amd.kernels import decode as Dk
    dtype = DTYPES[dtype_name]
    B, Hq, Hk, S = 2, 4, 2, 64
    lens = [5, 40]
    cos, sin = _rope_tables(S, D, dtype)
    qkv = torch.randn(B * R, (Hq + 2 * Hk) * D, generator=g(D + R)).to(dtype).to(DEV)
    stale = torch.randn(B, Hk, S, D, generator=g(1)).to(dtype).to(DEV)
    # R successive single appends, kv_len advanced by one in between
    qkv1, k1, v1 = qkv.clone(), stale.clone(), (stale * 2).clone()
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for j in range(R):
        rows = qkv1[j::R]                                      # token j of every sequence: a strided [B, ...] view
        Dk.rope_kv_append(rows, cos, sin, kv, k1, v1, Hq, Hk, D)
        kv += 1
    qkv2, k2, v2 = qkv.clone(), stale.clone(), (stale * 2).clone()
    kv0 = torch.tensor(lens, dtype=torch.int32, device=DEV)
    Dk.rope_kv_append_span(qkv2, cos, sin, kv0, k2, v2, R, Hq, Hk, D)
    assert kv0.tolist() == lens                                # not advanced
    assert torch.equal(qkv2, qkv1) and torch.equal(k2, k1) and torch.equal(v2, v1)
    assert not torch.equal(k2, stale)
    for b, L in enumerate(lens):                               # nothing outside the span's slots moved
        assert torch.equal(k2[b, :, :L], stale[b, :, :L]) and torch.equal(k2[b, :, L + R:], stale[b, :, L + R:])


# ---- the span attention ------------------------------------------------------------------------------------------------------
_BUILT = {}


def _case(name, D, dtype_name):
    """One case, computed once and shared (nothing in it is written to): inputs, fp64 reference, the rounding model's error."""
    key = (name, D, dtype_name)
    if key not in _BUILT:
        case = ref.SPAN_CASES[name]
        Hq, Hk, R, window, kv_len = case
        assert Hq % Hk == 0 and 1 <= R <= 16 and R * (Hq // Hk) <= 128 and kv_len + R <= ref.S_MAX
        dtype = DTYPES[dtype_name]
        q, kc, vc = ref.span_inputs(case, D, dtype, 4000 + D)
        ranges = ref.span_ranges(R, window, kv_len)
        scale = 1.0 / math.sqrt(D)
        kr, vr = kc.expand(R, Hk, ref.S_MAX, D), vc.expand(R, Hk, ref.S_MAX, D)
        want = ref64_ranges(q, kr, vr, ranges, scale, Hq, Hk)
        model = rounding_model(q, kr.double(), vr.double(), ranges, scale, Hq, Hk, dtype)
        _BUILT[key] = dict(D=D, Hq=Hq, Hk=Hk, R=R, B=R, window=window, kv_len=kv_len, dtype=dtype, q=q, kc=kc, vc=vc, scale=scale,
                           ranges=ranges, ref=want, model_err=row_err(model, want))
    return _BUILT[key]


def _span(c, q=None, kc=None, vc=None):
    """uamd_attn_decode_span on a cache that already holds the span's keys: out [R, Hq * D] on the host."""
    from unsloth_amd.kernels import decode as Dk
    R, Hq, D = c["R"], c["Hq"], c["D"]
    q = (c["q"] if q is None else q).to(DEV)
    kv = torch.tensor([c["kv_len"]], dtype=torch.int32, device=DEV)
    part = torch.full((R, Hq, ref.S_MAX // ref.SPLIT, D + 2), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((R, Hq * D), float("nan"), dtype=c["dtype"], device=DEV)
    Dk.attn_decode_span(q, (c["kc"] if kc is None else kc).to(DEV), (c["vc"] if vc is None else vc).to(DEV), kv, R, out, part,
                        ref.SPLIT, c["scale"], window=c["window"])
    return out.cpu()


SPAN_PARAMS = [(n, D, d) for n in ref.SPAN_CASES for D in (64, 128) for d in DTYPES]


@pytest.mark.parametrize("name,D,dtype_name", SPAN_PARAMS)
def test_span_edges_match_fp64(name, D, dtype_name):
    c = _case(name, D, dtype_name)
    got = _span(c)
    assert torch.isfinite(got.float()).all()
    err = row_err(got.view(c["R"], c["Hq"], D), c["ref"])
    model = c["model_err"]
    ratio = err / model if model > 0 else (0.0 if err == 0 else float("inf"))       # (one key: the model is exact)
    REPORT[f"{name}/d{D}/{dtype_name}"] = dict(kernel=err, model=model, ratio=ratio)
    print(f"{name}/d{D}/{dtype_name}: err {err:.3e} model_err {model:.3e} ratio {ratio:.2f}")
    assert err <= BOUND_FACTOR * model, (name, D, dtype_name, err, model, ratio)


def _thief(c):
    """A key every head of a KV head scores far above its edge keys (the sum of the queries that could read the slot) and a value
    no reference row uses: [Hk, D] each."""
    R, Hq, Hk, D = c["R"], c["Hq"], c["Hk"], c["D"]
    k = c["q"].float().view(R, Hk, Hq // Hk, D).sum((0, 2)).to(c["dtype"])
    v = (3.0 + torch.randn(Hk, D, generator=g(77))).to(c["dtype"])
    return k, v


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", ["len120_r16", "g1", "g7", "g8_r16", "win3_seam", "len0"])
def test_a_row_depends_on_nothing_behind_it(name, D, dtype_name):
    """Token j's rows with every later token's query, every key / value at or past t_j and every stale slot past the span
    overwritten -- once with values that would take the mass, once with NaN: bit-equal to the clean run."""
    c = _case(name, D, dtype_name)
    base = _span(c)
    R, kv_len = c["R"], c["kv_len"]
    tk, tv = _thief(c)
    js = sorted({0, R // 2, R - 1})
    for j in js:
        t = kv_len + j + 1
        for fill in ("thief", "nan"):
            q, kc, vc = c["q"].clone(), c["kc"].clone(), c["vc"].clone()
            if fill == "thief":
                q[j + 1:] = torch.randn(q[j + 1:].shape, generator=g(5)).to(c["dtype"])
                kc[0, :, t:], vc[0, :, t:] = tk[:, None], tv[:, None]
            else:
                q[j + 1:] = float("nan")
                kc[0, :, t:], vc[0, :, t:] = float("nan"), float("nan")
            got = _span(c, q, kc, vc)
            assert torch.isfinite(got[:j + 1].float()).all(), (j, fill)
            assert torch.equal(got[:j + 1], base[:j + 1]), (j, fill)
            if j + 1 < R and fill == "thief":
                assert not torch.equal(got[j + 1:], base[j + 1:])              # the later rows did read what was changed


def test_span_refusals_come_before_any_launch():
    from unsloth_amd import _lib
    dtype = torch.bfloat16

    def call(R, Hq, Hk, D, split_keys, nsplit=4):
        q = torch.zeros(16, Hq * D, dtype=dtype, device=DEV)
        kc = torch.zeros(1, Hk, 512, D, dtype=dtype, device=DEV)
        part = torch.full((16 * Hq * nsplit * (D + 2),), 7.0, dtype=torch.float32, device=DEV)
        out = torch.full((16, Hq * D), 7.0, dtype=dtype, device=DEV)
        kv = torch.zeros(1, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError, match="uamd_attn_decode_span.*invalid argument"):
            _lib.call("uamd_attn_decode_span", q, _lib.ptr(q), q.stride(0), _lib.ptr(kc), _lib.ptr(kc), kc.stride(0), kc.stride(1),
                      _lib.ptr(kv), R, _lib.ptr(part), _lib.ptr(out), out.stride(0), 1, Hq, Hk, D, nsplit, split_keys, 0,
                      0.1, _lib.dtype_code(dtype), _lib.stream_of(q))
        torch.cuda.synchronize()
        assert bool((part == 7.0).all()) and bool((out == 7.0).all())          # nothing ran

    call(0, 4, 1, 128, 128)
    call(17, 4, 1, 128, 128)
    call(9, 16, 1, 128, 128)          # R * G = 144
    call(4, 4, 1, 96, 128)
    call(4, 4, 1, 128, 24)            # no multiple of a block-load
    call(4, 4, 1, 64, 16)
    call(4, 4, 1, 128, 128, nsplit=0)


# ---- the draft and the accept kernels -------------------------------------------------------------------------------------------
def _dev(x, dtype=torch.long):
    return torch.tensor(x, dtype=dtype, device=DEV)


@pytest.mark.parametrize("case", ref.DRAFT_CASES, ids=[c[0] for c in ref.DRAFT_CASES])
def test_draft_kernel_is_the_python_rule(case):
    from unsloth_amd.kernels import decode as Dk
    _, hist, K, n_max, tok, nd = case
    assert ref.draft(hist, K, n_max) == (tok, nd)
    cap = len(hist) + 7
    h = _dev(hist + [hist[-1]] * 7)                            # slots past hist_len hold a token that would match
    got, n_draft = torch.full((16,), -5, dtype=torch.long, device=DEV), _dev([-1], torch.int32)
    Dk.ngram_draft(h, _dev([len(hist)], torch.int32), K, n_max, got, n_draft)
    assert h.numel() == cap and got[:K + 1].tolist() == tok and int(n_draft) == nd
    assert got[K + 1:].tolist() == [-5] * (15 - K)            # nothing written past the K + 1 rows


def test_draft_kernel_on_a_long_history():
    from unsloth_amd.kernels import decode as Dk
    hist = torch.randint(0, 50, (3000,), generator=g(3)).tolist()           # longer than one pass of the workgroup's threads
    for K, n_max in ((4, 2), (15, 3), (1, 1)):
        tok, nd = ref.draft(hist, K, n_max)
        got, n_draft = torch.zeros(16, dtype=torch.long, device=DEV), _dev([-1], torch.int32)
        Dk.ngram_draft(_dev(hist), _dev([len(hist)], torch.int32), K, n_max, got, n_draft)
        assert got[:K + 1].tolist() == tok and int(n_draft) == nd and nd > 0


@pytest.mark.parametrize("case", ref.ACCEPT_CASES, ids=[c[0] for c in ref.ACCEPT_CASES])
def test_accept_kernel_is_the_python_rule(case):
    from unsloth_amd.kernels import decode as Dk
    _, tok, a, eos, remaining, m, done = case
    assert ref.accept(tok, a, eos, remaining) == (m, done)
    K = len(tok) - 1
    hist = torch.full((32,), -1, dtype=torch.long, device=DEV)
    hist_len, kv_len = _dev([10], torch.int32), _dev([9], torch.int32)
    rem, dn, nd = _dev([remaining], torch.int32), _dev([0], torch.int32), _dev([2], torch.int32)
    stats = _dev([100, 200, 300, 400])
    Dk.accept_greedy(_dev(tok), _dev(a), K, _dev(eos) if eos else None, hist, hist_len, kv_len, rem, dn, nd, stats)
    assert hist[10:10 + m + 1].tolist() == a[:m + 1] and bool((hist[:10] == -1).all()) and bool((hist[10 + m + 1:] == -1).all())
    assert int(hist_len) == 10 + m + 1 and int(kv_len) == 9 + m + 1 and int(rem) == remaining - (m + 1)
    assert bool(int(dn)) == done and stats.tolist() == [101, 202, 300 + m, 400 + m + 1]
    if done:                                                   # a finished sequence: another call changes nothing
        Dk.accept_greedy(_dev(tok), _dev(a), K, _dev(eos) if eos else None, hist, hist_len, kv_len, rem, dn, nd, stats)
        assert int(hist_len) == 10 + m + 1 and int(kv_len) == 9 + m + 1 and stats.tolist() == [101, 202, 300 + m, 400 + m + 1]


# ---- the engine --------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _tiny64(load_in_4bit):
    """hidden 512, 2 layers, 8 / 2 heads of head_dim 64, vocab 1000, LoRA r = 8 with lora_B randomised; shared, never modified."""
    if load_in_4bit not in _MODELS:
        from transformers import LlamaConfig
        from unsloth_amd import FastLanguageModel
        cfg = LlamaConfig(hidden_size=512, intermediate_size=1408, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                          head_dim=64, vocab_size=1000, rms_norm_eps=1e-5, max_position_embeddings=512,
                          rope_parameters={"rope_type": "default", "rope_theta": 5e5}, tie_word_embeddings=False)
        model, _ = FastLanguageModel.from_pretrained(config=cfg, max_seq_length=256, load_in_4bit=load_in_4bit, device=DEV,
                                                     random_state=3407, use_gradient_checkpointing=False)
        model = FastLanguageModel.get_peft_model(model, r=8, lora_alpha=16, use_gradient_checkpointing=False, random_state=3407)
        gg = torch.Generator().manual_seed(11)
        for n, p in model.named_parameters():
            if "lora_B" in n:
                p.data.copy_((torch.randn(p.shape, generator=gg) * 0.05).to(DEV))
        model.eval()
        _MODELS[load_in_4bit] = model
    return _MODELS[load_in_4bit]


def _repeating_prompt(seed, n=10, vocab=1000):
    """A prompt that says everything twice, so that the first steps do find drafts: [1, 2 n]."""
    half = torch.randint(1, vocab, (n,), generator=g(seed))
    return torch.cat([half, half]).view(1, -1).to(DEV)


def _check_text_and_stats(model, eng, ids, out, K, n_max, max_new, eos=()):
    """Every generated token within 2 b of the reference row's maximum (one training-path forward over the returned text), and
    the engine's counters equal to the python rules replayed over that text."""
    T = ids.shape[1]
    assert torch.equal(out[:, :T], ids) and T < out.shape[1] <= T + max_new
    with torch.no_grad():
        full = model(input_ids=out).logits[0].float()                          # row p: the logits behind token p
    worst = 0.0
    for p in range(T, out.shape[1]):
        row = full[p - 1]
        b = LOGIT_BOUND * row.abs().max().item()
        gap = (row.max() - row[out[0, p]]).item()
        worst = max(worst, gap / b)
        assert gap <= 2 * b, (p, gap, b)
    seq = out[0].tolist()
    stats, per_step, new = ref.replay(seq, T, K, n_max, eos=list(eos), max_new_tokens=max_new)
    assert new == len(seq) - T
    got = eng.lookup_stats
    assert got["fallback"] is None and {k: got[k] for k in stats} == stats, (got, stats)
    print(f"lookup: {len(seq) - T} tokens in {stats['steps']} steps, drafted {stats['drafted']}, accepted {stats['accepted']}, "
          f"worst gap {worst:.3f} b")
    return stats, per_step


@pytest.mark.parametrize("load_in_4bit", [True, False])
@pytest.mark.parametrize("D", [128, 64])
def test_engine_text_is_the_models_and_the_counters_are_the_rules(D, load_in_4bit, monkeypatch):
    """Random weights: nearly every draft is rejected, so this is also the test that the K / V of rejected drafts never leak into
    later steps. Graph and eager engines give equal tokens and counters."""
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = tiny(load_in_4bit) if D == 128 else _tiny64(load_in_4bit)
    ids = _repeating_prompt(21)
    K, n_max, new = 4, 2, 24
    eng = DecodeEngine(model, max_seq_len=128, batch=1, use_graph=True)
    assert eng.D == D
    out = eng.generate(ids, max_new_tokens=new, prompt_lookup_num_tokens=K, max_matching_ngram_size=n_max)
    stats, _ = _check_text_and_stats(model, eng, ids, out, K, n_max, new)
    assert out.shape[1] == ids.shape[1] + new
    eng_e = DecodeEngine(model, max_seq_len=128, batch=1, use_graph=False)
    out_e = eng_e.generate(ids, max_new_tokens=new, prompt_lookup_num_tokens=K, max_matching_ngram_size=n_max)
    assert torch.equal(out_e, out) and eng_e.lookup_stats == eng.lookup_stats
    # K = 15, the widest step, on the same engine: another capture beside the first
    out15 = eng.generate(ids, max_new_tokens=new, prompt_lookup_num_tokens=15, max_matching_ngram_size=3)
    _check_text_and_stats(model, eng, ids, out15, 15, 3, new)


def test_engine_reuse_and_the_plain_path_beside_it(monkeypatch):
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = tiny(True)
    ids, ids2 = _repeating_prompt(22), _repeating_prompt(23, n=7)
    want = DecodeEngine(model, max_seq_len=128).generate(ids, max_new_tokens=8)
    eng = DecodeEngine(model, max_seq_len=128)
    before = eng.generate(ids, max_new_tokens=8)
    assert torch.equal(before, want) and eng.lookup_stats is None
    for prompt in (ids, ids2):                                  # a second generate, another prompt, the same engine and capture
        out = eng.generate(prompt, max_new_tokens=12, prompt_lookup_num_tokens=3)
        _check_text_and_stats(model, eng, prompt, out, 3, 2, 12)
    after = eng.generate(ids, max_new_tokens=8)
    assert torch.equal(after, want) and eng.lookup_stats is None
    # outside the path's scope: the plain steps' text, and the reason
    short = eng.generate(ids, max_new_tokens=8, prompt_lookup_num_tokens=16)
    assert torch.equal(short, want) and eng.lookup_stats["fallback"] and eng.lookup_stats["steps"] == 0
    tight = DecodeEngine(model, max_seq_len=128)               # capacity 128 < 20 + 106 + 3
    out = tight.generate(ids, max_new_tokens=106, prompt_lookup_num_tokens=3)
    assert "capacity" in tight.lookup_stats["fallback"] and out.shape[1] == 126


def test_for_inference_generate_takes_the_lookup_path():
    from unsloth_amd import FastLanguageModel
    model = tiny(True, fresh=True)                               # its own model: for_inference rebinds generate
    FastLanguageModel.for_inference(model)

    def no_hf_generate(*a, **k):
        raise AssertionError("generate went to HF's generate")
    model._old_generate = no_hf_generate
    ids = _repeating_prompt(24)
    out = model.generate(input_ids=ids, max_new_tokens=10, prompt_lookup_num_tokens=4)
    eng = model._uamd_decode_engine
    assert 21 < out.shape[1] <= 30 and eng.S >= 20 + 10 + 4
    assert eng.lookup_stats["fallback"] is None and eng.lookup_stats["steps"] >= 1
    assert eng.lookup_stats["tokens"] == out.shape[1] - 21              # (the first token is prefill's)


# ---- the periodic model: the next token depends on the current one only --------------------------------------------------------
V_PERIOD = 256


def _periodic():
    """A 16-bit model with LoRA whose o_proj, down_proj and lora_B are zero -- the residual stream stays the token's embedding --
    and whose lm_head row v is the embedding of token v - 1: the token after t is t + 1 mod 256, whatever came before. (The
    margin is a row's squared norm against the dot product of two random rows, far above any rounding.)"""
    if "periodic" not in _MODELS:
        from transformers import LlamaConfig
        from unsloth_amd import FastLanguageModel
        cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                          head_dim=64, vocab_size=V_PERIOD, rms_norm_eps=1e-5, max_position_embeddings=2048,
                          rope_parameters={"rope_type": "default", "rope_theta": 5e5}, tie_word_embeddings=False)
        model, _ = FastLanguageModel.from_pretrained(config=cfg, max_seq_length=2048, load_in_4bit=False, device=DEV,
                                                     random_state=3407, use_gradient_checkpointing=False)
        model = FastLanguageModel.get_peft_model(model, r=8, lora_alpha=16, use_gradient_checkpointing=False, random_state=3407)
        emb = None
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "lora_B" in n or (n.endswith("weight") and "lora_" not in n and ("o_proj" in n or "down_proj" in n)):
                    p.zero_()
                if "embed_tokens" in n:
                    p.copy_(torch.randn(p.shape, generator=g(9)).to(p.dtype))
                    emb = p
            for n, p in model.named_parameters():
                if "lm_head" in n:
                    p.copy_(torch.roll(emb, 1, 0))
                if "norm" in n:
                    p.fill_(1.0)
        model.eval()
        _MODELS["periodic"] = model
    return _MODELS["periodic"]


def _counting(first, n):
    return [(first + i) % V_PERIOD for i in range(n)]


def test_periodic_text_is_drafted_in_full(monkeypatch):
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = _periodic()
    K, n_max, new = 4, 2, 6 * V_PERIOD
    ids = torch.tensor([_counting(5, 5)], device=DEV)
    eng = DecodeEngine(model, max_seq_len=5 + new + K)
    out = eng.generate(ids, max_new_tokens=new, prompt_lookup_num_tokens=K, max_matching_ngram_size=n_max)
    assert out[0].tolist() == _counting(5, 5 + new)
    stats, per_step, _ = ref.replay(out[0].tolist(), 5, K, n_max, max_new_tokens=new)
    assert {k: eng.lookup_stats[k] for k in stats} == stats and eng.lookup_stats["fallback"] is None
    # the first period has nothing to look up; over the last half every step (but the one max_new_tokens cuts) is K + 1 tokens
    assert per_step[:150] == [1] * 150
    tail, seen = [], 0
    for n_tok in reversed(per_step):
        if seen + n_tok > new // 2:
            break
        tail.append(n_tok)
        seen += n_tok
    assert len(tail) > 100 and all(n_tok == K + 1 for n_tok in tail[1:]), tail[:5]
    assert stats["steps"] < new // 2 + new // 2 // (K + 1) + 3


def test_periodic_text_ends_on_an_eos_in_the_middle_of_a_draft_and_on_max_new_tokens():
    from unsloth_amd.models.decode import DecodeEngine
    model = _periodic()
    K = 4
    prompt = _counting(0, V_PERIOD + 3)                         # one whole period and 0 1 2: the drafts hit from the first step
    ids = torch.tensor([prompt], device=DEV)
    eng = DecodeEngine(model, max_seq_len=512)
    # first token 3, then the step drafts 4 5 6 7: eos 6 lands on its second draft
    out = eng.generate(ids, max_new_tokens=40, eos_token_id=6, prompt_lookup_num_tokens=K)
    assert out[0].tolist() == prompt + [3, 4, 5, 6]
    assert eng.lookup_stats == dict(steps=1, drafted=4, accepted=2, tokens=3, fallback=None)
    out = eng.generate(ids, max_new_tokens=40, eos_token_id=[3, 200], prompt_lookup_num_tokens=K)       # eos as the first token
    assert out[0].tolist() == prompt + [3] and eng.lookup_stats["steps"] == 0
    # 7 new tokens: the first, a step of 5, and a step that could accept 4 more but may emit 1
    out = eng.generate(ids, max_new_tokens=7, prompt_lookup_num_tokens=K)
    assert out[0].tolist() == prompt + _counting(3, 7)
    assert eng.lookup_stats == dict(steps=2, drafted=8, accepted=4, tokens=6, fallback=None)
    out = eng.generate(ids, max_new_tokens=1, prompt_lookup_num_tokens=K)
    assert out[0].tolist() == prompt + [3] and eng.lookup_stats["steps"] == 0
    # the plain steps give the same text
    assert eng.generate(ids, max_new_tokens=7)[0].tolist() == prompt + _counting(3, 7)
