"""-m gpu: decode over the FP8 KV cache -- uamd_attn_decode_fp8 on the key-range edge table, and DecodeEngine(kv_cache_dtype="fp8").

Attention: the whole table of tests/_decode_edges.py, both 16-bit types, on caches quantised by the torch reference quantiser
(tests/_kv_fp8.py), judged row by row against the fp64 reference over the DEQUANTISED caches; the bound is the 16-bit kernels':
4 x the error of that reference rounded once to the 16-bit type (the kernel multiplies exactly representable factors in fp32 and
rounds once, at the store). tests/test_kv_fp8_host.py shows that an off-by-one range moves the watching rows by >= 0.5 and that
the reference over the 16-bit caches lies >= 3 bounds away. Measured ratios go to decode_fp8_edge_report.json in the directory
UAMD_REPORT_DIR names (default: test_reports/ in the repository root, git-ignored); profiles/decode_fp8_edge_report.json is a
committed copy of one MI355X run.

Engine (the tiny model of tests/_decode_batched.py): layer 0's caches against the reference quantiser of the 16-bit engine's,
bitwise; cache memory; eager against hipGraph replay; row independence of the step; closeness to the 16-bit engine; generate."""
import json
import os

import pytest
import torch

from tests import _decode_edges as E
from tests import _kv_fp8 as K8
from tests._decode_batched import DEV, Recorder, g, left_padded, tiny

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
CASE_DTYPE = [(n, d) for n in E.CASES for d in E.DTYPES]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_fp8_edge_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


# ---- attention -----------------------------------------------------------------------------------------------------------------
def _launch(c, kc, ks, vc, vs):
    """uamd_attn_decode_fp8 with len_add = 1 on caches that already hold the new token: out [B, Hq * D] on the host."""
    from unsloth_amd.kernels import decode as Dk
    B, Hq, D = c["B"], c["Hq"], c["D"]
    kv_len = torch.tensor([L - 1 for L in c["lens"]], dtype=torch.int32, device=DEV)
    part = torch.empty(B, Hq, E.S_MAX // c["split_keys"], D + 2, dtype=torch.float32, device=DEV)
    out = torch.full((B, Hq * D), float("nan"), dtype=c["dtype"], device=DEV)
    Dk.attn_decode_fp8(c["q"].to(DEV), kc, vc, ks, vs, kv_len, out, part, c["split_keys"], c["scale"], len_add=1,
                       window=c["window"])
    return out.cpu()


def _caches(c):
    return (K8.as_bytes(c["k8"][0]).to(DEV), c["k8"][1].to(DEV), K8.as_bytes(c["v8"][0]).to(DEV), c["v8"][1].to(DEV))


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_attn_decode_fp8_edges_match_fp64(name, dtype_name):
    c = K8.build_case(name, dtype_name)
    got = _launch(c, *_caches(c))
    assert torch.isfinite(got.float()).all()
    err, model, ok = E.judge(c, got)
    ratio = err / model if model > 0 else (0.0 if err == 0 else float("inf"))       # (one key: the model is exact)
    far = E.row_err(got.view(c["B"], c["Hq"], c["D"]), c["ref16"])
    REPORT[f"{name}/{dtype_name}/attn_decode_fp8"] = dict(kernel=err, model=model, ratio=ratio, from_16_bit_reference=far)
    print(f"{name}/{dtype_name}: err {err:.3e} model_err {model:.3e} ratio {ratio:.2f}; from the 16-bit reference {far:.3e}")
    assert ok, (err, model, ratio)


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_slots_outside_the_range_are_never_used(name, dtype_name):
    """The slots at `len` and behind (an earlier prompt's keys) and below `first` (older than the window) are filled with a key
    that every head scores far above its edge key -- the sum of the group's queries, its scale times 64 -- and an unrelated
    value: the output is the same, bit for bit, as over the table's own content, and within the bound."""
    c = K8.build_case(name, dtype_name)
    B, Hq, Hk, D = c["B"], c["Hq"], c["Hk"], c["D"]
    k_bad = c["q"].float().view(B, Hk, Hq // Hk, D).sum(2).to(c["dtype"])
    v_bad = (3.0 + torch.randn(B, Hk, D, generator=torch.Generator().manual_seed(77))).to(c["dtype"])
    (kb_c, kb_s), (vb_c, vb_s) = K8.quantize_ref(k_bad), K8.quantize_ref(v_bad)
    kb_s, vb_s = kb_s * 64, vb_s * 64
    kc, ks, vc, vs = _caches(c)
    clean = _launch(c, kc, ks, vc, vs)
    n = 0
    for b, (first, L) in enumerate(c["ranges"]):
        for lo, hi in ((0, first), (L, E.S_MAX)):
            if hi > lo:
                kc[b, :, lo:hi] = K8.as_bytes(kb_c)[b].to(DEV)[:, None]
                vc[b, :, lo:hi] = K8.as_bytes(vb_c)[b].to(DEV)[:, None]
                ks[b, :, lo:hi] = kb_s[b].to(DEV)[:, None]
                vs[b, :, lo:hi] = vb_s[b].to(DEV)[:, None]
                n += hi - lo
    assert n > 0 or all(r == (0, E.S_MAX) for r in c["ranges"])
    got = _launch(c, kc, ks, vc, vs)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, clean)
    assert E.judge(c, got)[2], E.judge(c, got)


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def _engines(model, batch, **kw):
    from unsloth_amd.models.decode import DecodeEngine
    e16 = DecodeEngine(model, max_seq_len=256, batch=batch, **kw)
    e8 = DecodeEngine(model, max_seq_len=256, batch=batch, kv_cache_dtype="fp8", **kw)
    assert e16.kv_cache_dtype is None and e8.kv_cache_dtype == "fp8"
    return e16, e8


def _layer0_is_the_quantised_16_bit_cache(e16, e8):
    for c16, codes, scales in ((e16.k_cache[0], e8.k_cache[0], e8.k_scale[0]), (e16.v_cache[0], e8.v_cache[0], e8.v_scale[0])):
        want_c, want_s = K8.quantize_ref(c16.cpu())
        assert codes.dtype == torch.uint8 and scales.dtype == torch.float32
        assert torch.equal(codes.cpu(), K8.as_bytes(want_c)), "layer-0 codes differ from the quantised 16-bit cache"
        assert torch.equal(scales.cpu(), want_s), "layer-0 scales differ from the quantised 16-bit cache"


@pytest.mark.parametrize("how", ["unpadded", "left_padded", "repeat3"])
def test_layer0_cache_is_the_quantised_16_bit_cache(how):
    """Layer 0's K and V do not depend on attention, so the two engines quantise / store the same values: after prefill and after
    one step (the same token to both) the FP8 engine's layer-0 codes and scales ARE the reference quantiser of the 16-bit engine's
    layer-0 cache, unwritten slots included (codes 0, scale 1: the quantised zero row)."""
    model = tiny(True)
    mask, repeat = None, 1
    if how == "left_padded":
        ids, mask, _ = left_padded((4, 9), 9, seed=60)
        ids, mask = ids.to(DEV), mask.to(DEV)
    else:
        ids = torch.randint(1, 1000, (2, 11), generator=g(61)).to(DEV)
        repeat = 3 if how == "repeat3" else 1
    e16, e8 = _engines(model, ids.shape[0] * repeat)
    e16.prefill(ids, mask, repeat=repeat)
    e8.prefill(ids, mask, repeat=repeat)
    assert e8.kv_len.tolist() == e16.kv_len.tolist()
    assert float(e16.k_cache[0].float().abs().sum()) > 0
    _layer0_is_the_quantised_16_bit_cache(e16, e8)
    tok = torch.randint(1, 1000, (e8.B,), generator=g(62)).to(DEV)
    e16.step(tok)
    e8.step(tok)
    assert e8.kv_len.tolist() == e16.kv_len.tolist()
    _layer0_is_the_quantised_16_bit_cache(e16, e8)
    if how == "repeat3":                                               # the replicas are copies, at every layer
        for li in range(len(e8.k_cache)):
            for t in (e8.k_cache[li], e8.k_scale[li], e8.v_cache[li], e8.v_scale[li]):
                t5 = t[:, :, :11].reshape(2, 3, -1)
                assert torch.equal(t5[:, 0], t5[:, 1]) and torch.equal(t5[:, 0], t5[:, 2])


def test_cache_memory_is_d_plus_4_over_2d():
    model = tiny(True)
    e16, e8 = _engines(model, 2, use_graph=False)

    def nbytes(ts):
        return sum(t.numel() * t.element_size() for t in ts)
    b16 = nbytes(e16.k_cache + e16.v_cache)
    b8 = nbytes(e8.k_cache + e8.v_cache + e8.k_scale + e8.v_scale)
    D = e8.D
    assert e16.k_scale is None and e16.v_scale is None
    assert b8 * 2 * D == b16 * (D + 4), (b8, b16)


@pytest.mark.parametrize("B", [1, 4])
def test_graph_replay_equals_the_eager_step(B, monkeypatch):
    from unsloth_amd import _lib
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    ids = torch.randint(1, 1000, (B, 13), generator=g(63 + B)).to(DEV)
    eg = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=True, kv_cache_dtype="fp8")
    ee = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=False, kv_cache_dtype="fp8")
    assert eg.use_graph and not ee.use_graph
    lg, le = eg.prefill(ids), ee.prefill(ids)
    assert torch.equal(lg, le)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    for step in range(4):
        nxt = torch.argmax(lg, dim=-1)
        names.clear()
        le = ee.step(nxt).clone()
        assert "uamd_rope_kv_append_fp8" in names and "uamd_attn_decode_fp8" in names, names
        assert not {"uamd_rope_kv_append", "uamd_attn_decode", "uamd_attn_decode_fused"} & set(names), names
        lg = eg.step(nxt).clone()
        assert torch.equal(lg, le), f"graph replay differs from the eager step at step {step}"
    assert eg._graph is not None and eg.kv_len.tolist() == [17] * B
    for li in range(len(eg.k_cache)):
        assert torch.equal(eg.k_cache[li], ee.k_cache[li]) and torch.equal(eg.v_scale[li], ee.v_scale[li])


def test_a_rows_logits_do_not_depend_on_the_batch():
    """The step on uamd_gemv_rows computes a row from that row alone; the FP8 attention keeps that: rows 0 and 1 of a batch of 4
    and the same two sequences as a batch of 2 (the same cache bytes, copied) give the same logits, bit for bit."""
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    ids = torch.randint(1, 1000, (4, 15), generator=g(70)).to(DEV)
    e4 = DecodeEngine(model, max_seq_len=256, batch=4, kv_cache_dtype="fp8")
    e2 = DecodeEngine(model, max_seq_len=256, batch=2, kv_cache_dtype="fp8")
    lg4 = e4.prefill(ids)
    e2.prefill(ids[:2])
    for li in range(len(e4.k_cache)):
        for a, b in ((e2.k_cache, e4.k_cache), (e2.v_cache, e4.v_cache), (e2.k_scale, e4.k_scale), (e2.v_scale, e4.v_scale)):
            a[li].copy_(b[li][:2])
    for step in range(3):
        nxt = torch.argmax(lg4, dim=-1)
        lg4 = e4.step(nxt).clone()
        lg2 = e2.step(nxt[:2]).clone()
        assert torch.equal(lg4[:2], lg2), f"rows 0, 1 differ between batch 4 and batch 2 at step {step}"
        assert not torch.equal(lg4[2], lg4[0])


def _overwrite_with_round_trip(eng, lo, hi):
    """Slots [lo[b], hi[b]) of every layer's 16-bit caches <- their FP8 round trip, rounded to the cache type (torch reference)."""
    for cache in eng.k_cache + eng.v_cache:
        for b in range(eng.B):
            if hi[b] > lo[b]:
                cache[b, :, lo[b]:hi[b]] = K8.round_trip(cache[b, :, lo[b]:hi[b]].cpu()).to(DEV)


def test_the_fp8_engine_is_as_close_as_its_format_allows():
    """Teacher-forced, 8 steps, batch 2, the same tokens to three engines: the 16-bit engine, the 16-bit engine whose caches are
    overwritten after prefill and after every step by their FP8 round trip rounded to the 16-bit type (`fake`; torch reference
    quantiser, no new kernel), and the FP8 engine. row_err of the logits against the untouched 16-bit engine, worst step:
    the FP8 engine's is > 0 (the cache really is FP8) and <= 2 x the fake's -- the same perturbation up to the fake path's extra
    rounding to 16 bits and the fp32 summation order."""
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    B, T, steps = 2, 12, 8
    ids = torch.randint(1, 1000, (B, T), generator=g(80)).to(DEV)
    toks = torch.randint(1, 1000, (steps, B), generator=g(81)).to(DEV)
    e16 = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=False)
    fake = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=False)
    e8 = DecodeEngine(model, max_seq_len=256, batch=B, use_graph=False, kv_cache_dtype="fp8")
    l16, lf, l8 = e16.prefill(ids), fake.prefill(ids), e8.prefill(ids)
    assert torch.equal(l16, lf) and torch.equal(l16, l8)              # prefill attends the unquantised K and V
    _overwrite_with_round_trip(fake, [0] * B, [T] * B)
    e_fake = e_fp8 = 0.0
    for s in range(steps):
        l16, lf, l8 = e16.step(toks[s]), fake.step(toks[s]), e8.step(toks[s])
        _overwrite_with_round_trip(fake, [T + s] * B, [T + s + 1] * B)
        assert torch.isfinite(l8).all()
        e_fake = max(e_fake, E.row_err(lf, l16))
        e_fp8 = max(e_fp8, E.row_err(l8, l16))
    REPORT["engine/closeness"] = dict(e_fake=e_fake, e_fp8=e_fp8, ratio=e_fp8 / e_fake if e_fake > 0 else float("inf"))
    print(f"row_err against the 16-bit engine: fake {e_fake:.3e}, fp8 engine {e_fp8:.3e}")
    assert e_fp8 > 0
    assert e_fp8 <= 2 * e_fake, (e_fp8, e_fake)


def test_generate_with_the_keyword_and_without():
    from unsloth_amd import FastLanguageModel
    model = tiny(True, fresh=True)
    FastLanguageModel.for_inference(model)
    model._old_generate = Recorder(ret="hf")
    ids = torch.randint(1, 1000, (2, 9), generator=g(90)).to(DEV)
    out8 = model.generate(ids, max_new_tokens=8, kv_cache_dtype="fp8")
    assert tuple(out8.shape) == (2, 17) and not model._old_generate.calls
    assert torch.equal(out8[:, :9], ids)
    e8 = model._uamd_decode_engine
    assert e8.kv_cache_dtype == "fp8" and e8.k_cache[0].dtype == torch.uint8
    assert model.generate(ids, max_new_tokens=8, kv_cache_dtype="fp8").equal(out8) and model._uamd_decode_engine is e8
    out16 = model.generate(ids, max_new_tokens=8)                      # without the keyword: a 16-bit engine again
    e16 = model._uamd_decode_engine
    assert e16 is not e8 and e16.kv_cache_dtype is None and e16.k_cache[0].dtype == e16.dtype
    assert tuple(out16.shape) == (2, 17) and not model._old_generate.calls
    with pytest.raises(ValueError):
        model.generate(ids, max_new_tokens=8, kv_cache_dtype="int4")
    # the loader's and for_inference's spelling
    FastLanguageModel.for_inference(model, float8_kv_cache=True)
    assert model.generate(ids, max_new_tokens=8).equal(out8) and model._uamd_decode_engine.kv_cache_dtype == "fp8"
    FastLanguageModel.for_inference(model, float8_kv_cache=False)
    assert model.generate(ids, max_new_tokens=8).equal(out16) and model._uamd_decode_engine.kv_cache_dtype is None
