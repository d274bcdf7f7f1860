"""Host checks of shared-prompt decoding (tests/_decode_shared.py; the GPU side is tests/test_gpu_decode_shared.py).

The GPU tests hold uamd_attn_decode_shared to `row_err <= 4 x model_err` against an fp64 reference over the keys [first, total) of
prompt | suffix. That bound means something only if every wrong range a shared-prompt kernel can fall into moves the rows that
watch it by more than TWICE the bound (the triangle inequality: an output within the bound of a wrong range cannot then also be
within the bound of the right one). Here, on the very inputs the GPU tests use, in fp64 and without any kernel: the four
off-by-one ends, the prompt cache read one slot too far (its stale tail) or one short (the seam key), and the window placed without
the suffix. These are conditions on the INPUTS -- a case that misses one gets another seed, never another number. Then the routing
of `share_prompt_cache=` with a stub engine, and the cache bytes of the two layouts from shapes alone."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from tests import _decode_shared as H
from tests._decode_batched import Recorder, StubEngine

BOUND_FACTOR = H.BOUND_FACTOR
assert BOUND_FACTOR == 4
CASE_DTYPE = [(n, d) for n in H.CASES for d in H.DTYPES]


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_every_wrong_range_moves_the_rows_that_watch_it(name, dtype_name):
    c = H.build_case(name, dtype_name)
    assert torch.isfinite(c["ref"]).all()
    need = 2 * BOUND_FACTOR * c["model_err"]
    seen = {}
    for mname, roles, rows, (kc, vc), ranges in H.mutants(c):
        for r in rows:
            rng = list(c["ranges"])
            rng[r] = ranges[r]
            # (the other rows keep their own keys: only row r is read from the mutant's caches)
            other = c["ref"].clone()
            other[r] = H.ref64_ranges(c["q"][r:r + 1], kc[r:r + 1], vc[r:r + 1], [rng[r]], c["scale"], c["Hq"], c["Hk"])[0]
            for role in roles:
                seen[(r, mname, role)] = H.shift_of_rows(other, c["ref"], r, H.role_heads(c["Hq"], role))
    names = {k[1] for k in seen}
    print(name, dtype_name, "model_err %.3e" % c["model_err"], "least shift %.3f" % min(seen.values()), sorted(names))
    assert seen
    for key, shift in seen.items():
        assert shift > need and shift > 0, (key, shift, need)
    # every case has an end to move; a window that cuts into the range has a shifted twin; a prompt with a slot behind it that
    # the range reaches has its stale tail watched
    assert names & {"first+1", "total-1", "first-1", "total+1"}
    if c["window"] and any(f > 0 for f, _ in c["ranges"]):
        assert "shifted" in names
    if any(L < H.S_P and f <= L for L, (f, _) in zip(c["rows_L"], c["ranges"])):
        assert "prompt+1" in names


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_the_rounding_model_is_close_to_the_reference_and_exact_on_one_key(name, dtype_name):
    c = H.build_case(name, dtype_name)
    eps = 2.0 ** -8 if dtype_name == "bf16" else 2.0 ** -11
    # P rounded (relative eps / 2 per key, on numerator and denominator) and one rounding at the store: a few eps at the most
    assert c["model_err"] <= 4 * eps, c["model_err"]
    if all(t - f == 1 for f, t in c["ranges"]):
        assert c["model_err"] == 0.0                                  # one key: the output is that v row, exactly
    else:
        assert c["model_err"] > 0


def test_the_reference_is_the_concatenation():
    """Row r's reference over (prompt[:L_p] | suffix[:new]) equals the decode edge tests' reference on a cache that holds the
    same keys in one piece, and the stale slots of both caches are outside it."""
    c = H.build_case("d128_win101_first204", "bf16")
    r, p = 2, 0
    L, new = c["rows_L"][r], c["news"][r]
    kc = torch.cat([c["pk"][p, :, :L], c["sk"][r, :, :new]], dim=1)[None].double()
    vc = torch.cat([c["pv"][p, :, :L], c["sv"][r, :, :new]], dim=1)[None].double()
    assert c["ranges"][r] == (204, 305)
    one = H.ref64_ranges(c["q"][r:r + 1], kc, vc, [(204, 305)], c["scale"], c["Hq"], c["Hk"])
    assert torch.equal(one[0], c["ref"][r])


def test_the_table_sits_on_the_edges_it_names():
    firsts = {n: sorted({f for f, _ in H.geometry(c)[5]}) for n, c in H.CASES.items()}
    assert firsts["d128_win101_first204"] == [204]
    assert [firsts[n] for n in ("d128_win131_first127", "d128_win130_first128", "d128_win129_first129")] == [[127], [128], [129]]
    assert [firsts[n] for n in ("d128_win8_first_lp-1", "d128_win7_first_lp", "d128_win3_in_suffix", "d128_win1_new_key")] == \
        [[129], [130], [134], [136]]
    assert firsts["d128_win400_total300"] == [0]
    assert [firsts[n] for n in ("d64_win100_first31", "d64_win99_first32", "d64_win98_first33")] == [[31], [32], [33]]
    rows = {n: c[3] * c[1] // c[2] for n, c in H.CASES.items()}
    assert rows["d128_r2_new1"] == 2 and rows["d128_r21_split_seam"] == 21 and rows["d128_r128_last_slots"] == 128
    assert rows["d64_g7_r21"] == 21 and rows["d64_r128_last_slots"] == 128
    assert H.geometry(H.CASES["d128_rows_differ"])[4] == (1, 129)
    for n, c in H.CASES.items():
        assert c[4] % (2048 // c[0]) == 0 and c[1] // c[2] <= 8 and len(c[6]) * c[3] <= 16, n


# ---- routing -------------------------------------------------------------------------------------------------------------------
class _StubShared(StubEngine):
    """The stub engine, plus the attributes an engine with a shared prompt cache exposes."""

    def __init__(self, B, S, share_prompt=None, S_n=None, kv_cache_dtype=None):
        super().__init__(B, S)
        self.share_prompt, self.S_n, self.kv_cache_dtype = share_prompt, S_n if S_n is not None else S, kv_cache_dtype


def _model(B, S):
    m = SimpleNamespace(generation_config=None, model=None)
    m._uamd_decode_engine = StubEngine(B, S)             # the plain stub: only B and S
    m._old_generate = Recorder(ret="hf")
    return m


@pytest.fixture
def built(monkeypatch):
    """DecodeEngine replaced by a recorder that builds stubs: [(max_seq_len, batch, other kwargs) of every construction]."""
    from unsloth_amd.models import decode as MD
    made = []

    def make(model, max_seq_len=2048, batch=1, use_graph=True, **kw):
        made.append((max_seq_len, batch, dict(kw)))
        return _StubShared(batch, max_seq_len, kw.get("share_prompt"), kw.get("max_new_tokens"), kw.get("kv_cache_dtype"))
    monkeypatch.setattr(MD, "DecodeEngine", make)
    return made


SAMPLE = dict(do_sample=True, temperature=1.0)


def test_the_keyword_reaches_the_constructor_with_both_capacities(built):
    from unsloth_amd.models.decode import unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(6, 64)
    out = unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, share_prompt_cache=True, **SAMPLE)
    assert out.shape == (6, 7) and not m._old_generate.calls
    assert len(built) == 1
    S, batch, kw = built[0]
    assert batch == 6 and kw == dict(share_prompt=3, max_new_tokens=kw["max_new_tokens"]) and S >= 4 and kw["max_new_tokens"] >= 3
    eng = m._uamd_decode_engine
    assert "share_prompt_cache" not in eng.calls[-1] and eng.calls[-1]["num_return_sequences"] == 3
    # the same call again, and a shorter one: the engine that is there
    unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, share_prompt_cache=True, **SAMPLE)
    unsloth_fast_generate(m, ids[:, :2], max_new_tokens=2, num_return_sequences=3, share_prompt_cache=True, **SAMPLE)
    assert m._uamd_decode_engine is eng and len(built) == 1 and len(eng.calls) == 3
    # a longer prompt, more new tokens, another n: each outgrows a capacity or changes the layout
    unsloth_fast_generate(m, torch.zeros(2, S + 1, dtype=torch.long), max_new_tokens=3, num_return_sequences=3,
                          share_prompt_cache=True, **SAMPLE)
    assert len(built) == 2 and built[1][0] >= S + 1 and built[1][2]["share_prompt"] == 3
    unsloth_fast_generate(m, ids, max_new_tokens=built[1][2]["max_new_tokens"] + 1, num_return_sequences=3,
                          share_prompt_cache=True, **SAMPLE)
    assert len(built) == 3 and built[2][2]["max_new_tokens"] >= built[1][2]["max_new_tokens"] + 1
    unsloth_fast_generate(m, torch.zeros(3, 4, dtype=torch.long), max_new_tokens=3, num_return_sequences=2,
                          share_prompt_cache=True, **SAMPLE)
    assert len(built) == 4 and built[3][1] == 6 and built[3][2]["share_prompt"] == 2
    # without the keyword: the replicated engine again, built exactly as before the feature
    unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, **SAMPLE)
    assert len(built) == 5 and built[4] == (7, 6, {}) and m._uamd_decode_engine.share_prompt is None


@pytest.mark.parametrize("extra", [dict(), dict(share_prompt_cache=False), dict(share_prompt_cache=None),
                                   dict(share_prompt_cache=True, num_return_sequences=1)])
def test_absent_false_or_one_sequence_builds_todays_engine(built, extra):
    from unsloth_amd.models.decode import unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    n = extra.get("num_return_sequences", 3)
    m = _model(2 * n, 64)
    first = m._uamd_decode_engine
    kw = dict(dict(num_return_sequences=n), **extra)
    unsloth_fast_generate(m, ids, max_new_tokens=3, **kw, **SAMPLE)
    assert m._uamd_decode_engine is first and not built                # the plain stub (only B and S) keeps serving
    assert "share_prompt_cache" not in first.calls[-1]
    m2 = _model(1, 64)                                                 # a batch that does not fit: today's keywords exactly
    unsloth_fast_generate(m2, ids, max_new_tokens=3, **kw, **SAMPLE)
    assert built == [(7, 2 * n, {})]


def test_the_keyword_never_reaches_hf_generate(built):
    from unsloth_amd.models.decode import _ENGINE_KWARGS, route_generate, unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(6, 64)
    assert unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, share_prompt_cache=True,
                                 repetition_penalty=1.3, **SAMPLE) == "hf"
    assert "share_prompt_cache" not in m._old_generate.calls[-1][1] and not built
    assert "share_prompt_cache" in _ENGINE_KWARGS
    assert route_generate(m, ids, 3, dict(share_prompt_cache=True, num_return_sequences=3, do_sample=True))[0] == "engine"


def test_fp8_together_with_sharing_raises(built):
    from unsloth_amd.models.decode import unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(6, 64)
    with pytest.raises(NotImplementedError, match="share_prompt"):
        unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, share_prompt_cache=True, kv_cache_dtype="fp8",
                              **SAMPLE)
    assert not built and not m._uamd_decode_engine.calls
    # with one sequence per prompt the keyword does nothing, and FP8 is served as before
    m1 = _model(2, 64)
    unsloth_fast_generate(m1, ids, max_new_tokens=3, share_prompt_cache=True, kv_cache_dtype="fp8")
    assert built == [(7, 2, dict(kv_cache_dtype="fp8"))]


def test_a_marked_model_passes_the_choice_on(built):
    from unsloth_amd import FastLanguageModel
    from unsloth_amd.models.decode import unsloth_fast_generate, wanted_share_prompt
    from unsloth_amd.models.llama import FastLlamaModel
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(6, 64)
    m._uamd_share_prompt_cache = True
    unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, **SAMPLE)
    assert len(built) == 1 and built[0][2]["share_prompt"] == 3
    unsloth_fast_generate(m, ids, max_new_tokens=3, num_return_sequences=3, share_prompt_cache=False, **SAMPLE)
    assert len(built) == 2 and built[1][2] == {}                       # the keyword stands above the mark
    base = SimpleNamespace(_uamd_share_prompt_cache=True)
    assert wanted_share_prompt(SimpleNamespace(get_base_model=lambda: base)) is True
    assert wanted_share_prompt(SimpleNamespace()) is False and wanted_share_prompt(base, False) is False
    # for_inference records it; None leaves the record alone
    for cls in (FastLanguageModel, FastLlamaModel):
        assert inspect.signature(cls.for_inference).parameters["share_prompt_cache"].default is None
    cfg = SimpleNamespace(head_dim=32, hidden_size=64, num_attention_heads=2, hidden_act="silu")       # (no decode engine: D = 32)
    model = torch.nn.Linear(2, 2)
    model.config = cfg
    FastLanguageModel.for_inference(model)
    assert not hasattr(model, "_uamd_share_prompt_cache")
    FastLanguageModel.for_inference(model, share_prompt_cache=True)
    FastLanguageModel.for_inference(model)
    assert model._uamd_share_prompt_cache is True and not hasattr(model, "_uamd_float8_kv_cache")
    FastLanguageModel.for_inference(model, share_prompt_cache=False)
    assert model._uamd_share_prompt_cache is False


def test_the_entry_point_and_the_constructor_keywords_exist():
    import ctypes
    from unsloth_amd import _lib
    from unsloth_amd.kernels import decode as Dk
    from unsloth_amd.models.decode import DecodeEngine
    res, args = _lib.SIGNATURES["uamd_attn_decode_shared"]
    assert res is ctypes.c_int and len(args) == 28
    assert hasattr(Dk, "attn_decode_shared") and Dk.MAX_SHARE == 16
    sig = inspect.signature(DecodeEngine.__init__).parameters
    assert sig["share_prompt"].default is None and sig["max_new_tokens"].default is None


# ---- cache bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,n,ctx,new", [(1, 8, 2048, 256), (1, 16, 2048, 256), (2, 8, 2048, 256), (1, 16, 8192, 512)])
def test_cache_bytes_of_the_two_layouts(P, n, ctx, new):
    """Llama-3-8B: 32 layers, 8 KV heads, D = 128, 16-bit. Shapes on the `meta` device against the formula."""
    L, Hk, D = 32, 8, 128
    S_p, S_n, S = ctx, new, ctx + new
    shared, replicated = H.cache_bytes(L, Hk, D, 2, P, n, S_p, S_n, S)
    kw = dict(dtype=torch.bfloat16, device="meta")
    pk = torch.empty(P, Hk, S_p, D, **kw)
    sk = torch.empty(P * n, Hk, S_n, D, **kw)
    rk = torch.empty(P * n, Hk, S, D, **kw)
    nbytes = lambda t: t.numel() * t.element_size()
    assert shared == 2 * L * (nbytes(pk) + nbytes(sk)) and replicated == 2 * L * nbytes(rk)
    assert shared == 2 * L * Hk * D * 2 * (P * S_p + P * n * S_n) and replicated == 2 * L * Hk * D * 2 * P * n * S
    assert replicated - shared == 2 * L * Hk * D * 2 * P * (n - 1) * S_p         # n - 1 copies of every prompt
    print(P, n, ctx, new, "shared %.2f GB" % (shared / 1e9), "replicated %.2f GB" % (replicated / 1e9))
