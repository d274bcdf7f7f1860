"""CPU: the host side of the FP8 KV cache -- the torch restatement of the stored format (tests/_kv_fp8.py, the reference of the
GPU tests), the conditions under which the decode edge-case table means something over quantised caches, and where
`unsloth_fast_generate` sends `kv_cache_dtype=` / a model marked with `float8_kv_cache`."""
from types import SimpleNamespace

import pytest
import torch

from tests import _decode_edges as E
from tests import _kv_fp8 as K8
from tests._decode_batched import Recorder, StubEngine

BOUND_FACTOR = E.BOUND_FACTOR
MIN_SHIFT = 0.5             # row_err by which an off-by-one range moves the rows that watch the moved edge (test_decode_edge_inputs)
WATCHERS = {"first-1": (0, 2), "first+1": (0,), "len+1": (1, 2), "len-1": (1,)}
MIN_DISTANCE = 3            # the FP8 reference sits at least this many GPU bounds away from the 16-bit-cache reference
CASE_DTYPE = [(n, d) for n in E.CASES for d in E.DTYPES]


# ---- the reference quantiser ----------------------------------------------------------------------------------------------------
def _row(values, D=64, last=448.0):
    x = torch.zeros(D)
    x[:len(values)] = torch.tensor(values)
    x[-1] = last
    return x


def test_ties_go_to_even_and_the_largest_code_survives():
    # scale exactly 1 (amax = 448). e4m3 spacing is 2 in [16, 32), 4 in [32, 64), 2^-3 in [1, 2)
    vals = [17.0, 19.0, 21.0, -17.0, 34.0, 38.0, 1.0625, 1.1875, 448.0, -448.0, 447.0, 0.0, -0.0]
    want = [16.0, 20.0, 20.0, -16.0, 32.0, 40.0, 1.0, 1.25, 448.0, -448.0, 448.0, 0.0, -0.0]
    codes, scale = K8.quantize_ref(_row(vals)[None])
    assert scale.tolist() == [1.0]
    got = codes.float()[0, :len(vals)]
    assert got.tolist() == want
    assert K8.as_bytes(codes)[0, len(vals) - 1].item() == 0x80 and K8.as_bytes(codes)[0, len(vals) - 2].item() == 0x00
    assert K8.as_bytes(codes)[0, 8].item() == 0x7E and K8.as_bytes(codes)[0, 9].item() == 0xFE        # +-448, not NaN (0x7F)
    # a value too small for the format rounds to a zero of its sign
    # ... and the subnormal codes (multiples of 2^-9) tie to even too: 0.5 -> 0, 1.5 -> 2
    codes, _ = K8.quantize_ref(_row([2.0 ** -11, -2.0 ** -11, 3 * 2.0 ** -10, 2.0 ** -10, -2.0 ** -10])[None])
    assert K8.as_bytes(codes)[0, :5].tolist() == [0x00, 0x80, 0x02, 0x00, 0x80]


def test_a_row_of_ones_round_trips_exactly():
    x = (torch.randint(0, 2, (5, 128), generator=torch.Generator().manual_seed(1)) * 2 - 1).float()
    codes, scale = K8.quantize_ref(x)
    assert bool((scale == torch.tensor(1.0) / torch.tensor(448.0)).all())
    assert bool((codes.float().abs() == 448).all())
    # 448 x fl(1 / 448): +-1 once rounded to fp32 (or to a 16-bit type), within half an fp32 ulp of it in exact arithmetic
    assert torch.equal(codes.float() * scale[:, None], x)
    assert float((K8.dequantize_ref(codes, scale) - x.double()).abs().max()) <= 2.0 ** -24
    assert torch.equal(K8.round_trip(x.bfloat16()), x.bfloat16()) and torch.equal(K8.round_trip(x.half()), x.half())


def test_zero_rows_and_non_finite_rows():
    x = torch.zeros(4, 64)
    x[1, 3] = float("nan")
    x[2, 5] = float("inf")
    x[3, 7] = -0.0
    codes, scale = K8.quantize_ref(x)
    assert scale[0].item() == 1.0 and scale[3].item() == 1.0 and torch.isnan(scale[1]) and torch.isnan(scale[2])
    assert int(K8.as_bytes(codes)[0].sum()) == 0
    assert K8.as_bytes(codes)[3, 7].item() == 0x80 and int(K8.as_bytes(codes)[3].sum()) == 0x80
    assert torch.isnan(K8.dequantize_ref(codes, scale)[1]).all()


def test_the_error_of_a_round_trip_is_the_formats():
    """|x - dequant| <= amax / 448 x half a unit of a 4-bit significand at the top binade (2^-4 x 256 = 16 -> 16 / 448 of amax),
    and relative 2^-4 for every element that is not subnormal in the row's scale."""
    x = torch.randn(64, 128, generator=torch.Generator().manual_seed(2)).bfloat16()
    codes, scale = K8.quantize_ref(x)
    d = K8.dequantize_ref(codes, scale)
    err = (d - x.double()).abs()
    amax = x.double().abs().amax(-1, keepdim=True)
    assert bool((err <= amax * (16.0 / 448.0) * (1 + 1e-6)).all())
    normal = x.double().abs() >= amax / 448.0 * 2.0 ** -6
    assert bool((err[normal] <= x.double().abs()[normal] * 2.0 ** -4 * (1 + 1e-6)).all())
    assert float(err.max()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_the_sweep_rows_hold_every_value_at_scale_one(dtype, D):
    rows = K8.every_value_rows(dtype, D)
    n = {torch.bfloat16: 2 * (0x43E0 + 1), torch.float16: 2 * (0x5F00 + 1)}[dtype]          # bit patterns of [0, 448], two signs
    assert rows.shape == ((n + D - 2) // (D - 1), D)
    codes, scale = K8.quantize_ref(rows)
    assert bool((scale == 1).all())
    body = rows[:, :D - 1].reshape(-1)[:n]
    assert body.view(torch.int16).unique().numel() == n                                        # every pattern once
    assert torch.equal(codes[:, :D - 1].reshape(-1)[:n].view(torch.uint8), body.float().to(K8.F8).view(torch.uint8))


# ---- the edge-case table over quantised caches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_every_off_by_one_range_moves_the_rows_that_watch_it(name, dtype_name):
    """(a) over the dequantised caches: what tests/test_decode_edge_inputs.py holds for the 16-bit ones."""
    c = K8.build_case(name, dtype_name)
    assert torch.isfinite(c["ref"]).all()
    assert MIN_SHIFT > 20 * BOUND_FACTOR * c["model_err"], c["model_err"]
    seen = {}
    for b, (first, L) in enumerate(c["ranges"]):
        for mname, f, e in E.mutants(first, L, E.S_MAX):
            ranges = list(c["ranges"])
            ranges[b] = (f, e)
            other = E.ref64_ranges(c["q"], c["kd"], c["vd"], ranges, c["scale"], c["Hq"], c["Hk"])
            for role in WATCHERS[mname]:
                seen[(b, mname, role)] = E.shift_of_rows(other, c["ref"], b, E.role_heads(c["Hq"], role))
    assert seen
    print(name, dtype_name, "model_err %.3e" % c["model_err"], {k: round(v, 3) for k, v in seen.items()})
    for key, shift in seen.items():
        assert shift >= MIN_SHIFT, (key, shift)


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_the_fp8_reference_is_far_from_the_16_bit_one(name, dtype_name):
    """(b): a kernel that ignored the scales, or read 16-bit values, could not pass the GPU bound. A range of one key is its v
    row: there the bound is equality and any distance at all is far."""
    c = K8.build_case(name, dtype_name)
    dist = E.row_err(c["ref16"], c["ref"])
    print(name, dtype_name, "model_err %.3e distance %.3e = %.1f x model_err" % (c["model_err"], dist, dist / max(c["model_err"], 1e-300)))
    assert dist > 0 and dist >= MIN_DISTANCE * BOUND_FACTOR * c["model_err"], (dist, c["model_err"])
    mass = E.edge_mass(c["q"].double(), c["kd"], c["lens"], c["window"], c["scale"], c["Hq"], c["Hk"])
    assert min(mass.values()) >= 0.5


# ---- routing -------------------------------------------------------------------------------------------------------------------
class _Stub8(StubEngine):
    """The stub engine, plus the attribute an engine with a cache type exposes."""

    def __init__(self, B, S, kv_cache_dtype=None):
        super().__init__(B, S)
        self.kv_cache_dtype = kv_cache_dtype


def _model(B, S):
    m = SimpleNamespace(generation_config=None, model=None)
    m._uamd_decode_engine = StubEngine(B, S)             # the plain stub: only B and S
    m._old_generate = Recorder(ret="hf")
    return m


@pytest.fixture
def built(monkeypatch):
    """DecodeEngine replaced by a recorder that builds stubs: [(kwargs of every construction)]."""
    from unsloth_amd.models import decode as MD
    made = []

    def make(model, max_seq_len=2048, batch=1, use_graph=True, **kw):
        made.append(dict(kw))
        return _Stub8(batch, max_seq_len, MD.kv_cache_kind(kw.get("kv_cache_dtype")))
    monkeypatch.setattr(MD, "DecodeEngine", make)
    return made


def test_the_keyword_reaches_the_engine_and_rebuilds_only_on_a_change(built):
    from unsloth_amd.models.decode import route_generate, unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(2, 64)
    first = m._uamd_decode_engine
    unsloth_fast_generate(m, ids, max_new_tokens=3)                               # nothing asked: the engine that is there
    assert m._uamd_decode_engine is first and not built and not m._old_generate.calls
    out = unsloth_fast_generate(m, ids, max_new_tokens=3, kv_cache_dtype="fp8")
    assert out.shape == (2, 7) and not m._old_generate.calls
    assert built == [dict(kv_cache_dtype="fp8")]
    e8 = m._uamd_decode_engine
    assert e8 is not first and e8.kv_cache_dtype == "fp8"
    assert "kv_cache_dtype" not in e8.calls[-1]                                   # the engine's generate does not take it
    unsloth_fast_generate(m, ids, max_new_tokens=3, kv_cache_dtype="fp8")
    assert m._uamd_decode_engine is e8 and len(built) == 1 and len(e8.calls) == 2
    unsloth_fast_generate(m, ids, max_new_tokens=3)                               # without the keyword: a 16-bit engine again
    assert m._uamd_decode_engine is not e8 and m._uamd_decode_engine.kv_cache_dtype is None
    assert built == [dict(kv_cache_dtype="fp8"), {}]                              # ... built exactly as before the feature
    e16 = m._uamd_decode_engine
    unsloth_fast_generate(m, ids, max_new_tokens=3, kv_cache_dtype="auto")
    unsloth_fast_generate(m, ids, max_new_tokens=3, kv_cache_dtype=None)
    assert m._uamd_decode_engine is e16 and len(built) == 2
    assert route_generate(m, ids, 3, dict(kv_cache_dtype="fp8"))[0] == "engine"
    # a call HF's generate takes does not carry the keyword along
    assert unsloth_fast_generate(m, ids, max_new_tokens=3, kv_cache_dtype="fp8", repetition_penalty=1.3) == "hf"
    assert "kv_cache_dtype" not in m._old_generate.calls[-1][1]


def test_an_unknown_cache_type_raises(built):
    from unsloth_amd.models.decode import kv_cache_kind, unsloth_fast_generate
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(2, 64)
    for bad in ("fp16", "int8", "FP8", "e5m2", 8):
        with pytest.raises(ValueError):
            unsloth_fast_generate(m, ids, max_new_tokens=3, kv_cache_dtype=bad)
        with pytest.raises(ValueError):
            kv_cache_kind(bad)
    assert not built and not m._uamd_decode_engine.calls and not m._old_generate.calls
    assert kv_cache_kind(None) is None and kv_cache_kind("auto") is None and kv_cache_kind("fp8") == "fp8"


def test_a_marked_model_passes_the_choice_on(built):
    from unsloth_amd.models.decode import unsloth_fast_generate, wanted_kv_cache
    ids = torch.zeros(2, 4, dtype=torch.long)
    m = _model(2, 64)
    m._uamd_float8_kv_cache = True                       # what from_pretrained(float8_kv_cache=True) / for_inference(...) record
    unsloth_fast_generate(m, ids, max_new_tokens=3)
    assert built == [dict(kv_cache_dtype="fp8")] and m._uamd_decode_engine.kv_cache_dtype == "fp8"
    unsloth_fast_generate(m, ids, max_new_tokens=3, kv_cache_dtype="auto")        # the keyword stands above the mark
    assert built[-1] == {} and m._uamd_decode_engine.kv_cache_dtype is None
    m._uamd_float8_kv_cache = False
    assert wanted_kv_cache(m) is None and wanted_kv_cache(m, "fp8") == "fp8"
    # a PEFT-style wrapper: the mark sits on the base model
    base = SimpleNamespace(_uamd_float8_kv_cache=True)
    wrapper = SimpleNamespace(get_base_model=lambda: base)
    assert wanted_kv_cache(wrapper) == "fp8"


def test_for_inference_and_from_pretrained_record_the_choice():
    import inspect
    from unsloth_amd import FastLanguageModel
    from unsloth_amd.models.llama import FastLlamaModel
    assert inspect.signature(FastLanguageModel.for_inference).parameters["float8_kv_cache"].default is None
    assert inspect.signature(FastLlamaModel.for_inference).parameters["float8_kv_cache"].default is None
    cfg = SimpleNamespace(head_dim=32, hidden_size=64, num_attention_heads=2, hidden_act="silu")       # (no decode engine: D = 32)
    model = torch.nn.Linear(2, 2)
    model.config = cfg
    FastLanguageModel.for_inference(model)
    assert not hasattr(model, "_uamd_float8_kv_cache")
    FastLanguageModel.for_inference(model, float8_kv_cache=True)
    assert model._uamd_float8_kv_cache is True
    FastLanguageModel.for_inference(model)                                        # None leaves the record alone
    assert model._uamd_float8_kv_cache is True
    FastLanguageModel.for_inference(model, float8_kv_cache=False)
    assert model._uamd_float8_kv_cache is False


def test_the_fp8_entry_points_are_part_of_the_abi():
    import ctypes
    from unsloth_amd import _lib
    for name, nargs in (("uamd_kv_store_fp8", 15), ("uamd_rope_kv_append_fp8", 20), ("uamd_attn_decode_fp8", 23)):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    from unsloth_amd.kernels import decode as Dk
    assert all(hasattr(Dk, n) for n in ("kv_store_fp8", "rope_kv_append_fp8", "attn_decode_fp8"))


def test_the_engine_takes_the_cache_type():
    import inspect
    from unsloth_amd.models.decode import _ENGINE_KWARGS, DecodeEngine
    assert inspect.signature(DecodeEngine.__init__).parameters["kv_cache_dtype"].default is None
    assert "kv_cache_dtype" in _ENGINE_KWARGS
