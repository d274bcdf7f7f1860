"""Host checks of the LoRA block route cases (tests/_lora_blocks.py; the GPU side is tests/test_gpu_lora_block_routes.py).

The GPU tests hold every slice of every block output to `err <= BOUND_FACTOR x the rounding model's err` against an fp64 truth.
Here the reference side alone is shown to carry that: the truth agrees with the project's fp32 oracle up to the oracle's own
summation noise, the rounding model's error is positive on every slice and of the size 16-bit rounding has, and every wrong
variant of the block (a dropped LoRA term, a dropped rank, a scale applied once too few or too often, up and gate swapped, one
token row without its LoRA term, non-zero rank padding) lands beyond MAX_FACTOR, the largest factor any tensor may be given.
These are conditions on the CASES and the yardstick -- a case that misses one is changed, never the mutant list or a factor."""
import math

import pytest
import torch

from oracle import ref_ops as R
from tests import _lora_blocks as L

ALL = list(L.CASES)
# the oracle's gradient functions take a block with every adapter present and no bias
FULL = [n for n in ALL if all(r is not None for r in L.CASES[n]["ranks"]) and not L.CASES[n]["bias"]]
# An fp32 sum of K products whose rounding errors walk at random is off by about 2^-24 sqrt(K) times the size of what it sums; the
# blocked sums of a CPU GEMM stay below that. truth64 and the oracle differ by the oracle's share of it, through at most two
# dependent products per tensor: ORACLE_NOISE x 2^-24 sqrt(K) (||slice|| + rms of the tensor's slices), K = the block's longest
# contraction. Measured over the table (printed by the test): at most 0.34.
ORACLE_NOISE = 2
EPS16 = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}        # half an ulp at 1: the relative error of one rounding
FORWARD_BAND = (0.5, 8.0)                               # x EPS16 x ||slice||, the issue's band for the forward outputs
# The gradients, measured on the CPU over the whole table (printed by the test): the model's error per slice lies between 0.58
# and 3.3 x EPS16 x ||slice|| (dX 0.72 .. 3.25, dA 0.62 .. 3.09, dB 0.58 .. 3.08), the same size as the forward's 0.64 .. 3.6, so
# the same band holds them. (With M = 1 token dA and dB are one slice each: tests/_lora_blocks.py slices_of.)
GRADIENT_BAND = (0.5, 8.0)
MUTANT_MIN = L.MAX_FACTOR


def _norms(c, t):
    ref = c["truth"][t]
    return L.row_err(ref, torch.zeros_like(ref), L.slices_of(t, c["M"]))


def test_the_table_covers_what_it_has_to():
    C = L.CASES.values()
    assert 40 <= len(L.CASES) <= 75
    uniform = {c["ranks"][0] for c in C if len(set(c["ranks"])) == 1 and c["ranks"][0] is not None}
    assert {4, 8, 12, 16, 32, 64, 128} <= uniform
    assert {(8, 16, 64), (16, 8, 4), (64, 64, 64)} <= {c["ranks"] for c in C}
    assert {(16, None, 16), (16, None, None), (16, 16, None), (None, None, 16), (None, 16, None), (None, None, None),
            (None,)} <= {c["ranks"] for c in C}
    assert {1, 127, 129, 150, 257, 300} <= {c["M"] for c in C}
    for M in (127, 129):
        assert any(c["M"] == M and c["knobs"].get("FUSED_NF4_MAX_M") == 128 for c in C)
    assert {"swiglu", "geglu_exact", "geglu_approx"} <= {c["kind"] for c in C}
    assert {"bf16", "fp16"} <= {c["dtype"] for c in C}
    assert {"frozen", "train"} <= {c["bias"] for c in C}
    assert {True, False} <= {c["inplace"] for c in C} and {True, False} <= {c["quant"] for c in C}
    for block in L.PROJS:                               # every block on both GEMM families
        assert {"off", "on"} <= {c["knobs"]["GEMM256_MODE"] for c in C if c["block"] == block}
    for py in (L.TN, L.TERMS, ("lora_tn",)):            # the three MLP backward routes
        assert any(c["block"] == "mlp" and c["py"] == set(py) for c in C)
    for c in C:
        assert set(c["knobs"]) <= {"GEMM256_MODE", "FUSED_NF4", "FUSED_NF4_MAX_M", "GLU_FUSED", "GLU_TN", "LORA_XA_V2"}
        assert c["fwd"] <= set(L.GEMM.values()) and c["bwd"] <= set(L.GEMM.values()) and c["xa"] <= set(L.XA.values())
        assert c["py"] <= set(L.PY_ROUTES)


def test_cpu_nf4_quantiser_round_trips():
    """The weights of the NF4 cases: what the oracle decodes from the CPU-quantised bytes is NF4 of the weight (within one
    code step of it) in the activation dtype, and the state has the nested layout the kernels read."""
    W, pieces = L._weight("gate", True, "bf16")
    W0, _ = L._weight("gate", False, "bf16")
    assert W.dtype == torch.bfloat16 and W.shape == W0.shape
    packed, qs = L.quant_state(pieces)
    assert packed.shape == (W.numel() // 2, 1) and qs.nested and qs.blocksize == 64 and qs.state2.blocksize == 256
    blocks = W0.float().view(-1, 64)
    step = 0.17 * blocks.abs().amax(dim=1, keepdim=True)           # the widest gap between two NF4 levels, x absmax
    assert bool(((W.float().view(-1, 64) - blocks).abs() <= step).all())


@pytest.mark.parametrize("name", FULL)
def test_truth64_agrees_with_the_fp32_oracle(name):
    """R.lora_mlp_reference_grads / R.lora_linear_grads fed the factors rounded to the activation dtype (the oracle itself does
    not round them) against truth64, slice by slice, within the oracle's own fp32 summation noise."""
    c = L.build_case(name)
    dt = L.DTYPES[c["dtype"]]
    X, dYs, projs = L.case_inputs(name)
    cpu = {p: (W, A.to(dt), B.to(dt), s) for p, (W, _, A, B, s, _) in projs.items()}
    got = {}
    if c["block"] == "mlp":
        out, grads = R.lora_mlp_reference_grads(X, cpu["gate"], cpu["up"], cpu["down"], dYs["out"], c["kind"])
        got = dict(zip(["dX", "dA_gate", "dB_gate", "dA_up", "dB_up", "dA_down", "dB_down"], grads), out=out)
        K = L.I
    else:
        dX = 0
        for p, o in zip(L.PROJS[c["block"]], L.OUTPUTS[c["block"]]):
            dx, got[f"dA_{p}"], got[f"dB_{p}"] = R.lora_linear_grads(X, dYs[o], *cpu[p])
            dX = dX + dx
        got["dX"] = dX
        K = max(L.H, c["M"])
    worst = {}
    for t, g in got.items():
        err, norm = L.row_err(g, c["truth"][t], L.slices_of(t, c["M"])), _norms(c, t)
        assert bool((err[norm == 0] == 0).all()), t
        # (+ the rms over the tensor's slices, as tests/_attn_edges.py row_err: at M = 1 a rank row of dA is ONE number of
        # P = dY B times X, and where that dot product nearly cancels its own size says nothing about its error)
        scale = 2.0 ** -24 * math.sqrt(K) * (norm + norm.pow(2).mean().sqrt())
        worst[t] = float((err[norm > 0] / scale[norm > 0]).max())
    print(name, "oracle - truth64, x 2^-24 sqrt(K) ||slice||:", {t: round(v, 3) for t, v in worst.items()})
    assert max(worst.values()) <= ORACLE_NOISE, worst


@pytest.mark.parametrize("name", ALL)
def test_the_yardstick_is_usable(name):
    """The rounding model's error per slice: positive wherever the truth is not zero, exactly zero where it is, and of the size
    of 16-bit rounding -- the forward outputs within FORWARD_BAND, the gradients within GRADIENT_BAND x EPS16 x ||slice||."""
    c = L.build_case(name)
    spread = {}
    for t, ref in c["truth"].items():
        assert (ref is None) == (c["model"][t] is None), t
        if ref is None:
            continue
        assert c["model"][t].shape == ref.shape and bool(torch.isfinite(c["model"][t].float()).all()), t
        err, norm = c["model_err"][t], _norms(c, t)
        assert bool((err[norm == 0] == 0).all()), t
        if t.startswith("dbias_"):                   # one fp32 column sum, rounded once: its own bound, half an ulp of the sum
            assert float(err) <= EPS16[c["dtype"]] * float(norm)
            continue
        rel = err[norm > 0] / (EPS16[c["dtype"]] * norm[norm > 0])
        spread[t] = (float(rel.min()), float(rel.max()))
        lo, hi = FORWARD_BAND if t in L.OUTPUTS[c["block"]] else GRADIENT_BAND
        assert lo <= spread[t][0] and spread[t][1] <= hi, (t, spread[t])
    print(name, "model error, x EPS16 ||slice||:", {t: (round(a, 2), round(b, 2)) for t, (a, b) in spread.items()})


@pytest.mark.parametrize("name", [n for n in ALL if L.mutants(n)])
def test_every_mutant_is_rejected(name):
    c = L.build_case(name)
    seen = {}
    for mutant in L.mutants(name):
        res = L.rounding_model(name, mutant)
        ratios = {t: L.judge(c, t, res[t])[2] for t in res if c["truth"][t] is not None and res[t] is not None}
        t = max(ratios, key=ratios.get)
        seen[mutant] = (t, ratios[t])
    print(name, {f"{k}:{p}": (t, round(v, 1)) for (k, p), (t, v) in seen.items()})
    for mutant, (t, ratio) in seen.items():
        assert ratio > MUTANT_MIN, (mutant, t, ratio)


def test_the_rounding_model_passes_its_own_bound():
    for name in ("mlp-r16-plain", "qkv-r16", "w-r16"):
        c = L.build_case(name)
        for t, m in c["model"].items():
            if m is not None:
                err, model, ratio, ok = L.judge(c, t, m)
                assert ok and ratio <= 1.0 and torch.equal(err, model), t


def test_row_err_and_judge_on_hand_written_slices():
    ref = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    got = torch.tensor([[3.0, 4.0], [0.0, 2.0], [0.0, 0.0]])
    assert L.row_err(got, ref, "row").tolist() == [0.0, 2.0, 1.0]
    assert L.row_err(got, ref, "col").tolist() == [1.0, 2.0]
    assert L.row_err(got, ref, "all").tolist() == [math.sqrt(5.0)]
    assert (L.slices_of("dA_q"), L.slices_of("dB_q"), L.slices_of("dbias_q"), L.slices_of("dX"), L.slices_of("Q")) == \
        ("row", "col", "all", "row", "row")
    assert (L.slices_of("dA_q", 1), L.slices_of("dB_q", 1), L.slices_of("dX", 1), L.slices_of("dA_q", 2)) == \
        ("all", "all", "row", "row")
    # a token whose dY is zero: its dX row is exactly zero in the truth and in the model, and anything else there fails
    c = L.build_case("w-r16")
    row = c["M"] // 2
    assert float(c["truth"]["dX"][row].abs().max()) == 0.0 and float(c["model"]["dX"][row].abs().max()) == 0.0
    dust = c["model"]["dX"].clone()
    assert L.judge(c, "dX", dust)[3]
    dust[row, 0] = 1e-30
    assert not L.judge(c, "dX", dust)[3] and L.judge(c, "dX", dust)[2] == float("inf")
