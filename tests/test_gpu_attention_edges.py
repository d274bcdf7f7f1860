"""-m gpu: the mask edges of the attention kernels (csrc/attention.hip, csrc/attn_kd4_loop.inc) with the softmax mass placed ON them.

Every other masked attention test feeds randn: the mass is spread over the band and a key wrongly taken in or left out at an edge
moves 1/n of a row. Here (tests/_attn_edges.py) the oldest / newest allowed key of a row holds most of its mass and the first
forbidden key beside it would hold more, so an off-by-one in any of the five places that decide which keys a query sees changes
whole rows of O, dQ, dK and dV. Each output is judged row by row against an fp64 reference, and the bound is 4 x what a plain fp32
model with the kernels' documented 16-bit rounding points loses on the same inputs -- a multiple of the reference side's error,
not of anything the kernels produce. tests/test_attention_edge_inputs.py shows on the host that every off-by-one mask lies at
least 3 x above that bound. The measured ratios go to attention_edge_report.json in the directory UAMD_REPORT_DIR names (default:
test_reports/ in the repository root, git-ignored); profiles/attention_edge_report.json is a committed copy of one MI355X run."""
import json
import os

import pytest
import torch

from tests import _attn_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}

CASE_DTYPE = [(n, d) for n in E.CASES for d in E.DTYPES]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "attention_edge_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _on_gpu(c):
    """Q / K / V as column slices of one [B, T, (Hq + 2 Hk) D] buffer (the fused QKV projection's layout), dO, and the product's band."""
    from unsloth_amd.kernels.attention import attention_band, document_band
    B, T, Hq, Hk, D = c["shape"]
    qkv = torch.cat([c[x].flatten(2) for x in ("q", "k", "v")], dim=-1).to(DEV)
    q = qkv[..., :Hq * D].view(B, T, Hq, D)
    k = qkv[..., Hq * D:(Hq + Hk) * D].view(B, T, Hk, D)
    v = qkv[..., (Hq + Hk) * D:].view(B, T, Hk, D)
    if not c["causal"]:
        band = document_band(T, batch=B, seq_lengths=c["lengths"], device=DEV)
    elif c["lengths"] or c["window"]:
        band = attention_band(T, batch=B, seq_lengths=c["lengths"], sliding_window=c["window"], device=DEV)
    else:
        band = None
    if band is not None:           # the kernels get the product's band, the reference the helper's: the same band
        assert torch.equal(band[0].cpu().long(), c["lo"]) and torch.equal(band[1].cpu().long(), c["hi"])
    return q, k, v, c["do"].to(DEV), band


def _hold(c, name, dtype_name, variant, tensor, got):
    assert not torch.isnan(got.float()).any(), (tensor, "NaN")
    err, model, ok = E.judge(c, tensor, got)
    ratio = err / model if model > 0 else (0.0 if err == 0 else float("inf"))       # (window 1: the model's O and dV are exact)
    REPORT[f"{name}/{dtype_name}/{variant}/{tensor}"] = dict(kernel=err, model=model, ratio=ratio)
    print(f"{name}/{dtype_name}/{variant}/{tensor}: kernel {err:.3e} model {model:.3e} ratio {ratio:.2f}")
    return None if ok else (tensor, err, model, ratio)


@pytest.mark.parametrize("var,variant", [(1, "one_block_per_item"), (2, "persistent_claimed"), (10, "persistent_static")])
@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_forward_on_edge_inputs(name, dtype_name, var, variant):
    """UAMD_TUNE_ATTN_VAR 1 / 2 / 10: attn_fwd_kernel, attn_fwd_ps_kernel with claimed items, with the static deal (the host takes
    the persistent kernel only for causal head_dim-128 launches; every other case runs one block per item under all three)."""
    from unsloth_amd import _lib
    from unsloth_amd.kernels.attention import attn_forward
    c = E.build_case(name, dtype_name)
    q, k, v, _, band = _on_gpu(c)
    L = _lib.lib()
    try:
        assert L.uamd_set_tuning(4, var) == 0
        o, lse = attn_forward(q, k, v, c["scale"], band, c["causal"])
        o, lse = o.cpu(), lse.cpu()
    finally:
        L.uamd_set_tuning(4, 0)
    assert not torch.isnan(lse).any()
    torch.testing.assert_close(lse.double(), c["ref"]["lse"], rtol=1e-4, atol=2e-3)
    bad = _hold(c, name, dtype_name, variant, "o", o)
    assert bad is None, bad
    if c["window"] == 1:
        # one key per row: P = 1 and l = 1 exactly, O is V of the row's KV head bit for bit
        G = c["shape"][2] // c["shape"][3]
        assert torch.equal(o, c["v"].repeat_interleave(G, dim=2))


@pytest.mark.parametrize("var,variant", [(0, "generated_loops"), (4, "cxx_body")])
@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_backward_on_edge_inputs(name, dtype_name, var, variant):
    """attn_bwd_dq_kernel + attn_bwd_dkdv4_kernel behind the default forward; UAMD_TUNE_ATTN_VAR bit 2 sends every dK / dV step
    through the C++ body instead of the generated loops of attn_kd4_loop.inc."""
    from unsloth_amd import _lib
    from unsloth_amd.kernels.attention import attn_backward, attn_forward
    c = E.build_case(name, dtype_name)
    B, T, Hq, Hk, D = c["shape"]
    G = Hq // Hk
    q, k, v, do, band = _on_gpu(c)
    L = _lib.lib()
    o, lse = attn_forward(q, k, v, c["scale"], band, c["causal"])
    try:
        assert L.uamd_set_tuning(4, var) == 0
        dq, dk, dv = (t.cpu() for t in attn_backward(do, q, k, v, o, lse, c["scale"], band, c["causal"]))
    finally:
        L.uamd_set_tuning(4, 0)
    if c["window"] != 1:
        bad = [b for b in (_hold(c, name, dtype_name, variant, t, g) for t, g in (("dq", dq), ("dk", dk), ("dv", dv))) if b]
        assert not bad, bad
        return
    bad = _hold(c, name, dtype_name, variant, "dv", dv)
    assert bad is None, bad
    # one key per row, P = 1: dV is the sum of the group's dO, formed in fp32 and rounded once
    want = c["do"].float().view(B, T, Hk, G, D).sum(3).to(c["dtype"])
    assert torch.equal(dv, want)
    # dS = P (dP - Delta) with dP = dO . v and Delta = dO . O = dO . v: zero in exact arithmetic. What a kernel may leave is
    # the fp32 error of those two length-D dot products, each at most D 2^-24 sum_i |dO_i v_i| whatever the order of the sum, so
    # |dS| <= 2 D 2^-24 sum_i |dO_i v_i| per (row, head). dQ = scale dS k has one term per row: ||dq_row|| <= scale ||k_row|| |dS|;
    # dK sums the group's heads: ||dk_row|| <= scale sum_h ||q_row_h|| |dS_h|.
    d64, v64 = c["do"].double(), c["v"].double().repeat_interleave(G, dim=2)
    ds = 2.0 * D * 2.0 ** -24 * (d64 * v64).abs().sum(-1)                                    # [B, T, Hq]
    dq_bound = c["scale"] * c["k"].double().repeat_interleave(G, dim=2).norm(dim=-1) * ds
    dk_bound = c["scale"] * (c["q"].double().norm(dim=-1) * ds).view(B, T, Hk, G).sum(-1)
    for t, got, bound in (("dq", dq, dq_bound), ("dk", dk, dk_bound)):
        assert not torch.isnan(got.float()).any(), t
        norm = got.double().norm(dim=-1)
        REPORT[f"{name}/{dtype_name}/{variant}/{t}"] = dict(kernel_max_row_norm=float(norm.max()), bound_min=float(bound.min()),
                                                            worst_fraction_of_bound=float((norm / bound).max()))
        assert bool((norm <= bound).all()), (t, float((norm / bound).max()))


@pytest.mark.parametrize("dtype_name", list(E.DTYPES))
@pytest.mark.parametrize("name", ["packed_d64", "docs_nc_d80", "packed_d36"])
def test_flash_attention_autograd_on_edge_inputs(name, dtype_name):
    """Through FlashAttention.apply: native head dims, and with head_dim 36 the saved-padded-operands path of its backward."""
    from unsloth_amd.kernels.attention import flash_attention, native
    c = E.build_case(name, dtype_name)
    q, k, v, do, band = _on_gpu(c)
    assert native(q, k, v) == (c["shape"][4] % 8 == 0)
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o = flash_attention(q, k, v, c["scale"], band, c["causal"])
    o.backward(do)
    got = (("o", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad))
    bad = [b for b in (_hold(c, name, dtype_name, "autograd", t, g.cpu()) for t, g in got) if b]
    assert not bad, bad
