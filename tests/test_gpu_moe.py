"""The MoE expert block (csrc/moe.hip, kernels/moe.py) against an fp64 restatement of transformers' Qwen3MoeExperts loop.

Shapes: H = 128, I = 192 (an N edge inside a 128-column tile, three K steps), E = 8, k = 2, T = 200. The routing is written by
hand: expert 7 has no token, expert 6 exactly one, expert 5 has 129 rows (one more than a row tile) and one slot carries the id E,
HF's sentinel for a masked expert, which contributes nothing."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests._util import EPS, rel_fro
from unsloth_amd.kernels import moe_experts_forward, moe_grouped_gemm, moe_plan, patch_moe_experts
from unsloth_amd.models.llama import unpatch_all

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
T, K_TOP, E, H, I = 200, 2, 8, 128, 192


def _routing():
    idx = torch.empty(T, K_TOP, dtype=torch.int64)
    idx[:, 0] = torch.arange(T) % 4
    idx[:, 1] = 4
    idx[:129, 1] = 5
    idx[150, 1] = 6
    idx[160, 1] = E
    return idx


def _sorted_rows(idx):
    flat = idx.reshape(-1)
    order = torch.sort(flat, stable=True).indices
    return order[flat[order] < E]


def _experts64(x, gu, dn, idx, w):
    """The HF loop, fp64: out[t] = sum_j w[t, j] * down_e(silu(gate_e x_t) * up_e x_t), a slot with id E skipped."""
    out = torch.zeros_like(x)
    for e in range(E):
        j, t = torch.where((idx == e).T)
        gate, up = F.linear(x[t], gu[e]).chunk(2, dim=-1)
        out = out.index_add(0, t, F.linear(F.silu(gate) * up, dn[e]) * w[t, j, None])
    return out


@functools.lru_cache(maxsize=None)
def _case(dtype):
    """Inputs in `dtype` on the CPU (weights scaled so that activations stay O(1); routing weights positive, rows summing to 1),
    and the fp64 truth of the output, d hidden and d top_k_weights for the upstream gradient dOut."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T, H, generator=g).to(dtype)
    gu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dtype)
    dn = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(dtype)
    w = torch.rand(T, K_TOP, generator=g) + 0.1
    w = (w / w.sum(-1, keepdim=True)).to(dtype)
    dout = torch.randn(T, H, generator=g).to(dtype)
    idx = _routing()
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    out64 = _experts64(x64, gu.double(), dn.double(), idx, w64)
    dx64, dw64 = torch.autograd.grad(out64, (x64, w64), dout.double())
    return dict(x=x, gu=gu, dn=dn, w=w, dout=dout, idx=idx, truth=(out64.detach(), dx64, dw64))


def _run(fn, c, n=T):
    """(out, d hidden, d top_k_weights) of fn(hidden, gate_up, down, index, weights) on the GPU for the first n tokens."""
    x, w = c["x"][:n].cuda().requires_grad_(), c["w"][:n].cuda().requires_grad_()
    out = fn(x, c["gu"].cuda(), c["dn"].cuda(), c["idx"][:n].cuda(), w)
    return (out.detach(), *torch.autograd.grad(out, (x, w), c["dout"][:n].cuda()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gather,scatter,scale,acc", [(0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1), (1, 1, 1, 1)])
@pytest.mark.parametrize("form,N,K", [("nt", 192, 128), ("nt", 128, 192), ("nn", 192, 128), ("nn", 128, 192)])
def test_grouped_gemm_rows_against_fp64(form, N, K, gather, scatter, scale, acc, dtype):
    g = torch.Generator().manual_seed(11)
    idx, S = _routing(), T * K_TOP
    A = torch.randn(T if gather else S, K, generator=g).to(dtype)
    W = (torch.randn(E, *((N, K) if form == "nt" else (K, N)), generator=g) / K ** 0.5).to(dtype)
    rs = torch.rand(S, generator=g) + 0.5 if scale else None
    C0 = torch.randn(S, N, generator=g).to(dtype) if acc else torch.full((S, N), 7.0, dtype=dtype)
    rows = _sorted_rows(idx)
    plan = moe_plan(idx.cuda(), E)
    assert torch.equal(plan.rows[:len(rows)].cpu().long(), rows)
    C = moe_grouped_gemm(A.cuda(), W.cuda(), plan, C0.clone().cuda(), form=form, gather=bool(gather), scatter=bool(scatter),
                         row_scale=None if rs is None else rs.cuda(), accumulate=bool(acc)).cpu()
    s = torch.arange(len(rows))
    a_row, c_row, e = (rows // K_TOP if gather else s), (rows if scatter else s), idx.reshape(-1)[rows]
    W64 = W.double() if form == "nn" else W.double().transpose(1, 2)
    ref = torch.stack([A[a].double() @ W64[x] for a, x in zip(a_row.tolist(), e.tolist())])
    if scale:
        ref = ref * rs[rows, None].double()
    if acc:
        ref = ref + C0[c_row].double()
    # one rounding of an fp32 sum to the dtype: at most eps / 2 per element; fp32 accumulation over K <= 192 is far below it
    assert rel_fro(C[c_row], ref) <= EPS[dtype]
    untouched = torch.ones(S, dtype=torch.bool)
    untouched[c_row] = False
    assert untouched.sum() == 1 and torch.equal(C[untouched], C0[untouched])


@pytest.mark.parametrize("dtype", DTYPES)
def test_experts_forward_and_backward_no_worse_than_hf(dtype):
    """Error against the fp64 truth at most 1.5 x the error of HF's own loop in the same dtype on the same GPU: both round e, g,
    h and y at the same points, the new path sums the k slots in fp32 where HF sums in 16 bits, so it should sit at or below
    1.0; the margin covers the MFMA summation order. Measured on an MI355X, relative Frobenius error new / HF:
    bf16 out 4.26e-3 / 4.65e-3, d hidden 4.42e-3 / 4.55e-3, d top_k_weights 4.34e-3 / 4.64e-3;
    fp16 out 5.32e-4 / 5.74e-4, d hidden 5.44e-4 / 5.69e-4, d top_k_weights 5.13e-4 / 5.68e-4."""
    from transformers.models.qwen3_moe.configuration_qwen3_moe import Qwen3MoeConfig
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts
    c = _case(dtype)
    cfg = Qwen3MoeConfig(hidden_size=H, moe_intermediate_size=I, num_experts=E, num_experts_per_tok=K_TOP, hidden_act="silu")
    cfg._experts_implementation = "eager"
    hf = Qwen3MoeExperts(cfg).to(dtype).cuda().requires_grad_(False)

    def hf_loop(x, gu, dn, idx, w):
        # this transformers' one_hot(num_classes = E) refuses the sentinel id it later tests for, so HF gets the masked slot
        # as expert 0 with weight 0: the same function of hidden and of the other weights, and a zero gradient at that slot
        hf.gate_up_proj.copy_(gu), hf.down_proj.copy_(dn)
        return hf(x, idx.clamp(max=E - 1) * (idx < E), w * (idx < E))

    new, old = _run(moe_experts_forward, c), _run(hf_loop, c)
    for name, a, b, truth in zip(("out", "d hidden", "d top_k_weights"), new, old, c["truth"]):
        err_new, err_hf = rel_fro(a, truth), rel_fro(b, truth)
        print(f"moe {dtype} {name}: new {err_new:.3e} hf {err_hf:.3e}")
        assert err_new <= 1.5 * err_hf, (name, err_new, err_hf)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_independent_and_runs_are_bit_equal(dtype):
    c = _case(dtype)
    full, again, head = _run(moe_experts_forward, c), _run(moe_experts_forward, c), _run(moe_experts_forward, c, n=64)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    assert torch.equal(head[0], full[0][:64])


@pytest.mark.parametrize("dtype", DTYPES)
def test_patched_sparse_moe_block(dtype):
    """A tiny Qwen3MoeSparseMoeBlock, router included: the patched block in `dtype` against the unpatched block in fp64, held to
    1.5 x the error of the unpatched block in `dtype` (the router, and so the routing, is the same code in both)."""
    from transformers.models.qwen3_moe import modeling_qwen3_moe as hf
    from transformers.models.qwen3_moe.configuration_qwen3_moe import Qwen3MoeConfig
    cfg = Qwen3MoeConfig(hidden_size=128, moe_intermediate_size=64, num_experts=8, num_experts_per_tok=2, hidden_act="silu",
                         norm_topk_prob=True)
    cfg._experts_implementation = "eager"
    torch.manual_seed(3)
    block = hf.Qwen3MoeSparseMoeBlock(cfg)
    with torch.no_grad():
        for p in block.parameters():
            p.copy_(torch.randn_like(p) / p.shape[-1] ** 0.5)
    block = block.to(dtype)                                   # the 16-bit values are the inputs of all three runs
    block.experts.requires_grad_(False)
    x = torch.randn(2, 37, 128).to(dtype)
    dout = torch.randn(2, 37, 128).to(dtype)

    def run(b, cast):
        b.zero_grad()
        xx = cast(x).requires_grad_()
        out = b(xx)
        out.backward(cast(dout))
        return out.detach(), xx.grad, b.gate.weight.grad.clone()

    original = hf.Qwen3MoeExperts.forward
    truth = run(block.double(), lambda t: t.double())
    block = block.to(dtype).cuda()
    base = run(block, lambda t: t.cuda())
    try:
        patch_moe_experts()
        assert hf.Qwen3MoeExperts.forward is not original
        got = run(block, lambda t: t.cuda())
    finally:
        unpatch_all()
    assert hf.Qwen3MoeExperts.forward is original
    for name, a, b, t in zip(("out", "d hidden", "d router weight"), got, base, truth):
        assert rel_fro(a, t) <= 1.5 * rel_fro(b, t), (name, rel_fro(a, t), rel_fro(b, t))
