"""-m gpu: Qwen3's fused per-head RMSNorm + RoPE kernels (csrc/qk_norm_rope.hip) against a plain fp64 reference (the norm, the
rotation, torch autograd), on the strided q|k|v views of ONE fused projection buffer with non-unit norm weights, a row of zeros
(r = rsqrt(eps), finite output and gradient) and a row spanning 2^-12 .. 2^8. Bounds per (token, head) row (_attn_edges.row_err):
forward BOUND_FACTOR x the error of `rounded`, the documented roundings restated on the host; backward BOUND_FACTOR x the error of
the fp64 gradient rounded once to the 16-bit type; r 2e-6 relative (an fp32 tree sum of D squares: <= 14 roundings of 2^-24, halved
by the rsqrt, + 2 ulp). The decode append kernel's q and key must be bit-equal to the training kernel's on the same token."""
import pytest
import torch

from tests._attn_edges import BOUND_FACTOR, row_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = {1: (1, 1), 3: (1, 3), 65: (5, 13)}        # B.T -> (B, T): one row alone, less than a wave's rows, a ragged last workgroup
POSITIONS = 97


def _inputs(D, Hq, Hk, dt, B, T, gather, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * D + 17 * Hq + B * T)
    N, H = B * T, Hq + 2 * Hk
    qkv = torch.randn(N, H, D, generator=g)
    qkv[0, 0] = 0                                                                    # a q row of zeros
    qkv[0, Hq + Hk - 1] = torch.exp2(torch.rand(D, generator=g) * 20 - 12) * (torch.randint(0, 2, (D,), generator=g) * 2 - 1)
    w = torch.rand(2, D, generator=g) * 1.5 + 0.25                                   # q_norm, k_norm weights
    ang = torch.arange(POSITIONS)[:, None] * (1e4 ** (-torch.arange(D // 2) * 2.0 / D))[None]
    idx = torch.randint(0, POSITIONS, (N,), generator=g, dtype=torch.int32) if gather else None
    dy = torch.randn(N, Hq + Hk, D, generator=g)
    to = lambda t: t.to(dt).to(DEV)
    return to(qkv.reshape(N, H * D)), to(w), to(ang.cos()), to(ang.sin()), None if idx is None else idx.to(DEV), to(dy)


def _rotate(z, c, s, rn=lambda t: t):
    z1, z2 = z.chunk(2, -1)
    return torch.cat([rn(rn(z1 * c) - rn(z2 * s)), rn(rn(z2 * c) + rn(z1 * s))], -1)


def ref64(x, w, c, s):
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
    return _rotate(x * r * w, c, s), r


def rounded(x, w, c, s, dt):             # the documented rounding points on the host, fp64 arithmetic between them
    rn = lambda t: t.to(dt).double()
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + EPS).double()
    return _rotate(rn(rn(x * r) * w), c, s, rn)


@pytest.mark.parametrize("gather", [False, True], ids=["rows", "gathered"])
@pytest.mark.parametrize("BT", list(SHAPES))
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("Hq,Hk", [(4, 2), (7, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_forward_and_backward_against_fp64(D, Hq, Hk, dtype_name, BT, gather):
    from unsloth_amd.kernels import fast_qk_norm_rope_embedding
    from unsloth_amd.kernels.rope_embedding import qk_norm_rope_fwd_
    dt, (B, T) = DTYPES[dtype_name], SHAPES[BT]
    qkv0, w, cos, sin, idx, dy = _inputs(D, Hq, Hk, dt, B, T, gather)
    nq, nk = Hq * D, Hk * D
    qkv = (leaf := qkv0.clone().requires_grad_(True)) * 1       # the fused projection output the kernel overwrites
    Q, K = (qkv[:, a:b].view(B, T, h, D).transpose(1, 2) for a, b, h in ((0, nq, Hq), (nq, nq + nk, Hk)))
    Qo, Ko = fast_qk_norm_rope_embedding(Q, K, w[0], w[1], EPS, cos, sin, idx)
    assert Qo.data_ptr() == qkv.data_ptr() and Ko.data_ptr() == qkv.data_ptr() + nq * qkv.element_size() and \
        torch.equal(qkv[:, nq + nk:], qkv0[:, nq + nk:]), "not in place, or v was touched"
    got = qkv.detach()[:, :nq + nk].reshape(B * T, Hq + Hk, D)
    x64 = qkv0[:, :nq + nk].reshape(B * T, Hq + Hk, D).double().cpu().requires_grad_(True)
    w64 = torch.cat([w[:1].expand(Hq, D), w[1:].expand(Hk, D)]).double().cpu()
    pos = (idx.long() if gather else torch.arange(B * T, device=DEV) % T).cpu()
    c64, s64 = cos.double().cpu()[pos][:, None], sin.double().cpu()[pos][:, None]
    ref, r64 = ref64(x64, w64, c64, s64)
    err, model = row_err(got, ref), row_err(rounded(x64.detach(), w64, c64, s64, dt), ref.detach())
    assert torch.isfinite(got).all() and not bool(got[0, 0].any()) and err <= BOUND_FACTOR * model, (err, model)
    again = qkv0.clone()                                        # what the launch keeps for the backward: r and the pre-norm rows
    ctx_r, ctx_x = qk_norm_rope_fwd_(again[:, :nq].view(B, T, Hq, D).transpose(1, 2), again[:, nq:nq + nk].view(B, T, Hk, D).transpose(1, 2),
                                     w[0], w[1], EPS, cos, sin, idx, True)
    assert torch.equal(again, qkv.detach()) and torch.equal(ctx_x, qkv0[:, :nq + nk].reshape(B * T, Hq + Hk, D))
    r_err = float(((ctx_r.double().cpu() - r64.detach()[..., 0]) / r64.detach()[..., 0]).abs().max())
    assert r_err <= 2e-6 and abs(float(ctx_r[0, 0]) - EPS ** -0.5) <= 2e-6 * EPS ** -0.5, r_err
    dy64, dy4 = dy.double().cpu(), dy.view(B, T, Hq + Hk, D)
    ((Qo.transpose(1, 2) * dy4[:, :, :Hq]).sum() + (Ko.transpose(1, 2) * dy4[:, :, Hq:]).sum()).backward()
    assert not bool(leaf.grad[:, nq + nk:].any())
    dgot = leaf.grad[:, :nq + nk].reshape(B * T, Hq + Hk, D)
    (dref,) = torch.autograd.grad((ref * dy64).sum(), x64)
    derr, dmodel = row_err(dgot, dref), row_err(dref.to(dt), dref)
    assert torch.isfinite(dgot).all() and derr <= BOUND_FACTOR * dmodel, (derr, dmodel)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("D", [64, 128])
def test_decode_append_is_bit_equal_to_the_training_kernel(D, dtype_name):           # cache lengths 0, 5 and s_max (no write)
    from unsloth_amd.kernels import decode as dk, fast_qk_norm_rope_embedding
    dt, Hq, Hk, S = DTYPES[dtype_name], 4, 2, 8
    qkv0, w, cos, sin, _, _ = _inputs(D, Hq, Hk, dt, 3, 1, False, seed=7)
    kv_len = torch.tensor([0, 5, S], dtype=torch.int32, device=DEV)
    nq, nk = Hq * D, Hk * D
    train = qkv0.clone()
    fast_qk_norm_rope_embedding(train[:, :nq].view(3, 1, Hq, D).transpose(1, 2), train[:, nq:nq + nk].view(3, 1, Hk, D).transpose(1, 2),
                                w[0], w[1], EPS, cos, sin, kv_len)
    step, kc = qkv0.clone(), torch.full((3, Hk, S, D), 7.0, dtype=dt, device=DEV)
    vc = kc.clone()
    dk.qk_norm_rope_kv_append(step, w[0], w[1], EPS, cos, sin, kv_len, kc, vc, Hq, Hk, D)
    assert torch.equal(step, train) and not torch.equal(step[:, :nq + nk], qkv0[:, :nq + nk])
    for b, L in enumerate(kv_len.tolist()):
        want_k, want_v = torch.full_like(kc[b], 7.0), torch.full_like(vc[b], 7.0)
        if L < S:
            want_k[:, L], want_v[:, L] = train[b, nq:nq + nk].view(Hk, D), qkv0[b, nq + nk:].view(Hk, D)
        assert torch.equal(kc[b], want_k) and torch.equal(vc[b], want_v), b
