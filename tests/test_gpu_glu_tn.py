"""-m gpu: the SwiGLU backward that also forms the MLP's three wide LoRA gradients (uamd_glu_bwd_tn_ws, csrc/glu.hip
glu_tn_kernel + glu_tn_reduce_kernel): df / de BIT-IDENTICAL to the plain activation kernel and DW untouched, the row
products equal to the separate uamd_lora_xa2 launches and the gradients equal to uamd_lora_tn on the plain kernel's h, df, de
up to fp32 summation order, accumulation a plain +=, run-to-run bitwise, and the whole LoRA_MLP block unchanged within the
bound of tests/test_gpu_glu_fused.py."""
import pytest
import torch

from tests._util import rel_fro

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S = 2.0


def _proj(n_out, n_in, r, g, dtype):
    W = (torch.randn(n_out, n_in, generator=g) * 0.02).to(dtype).to(DEV)
    A = (torch.randn(r, n_in, generator=g) * 0.02).to(DEV)
    B = (torch.randn(n_out, r, generator=g) * 0.02).to(DEV)
    return (W, None, A, B, S)


@pytest.fixture(autouse=True)
def _any_size():
    from unsloth_amd.kernels import utils as U
    keep = U.GLU_FUSED, U.GLU_TN
    U.GLU_FUSED, U.GLU_TN = "all", True         # the direct calls below must not be refused by the size policy
    yield
    U.GLU_FUSED, U.GLU_TN = keep


def _inputs(M, K, r, dtype, halves=False, act_ranks=None):
    """Seeded inputs as in tests/test_gpu_glu_fused.py. `halves`: e | g are the column halves of ONE buffer with ld = 2 K + 64
    (fast_lora._gate_up) and DW sits on the same row stride."""
    g_ = torch.Generator().manual_seed(M + K)
    e = torch.randn(M, K, generator=g_).to(dtype).to(DEV)
    g = torch.randn(M, K, generator=g_).to(dtype).to(DEV)
    DW = (torch.randn(M, K, generator=g_) * 0.1).to(dtype).to(DEV)
    H = 512
    ru, rg, rd = act_ranks or (r, r, r)
    down, up, gate = _proj(H, K, rd, g_, dtype), _proj(K, H, ru, g_, dtype), _proj(K, H, rg, g_, dtype)
    X = torch.randn(M, H, generator=g_).to(dtype).to(DEV)
    dY = (torch.randn(M, H, generator=g_) * 0.1).to(dtype).to(DEV)
    p_d = dY.float() @ down[3].to(dtype).float()                    # [M, r]: dY @ B_down
    xa_u = X.float() @ up[2].to(dtype).float().t()                  # X @ A_up^T
    xa_g = X.float() @ gate[2].to(dtype).float().t()
    if halves:
        ld = 2 * K + 64
        eg = torch.full((M, ld), 3.0, dtype=dtype, device=DEV)
        eg[:, :K], eg[:, K:2 * K] = e, g
        dwb = torch.full((M, ld), 5.0, dtype=dtype, device=DEV)
        dwb[:, :K] = DW
        e, g, DW = eg[:, :K], eg[:, K:2 * K], dwb[:, :K]
        DW._whole, e._whole = dwb, eg
    return DW, e, g, up, gate, down, p_d, xa_u, xa_g


def _tn_truth(P, Z, dtype, out_nr):
    """fp64 product of the operands as the kernels round them: s * T(P)^T @ Z"""
    t = S * (P.to(dtype).double().t() @ Z.double())
    return t.t() if out_nr else t


CASES = [(17, 264, 16, False), (300, 1024, 8, False), (33, 520, 16, False), (513, 264, 16, False), (1000, 5632, 16, False),
         (2048, 14336, 16, False), (64, 512, 16, True)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,K,r,halves", CASES)
def test_activation_row_products_and_gradients(M, K, r, halves, dtype):
    from unsloth_amd.kernels import utils as U
    from unsloth_amd.kernels.swiglu import swiglu_DWf_DW_dfg_kernel
    DW, e, g, up, gate, down, p_d, xa_u, xa_g = _inputs(M, K, r, dtype, halves)
    # the plain kernel (flat buffers) and the launches the new path replaces
    h, df, de = swiglu_DWf_DW_dfg_kernel(DW.contiguous().clone(), e.contiguous().clone(), g.contiguous().clone())
    tu, tg = U.lora_dx_terms([df, de], [up, gate])
    ref = U.lora_tn([(p_d, h, r, False, S), (xa_u, df, r, True, S), (xa_g, de, r, True, S)])
    dwb0 = DW._whole.clone() if halves else None
    DW0 = DW.clone()
    res = U.glu_bwd_tn("swiglu", DW, e, g, up, gate, down, p_d, xa_u, xa_g)
    assert res is not None
    df2, de2, (pu, pg), grads = res
    # element-wise: bit-identical, DW read-only
    assert torch.equal(df2, df) and torch.equal(de2, de) and torch.equal(DW, DW0)
    assert df2.data_ptr() == e.data_ptr() and de2.data_ptr() == g.data_ptr()
    if halves:                                   # nothing outside the [M, K] views was written
        assert e.stride(0) == 2 * K + 64 and torch.equal(DW._whole, dwb0) and torch.all(e._whole[:, 2 * K:] == 3.0)
    # row products
    assert rel_fro(pu.P, tu.P) < 1e-5 and rel_fro(pg.P, tg.P) < 1e-5
    for p_new, p_ref, Z, B in ((pu.P, tu.P, df, up[3]), (pg.P, tg.P, de, gate[3])):
        truth = Z.double() @ B.to(dtype).double()
        e_new, e_ref = rel_fro(p_new.double(), truth), rel_fro(p_ref.double(), truth)
        print(f"row product: new {e_new:.3e} existing {e_ref:.3e}")
        assert e_new <= 2 * e_ref + 1e-6
    assert (pu.xk is None) == (tu.xk is None)
    if pu.xk is not None:
        assert pu.xk is pg.xk and pu.col == tu.col and pg.col == tg.col and pu.xk.shape == tu.xk.shape
        assert torch.all(pu.xk[:, 2 * r:] == 0)
        assert rel_fro(pu.xk.float(), tu.xk.float()) < 2e-3
    # the three gradients
    for name, got, want, P, Z, nr in (("dA_down", grads[0], ref[0], p_d, h, False), ("dB_up", grads[1], ref[1], xa_u, df, True),
                                      ("dB_gate", grads[2], ref[2], xa_g, de, True)):
        assert got.shape == want.shape and got.dtype == torch.float32
        truth = _tn_truth(P, Z, dtype, nr)
        e_new, e_ref, d = rel_fro(got.double(), truth), rel_fro(want.double(), truth), rel_fro(got, want)
        print(f"{name}: vs lora_tn {d:.3e}, vs fp64 new {e_new:.3e} lora_tn {e_ref:.3e}")
        assert d < 1e-5, name
        assert e_new <= 2 * e_ref + 1e-6, name


@pytest.mark.parametrize("M,K,ranks,act", [(5, 8, (4, 4, 4), "swiglu"), (300, 1024, (32, 32, 32), "swiglu"),
                                           (300, 1024, (16, 16, 32), "swiglu"), (300, 1024, (16, 16, 16), "geglu_exact"),
                                           (300, 1024, (16, 16, 16), "geglu_approx")])
def test_shapes_not_taken_return_none_and_touch_nothing(M, K, ranks, act):
    from unsloth_amd.kernels import utils as U
    DW, e, g, up, gate, down, p_d, xa_u, xa_g = _inputs(M, K, None, torch.bfloat16, act_ranks=ranks)
    keep = [t.clone() for t in (DW, e, g)]
    assert U.glu_bwd_tn(act, DW, e, g, up, gate, down, p_d, xa_u, xa_g) is None
    assert all(torch.equal(a, b) for a, b in zip((DW, e, g), keep))


def test_switch_off_returns_none():
    from unsloth_amd.kernels import utils as U
    DW, e, g, up, gate, down, p_d, xa_u, xa_g = _inputs(300, 1024, 16, torch.bfloat16)
    U.GLU_TN = False
    assert U.glu_bwd_tn("swiglu", DW, e, g, up, gate, down, p_d, xa_u, xa_g) is None


def test_accumulate_is_a_plain_add_and_runs_are_bitwise_equal():
    from unsloth_amd.kernels import utils as U
    M, K, r = 1000, 5632, 16
    DW, e, g, up, gate, down, p_d, xa_u, xa_g = _inputs(M, K, r, torch.bfloat16)
    runs = []
    for _ in range(4):
        df, de, (pu, pg), grads = U.glu_bwd_tn("swiglu", DW, e.clone(), g.clone(), up, gate, down, p_d, xa_u, xa_g)
        xk = pu.xk if pu.xk is not None else pu.P
        runs.append([df.clone(), de.clone(), pu.P.clone(), pg.P.clone(), xk.clone()] + [x.clone() for x in grads])
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
    g_ = torch.Generator().manual_seed(1)
    fill = [torch.randn(s, generator=g_).to(DEV) for s in ((r, K), (K, r), (K, r))]
    tgt = [f.clone() for f in fill]
    _, _, _, grads = U.glu_bwd_tn("swiglu", DW, e.clone(), g.clone(), up, gate, down, p_d, xa_u, xa_g, targets=tgt)
    for t, f, fresh, out in zip(tgt, fill, runs[0][5:], grads):
        assert out is t and torch.equal(t, f + fresh)
    # one target only: the other two are fresh tensors
    tgt = [None, fill[1].clone(), None]
    _, _, _, grads = U.glu_bwd_tn("swiglu", DW, e.clone(), g.clone(), up, gate, down, p_d, xa_u, xa_g, targets=tgt)
    assert torch.equal(grads[0], runs[0][5]) and torch.equal(grads[1], fill[1] + runs[0][6]) and torch.equal(grads[2], runs[0][7])


def test_lora_mlp_block_with_and_without_glu_tn():
    from unsloth_amd.kernels import fast_lora, utils as U
    from unsloth_amd.kernels.fast_lora import LoRA_MLP
    from unsloth_amd.kernels.swiglu import swiglu_DWf_DW_dfg_kernel, swiglu_fg_kernel
    g_ = torch.Generator().manual_seed(0)
    T, H, I, r = 2048, 1024, 2816, 16
    dtype = torch.bfloat16
    gate, up, down = _proj(I, H, r, g_, dtype), _proj(I, H, r, g_, dtype), _proj(H, I, r, g_, dtype)
    X = torch.randn(1, T, H, generator=g_).to(dtype).to(DEV)
    dY = (torch.randn(1, T, H, generator=g_) * 0.1).to(dtype).to(DEV)
    U.GLU_FUSED = "both"                         # the step's own policy: 2048 rows are taken
    taken = []
    real = fast_lora.glu_bwd_tn

    def spy(*a, **k):
        out = real(*a, **k)
        taken.append(out is not None)
        return out
    fast_lora.glu_bwd_tn = spy
    res = {}
    try:
        for on in (True, False):
            U.GLU_TN = on
            ps = [torch.nn.Parameter(t.clone()) for p in (gate, up, down) for t in (p[2], p[3])]
            x = X.clone().requires_grad_(True)
            out = LoRA_MLP.apply(x, gate[0], None, ps[0], ps[1], 2.0, up[0], None, ps[2], ps[3], 2.0, down[0], None, ps[4],
                                 ps[5], 2.0, swiglu_fg_kernel, swiglu_DWf_DW_dfg_kernel, False)
            out.backward(dY.clone())
            res[on] = [out.detach().float(), x.grad.float()] + [p.grad.float() for p in ps]
    finally:
        fast_lora.glu_bwd_tn = real
    assert taken == [True]                       # on: the new path ran; off: it was not even asked
    for a, b in zip(res[True], res[False]):
        assert rel_fro(a, b) < 3e-3
