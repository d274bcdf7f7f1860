"""-m gpu: the row-wise kernels (RMSNorm, fused add+RMSNorm, the norm weight gradient, LayerNorm, cross entropy and the log-prob /
entropy forward, RoPE, the gated activations and QuickGELU) on the views the model hands them: a row stride wider than the row,
an odd row stride, a base pointer off the 16-byte grid. Every host function picks its kernel from the layout it is given; each
layout below drives one branch of that choice, and next to each test a comment says which.

A view lives in a 1-D pool (`pool_view`). Around an INPUT every pool element is NaN, so a read past a row end or in front of the
base poisons a reduction; around an OUTPUT or an in-place buffer every element is a finite sentinel that must keep its bits.
References are fp64 on the CPU (oracle/ref_ops.py with its arithmetic switched to double: it keeps the reference's rounding
points), the bounds are those of the aligned-data tests of the same kernel (tests/test_gpu_elementwise.py, tests/test_layernorm.py,
tests/test_gpu_full_finetune.py, tests/test_gpu_logprob_entropy.py). RoPE and the activations have no reduction: there the view's
result must also equal, bit for bit, the run on an aligned contiguous copy.

    layout          row stride    base offset      what it selects (VEC = 16 bytes / itemsize)
    aligned         cols          0                control: the vector kernels
    padded          cols + VEC    0                vector kernels with stride != cols
    odd_stride      cols + 1      0                scalar / block kernels, or the wrapper's fallback
    offset          cols          1                pointer off the 16-byte grid
    offset_padded   cols + VEC    VEC + 1          both
"""
import contextlib
import functools
import math

import pytest
import torch

from oracle import ref_ops as R
from tests._util import assert_ulp, rel_fro
from tests.test_gpu_elementwise import U
from tests.test_gpu_logprob_entropy import ref_entropy, ref_transform

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

SENTINEL = 123.0                    # exact in bf16 / fp16 / fp32
GUARD = 64                          # pool elements behind the last row
LAYOUTS = ("aligned", "padded", "odd_stride", "offset", "offset_padded")
# bf16 and fp32 (VEC 8 and 4: different template instances and limits) on every layout, fp16 on `offset` only
DTYPE_LAYOUT = [(dt, lay) for dt in (BF16, F32) for lay in LAYOUTS] + [(F16, "offset")]
RMS_VAR = 5                         # UAMD_TUNE_RMS_VAR: 0 = one wave per row, 1 = one block per row (the default)


def vec_of(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def layout(name, cols, dtype):
    """(row stride, base offset) in elements."""
    v = vec_of(dtype)
    return {"aligned": (cols, 0), "padded": (cols + v, 0), "odd_stride": (cols + 1, 0), "offset": (cols, 1),
            "offset_padded": (cols + v, v + 1)}[name]


def vectorizable(name):
    return name in ("aligned", "padded")


def pool_view(data, row_stride, base, fill):
    """(pool, view): `data` [rows, cols] (a CPU tensor) as a [rows, cols] view with `row_stride`, `base` elements into a fresh 1-D
    device pool whose every other element is `fill`."""
    rows, cols = data.shape
    pool = torch.full((base + (rows - 1) * row_stride + cols + GUARD,), fill, dtype=data.dtype, device=DEV)
    assert pool.data_ptr() % 16 == 0
    view = pool.as_strided((rows, cols), (row_stride, 1), base)
    view.copy_(data)
    assert (view.data_ptr() % 16 == 0) == (base % vec_of(data.dtype) == 0)
    return pool, view


def in_view(data, lay):
    """An input: NaN everywhere outside the view."""
    return pool_view(data, *layout(lay, data.shape[1], data.dtype), float("nan"))


def out_view(data, lay):
    """An output or in-place buffer: (pool, view, snapshot of the pool), the sentinel everywhere outside the view."""
    pool, view = pool_view(data, *layout(lay, data.shape[1], data.dtype), SENTINEL)
    return pool, view, pool.clone()


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def outside(pool, view):
    """bool mask over the pool: True on every element that is not part of `view`."""
    m = torch.ones(pool.numel(), dtype=torch.bool, device=pool.device)
    m.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
    return m


def assert_outside_untouched(pool, view, before, what):
    m = outside(pool, view)
    assert int(m.sum()) == pool.numel() - view.numel()
    assert torch.equal(bits(pool)[m], bits(before)[m]), f"{what}: the kernel wrote outside its view"


def assert_unchanged(pool, before, what):
    assert torch.equal(bits(pool), bits(before)), f"{what}: an input buffer was written"


@contextlib.contextmanager
def oracle_in_double():
    """oracle/ref_ops.py computes in `F32` and rounds where the reference rounds; with F32 = float64 it is the fp64 reference
    with the same rounding points."""
    old = R.F32
    R.F32 = torch.float64
    try:
        yield
    finally:
        R.F32 = old


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture
def tuning():
    from unsloth_amd import _lib
    L = _lib.lib()
    yield L
    L.uamd_set_tuning(RMS_VAR, 1)


# ---------------------------------------------------------------------------------------------------------------- RMSNorm
# rms_layernorm.hip launch_fwd / launch_bwd, `vec_ok`:
#   aligned, padded                         -> the 16-byte vector kernels rms_*_rows (a row per wave, TPR 64, with
#                                              UAMD_TUNE_RMS_VAR 0; a row per block, TPR 256, with 1)
#   odd_stride (stride % VEC), offset and
#   offset_padded (pointer), cols = 100     -> rms_fwd_block / rms_bwd_block, scalar loads
#   cols 64 VEC 8 | 64 VEC 8 + VEC          -> the backward's width limit: vector | block, on aligned data too
#   cols 64 VEC 16 + VEC                    -> past the forward's limit: block kernels both ways
#   cols 64 VEC k + VEC, k = 1, 2, 4        -> 2, 3, 5 vectors per lane of a wave: with 1 (33 VEC), 8 and 9 every ITERS of the
#                                              ladders 1, 2, 4, 8, 16 (a row per wave) and 1, 2, 4 (per block: a quarter) runs
RMS_ROWS = 5                        # four rows per block in the wave kernels: one full group and a one-row group


def rms_cols(dtype):
    v = vec_of(dtype)
    return [33 * v, 64 * v * 8, 64 * v * 8 + v, 64 * v * 16 + v, 100, 64 * v + v, 64 * v * 2 + v, 64 * v * 4 + v]


@functools.lru_cache(maxsize=None)
def rms_case(dtype, cols, gemma, wdtype):
    """(X, W, dY, Y, r, dX): inputs on the CPU and the fp64 reference, computed once for all layouts."""
    X = torch.randn(RMS_ROWS, cols, generator=g(3407)).to(dtype)
    W = torch.rand(cols, generator=g(42)).to(wdtype)
    dY = torch.randn(RMS_ROWS, cols, generator=g(7)).to(dtype)
    with oracle_in_double():
        Y, r = R.rms_layernorm_forward(X, W, 1e-5, gemma)
        dX = R.rms_layernorm_backward(dY, X, W, r, gemma)
    assert r.dtype == torch.float64
    return X, W, dY, Y, r, dX


@pytest.mark.parametrize("gemma", [False, True], ids=["llama", "gemma"])
@pytest.mark.parametrize("ci", range(8), ids=["33v", "64v8", "64v8+v", "64v16+v", "c100", "64v+v", "64v2+v", "64v4+v"])
@pytest.mark.parametrize("dtype,lay", DTYPE_LAYOUT)
def test_rmsnorm_on_views(tuning, dtype, lay, ci, gemma):
    from unsloth_amd.kernels.rms_layernorm import rms_bwd_, rms_fwd
    cols = rms_cols(dtype)[ci]
    for wdtype in sorted({dtype, F32}, key=str):
        X, W, dY, Yo, ro, dXo = rms_case(dtype, cols, gemma, wdtype)
        xpool, Xv = in_view(X, lay)
        xbefore = xpool.clone()
        Wd = W.to(DEV)
        for var in (0, 1):
            what = f"rms {lay} cols {cols} W {wdtype} var {var}"
            assert tuning.uamd_set_tuning(RMS_VAR, var) == 0
            Y, r = rms_fwd(Xv, Wd, 1e-5, gemma)
            assert_ulp(Y, Yo, dtype, ulps=U(dtype, 1), what=what + " fwd", allow_frac=2e-3)
            assert_ulp(r, ro, F32, ulps=32, what=what + " r")
            dpool, dYv, dbefore = out_view(dY, lay)
            dX = rms_bwd_(dYv, Xv, Wd, r, gemma=gemma)
            assert_ulp(dX, dXo, dtype, ulps=U(dtype, 2), what=what + " bwd", allow_frac=2e-3)
            if gemma:
                assert torch.equal(dYv, dY.to(DEV)), "the Gemma form leaves dY alone"
            else:
                assert dX.data_ptr() == dYv.data_ptr() and dX.stride() == dYv.stride(), "dX is written over dY"
            assert_outside_untouched(dpool, dYv, dbefore, what)
            assert_unchanged(xpool, xbefore, what)


# ---------------------------------------------------------------------------------------------------- norm weight gradient
# rms_layernorm.hip launch_dw, `vec_ok`:
#   aligned, padded                         -> rms_dw_partial<T, true>, one 16-byte vector of columns per thread
#   odd_stride, offset, offset_padded       -> rms_dw_partial<T, false>, one column per thread (this layout used to return
#                                              UAMD_ERR_ALIGN and `rms_dw` raised)
# rows 5: one row chunk; rows 300: 38 chunks of 8 rows through the second, ordered, reduction stage.
@functools.lru_cache(maxsize=None)
def dw_case(adtype, wdtype, rows, cols):
    dY = (torch.randn(rows, cols, generator=g(rows)) * 0.1).to(adtype)
    X = torch.randn(rows, cols, generator=g(rows + 1)).to(adtype)
    r = (0.5 + torch.rand(rows, generator=g(rows + 2))).float()
    out0 = torch.randn(cols, generator=g(rows + 3)).to(wdtype)
    dW = (dY.double() * X.double() * r.double()[:, None]).sum(0)
    return dY, X, r, out0, dW


@pytest.mark.parametrize("rows", [5, 300])
@pytest.mark.parametrize("ci", [0, 2], ids=["33v", "64v8+v"])
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("adtype,wdtype", [(BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)])
def test_rms_weight_gradient_on_views(adtype, wdtype, lay, ci, rows):
    from unsloth_amd.kernels.rms_layernorm import rms_dw
    cols = rms_cols(adtype)[ci]
    dY, X, r, out0, dWo = dw_case(adtype, wdtype, rows, cols)
    dpool, dYv = in_view(dY, lay)
    xpool, Xv = in_view(X, lay)
    dbefore, xbefore = dpool.clone(), xpool.clone()
    rd = r.to(DEV)
    W = torch.empty(cols, dtype=wdtype, device=DEV)
    bound = 6e-3 if wdtype != F32 else 1e-4                 # test_rms_layernorm_weight_gradient's
    for accumulate in (False, True):
        want = dWo + out0.double() if accumulate else dWo
        runs = []
        for _ in range(2):
            opool, ov, obefore = out_view(out0.view(1, cols), "aligned")
            got = rms_dw(dYv, Xv, rd, W, out=ov[0], accumulate=accumulate)
            assert got.data_ptr() == ov.data_ptr()
            assert torch.isfinite(got.float()).all(), "a NaN from outside an input view reached dW"
            err = rel_fro(got.double().cpu(), want)
            assert err < bound, (lay, cols, rows, accumulate, err)
            assert_outside_untouched(opool, ov, obefore, f"dw {lay}")
            runs.append(got.clone())
        assert torch.equal(runs[0], runs[1]), "the two-stage column sum has a fixed order"
    assert_unchanged(dpool, dbefore, "dw dY")
    assert_unchanged(xpool, xbefore, "dw X")


def test_rms_weight_gradient_width_100():
    """A trainable norm whose width is no multiple of the vector (the width test_rms_layernorm runs forward and backward)."""
    from unsloth_amd.kernels.rms_layernorm import rms_dw
    dY, X, r, _, dWo = dw_case(BF16, F32, 37, 100)
    got = rms_dw(dY.to(DEV), X.to(DEV), r.to(DEV), torch.empty(100, dtype=F32, device=DEV))
    assert rel_fro(got.double().cpu(), dWo) < 1e-4


# --------------------------------------------------------------------------------------------------- fused add + RMSNorm
# kernels/rms_layernorm.py add_rms_supported / rms_bwd_ (the fused kernels have no scalar form: uamd_add_rms_layernorm_*
# return UAMD_ERR_ALIGN):
#   aligned, padded, cols <= 64 VEC 8       -> uamd_add_rms_layernorm_fwd / _bwd
#   odd_stride, offset, offset_padded       -> torch add + Fast_RMS_Layernorm (these used to raise)
#   cols 64 VEC 8 + VEC                     -> the two-op path by width
class _Norm:
    def __init__(self, weight):
        self.weight, self.variance_epsilon = weight, 1e-5


@functools.lru_cache(maxsize=None)
def add_case(dtype, cols):
    gen = g(cols)
    return tuple(torch.randn(RMS_ROWS, cols, generator=gen).to(dtype) for _ in range(4)) + (torch.rand(cols, generator=gen).to(dtype),)


def _add_rms_reference(x, res, W, dh_v, dy_v):
    """`residual + X`, then the norm; the gradients arrive in the buffers given (the norm's backward is in place over dY)."""
    from unsloth_amd.kernels.rms_layernorm import Fast_RMS_Layernorm
    x1, r1 = x.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True)
    h1 = r1 + x1
    y1 = Fast_RMS_Layernorm.apply(h1, W, 1e-5, False)
    torch.autograd.backward([h1, y1], [dh_v, dy_v])
    return h1.detach(), y1.detach(), x1.grad, r1.grad


@pytest.mark.parametrize("ci", [0, 1, 2, 5, 6, 7], ids=["33v", "64v8", "64v8+v", "64v+v", "64v2+v", "64v4+v"])
@pytest.mark.parametrize("dtype,lay", DTYPE_LAYOUT)
def test_fused_add_rmsnorm_on_views_equals_add_then_norm(dtype, lay, ci):
    from unsloth_amd.kernels import rms_layernorm as M
    cols = rms_cols(dtype)[ci]
    x, res, dh, dy, W = add_case(dtype, cols)
    W = W.to(DEV)
    # the reference's gradients sit in the same layout: whether the norm's backward takes its vector or its block kernel
    # (which sum a row in different orders) depends on dY's layout on either path
    _, dh1, _ = out_view(dh, lay)
    _, dy1, _ = out_view(dy, lay)
    h1, y1, gx1, gr1 = _add_rms_reference(x, res, W, dh1, dy1)

    xpool, xv = in_view(x, lay)
    rpool, rv = in_view(res, lay)
    xbefore, rbefore = xpool.clone(), rpool.clone()
    hpool, dhv, hbefore = out_view(dh, lay)
    ypool, dyv, ybefore = out_view(dy, lay)
    fused = []
    real = M.Fast_Add_RMS_Layernorm.apply
    M.Fast_Add_RMS_Layernorm.apply = staticmethod(lambda *a: (fused.append(1), real(*a))[1])
    try:
        h2, y2 = M.fast_add_rms_layernorm(_Norm(W), xv.requires_grad_(True), rv.requires_grad_(True))    # must not raise
    finally:
        del M.Fast_Add_RMS_Layernorm.apply
    assert bool(fused) == (vectorizable(lay) and cols <= 64 * vec_of(dtype) * 8), "which path ran"
    assert torch.isfinite(h2.float()).all() and torch.isfinite(y2.float()).all()
    assert torch.equal(h2, h1) and torch.equal(y2, y1)
    torch.autograd.backward([h2, y2], [dhv, dyv])
    assert torch.isfinite(xv.grad.float()).all()
    assert torch.equal(xv.grad, gx1) and torch.equal(rv.grad, gr1)
    assert_outside_untouched(ypool, dyv, ybefore, f"add+rms {lay} dY")
    assert_outside_untouched(hpool, dhv, hbefore, f"add+rms {lay} dH")
    assert_unchanged(xpool, xbefore, "add+rms X")
    assert_unchanged(rpool, rbefore, "add+rms residual")


@pytest.mark.parametrize("lay", ["odd_stride", "offset"])
def test_fused_add_rmsnorm_backward_takes_misaligned_gradients(lay):
    """The forward ran fused on aligned activations; autograd then hands the backward gradients that are views."""
    from unsloth_amd.kernels import rms_layernorm as M
    x, res, dh, dy, W = add_case(BF16, 33 * 8)
    W = W.to(DEV)
    _, dh1, _ = out_view(dh, lay)
    _, dy1, _ = out_view(dy, lay)
    h1, y1, gx1, gr1 = _add_rms_reference(x, res, W, dh1, dy1)
    xd, rd = x.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True)
    h2, y2 = M.Fast_Add_RMS_Layernorm.apply(xd, rd, W, 1e-5)
    hpool, dhv, hbefore = out_view(dh, lay)
    ypool, dyv, ybefore = out_view(dy, lay)
    torch.autograd.backward([h2, y2], [dhv, dyv])
    assert torch.equal(h2, h1) and torch.equal(y2, y1) and torch.equal(xd.grad, gx1) and torch.equal(rd.grad, gr1)
    assert_outside_untouched(ypool, dyv, ybefore, "dY")
    assert_unchanged(hpool, hbefore, "dH")


# -------------------------------------------------------------------------------------------------------------- LayerNorm
# layernorm.hip ln_fwd / ln_bwd, `fast` (iters = ceil(cols / (256 VEC))):
#   aligned, padded                         -> layernorm_fwd_kernel / layernorm_bwd_kernel (row in registers)
#   odd_stride, offset, offset_padded       -> layernorm_*_generic, scalar loops
#   cols 256 VEC 4 | 256 VEC 4 + VEC        -> the backward's `iters <= 4`: fast | generic (the forward stays fast: ITERS 4 | 8)
#   cols 256 VEC 8 | 256 VEC 8 + VEC        -> the forward's LN_MAX_ITERS: fast | generic (the backward is generic for both)
LN_ROWS = 5


def ln_cols(dtype):
    v = vec_of(dtype)
    return [33 * v, 256 * v * 4, 256 * v * 4 + v, 256 * v * 8, 256 * v * 8 + v]


@functools.lru_cache(maxsize=None)
def ln_case(dtype, cols, wdtype):
    gen = g(cols)
    X = (torch.randn(LN_ROWS, cols, generator=gen) * 2 + 0.5).to(dtype)
    dY = torch.randn(LN_ROWS, cols, generator=gen).to(dtype)
    W, b = torch.rand(cols, generator=gen).to(wdtype), torch.rand(cols, generator=gen).to(wdtype)
    x, w = X.double(), W.double()
    mu = x.mean(-1, keepdim=True)
    r = torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
    nrm = (x - mu) * r
    Y = nrm * w + b.double()
    gg = dY.double() * w
    dX = (gg - gg.mean(-1, keepdim=True) - nrm * (gg * nrm).mean(-1, keepdim=True)) * r
    return X, dY, W, b, Y, dX


@pytest.mark.parametrize("ci", range(5), ids=["33v", "256v4", "256v4+v", "256v8", "256v8+v"])
@pytest.mark.parametrize("dtype,lay", DTYPE_LAYOUT)
def test_layernorm_on_views(dtype, lay, ci):
    from unsloth_amd.kernels.layernorm import Fast_Layernorm
    cols = ln_cols(dtype)[ci]
    for wdtype in sorted({dtype, F32}, key=str):
        X, dY, W, b, Yo, dXo = ln_case(dtype, cols, wdtype)
        what = f"layernorm {lay} cols {cols} W {wdtype}"
        xpool, Xv = in_view(X, lay)
        xbefore = xpool.clone()
        dpool, dYv, dbefore = out_view(dY, lay)
        Y = Fast_Layernorm.apply(Xv.requires_grad_(True), W.to(DEV), b.to(DEV), 1e-6)
        Y.backward(dYv)
        assert torch.isfinite(Y.float()).all() and torch.isfinite(dYv.float()).all(), what
        if dtype == F32:                                            # test_hip_layernorm_vs_oracle_and_torch's bounds
            torch.testing.assert_close(Y.detach().cpu(), Yo.float(), rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(dYv.cpu(), dXo.float(), rtol=1e-4, atol=1e-5)
        else:
            assert_ulp(Y, Yo, dtype, ulps=1.0, what=what + " Y", allow_frac=2e-3)
            assert_ulp(dYv, dXo, dtype, ulps=1.0, what=what + " dX", allow_frac=2e-3)
        assert torch.equal(Xv.grad, dYv), "dX is written over dY"
        assert_outside_untouched(dpool, dYv, dbefore, what)
        assert_unchanged(xpool, xbefore, what)


# ---------------------------------------------------------------------------------------------------------- cross entropy
# cross_entropy_loss.hip rows_vectorizable (pointer 16-byte aligned and row stride % VEC == 0) picks the V template argument of
# the forward, of the log-prob / entropy forward and of the backward:
#   aligned (V = 1000), padded              -> <V = true>; V = 4099 and chunk + 5 are no multiples of VEC: the scalar tail of the
#                                              vector kernels
#   aligned with V = 4099 or chunk + 5
#   (stride = V), odd_stride, offset,
#   offset_padded                           -> <V = false>
# V = 256 VEC 4 + 5 is one full backward chunk (the branch-free four-vector form) and a five-column second chunk.
CE_ROWS = 5
CE_MODES = [(0.0, 0.0), (30.0, 0.5)]


def ce_vocab(dtype):
    return [1000, 4099, 256 * vec_of(dtype) * 4 + 5]


@functools.lru_cache(maxsize=None)
def ce_case(dtype, V, cap, scale):
    logits = (torch.randn(CE_ROWS, V, generator=g(21)) * 4).to(dtype)
    labels = torch.tensor([-100, 0, V - 1, 17, V // 2])
    dl = torch.rand(CE_ROWS, generator=g(23))
    with oracle_in_double():
        loss, lse = R.cross_entropy_forward(logits, labels, cap, scale)
        grad = R.cross_entropy_backward(logits, dl, lse, labels, cap, scale)
    assert lse.dtype == torch.float64
    ent = ref_entropy(ref_transform(logits.double(), cap, scale))
    return logits, labels, dl, loss, lse, grad, ent


@pytest.mark.parametrize("cap,scale", CE_MODES, ids=["plain", "cap_scale"])
@pytest.mark.parametrize("vi", range(3), ids=["v1000", "v4099", "chunk+5"])
@pytest.mark.parametrize("dtype,lay", DTYPE_LAYOUT)
def test_cross_entropy_on_views(dtype, lay, vi, cap, scale):
    from unsloth_amd.kernels.cross_entropy_loss import _ce_backward_, _ce_forward, _logprob_entropy_forward
    V = ce_vocab(dtype)[vi]
    logits, labels, dl, loss_o, lse_o, grad_o, ent_o = ce_case(dtype, V, cap, scale)
    what = f"ce {lay} V {V}"
    lab = labels.to(DEV)
    ipool, xv = in_view(logits, lay)
    ibefore = ipool.clone()
    assert xv.stride(0) == layout(lay, V, dtype)[0]                  # the launchers pass the view's own stride: no copy
    loss, lse = _ce_forward(xv, lab, cap, scale)
    torch.testing.assert_close(loss.cpu(), loss_o.float(), rtol=2e-5, atol=2e-5)         # test_cross_entropy's bound
    torch.testing.assert_close(lse.cpu(), lse_o.float(), rtol=2e-5, atol=2e-5)
    assert loss[0].item() == 0.0
    lp, lse1, ent = _logprob_entropy_forward(xv, lab, cap, scale)
    assert torch.equal(lse1, lse) and torch.equal(lp, -loss)
    err = (ent.double().cpu() - ent_o).abs().max().item()
    assert torch.isfinite(ent).all() and err <= 1e-3 * (math.log(V) + 1), (what, err)    # test_gpu_logprob_entropy's bound
    assert_unchanged(ipool, ibefore, what)
    # backward, in place over the logits: the padding between the rows must survive
    opool, gv, obefore = out_view(logits, lay)
    got = _ce_backward_(gv, dl.to(DEV), lse, lab, cap, scale)
    assert got.data_ptr() == gv.data_ptr()
    assert_ulp(gv, grad_o, dtype, ulps=U(dtype, 2), atol=1e-6 if dtype != F32 else 1e-8, what=what + " bwd", allow_frac=5e-3)
    assert torch.all(gv[0] == 0), "an ignored row has an exactly zero gradient"
    assert_outside_untouched(opool, gv, obefore, what)


# ------------------------------------------------------------------------------------------------------------------- RoPE
# rope_embedding.hip launch, `vec_ok` (half % VEC, the pointers, the batch / head / seq strides of Q and of K):
#   aligned, padded                         -> rope_vec_kernel
#   odd_stride (seq and batch strides),
#   offset, offset_padded (pointers)        -> rope_scalar_kernel
#   k_offset (Q aligned, K one element in)  -> rope_scalar_kernel, through the K half of the predicate alone
#   mrope sections (10, 14, 16) at D = 80   -> rope_scalar_kernel through `sec % VEC` alone on the aligned layouts
# Q and K are [B, H, T, D] views of token-major pools, as the slices of a fused projection are: seq stride = H D + the layout's
# padding, head stride D, batch stride T seq strides.
ROPE_B, ROPE_T, ROPE_HQ, ROPE_HK, ROPE_POS = 2, 7, 4, 2, 64
ROPE_LAYOUTS = LAYOUTS + ("k_offset",)
ROPE_DTYPE_LAYOUT = [(dt, lay) for dt in (BF16, F32) for lay in ROPE_LAYOUTS] + [(F16, "offset")]
MROPE_SECTIONS = {128: [(16, 24, 24)], 80: [(8, 16, 16), (10, 14, 16)]}


def rope_tables(D, dtype, theta=5e5):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    fr = torch.outer(torch.arange(ROPE_POS, dtype=torch.int64).float(), inv)
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def rope_ref(Q, K, cos, sin, pos, backward):
    """The rotation in fp64 with the kernel's (and the reference's) rounding points: every product is rounded to the dtype the
    arithmetic runs in -- the shared 16-bit dtype when Q and the table have one, fp32 otherwise (the library is built with
    -ffp-contract=off) -- and the sum, exact in fp64, once to Q's dtype. Without the products' rounding no fp32 implementation
    meets a bound in ulps of the RESULT where q0 cos and q1 sin cancel: torch's own fp32 arithmetic on the CPU is then beyond
    test_rope_qk_indexed_and_dense's rule at 4 of 7168 elements of this test's Q (worst error 2.4e-7, one ulp of a product).
    pos int64 [B T, D / 2]: the position every rotary pair of every token takes its angle from (one column repeated for ordinary
    RoPE, three streams for mrope)."""
    B, _, T, D = Q.shape
    half = D // 2
    native = Q.dtype == cos.dtype and Q.dtype != F32
    arith = Q.dtype if native else F32
    rnd = lambda v: v.to(arith).double()
    j = torch.arange(half)
    c = cos[pos, j].double().view(B, 1, T, half)
    s = sin[pos, j].double().view(B, 1, T, half)
    if backward:
        s = -s
    out = []
    for X in (Q, K):
        x0, x1 = X.double()[..., :half], X.double()[..., half:]
        out.append(torch.cat((rnd(x0 * c) - rnd(x1 * s), rnd(x1 * c) + rnd(x0 * s)), dim=-1).to(X.dtype))
    return out


def rope_view(data, lay):
    """data [B, T, H, D] (CPU) -> (pool, [B, H, T, D] view, snapshot); the sentinel outside (the rotation is in place)."""
    B, T, H, D = data.shape
    seq, base = layout(lay, H * D, data.dtype)
    pool, rows = pool_view(data.reshape(B * T, H * D), seq, base, SENTINEL)
    view = pool.as_strided((B, H, T, D), (T * seq, D, seq, 1), base)
    assert torch.equal(view, data.to(DEV).transpose(1, 2)) and rows.data_ptr() == view.data_ptr()
    return pool, view, pool.clone()


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("D", [128, 80])
@pytest.mark.parametrize("dtype,lay", ROPE_DTYPE_LAYOUT)
def test_rope_on_views(dtype, lay, D, backward):
    from unsloth_amd.kernels.rope_embedding import Fast_MRoPE_Embedding_QK, _launch_qk
    B, T, Hq, Hk = ROPE_B, ROPE_T, ROPE_HQ, ROPE_HK
    half = D // 2
    cos, sin = rope_tables(D, dtype)
    cosd, sind = cos.to(DEV), sin.to(DEV)
    Q = torch.randn(B, T, Hq, D, generator=g(3)).to(dtype)
    K = torch.randn(B, T, Hk, D, generator=g(4)).to(dtype)
    idx = torch.randint(0, ROPE_POS, (B * T,), generator=g(5)).to(torch.int32)
    pos3 = torch.randint(0, ROPE_POS, (3, B * T), generator=g(6)).to(torch.int32)
    idxd, pos3d = idx.to(DEV), pos3.to(DEV)
    native = dtype != F32                                            # Q and the table share a 16-bit dtype
    entries = [("indexed", lambda q, k: _launch_qk(q, k, cosd, sind, idxd, backward), idx.long()[:, None].expand(-1, half))]
    for sec in MROPE_SECTIONS[D]:
        stream = torch.repeat_interleave(torch.arange(3), torch.tensor(sec))
        entries.append((f"mrope{sec}", lambda q, k, sec=sec: Fast_MRoPE_Embedding_QK._run(q, k, cosd, sind, pos3d, sec[0],
                                                                                           sec[1], backward),
                        pos3.long()[stream].t()))
    for name, run, pos in entries:
        what = f"rope {name} {lay} D {D}"
        # the aligned contiguous copy, against the fp64 rotation at test_rope_qk_indexed_and_dense's 0-ulp / 1-ulp rule
        Qa, Ka = Q.to(DEV).transpose(1, 2), K.to(DEV).transpose(1, 2)
        run(Qa, Ka)
        Qo, Ko = rope_ref(Q.transpose(1, 2), K.transpose(1, 2), cos, sin, pos, backward)
        assert_ulp(Qa, Qo, dtype, ulps=0 if native else 1, atol=0 if native else None, what=what + " Q")
        assert_ulp(Ka, Ko, dtype, ulps=0 if native else 1, atol=0 if native else None, what=what + " K")
        # the views: no reduction, so the same bits
        qpool, Qv, qbefore = rope_view(Q, "aligned" if lay == "k_offset" else lay)
        kpool, Kv, kbefore = rope_view(K, "offset" if lay == "k_offset" else lay)
        run(Qv, Kv)
        assert torch.equal(Qv, Qa) and torch.equal(Kv, Ka), what
        assert_outside_untouched(qpool, Qv, qbefore, what + " Q")
        assert_outside_untouched(kpool, Kv, kbefore, what + " K")


# ------------------------------------------------------------------------------------------- gated activations, QuickGELU
# glu.hip launch_fwd / launch_bwd / launch_quick_gelu return UAMD_ERR_ALIGN for a pointer off the 16-byte grid; the wrappers
# (kernels/swiglu.py _glu_fwd / _glu_bwd, kernels/quick_gelu.py) hand the kernel
#   aligned                                 -> the tensors themselves
#   offset (contiguous, one element in)     -> aligned copies, copied back where the contract is in place (these used to raise)
# n = 3 VEC + 1: three vectors and the scalar tail in one block; n = 256 VEC + 3: a second vector per thread / a second block.
GLU_KINDS = {"swiglu": ("swiglu_fg_kernel", "swiglu_DWf_DW_dfg_kernel"),
             "geglu_exact": ("geglu_exact_forward_kernel", "geglu_exact_backward_kernel"),
             "geglu_approx": ("geglu_approx_forward_kernel", "geglu_approx_backward_kernel")}


def flat_sizes(dtype):
    v = vec_of(dtype)
    return [3 * v + 1, 256 * v + 3]


def offset_flat(data, fill):
    """data [n] -> (pool, contiguous view one element into the pool, snapshot)."""
    pool, view = pool_view(data.view(1, -1), data.numel(), 1, fill)
    view = view[0]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return pool, view, pool.clone()


@pytest.mark.parametrize("ni", [0, 1], ids=["3v+1", "256v+3"])
@pytest.mark.parametrize("kind", list(GLU_KINDS))
@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_glu_at_a_storage_offset(dtype, kind, ni):
    import unsloth_amd.kernels as K
    fwd, bwd = getattr(K, GLU_KINDS[kind][0]), getattr(K, GLU_KINDS[kind][1])
    n = flat_sizes(dtype)[ni]
    e = torch.randn(n, generator=g(11)).to(dtype)
    gg = torch.randn(n, generator=g(12)).to(dtype)
    DW = torch.randn(n, generator=g(13)).to(dtype)
    with oracle_in_double():
        ho = R.glu_forward(e, gg, kind)
        bo = R.glu_backward(DW, e, gg, kind)
    # aligned run against the oracle, test_glu's bounds
    h = fwd(e.to(DEV), gg.to(DEV))
    assert_ulp(h, ho, dtype, ulps=U(dtype, 1), atol=1e-6 if dtype == F32 else None, what=f"{kind} fwd", allow_frac=5e-3)
    a = [DW.to(DEV), e.to(DEV), gg.to(DEV)]
    ptrs = [t.data_ptr() for t in a]
    assert [t.data_ptr() for t in bwd(*a)] == ptrs
    for got, want, nm, u in zip(a, bo, ("h", "df", "de"), (1, 1, 2)):
        assert_ulp(got, want, dtype, ulps=U(dtype, u), atol=4e-6 if dtype == F32 else None, what=f"{kind} bwd {nm}", allow_frac=5e-3)
    # one element into the storage: the same bits, in place where the contract says so, nothing outside touched
    epool, ev, ebefore = offset_flat(e, float("nan"))
    gpool, gv, gbefore = offset_flat(gg, float("nan"))
    h2 = fwd(ev, gv)
    assert torch.isfinite(h2.float()).all() and torch.equal(h2, h)
    assert_unchanged(epool, ebefore, "e")
    assert_unchanged(gpool, gbefore, "g")
    pools = [offset_flat(t, SENTINEL) for t in (DW, e, gg)]
    views = [p[1] for p in pools]
    out = bwd(*views)
    assert [t.data_ptr() for t in out] == [t.data_ptr() for t in views], "backward must overwrite DW, e, g"
    for (pool, view, before), want, nm in zip(pools, a, ("h", "df", "de")):
        assert torch.equal(view, want), f"{kind} bwd {nm} at an offset"
        assert_outside_untouched(pool, view, before, f"{kind} bwd {nm}")


@pytest.mark.parametrize("ni", [0, 1], ids=["3v+1", "256v+3"])
@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_quick_gelu_at_a_storage_offset(dtype, ni):
    from unsloth_amd.kernels.quick_gelu import fast_quick_gelu
    n = flat_sizes(dtype)[ni]
    x = (torch.randn(n, generator=g(1)) * 2).to(dtype)
    dy = torch.randn(n, generator=g(2)).to(dtype)
    xr = x.double().requires_grad_(True)
    yr = xr * torch.sigmoid(1.702 * xr)
    yr.backward(dy.double())
    # aligned run against fp64, test_quick_gelu_kernel_matches_torch_fp32's bounds (half an ulp of the dtype; fp32: U()'s 32 ulp)
    xa, dya = x.to(DEV).requires_grad_(True), dy.to(DEV)
    ya = fast_quick_gelu(xa)
    ya.backward(dya)
    ulp = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 32 * 2.0 ** -23}[dtype]
    assert (ya.double().cpu() - yr.detach()).abs().max() <= ulp * max(1.0, yr.abs().max().item())
    assert (xa.grad.double().cpu() - xr.grad).abs().max() <= 2 * ulp * max(1.0, xr.grad.abs().max().item())
    assert xa.grad.data_ptr() == dya.data_ptr() or torch.equal(dya, xa.grad), "dX is written over dY"
    # one element into the storage
    xpool, xv, xbefore = offset_flat(x, float("nan"))
    dpool, dv, dbefore = offset_flat(dy, SENTINEL)
    y = fast_quick_gelu(xv.requires_grad_(True))
    assert torch.isfinite(y.float()).all() and torch.equal(y, ya)
    y.backward(dv)
    assert torch.equal(xv.grad, xa.grad) and torch.equal(dv, xa.grad), "the same bits, written over dY"
    assert_outside_untouched(dpool, dv, dbefore, "quick_gelu dY")
    assert_unchanged(xpool, xbefore, "quick_gelu x")
