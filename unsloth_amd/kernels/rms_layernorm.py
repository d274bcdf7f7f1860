"""RMSNorm through the HIP kernels; mirror of unsloth/kernels/rms_layernorm.py.

Same autograd contract as the reference's Fast_RMS_Layernorm (:162-240): saves (X, W, r); the
backward writes dX IN PLACE over dY for the non-Gemma case (:92-95, :218). The reference returns no dW
(norm weights are frozen under LoRA; with full_finetuning=True it leaves trainable norms to HF's torch module).
Here a weight that requires grad gets it from `uamd_rms_layernorm_dw` (csrc/rms_layernorm.hip), computed from dY
before the in-place dX pass overwrites it.
"""
import torch

from .. import _lib


# ---- plain launchers (no autograd), shared by the Functions below and by models/fast_layer.py ---------------------
def _rows(X):
    X2 = X.reshape(-1, X.shape[-1])
    return X2 if X2.stride(1) == 1 else X2.contiguous()


def _vec_layout(*tensors):
    """What the 16-byte vector kernels need of every operand: unit stride along the row, the base pointer and every other
    stride a multiple of 16 bytes."""
    for t in tensors:
        vec = 16 // t.element_size()
        if t.data_ptr() % 16 or t.stride(-1) != 1 or any(s % vec for s in t.stride()[:-1]):
            return False
    return True


def _add_width_ok(X):
    """The fused add + norm kernels keep a row of up to 64 x 8 16-byte vectors (they have no scalar form)."""
    return X.shape[-1] <= 64 * (16 // X.element_size()) * 8


def rms_fwd(X, W, eps, gemma=False):
    """(Y, r) for X [..., dim]; Y [rows, dim]."""
    _lib.require_gpu(X, W)
    X2 = _rows(X)
    n_rows, n_cols = X2.shape
    Y = torch.empty((n_rows, n_cols), dtype=X2.dtype, device=X2.device)
    r = torch.empty(n_rows, dtype=torch.float32, device=X2.device)
    W = W.contiguous()
    _lib.call("uamd_rms_layernorm_fwd", X2, _lib.ptr(X2), _lib.ptr(W), _lib.ptr(Y), _lib.ptr(r), n_rows, n_cols,
              X2.stride(0), Y.stride(0), float(eps), int(bool(gemma)), _lib.dtype_code(X2.dtype), _lib.dtype_code(W.dtype),
              _lib.stream_of(X2))
    return Y, r


def add_rms_fwd(X, residual, W, eps):
    """(H, Y, r): H = X + residual, Y = rmsnorm(H) * W."""
    _lib.require_gpu(X, residual, W)
    X2, R2 = _rows(X), _rows(residual)
    n_rows, dim = X2.shape
    H = torch.empty((n_rows, dim), dtype=X2.dtype, device=X2.device)
    Y = torch.empty((n_rows, dim), dtype=X2.dtype, device=X2.device)
    r = torch.empty(n_rows, dtype=torch.float32, device=X2.device)
    W = W.contiguous()
    _lib.call("uamd_add_rms_layernorm_fwd", X2, _lib.ptr(X2), _lib.ptr(R2), _lib.ptr(W), _lib.ptr(H), _lib.ptr(Y),
              _lib.ptr(r), n_rows, dim, X2.stride(0), R2.stride(0), H.stride(0), Y.stride(0), float(eps),
              _lib.dtype_code(X2.dtype), _lib.dtype_code(W.dtype), _lib.stream_of(X2))
    return H, Y, r


def rms_dw(dY, X, r, W, out=None, accumulate=False):
    """dW[c] (+)= sum_rows dY[row, c] * X[row, c] * r[row] in W's dtype (X = the norm's input). Deterministic."""
    from .. import nf4 as _nf4
    dY2, X2 = _rows(dY), _rows(X)
    n_rows, dim = dY2.shape
    if out is None:
        out = torch.empty(dim, dtype=W.dtype, device=W.device)
        accumulate = False
    assert out.is_contiguous() and out.numel() == dim and out.dtype == W.dtype
    vec = 16 // dY2.element_size()
    col_blocks = ((dim + vec - 1) // vec + 255) // 256
    chunks = max(1, min((2048 + col_blocks - 1) // col_blocks, (n_rows + 7) // 8))
    ws = _nf4.scratch(dY2.device, chunks * dim, torch.float32, slot=41)
    _lib.call("uamd_rms_layernorm_dw", dY2, _lib.ptr(dY2), _lib.ptr(X2), _lib.ptr(r), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
              n_rows, dim, dY2.stride(0), X2.stride(0), int(bool(accumulate)), _lib.dtype_code(dY2.dtype),
              _lib.dtype_code(W.dtype), _lib.stream_of(dY2))
    return out


def _weight_grad(dY, X, r, W, needed):
    """The norm weight's gradient for autograd (None when the weight is frozen): added straight into the parameter's
    gradient sink when it has one (full fine-tuning's flat gradient buckets), else returned."""
    if not needed:
        return None
    from .utils import grad_sink
    sink = grad_sink(W)
    if sink is not None:
        first = sink.first_write(W) if hasattr(sink, "first_write") else False
        rms_dw(dY, X, r, W, out=sink.grad_view(W).view(-1), accumulate=not first)
        sink.ready(W)
        return None
    return rms_dw(dY, X, r, W)


def rms_bwd_(dY, H, W, r, dH=None, gemma=False):
    """dX = rmsnorm_backward(dY; H, W, r) (+ dH, the gradient reaching H from the residual path), [rows, dim]. Llama-style
    norm: written IN PLACE over dY (rms_layernorm.py:218); `gemma`: the (1 + W) form, into a fresh tensor (:92-95)."""
    dY2, H2 = _rows(dY), _rows(H)
    n_rows, dim = dY2.shape
    dX = torch.empty_like(dY2) if gemma else dY2
    if dH is not None and not (_add_width_ok(dY2) and _vec_layout(dY2, H2, W, _rows(dH))):
        # the fused kernel has no scalar form: the norm's backward (which has one), then the add, with the same two roundings
        assert not gemma
        return rms_bwd_(dY2, H2, W, r).add_(_rows(dH))
    if dH is None:
        _lib.call("uamd_rms_layernorm_bwd", dY2, _lib.ptr(dY2), _lib.ptr(dX), _lib.ptr(H2), _lib.ptr(W), _lib.ptr(r), n_rows,
                  dim, dY2.stride(0), dX.stride(0), H2.stride(0), int(gemma), _lib.dtype_code(dY2.dtype),
                  _lib.dtype_code(W.dtype), _lib.stream_of(dY2))
    else:
        assert not gemma
        dH2 = _rows(dH)
        _lib.call("uamd_add_rms_layernorm_bwd", dY2, _lib.ptr(dY2), _lib.ptr(dH2), _lib.ptr(dY2), _lib.ptr(H2), _lib.ptr(W),
                  _lib.ptr(r), n_rows, dim, dY2.stride(0), dH2.stride(0), dY2.stride(0), H2.stride(0),
                  _lib.dtype_code(dY2.dtype), _lib.dtype_code(W.dtype), _lib.stream_of(dY2))
    return dX


class Fast_RMS_Layernorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, W, eps, gemma=False):
        X2, W = _rows(X), W.contiguous()
        Y, r = rms_fwd(X2, W, eps, gemma)
        ctx.eps = eps
        ctx.GEMMA = bool(gemma)
        ctx.save_for_backward(X2, W, r)
        return Y.view(*X.shape)

    @staticmethod
    def backward(ctx, dY):
        dY2 = _rows(dY)
        X, W, r = ctx.saved_tensors
        dW = _weight_grad(dY2, X, r, W, ctx.needs_input_grad[1])       # (before the in-place pass overwrites dY)
        dX = rms_bwd_(dY2, X, W, r, gemma=ctx.GEMMA)
        return dX.view(*dY.shape), dW, None, None


class Fast_Add_RMS_Layernorm(torch.autograd.Function):
    """(h, y) = (X + residual, rmsnorm(X + residual) * W) in one pass over the activations; the backward adds the
    gradient that reaches h from the residual path inside the norm's backward kernel. Same numbers as
    `h = residual + X; y = Fast_RMS_Layernorm(h)` (llama.py:823-844) with the autograd accumulation of dh."""

    @staticmethod
    def forward(ctx, X, residual, W, eps):
        W = W.contiguous()
        H, Y, r = add_rms_fwd(X, residual, W, eps)
        ctx.set_materialize_grads(False)           # an unused h (last layer) arrives as dH = None, not as a zero tensor
        ctx.save_for_backward(H, W, r)
        return H.view(*X.shape), Y.view(*X.shape)

    @staticmethod
    def backward(ctx, dH, dY):
        H, W, r = ctx.saved_tensors
        if dY is None:                             # only the residual stream was used downstream
            return dH, dH, None, None
        dY2 = _rows(dY)
        dW = _weight_grad(dY2, H, r, W, ctx.needs_input_grad[2])
        dX = rms_bwd_(dY2, H, W, r, dH=dH).view(*dY.shape)        # written over dY, like rms_layernorm.py:218
        return dX, dX, dW, None


def add_rms_supported(X, W, residual=None):
    """shapes and layouts the fused kernel takes (otherwise: torch add + fast_rms_layernorm)."""
    vec = 16 // X.element_size()
    return (X.is_cuda and X.dtype in (torch.bfloat16, torch.float16, torch.float32) and X.shape[-1] % vec == 0
            and _add_width_ok(X) and W.dtype in (X.dtype, torch.float32)
            and _vec_layout(X, W, *(() if residual is None else (residual,))))


@torch.compiler.disable
def fast_add_rms_layernorm(layernorm, X, residual):
    """(residual + X, layernorm(residual + X)) -- the add of llama.py:833/:840 fused into the following norm."""
    W = layernorm.weight
    eps = layernorm.variance_epsilon if hasattr(layernorm, "variance_epsilon") else layernorm.eps
    if not add_rms_supported(X, W, residual):
        h = residual + X
        return h, Fast_RMS_Layernorm.apply(h, W, eps, False)
    return Fast_Add_RMS_Layernorm.apply(X, residual, W, eps)


@torch.compiler.disable
def fast_rms_layernorm(layernorm, X, gemma=False):
    """rms_layernorm.py:244-255."""
    W = layernorm.weight
    eps = layernorm.variance_epsilon if hasattr(layernorm, "variance_epsilon") else layernorm.eps
    return Fast_RMS_Layernorm.apply(X, W, eps, gemma)


from transformers.models.llama.modeling_llama import LlamaRMSNorm


class Unsloth_LlamaRMSNorm(LlamaRMSNorm):
    def forward(self, X):
        if not X.is_cuda:                        # a stock model on the host (e.g. an fp32 reference): HF's own forward
            return super().forward(X)
        return fast_rms_layernorm(self, X, gemma=False)


def patch_rms_layernorm():
    """rms_layernorm.py:277-286: swap the HF class so newly built models use the fast norm."""
    import transformers.models.llama.modeling_llama as m
    m.LlamaRMSNorm = Unsloth_LlamaRMSNorm


def unpatch_rms_layernorm():
    import transformers.models.llama.modeling_llama as m
    m.LlamaRMSNorm = LlamaRMSNorm
