"""QuickGELU (x * sigmoid(1.702 x)) through the HIP kernels (csrc/glu.hip: uamd_quick_gelu_forward / _backward): the activation
of Qwen2-VL's vision MLP (BASELINE config 4). The reference's VLM path compiles HF's module tree (unsloth/models/vision.py:
881-1990, unsloth_zoo compiler -- third party); the semantics restated here are transformers' QuickGELUActivation. The backward
writes dX IN PLACE over dY, like the SwiGLU / GeGLU backward kernels of the language tower."""
import torch

from .. import _lib
from .swiglu import _flat16


class Fast_QuickGELU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X):
        _lib.require_gpu(X)
        Xc = _flat16(X)
        Y = torch.empty_like(Xc)
        _lib.call("uamd_quick_gelu_forward", Xc, _lib.ptr(Xc), _lib.ptr(Y), Xc.numel(), _lib.dtype_code(Xc.dtype),
                  _lib.stream_of(Xc))
        ctx.save_for_backward(Xc)
        return Y.view(X.shape)

    @staticmethod
    def backward(ctx, dY):
        (X,) = ctx.saved_tensors
        d = dY if (dY.is_contiguous() and dY.dtype == X.dtype) else dY.to(X.dtype).contiguous()
        buf = _flat16(d)
        _lib.call("uamd_quick_gelu_backward", d, _lib.ptr(X), _lib.ptr(buf), X.numel(), _lib.dtype_code(X.dtype),
                  _lib.stream_of(d))
        if buf is not d:                        # dY off the 16-byte grid went through an aligned copy: back in place
            d.copy_(buf)
        return d.view(dY.shape)


def fast_quick_gelu(X):
    return Fast_QuickGELU.apply(X)
