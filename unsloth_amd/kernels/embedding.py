"""Token embedding through the HIP kernels (csrc/embedding.hip).

The reference leaves `embed_tokens` to torch.nn.Embedding: the lookup is an index_select and, when the table trains
(full_finetuning=True), the backward is `embedding_dense_backward` -- a dense [V, H] 16-bit temporary that is then copied or
added into the flat gradient bucket. Here the forward is a row gather with the weight's own bits and the backward sums each
run of equal (sorted) ids in fp32, rounds once and writes straight into the gradient's home: the parameter's sink
(full_finetune.FullGradBuckets), a caller-supplied view, or a fresh tensor for plain autograd. Deterministic: no atomics.
"""
import torch

from .. import _lib

_HALF = (torch.bfloat16, torch.float16)
_WS_SLOT = 42


def _rows_view(t, what):
    """`t` as the kernels take a matrix: 16-bit, unit column stride, 16-byte aligned rows. Raises otherwise."""
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16 or t.stride(0) < t.shape[1]:
        raise ValueError(f"fast_embedding: {what} must be a 2-D view with unit column stride and 16-byte aligned rows, got "
                         f"shape {tuple(t.shape)} strides {t.stride()}")
    return t


def _check(ids, weight):
    _lib.require_gpu(ids, weight)
    if weight.dtype not in _HALF or weight.dim() != 2 or weight.shape[1] % 8:
        raise TypeError(f"fast_embedding: the table must be bf16 / fp16 [V, H] with H % 8 == 0, got {weight.dtype} "
                        f"{tuple(weight.shape)}")
    if ids.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"fast_embedding: ids must be int64 / int32, got {ids.dtype}")


def embedding_fwd(ids, weight, out=None):
    """weight[ids] with the weight's bits, [*ids.shape, H]; `out`: a [ids.numel(), H] view to fill instead."""
    _check(ids, weight)
    W = _rows_view(weight, "the table")
    flat = ids.reshape(-1).to(torch.int64).contiguous()
    n, (V, H) = flat.numel(), W.shape
    if out is None:
        out = torch.empty((n, H), dtype=W.dtype, device=W.device)
    else:
        assert out.shape == (n, H) and out.dtype == W.dtype
    _rows_view(out, "out")
    _lib.call("uamd_embedding_fwd", W, _lib.ptr(flat), n, _lib.ptr(W), W.stride(0), V, H, _lib.ptr(out), out.stride(0),
              _lib.dtype_code(W.dtype), _lib.stream_of(W))
    return out.view(*ids.shape, H) if out.is_contiguous() else out


def embedding_bwd(ids, dY, num_embeddings, padding_idx=None, out=None, accumulate=False):
    """The table's gradient [V, H] in dY's dtype: out[v] (+)= sum of dY[t] over the tokens with ids[t] == v, each run summed in
    fp32 and rounded once. `out` None: a fresh tensor, every row defined. `out` given: overwritten entirely (rows without a
    token become zero) or, with `accumulate`, added to -- only the rows that have a token are touched."""
    _lib.require_gpu(ids, dY)
    H = dY.shape[-1]
    dY2 = dY.reshape(-1, H)
    if dY2.stride(1) != 1 or dY2.stride(0) % 8 or dY2.data_ptr() % 16:
        dY2 = dY2.contiguous()
    if out is None:
        out = torch.empty((num_embeddings, H), dtype=dY2.dtype, device=dY2.device)
        accumulate = False
    if tuple(out.shape) != (num_embeddings, H) or out.dtype != dY2.dtype or dY2.dtype not in _HALF:
        raise ValueError(f"fast_embedding: gradient target {out.dtype} {tuple(out.shape)} for dY {dY2.dtype} [*, {H}], "
                         f"V = {num_embeddings}")
    _rows_view(out, "the gradient target")
    # plumbing: ONE stable sort; the kernel finds the runs in it
    sorted_ids, order = torch.sort(ids.reshape(-1).to(torch.int64), stable=True)
    n = sorted_ids.numel()
    assert n == dY2.shape[0], (n, tuple(dY2.shape))
    from .. import nf4 as _nf4
    ws_elems = int(_lib.lib().uamd_embedding_bwd_workspace(n, H))
    ws = _nf4.scratch(dY2.device, max(ws_elems, 4), torch.float32, slot=_WS_SLOT)
    _lib.call("uamd_embedding_bwd", dY2, _lib.ptr(sorted_ids), _lib.ptr(order), n, _lib.ptr(dY2), dY2.stride(0), _lib.ptr(out),
              out.stride(0), num_embeddings, H, -1 if padding_idx is None else int(padding_idx), int(bool(accumulate)),
              _lib.ptr(ws), ws.numel(), _lib.dtype_code(dY2.dtype), _lib.stream_of(dY2))
    return out


class Fast_Embedding(torch.autograd.Function):
    """weight[ids]; the backward runs only when the table requires grad. Where its gradient goes: `grad_out` (a [V, H] view
    the caller owns: overwritten, or added to with `accumulate`; autograd then receives None), else the parameter's gradient
    sink (kernels/utils.GRAD_SINKS: overwritten by the step's first producer, added to after it), else it is returned."""

    @staticmethod
    def forward(ctx, ids, weight, padding_idx=None, grad_out=None, accumulate=False):
        ctx.save_for_backward(ids, weight)
        ctx.padding_idx, ctx.grad_out, ctx.accumulate = padding_idx, grad_out, bool(accumulate)
        return embedding_fwd(ids, weight)

    @staticmethod
    def backward(ctx, dY):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        ids, weight = ctx.saved_tensors
        V = weight.shape[0]
        if ctx.grad_out is not None:
            embedding_bwd(ids, dY, V, ctx.padding_idx, out=ctx.grad_out, accumulate=ctx.accumulate)
            return None, None, None, None, None
        from .utils import grad_sink
        sink = grad_sink(weight)
        if sink is not None:
            first = sink.first_write(weight) if hasattr(sink, "first_write") else False
            embedding_bwd(ids, dY, V, ctx.padding_idx, out=sink.grad_view(weight), accumulate=not first)
            sink.ready(weight)
            return None, None, None, None, None
        return None, embedding_bwd(ids, dY, V, ctx.padding_idx), None, None, None


@torch.compiler.disable
def fast_embedding(ids, weight, padding_idx=None, grad_out=None, accumulate=False):
    """torch.nn.functional.embedding(ids, weight, padding_idx) on the HIP kernels (bit-identical forward). `grad_out`: a
    [V, H] view that receives the table's gradient directly (a slice of a flat gradient bucket), `accumulate`: add to it."""
    _check(ids, weight)
    if padding_idx is not None and padding_idx < 0:
        padding_idx += weight.shape[0]
    return Fast_Embedding.apply(ids, weight, padding_idx, grad_out, accumulate)
