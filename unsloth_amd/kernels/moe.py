"""Mixture-of-experts expert block on the HIP kernels of csrc/moe.hip: the contract of transformers'
Qwen3MoeExperts.forward (modeling_qwen3_moe.py) without its Python loop over experts, its host sync and its 16-bit sum over
the k slots of a token. Routing plan, ragged grouped GEMMs with the permutation fused into their loads and stores, the existing
SwiGLU kernels, and a one-pass combine; frozen expert weights (the grouped dW kernel does not exist yet)."""
from collections import namedtuple

import torch

from .. import _lib
from .swiglu import swiglu_DWf_DW_dfg_kernel, swiglu_fg_kernel

MoePlan = namedtuple("MoePlan", "offsets rows tiles S E k")


def _ids(top_k_index):
    if top_k_index.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"top_k_index must be int64 or int32, got {top_k_index.dtype}")
    return top_k_index.contiguous(), int(top_k_index.dtype == torch.int64)


def moe_plan(top_k_index, num_experts):
    """Routing metadata of `top_k_index` [T, k] on its device, no host sync: MoePlan(offsets [E + 1], rows [S], tiles)."""
    _lib.require_gpu(top_k_index)
    ids, idx64 = _ids(top_k_index)
    S, E, k = ids.numel(), int(num_experts), ids.shape[-1]
    lib = _lib.lib()
    new = lambda n: torch.empty(n, dtype=torch.int32, device=ids.device)
    offsets, rows, tiles = new(E + 1), new(S), new(1 + 2 * lib.uamd_moe_max_tiles(S, E))
    ws = new(lib.uamd_moe_plan_workspace(S, E))
    _lib.call("uamd_moe_plan", ids, _lib.ptr(ids), idx64, S, E, _lib.ptr(offsets), _lib.ptr(rows), _lib.ptr(tiles), _lib.ptr(ws),
              ws.numel(), _lib.stream_of(ids))
    return MoePlan(offsets, rows, tiles, S, E, k)


def moe_grouped_gemm(A, W, plan, C, form="nt", gather=False, scatter=False, row_scale=None, accumulate=False):
    """C[c_row(s)] (+)= row_scale(s) * (A[a_row(s)] @ op(W[e])) for every sorted row s of every expert e of `plan`.

    W: [E, N, K] (form "nt") or [E, K, N] (form "nn"), any view with contiguous rows. gather: a_row(s) = rows[s] // k (A is
    [T, K]), else s; scatter: c_row(s) = rows[s], else s; row_scale: fp32 [S] indexed by rows[s]. C is written in place."""
    _lib.require_gpu(A, W, C, row_scale)
    if form not in ("nt", "nn"):
        raise ValueError(f"form must be 'nt' or 'nn', got {form!r}")
    N, K = (W.shape[1], W.shape[2]) if form == "nt" else (W.shape[2], W.shape[1])
    if W.shape[0] != plan.E or A.shape[1] != K or C.shape[1] != N or A.dtype != W.dtype or A.dtype != C.dtype:
        raise ValueError("moe_grouped_gemm: shapes / dtypes of A, W, C and the plan do not agree")
    if A.stride(1) != 1 or W.stride(2) != 1 or C.stride(1) != 1:
        raise ValueError("moe_grouped_gemm: rows of A, W and C must be contiguous")
    if A.shape[0] < (plan.S // plan.k if gather else plan.S) or C.shape[0] < plan.S:
        raise ValueError("moe_grouped_gemm: A or C has fewer rows than the plan addresses")
    if row_scale is not None and (row_scale.dtype != torch.float32 or not row_scale.is_contiguous() or row_scale.numel() != plan.S):
        raise ValueError("moe_grouped_gemm: row_scale must be a contiguous fp32 tensor with one entry per slot")
    _lib.call("uamd_moe_gemm", A, _lib.ptr(A), A.stride(0), _lib.ptr(W), W.stride(1), W.stride(0), _lib.ptr(C), C.stride(0),
              _lib.ptr(plan.offsets), _lib.ptr(plan.rows), _lib.ptr(plan.tiles), _lib.ptr(row_scale), plan.S, plan.E, N, K, plan.k,
              int(form == "nn"), int(gather), int(scatter), int(accumulate), _lib.dtype_code(A.dtype), _lib.stream_of(A))
    return C


def _combine_fwd(Y, w, ids, idx64, E, T, k):
    out = torch.empty(T, Y.shape[1], dtype=Y.dtype, device=Y.device)
    _lib.call("uamd_moe_combine_fwd", Y, _lib.ptr(Y), Y.stride(0), _lib.ptr(w), _lib.ptr(ids), idx64, E, _lib.ptr(out),
              out.stride(0), T, k, Y.shape[1], _lib.dtype_code(Y.dtype), _lib.stream_of(Y))
    return out


class Fast_MoeExperts(torch.autograd.Function):
    """out[t] = sum_j w[t, j] * down_e(silu(gate_e(x_t)) * up_e(x_t)), e = top_k_index[t, j]. Kept for the backward: the two
    [S, I] GEMM outputs e and g in sorted order, the per-slot down output Y [S, H], the fp32 weights and the plan."""

    @staticmethod
    def forward(ctx, hidden, gate_up_proj, down_proj, top_k_index, top_k_weights):
        T, H = hidden.shape
        E, I2, _ = gate_up_proj.shape
        I, k = I2 // 2, top_k_index.shape[-1]
        X = hidden if hidden.stride(1) == 1 and hidden.stride(0) % 8 == 0 and hidden.data_ptr() % 16 == 0 else hidden.contiguous().clone()
        plan = moe_plan(top_k_index, E)
        ids, idx64 = _ids(top_k_index)
        wf = top_k_weights.detach().float().contiguous().view(-1)
        new = lambda n: torch.empty(plan.S, n, dtype=X.dtype, device=X.device)
        e = moe_grouped_gemm(X, gate_up_proj[:, :I], plan, new(I), gather=True)
        g = moe_grouped_gemm(X, gate_up_proj[:, I:], plan, new(I), gather=True)
        h = swiglu_fg_kernel(e, g)
        Y = moe_grouped_gemm(h, down_proj, plan, new(H), scatter=True)
        out = _combine_fwd(Y, wf, ids, idx64, E, T, k)
        ctx.save_for_backward(gate_up_proj, down_proj, ids, wf, e, g, Y, *plan[:3])
        ctx.meta = (idx64, T, k, E, I, top_k_weights.dtype)
        return out

    @staticmethod
    def backward(ctx, dOut):
        gate_up_proj, down_proj, ids, wf, e, g, Y, offsets, rows, tiles = ctx.saved_tensors
        idx64, T, k, E, I, w_dtype = ctx.meta
        plan = MoePlan(offsets, rows, tiles, T * k, E, k)
        dOut = dOut if dOut.stride(1) == 1 and dOut.stride(0) % 8 == 0 and dOut.data_ptr() % 16 == 0 else dOut.contiguous().clone()
        H = dOut.shape[1]
        dw = torch.empty(T, k, dtype=torch.float32, device=dOut.device)
        _lib.call("uamd_moe_combine_bwd", dOut, _lib.ptr(dOut), dOut.stride(0), _lib.ptr(Y), Y.stride(0), _lib.ptr(ids), idx64, E,
                  _lib.ptr(dw), T, k, H, _lib.dtype_code(dOut.dtype), _lib.stream_of(dOut))
        # dH[s] = w[rows[s]] * dOut[rows[s] // k] @ down_e, then the in-place SwiGLU backward: e <- d(up), g <- d(gate). e and g
        # are rewritten in place, so a second backward through the same graph is refused by autograd's version check.
        dH = torch.empty_like(e)
        moe_grouped_gemm(dOut, down_proj, plan, dH, form="nn", gather=True, row_scale=wf)
        swiglu_DWf_DW_dfg_kernel(dH, e, g)
        dX = torch.empty(plan.S, H, dtype=dOut.dtype, device=dOut.device)
        moe_grouped_gemm(g, gate_up_proj[:, :I], plan, dX, form="nn", scatter=True)
        moe_grouped_gemm(e, gate_up_proj[:, I:], plan, dX, form="nn", scatter=True, accumulate=True)
        return _combine_fwd(dX, None, ids, idx64, E, T, k), None, None, None, dw.to(w_dtype)


def moe_experts_forward(hidden, gate_up_proj, down_proj, top_k_index, top_k_weights):
    """Qwen3MoeExperts.forward (SiLU gate) on the HIP kernels: hidden [T, H], gate_up_proj [E, 2I, H], down_proj [E, H, I],
    top_k_index / top_k_weights [T, k] -> [T, H]. Differentiable in `hidden` and `top_k_weights`; the expert weights are frozen."""
    _lib.require_gpu(hidden, gate_up_proj, down_proj, top_k_index, top_k_weights)
    if gate_up_proj.requires_grad or down_proj.requires_grad:
        raise NotImplementedError("moe_experts_forward: the expert weights must be frozen -- the grouped dW kernel (the weight "
                                  "gradient of the ragged grouped GEMM) is not implemented")
    if hidden.dtype not in (torch.bfloat16, torch.float16) or gate_up_proj.dtype != hidden.dtype or down_proj.dtype != hidden.dtype:
        raise TypeError("moe_experts_forward: hidden and the expert weights must share bf16 or fp16")
    return Fast_MoeExperts.apply(hidden, gate_up_proj, down_proj, top_k_index, top_k_weights)


def _hf_experts_forward(original):
    def forward(self, hidden_states, top_k_index, top_k_weights):
        if (not hidden_states.is_cuda or hidden_states.dtype not in (torch.bfloat16, torch.float16)
                or hidden_states.dim() != 2 or self.gate_up_proj.dtype != hidden_states.dtype
                or self.gate_up_proj.requires_grad or self.down_proj.requires_grad
                or getattr(getattr(self, "config", None), "hidden_act", None) != "silu"):
            return original(self, hidden_states, top_k_index, top_k_weights)
        return moe_experts_forward(hidden_states, self.gate_up_proj, self.down_proj, top_k_index, top_k_weights)
    return forward


def patch_moe_experts():
    """Route transformers' Qwen3MoeExperts.forward through moe_experts_forward (CUDA tensors in bf16 / fp16, frozen expert
    weights, SiLU); anything else still reaches the original. models.llama.unpatch_all() restores the class."""
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts
    from ..models.llama import _patch_method
    _patch_method(Qwen3MoeExperts, "forward", _hf_experts_forward)
