"""MoE expert block: the grouped HIP path against transformers' loop and against a loop over the dense GEMM.

Event-timed on one GPU in one process at the Qwen3-30B-A3B layer: T = 8192 tokens, k = 8, E = 128, H = 2048, I = 768, bf16,
once with uniform random routing (k distinct experts per token) and once with a skewed one (expert popularity ~ 1 / rank).
Series, run in turn (a / b / c / a / b / c, ...) so that drift hits all alike:

  a      moe_experts_forward                          plan, 3 grouped launches, SwiGLU, combine
  a_bwd  ... and its backward (d hidden, d top_k_weights)
  b      transformers' Qwen3MoeExperts.forward ("eager": the Python loop over the experts that were hit), b_bwd with autograd
  c      what the library could do before the grouped kernel: rows gathered by torch beforehand (not timed; the segment
         bounds are host integers, i.e. after a sync), then per expert one uamd_gemm_nt (gate and up as two groups sharing A)
         and one for down, SwiGLU over the whole buffer, un-permute and weighted sum in torch. Forward only.

and each of the three grouped launches alone (gate, up, down): FLOPs of the live rows (2 rows N K) / median time as a share of
the 2.5 PFLOP/s dense bf16 peak, plus the share of issued MFMA work spent on padding rows -- a wave issues MFMAs for its
64-row half of a 128-row tile iff the half holds a live row. One JSON line per (routing, series); needs the GPU.

    python tools/moe_experts_bench.py [--iters 30] [--warmup 5] [--out profiles/moe_experts_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unsloth_amd import _lib                                                                       # noqa: E402
from unsloth_amd.kernels import moe_experts_forward, moe_grouped_gemm, moe_plan, swiglu_fg_kernel  # noqa: E402
from unsloth_amd.kernels.utils import _group                                                       # noqa: E402

MFMA_PEAK = 2.5e15
T, K_TOP, E, H, I = 8192, 8, 128, 2048, 768


def routing(kind, g):
    p = torch.ones(E) if kind == "uniform" else 1.0 / torch.arange(1, E + 1)
    return torch.multinomial(p.expand(T, E), K_TOP, replacement=False, generator=g)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def dense_loop(Xs, gu, dn, bounds, inv, w):
    """Series c. Xs: hidden rows in sorted order [S, H]; bounds: host list of segment offsets; inv: slot -> sorted position."""
    S = Xs.shape[0]
    e, g, Ys = (torch.empty(S, n, dtype=Xs.dtype, device=Xs.device) for n in (I, I, H))
    code, st = _lib.dtype_code(Xs.dtype), _lib.stream_of(Xs)

    def gemm(A, groups):
        arr = (_lib.GemmGroup * len(groups))(*groups)
        _lib.call("uamd_gemm_nt", A, ctypes.c_void_p(A.data_ptr()), A.stride(0), A.shape[0], A.shape[1], arr, len(groups), 0, code, st)

    for x in range(E):
        a, b = bounds[x], bounds[x + 1]
        if b > a:
            gemm(Xs[a:b], [_group(gu[x, :I], e[a:b], I, H), _group(gu[x, I:], g[a:b], I, H)])
    h = swiglu_fg_kernel(e, g)
    for x in range(E):
        a, b = bounds[x], bounds[x + 1]
        if b > a:
            gemm(h[a:b], [_group(dn[x], Ys[a:b], H, I)])
    return (Ys[inv].view(T, K_TOP, H).float() * w[..., None].float()).sum(1).to(Xs.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_experts_bench: needs the GPU (a CPU run measures nothing)")
    from transformers.models.qwen3_moe.configuration_qwen3_moe import Qwen3MoeConfig
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts
    dev, dtype = torch.device("cuda"), torch.bfloat16
    g = torch.Generator().manual_seed(0)
    cfg = Qwen3MoeConfig(hidden_size=H, moe_intermediate_size=I, num_experts=E, num_experts_per_tok=K_TOP, hidden_act="silu")
    cfg._experts_implementation = "eager"
    with torch.device(dev):
        hf = Qwen3MoeExperts(cfg).to(dtype).requires_grad_(False)
    hf.gate_up_proj.copy_((torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dtype))
    hf.down_proj.copy_((torch.randn(E, H, I, generator=g) / I ** 0.5).to(dtype))
    gu, dn = hf.gate_up_proj.data, hf.down_proj.data
    x = torch.randn(T, H, generator=g).to(dtype).to(dev).requires_grad_()
    dout = torch.randn(T, H, generator=g).to(dtype).to(dev)
    out_path = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "moe_experts_bench.jsonl")
    lines = []
    for kind in ("uniform", "skewed"):
        idx = routing(kind, g).to(dev)
        w = torch.rand(T, K_TOP, generator=g)
        w = (w / w.sum(-1, keepdim=True)).to(dtype).to(dev).requires_grad_()
        plan = moe_plan(idx, E)
        bounds = plan.offsets.tolist()
        counts = torch.tensor(bounds[1:]) - torch.tensor(bounds[:-1])
        live, issued = int(counts.sum()), int(((counts + 63) // 64).sum()) * 64
        rows = plan.rows.long()
        Xs = x.detach()[rows // K_TOP].contiguous()
        inv = torch.empty_like(rows)
        inv[rows] = torch.arange(rows.numel(), device=dev)
        bufs = [torch.empty(plan.S, n, dtype=dtype, device=dev) for n in (I, I, H)]

        def fwd_bwd(f):
            out = f(x, idx, w)
            torch.autograd.grad(out, (x, w), dout)

        new = lambda x_, i_, w_: moe_experts_forward(x_, gu, dn, i_, w_)
        series = {
            "a": lambda: new(x.detach(), idx, w.detach()), "b": lambda: hf(x.detach(), idx, w.detach()),
            "c": lambda: dense_loop(Xs, gu, dn, bounds, inv, w.detach()),
            "a_bwd": lambda: fwd_bwd(new), "b_bwd": lambda: fwd_bwd(hf),
            "gate": lambda: moe_grouped_gemm(x.detach(), gu[:, :I], plan, bufs[0], gather=True),
            "up": lambda: moe_grouped_gemm(x.detach(), gu[:, I:], plan, bufs[1], gather=True),
            "down": lambda: moe_grouped_gemm(bufs[0], dn, plan, bufs[2], scatter=True),
        }
        ref = series["b"]().float()
        for name in ("a", "c"):
            diff = float((series[name]().float() - ref).norm() / ref.norm())
            assert diff < 2e-2, (name, diff)            # same function: bf16 rounding of three GEMMs apart
        times = {n: [] for n in series}
        for it in range(args.warmup + args.iters):
            for n, fn in series.items():
                t = timed(fn)
                if it >= args.warmup:
                    times[n].append(t)
        for n, ts in times.items():
            rec = dict(routing=kind, series=n, T=T, k=K_TOP, E=E, H=H, I=I, dtype="bf16", iters=args.iters,
                       median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                       largest_segment=int(counts.max()), smallest_segment=int(counts.min()))
            if n in ("gate", "up", "down"):
                flops = 2.0 * live * I * H
                rec.update(live_rows=live, mfma_rows_issued=issued, padding_share=round(1 - live / issued, 4),
                           tflops=round(flops / (rec["median_ms"] * 1e-3) / 1e12, 1),
                           frac_mfma_peak=round(flops / (rec["median_ms"] * 1e-3) / MFMA_PEAK, 4))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
