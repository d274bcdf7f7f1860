"""Qwen3's per-head q_norm / k_norm + RoPE: the fused launch against the torch formulation it replaces.

Two things, event-timed on one GPU in one process, alternating A / B / A / B so that drift hits both alike. Both work in
place on the strided q|k views of one fused [tokens, (Hq + 2 Hk) D] projection buffer (their outputs feed back as the next
inputs: a norm followed by a rotation keeps the magnitudes where they are):

  A  uamd_qk_norm_rope_fwd        one launch, nothing kept for a backward (r and the pre-norm rows are extra writes of a
                                  training forward; a second series "A_keep" times the launch that writes them)
  B  the torch formulation        per head: reshape, fp32 upcast, pow / mean / rsqrt, two multiplies, a cast -- transformers'
                                  Qwen3RMSNorm on q and on k -- written back, then fast_rope_embedding (uamd_rope_embedding_qk)

Shape: 8192 tokens x (32 + 8) heads x 128, bf16 (Qwen3-8B at 4 x 2048 tokens). Warm-up first, then the median of --iters runs.
For A: bytes moved = one read and one write of q|k (A_keep: plus r and the pre-norm copy), over the median, as a fraction of
the 8.0 TB/s HBM peak. The q|k views are 84 MB, less than the 256 MB Infinity Cache: each series finds what the pass before
it left there, so the fraction is an upper figure for a training step, where a GEMM's output arrives from HBM. One JSON line
per series; needs the GPU.

    python tools/qk_norm_rope_bench.py [--iters 30] [--warmup 5] [--out profiles/qk_norm_rope_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unsloth_amd.kernels.rope_embedding import fast_rope_embedding, qk_norm_rope_fwd_          # noqa: E402

HBM_PEAK = 8.0e12
B, T, HQ, HK, D = 4, 2048, 32, 8, 128
EPS = 1e-6


def torch_norm(x4, w):
    """transformers' Qwen3RMSNorm on a [B, T, H, D] view, written back where it was read."""
    h = x4.to(torch.float32)
    h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS)
    x4.copy_(w * h.to(x4.dtype))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qk_norm_rope_bench: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    N = B * T
    qkv = torch.randn(N, (HQ + 2 * HK) * D, device=dev, generator=gen).to(torch.bfloat16)
    w = (torch.rand(2, D, device=dev, generator=gen) * 0.5 + 0.75).to(torch.bfloat16)
    ang = torch.arange(T, device=dev)[:, None] * (1e6 ** (-torch.arange(D // 2, device=dev) * 2.0 / D))[None]
    cos, sin = ang.cos().to(torch.bfloat16), ang.sin().to(torch.bfloat16)
    q4 = qkv[:, :HQ * D].view(B, T, HQ, D)
    k4 = qkv[:, HQ * D:(HQ + HK) * D].view(B, T, HK, D)
    Q, K = q4.transpose(1, 2), k4.transpose(1, 2)

    def torch_formulation():
        torch_norm(q4, w[0])
        torch_norm(k4, w[1])
        fast_rope_embedding(Q, K, cos, sin, None)

    with torch.no_grad():
        series = {"uamd_qk_norm_rope_fwd": lambda: qk_norm_rope_fwd_(Q, K, w[0], w[1], EPS, cos, sin, None, False),
                  "torch_norm_then_uamd_rope": torch_formulation,
                  "uamd_qk_norm_rope_fwd_keep": lambda: qk_norm_rope_fwd_(Q, K, w[0], w[1], EPS, cos, sin, None, True)}
        ms = {k: [] for k in series}
        for group in (("uamd_qk_norm_rope_fwd", "torch_norm_then_uamd_rope"), ("uamd_qk_norm_rope_fwd_keep",)):
            for i in range(args.warmup + args.iters):
                for name in group:
                    t = timed(series[name])
                    if i >= args.warmup:
                        ms[name].append(t)
    rows = N * (HQ + HK)
    moved = {"uamd_qk_norm_rope_fwd": rows * (2 * D * 2), "uamd_qk_norm_rope_fwd_keep": rows * (3 * D * 2 + 4)}
    lines = []
    for name in series:
        med = statistics.median(ms[name])
        rec = dict(series=name, tokens=N, heads_q=HQ, heads_k=HK, head_dim=D, dtype="bf16", iters=args.iters,
                   ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4))
        if name in moved:
            rec.update(bytes_moved=moved[name], tb_per_s=round(moved[name] / med / 1e9, 3),
                       hbm_peak_fraction=round(moved[name] / (med * 1e-3) / HBM_PEAK, 3))
        lines.append(json.dumps(rec))
    lines.append(json.dumps(dict(series="torch_over_fused", ratio=round(
        statistics.median(ms["torch_norm_then_uamd_rope"]) / statistics.median(ms["uamd_qk_norm_rope_fwd"]), 3))))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
