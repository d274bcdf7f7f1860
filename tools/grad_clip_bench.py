"""Gradient clipping inside the optimizer step (max_grad_norm): what it costs and what the host round trip cost before it.

Device events, median of --iters after --warmup, one process, the series alternating round by round on the SAME buffers; one
timed window is --burst back-to-back steps. Two shapes:

  lora   optim.FlatAdamW over the flat fp32 arena of Llama-3-8B r=16: 41.9 M parameters, 168 MB per stream
  shard  one rank's bf16 shard (DP = 8) of a Llama-3-8B decoder-layer bucket, 27.3 M parameters: the launches of
         full_finetune.ShardedAdamW on raw buffers (uamd_adamw_shard / _clip), no model behind them

Series:
  a_host_clip   the only way to clip before: norm by torch (`arena.norm()` / the shard's `.float().pow(2).sum().sqrt()`) ->
                float() -> step(grad_scale=...). The events see the device idle while the host waits and relaunches.
  b_device_clip step() with max_grad_norm: uamd_grad_sumsq + uamd_grad_clip_coef + the *_clip AdamW, nothing read back
  c_no_clip     the plain step
  norm_only     uamd_grad_sumsq + uamd_grad_clip_coef alone; bytes read / time against the 8.0 TB/s HBM peak. Between two of its
                windows the other series stream four to eight times the gradient's size, so it does not find the gradient cached.
The step zeroes the LoRA gradient arena, so after the first round the norms are taken over zeros: the kernels' time does not
depend on the values.

    python tools/grad_clip_bench.py [--iters 30] [--warmup 5] [--burst 5] [--out profiles/grad_clip_bench.jsonl]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from token_logprob_bench import alternate, stats  # noqa: E402

HBM_PEAK = 8.0e12
HYPER = (2e-4, 0.9, 0.999, 1e-8, 0.01, 1 - 0.9 ** 5, math.sqrt(1 - 0.999 ** 5))


class Factors(torch.nn.Module):
    """32 layers x 7 projections' worth of LoRA factors as two parameters per layer: 41,943,040 fp32 elements in all."""

    def __init__(self, dev):
        super().__init__()
        self.layers = torch.nn.ModuleList()
        for _ in range(32):
            m = torch.nn.Module()
            m.lora_A = torch.nn.Parameter(torch.randn(16, 40960, device=dev) * 0.02)
            m.lora_B = torch.nn.Parameter(torch.zeros(40960, 16, device=dev))
            self.layers.append(m)


def lora(dev):
    from unsloth_amd.optim import FlatAdamW
    opt = FlatAdamW(Factors(dev), lr=2e-4)
    opt.arena.arena.normal_(0.0, 1e-3)

    def host_clip(_):
        opt.max_grad_norm = None
        opt.step(grad_scale=min(1.0, 1.0 / (float(opt.arena.arena.norm()) + 1e-6)))

    def device_clip(_):
        opt.max_grad_norm = 1.0
        opt.step()

    def no_clip(_):
        opt.max_grad_norm = None
        opt.step()
    series = {"a_host_clip": host_clip, "b_device_clip": device_clip, "c_no_clip": no_clip,
              "norm_only": lambda _: opt._norm([[0, opt.flat_p.numel()]], 1.0, 1)}
    return series, opt.flat_p.numel(), 4, opt


def shard(dev):
    from unsloth_amd import _lib
    from unsloth_amd.optim import GradNorm
    n = 27_264_000
    p32, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    g16, p16 = (torch.randn(n, device=dev) * 1e-3).bfloat16(), torch.empty(n, dtype=torch.bfloat16, device=dev)
    gn = GradNorm(dev, 1024)

    def step(scale, clip=()):
        _lib.call("uamd_adamw_shard_clip" if clip else "uamd_adamw_shard", p32, p32.data_ptr(), g16.data_ptr(), p16.data_ptr(),
                  m.data_ptr(), v.data_ptr(), n, *HYPER, scale, _lib.UAMD_BF16, *clip, _lib.stream_of(p32))
    series = {"a_host_clip": lambda _: step(min(1.0, 1.0 / (float(g16.float().pow(2).sum().sqrt()) + 1e-6))),
              "b_device_clip": lambda _: step(1.0, (gn.run([g16], 1.0, 0).data_ptr() + 4,)),
              "c_no_clip": lambda _: step(1.0),
              "norm_only": lambda _: gn.run([g16], 1.0, 1)}
    return series, n, 2, (p32, m, v, g16, p16, gn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench: needs the GPU; nothing is measured without one")
    out = open(a.out, "w") if a.out else None
    dev = torch.device("cuda", 0)
    for shape, build in (("lora", lora), ("shard", shard)):
        series, n, elem, keep = build(dev)
        ms = alternate(series, a.iters, a.warmup, a.burst)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            d = dict(metric="grad_clip", shape=shape, series=k, elements=n, grad_bytes=n * elem, burst=a.burst, iters=a.iters,
                     **stats(v))
            if k == "b_device_clip":
                d.update(clip_cost_ms=round(med[k] - med["c_no_clip"], 5), saved_vs_host_ms=round(med["a_host_clip"] - med[k], 5))
            if k == "norm_only":
                d.update(tb_per_s=round(n * elem / med[k] / 1e9, 3), hbm_peak_fraction=round(n * elem / (med[k] * 1e-3) / HBM_PEAK, 3))
            print(json.dumps(d), flush=True)
            if out:
                out.write(json.dumps(d) + "\n")
                out.flush()
        del series, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
