"""AdamW step kernels, fp32 moments against 8-bit moments (csrc/adamw.hip), on the two sizes that matter:

  flat   42 M fp32 LoRA parameters (the 168 MB arena of Llama-3-8B r=16): uamd_adamw_flat  vs uamd_adamw8_flat
  shard  218 M bf16 parameters (one Llama-3-8B decoder layer):            uamd_adamw_shard vs uamd_adamw8_shard

Per launch: device events around the launch alone (the gradient is refilled outside the timed pair, because the flat step
zeroes it), warm-up launches first, median / min / max over --iters. The order is fp32, 8-bit, fp32 again: the two fp32
series of one session give the run-to-run spread the 8-bit figure is read against. GB/s = each kernel's own bytes per
parameter (flat 32 / 20 B, shard 28 / 16 B) over the median. One JSON line per series; needs the GPU.

    python tools/adamw8_bench.py [--iters 40] [--warmup 10] [--out profiles/adamw8_bench.jsonl]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unsloth_amd import _lib                                           # noqa: E402
from unsloth_amd.optim import QBLOCK, adam8_maps, adam8_zero_code      # noqa: E402

LAYER = 2 * 4096 * 4096 + 2 * 4096 * 1024 + 3 * 4096 * 14336 + 2 * 4096          # Llama-3-8B decoder layer: 218 112 000
SIZES = dict(flat=42 * 1000 * 1000, shard=LAYER)
BYTES = {("flat", 32): 32, ("flat", 8): 20, ("shard", 32): 28, ("shard", 8): 16}
LR, B1, B2, EPS, WD = 2e-4, 0.9, 0.999, 1e-8, 0.01


class Case:
    def __init__(self, kind, bits, n, dev):
        self.kind, self.bits, self.n, self.t = kind, bits, n, 0
        gen = torch.Generator(device=dev).manual_seed(0)
        self.p = torch.randn(n, device=dev, generator=gen) * 0.02
        gdt = torch.float32 if kind == "flat" else torch.bfloat16
        self.g_src = (torch.randn(n, device=dev, generator=gen) * 0.01).to(gdt)
        self.g = self.g_src.clone()
        self.p16 = self.p.to(torch.bfloat16) if kind == "shard" else None
        if bits == 8:
            self.code_m, self.code_v = adam8_maps(dev)
            nblk = (n + QBLOCK - 1) // QBLOCK
            self.m = torch.full((n,), adam8_zero_code(self.code_m), dtype=torch.uint8, device=dev)
            self.v = torch.full((n,), adam8_zero_code(self.code_v), dtype=torch.uint8, device=dev)
            self.am, self.av = torch.zeros(nblk, device=dev), torch.zeros(nblk, device=dev)
        else:
            self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)

    def state_bytes(self):
        t = [self.m, self.v] + ([self.am, self.av] if self.bits == 8 else [])
        return sum(x.numel() * x.element_size() for x in t)

    def launch(self):
        self.t += 1
        hyper = (LR, B1, B2, EPS, WD, 1.0 - B1 ** self.t, math.sqrt(1.0 - B2 ** self.t), 1.0)
        st = _lib.stream_of(self.p)
        L, P = _lib.lib(), (lambda x: x.data_ptr())
        if self.kind == "flat" and self.bits == 32:
            rc = L.uamd_adamw_flat(P(self.p), P(self.g), P(self.m), P(self.v), self.n, *hyper, 1, st)
        elif self.kind == "flat":
            rc = L.uamd_adamw8_flat(P(self.p), P(self.g), P(self.m), P(self.v), P(self.am), P(self.av), P(self.code_m),
                                    P(self.code_v), self.n, *hyper, 1, st)
        elif self.bits == 32:
            rc = L.uamd_adamw_shard(P(self.p), P(self.g), P(self.p16), P(self.m), P(self.v), self.n, *hyper,
                                    _lib.UAMD_BF16, st)
        else:
            rc = L.uamd_adamw8_shard(P(self.p), P(self.g), P(self.p16), P(self.m), P(self.v), P(self.am), P(self.av),
                                     P(self.code_m), P(self.code_v), self.n, 0, self.n - 4096, *hyper, _lib.UAMD_BF16, st)
        _lib.check(rc, f"adamw {self.kind} {self.bits}")

    def series(self, warmup, iters):
        ms = []
        for i in range(warmup + iters):
            self.g.copy_(self.g_src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.launch()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw8_bench: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    lines = []
    for kind, n in SIZES.items():
        for label, bits in (("fp32", 32), ("8bit", 8), ("fp32-again", 32)):
            c = Case(kind, bits, n, dev)
            ms = c.series(args.warmup, args.iters)
            med = statistics.median(ms)
            rec = dict(kernel=f"uamd_adamw{'8' if bits == 8 else ''}_{kind}", series=label, n=n, ms_median=round(med, 4),
                       ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), bytes_per_param=BYTES[(kind, bits)],
                       gb_per_s=round(BYTES[(kind, bits)] * n / med / 1e6, 1), state_bytes=c.state_bytes(),
                       finite=bool(torch.isfinite(c.p).all()))
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            del c
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
