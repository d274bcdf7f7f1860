"""A/B of the MLP backward's streaming group at Llama-3-8B widths (8192 / 4096 / 2048 x 14336, r = 16, bf16):
  old = glu_bwd_terms (activation backward + row products, writes h) + the six-problem lora_tn launch
  new = glu_bwd_tn (the same + the three wide gradients, h never written) + the three-problem lora_tn launch
Both variants interleaved in one process, each timed `cold` (straight after the copies that restore e and g: 470 MB through the
caches) and `burst` (after a burst of large GEMMs, as in the training step). Prints one JSON line per token count."""
import json
import sys

import torch

sys.path.insert(0, ".")
from unsloth_amd.kernels import utils as U  # noqa: E402

U.GLU_FUSED = "all"
dev = torch.device("cuda", 0)
g_ = torch.Generator().manual_seed(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def mk(o, i, r, dt):
    return ((torch.randn(o, i, generator=g_) * 0.02).to(dt).to(dev), None, (torch.randn(r, i, generator=g_) * 0.02).to(dev),
            (torch.randn(o, r, generator=g_) * 0.02).to(dev), 2.0)


for M in (8192, 4096, 2048):
    K, H, r, dt = 14336, 4096, 16, torch.bfloat16
    ld = 2 * K + 64                                         # e | g as the step has them (fast_lora._gate_up)
    eg0 = torch.randn(M, ld, generator=g_).to(dt).to(dev)
    eg = eg0.clone()
    e, g = eg[:, :K], eg[:, K:2 * K]
    DW0 = (torch.randn(M, ld, generator=g_) * 0.1).to(dt).to(dev)
    DWb = DW0.clone()
    DW = DWb[:, :K]
    X = torch.randn(M, H, generator=g_).to(dt).to(dev)
    dY = (torch.randn(M, H, generator=g_) * 0.1).to(dt).to(dev)
    down, up, gate = mk(H, K, r, dt), mk(K, H, r, dt), mk(K, H, r, dt)
    p_d = dY.float() @ down[3].to(dt).float()
    xa_d = torch.randn(M, r, generator=g_).to(dev)
    xa_u = X.float() @ up[2].to(dt).float().t()
    xa_g = X.float() @ gate[2].to(dt).float().t()
    ga, gb = torch.randn(8192, 4096, device=dev, dtype=dt), torch.randn(4096, 8192, device=dev, dtype=dt)

    def old():
        h, df, de, (pu, pg) = U.glu_bwd_terms("swiglu", DW, e, g, up, gate)
        U.lora_tn([(p_d, h, r, False, 2.0), (xa_d, dY, r, True, 2.0), (pu.P, X, r, False, 2.0), (xa_u, df, r, True, 2.0),
                   (pg.P, X, r, False, 2.0), (xa_g, de, r, True, 2.0)])

    def new():
        df, de, (pu, pg), _ = U.glu_bwd_tn("swiglu", DW, e, g, up, gate, down, p_d, xa_u, xa_g)
        U.lora_tn([(xa_d, dY, r, True, 2.0), (pu.P, X, r, False, 2.0), (pg.P, X, r, False, 2.0)])

    def once(fn, burst):
        eg.copy_(eg0)                                       # both variants work in place: the same inputs every time
        DWb.copy_(DW0)
        if burst:
            for _ in range(6):
                ga @ gb
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        return s.elapsed_time(t) * 1e3

    for fn in (old, new):
        for _ in range(2):
            once(fn, True)
    times = {"old_cold": [], "new_cold": [], "old_burst": [], "new_burst": []}
    for _ in range(REPS):
        for name, fn in (("old", old), ("new", new)):
            for mode in ("cold", "burst"):
                times[f"{name}_{mode}"].append(once(fn, mode == "burst"))
    med = {k: round(sorted(v)[len(v) // 2], 1) for k, v in times.items()}
    print(json.dumps(dict(tokens=M, width=K, r=r, reps=REPS, unit="us, median", **med,
                          min={k: round(min(v), 1) for k, v in times.items()})), flush=True)
