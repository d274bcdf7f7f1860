"""Batched decode: ms per step and aggregate tokens/s of the token step at batch 1, 2, 4, 8, 16, 24, 32, 48, 64 -- Llama-3-8B
shape, NF4, LoRA r = 16, the benchmark's synthetic weights, context 2048.

Route `rows` is the step on uamd_gemv_rows (17 rows and up: uamd_gemv_rows64), replayed as a hipGraph (batch 1: the fused
single-sequence step, replayed). Route
`gemm` is the step through the 128 x 128-tile NF4 GEMM + separate LoRA / bias launches, eager, selected in the same process
with models.decode.BATCH_ROWS = False: what a batch > 1 cost before the rows kernel. The two routes alternate round by round;
every round decodes the same positions (the cache holds random keys: the step's traffic does not depend on their values).
One JSON line per (batch, route): median / min / max ms per step over the rounds, aggregate tokens/s at the median, and the
clocks the device reports.

`--kv-cache auto,fp8` measures the cache types of DecodeEngine instead: both on the `rows` route (batch 1: the 16-bit cache takes
the fused single-sequence step, the FP8 cache the 14-launch step -- the cost of leaving it), alternating round by round in the
one process; `--context` takes a list. Each line then also carries `kv_cache` and the KV bytes a step reads.

    python tools/decode_batch_bench.py [--layers 32] [--context 2048[,8192]] [--kv-cache auto[,fp8]] [--steps 32] [--rounds 5]
                                       [--out decode_batch.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def clocks():
    p = torch.cuda.get_device_properties(0)
    max_khz = getattr(p, "clock_rate", None)
    d = dict(device=p.name, cus=p.multi_processor_count, max_sclk_mhz=round(max_khz / 1e3) if max_khz else None)
    try:
        d["sclk_mhz_now"] = int(torch.cuda.clock_rate())          # the management library's current shader clock
    except Exception:
        d["sclk_mhz_now"] = None                                  # not reported here
    return d


def engine(model, batch, rows, context, start, kv_cache="auto"):
    from unsloth_amd.models import decode as MD
    MD.BATCH_ROWS = rows
    try:
        eng = MD.DecodeEngine(model, max_seq_len=context, batch=batch, use_graph=True,
                              **(dict(kv_cache_dtype=kv_cache) if kv_cache != "auto" else {}))
    finally:
        MD.BATCH_ROWS = True
    for c in eng.k_cache + eng.v_cache:
        if c.dtype == torch.uint8:
            c.random_(0, 0x78)                           # finite e4m3 codes (0x7f / 0xff are its NaNs)
        else:
            c.normal_()
    for c in (eng.k_scale or []) + (eng.v_scale or []):
        c.fill_(1.0 / 64)
    eng.kv_len.fill_(start)
    return eng


def kv_bytes_per_step(eng, start, steps):
    """Bytes of K and V (codes and scales) the attention of one step reads, at the middle position of a round."""
    pos = min(start + 1 + steps // 2, eng.S)
    row = eng.D * eng.k_cache[0].element_size() + (4 if eng.k_scale is not None else 0)
    return 2 * len(eng.k_cache) * eng.B * eng.Hk * pos * row


def run_round(eng, start, steps):
    eng.kv_len.fill_(start)
    tok = torch.zeros(eng.B, dtype=torch.long, device=eng.dev)
    eng.step(tok)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step(eng.next_tok)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="llama3-8b")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--context", default="2048", help="context length, or a comma-separated list of them")
    ap.add_argument("--kv-cache", default="auto", help="auto (the activation type), or a list such as auto,fp8: compare cache types")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1,2,4,8,16,24,32,48,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_batch_bench: needs the GPU; nothing is measured without one")
    import decode_bench
    out = open(a.out, "w") if a.out else None

    def emit(d):
        print(json.dumps(d), flush=True)
        if out:
            out.write(json.dumps(d) + "\n")
            out.flush()
    contexts = [int(c) for c in str(a.context).split(",")]
    kinds = a.kv_cache.split(",")
    a.context = max(contexts)                            # (the model's rotary tables cover the longest one)
    model = decode_bench.whole_model(a, "cuda")
    for context in contexts:
        a.context = context
        bench_context(a, model, kinds, emit)


def bench_context(a, model, kinds, emit):
    start = a.context - a.steps - 8
    base_ms = None
    for B in [int(b) for b in a.batches.split(",")]:
        if kinds != ["auto"]:
            routes = {"rows" if k == "auto" else f"rows_{k}": engine(model, B, True, a.context, start, k) for k in kinds}
        else:
            routes = {"rows": engine(model, B, True, a.context, start)}
            if B > 1:
                routes["gemm"] = engine(model, B, False, a.context, start)
                assert routes["rows"].rows and routes["rows"].use_graph and not routes["gemm"].rows and not routes["gemm"].use_graph
        ms = {k: [] for k in routes}
        for r in range(a.rounds + 1):                    # round 0 captures the graph and warms every launch
            for k, eng in routes.items():
                t = run_round(eng, start, a.steps if r else 3)
                if r:
                    ms[k].append(t)
        for k, v in ms.items():
            v = sorted(v)
            med = v[len(v) // 2]
            if B == 1 and base_ms is None:
                base_ms = med
            eng = routes[k]
            emit(dict(metric="decode step", batch=B, route=k, kv_cache=eng.kv_cache_dtype or "auto", hipgraph=eng.use_graph,
                      layers=a.layers, context=a.context, first_position=start, steps=a.steps, rounds=a.rounds,
                      ms_per_step=round(med, 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                      tokens_per_s=round(B / med * 1e3, 1), kv_bytes_per_step=kv_bytes_per_step(eng, start, a.steps),
                      step_over_batch1_step=round(med / base_ms, 3) if base_ms else None, **clocks()))
        del routes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
