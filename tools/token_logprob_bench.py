"""Log-prob / entropy of the chosen token inside the decode step (uamd_token_logprob_f32): what it costs and what it saves.

Three measurements, device events, median of --iters after --warmup, one process, series alternating round by round:

  pair     the two launches alone on fp32 logits [1, 128256] and [64, 128256] next to uamd_argmax_f32 on the same logits (the
           launch pair the greedy step already has). One timed window is --burst back-to-back calls (a single 8 us call is below
           what an event pair resolves). `hot`: every call reads the same logits -- where the step finds them, the lm_head just
           wrote them; `cold`: the calls walk buffers of 640 MB in turn, past the 256 MB Infinity Cache. Bytes read / time against
           the 8.0 TB/s HBM peak (a plain copy reaches about 6.3).
  step     the captured token step of the benchmark's Llama-3-8B-shaped NF4 model at context 2048, batch 1 and batch 64: tracking
           on (log-prob + entropy) against tracking off, two engines in one session.
  rollout  one get_per_token_logps_and_entropies call over a 64 x (2048 + 256) rollout: the forward a tracked generation spares.

    python tools/token_logprob_bench.py [--layers 32] [--iters 30] [--warmup 5] [--skip-rollout] [--out profiles/token_logprob_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12
V = 128256


def window(fn, n):
    """ms per call of n back-to-back calls between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(series, iters, warmup, n):
    """{name: sorted ms per call}: the series take turns, round by round."""
    ms = {k: [] for k in series}
    for r in range(warmup + iters):
        for k, fn in series.items():
            t = window(fn, n)
            if r >= warmup:
                ms[k].append(t)
    return {k: sorted(v) for k, v in ms.items()}


def stats(v):
    return dict(ms_median=round(statistics.median(v), 5), ms_min=round(v[0], 5), ms_max=round(v[-1], 5))


def pair(a, emit):
    from unsloth_amd.kernels import decode as D
    dev = torch.device("cuda", 0)
    for rows in (1, 64):
        nbytes = rows * V * 4
        for mode, nbuf in (("hot", 1), ("cold", -(-640 * 2 ** 20 // nbytes))):
            bufs = [4.0 * torch.randn(rows, V, device=dev) for _ in range(nbuf)]
            tok = torch.randint(0, V, (rows,), device=dev)
            prm, slot = D.sample_params(dev, temperature=0.8), torch.zeros(1, dtype=torch.int32, device=dev)
            lp, ent, ws = torch.zeros(rows, 8, device=dev), torch.zeros(rows, 8, device=dev), torch.empty(rows * 192, device=dev)
            out = torch.empty(rows, dtype=torch.long, device=dev)
            aws = (torch.empty(rows * 64, device=dev), torch.empty(rows * 64, dtype=torch.long, device=dev))
            calls = [0]

            def logits():                                # the next buffer, across windows and series
                calls[0] += 1
                return bufs[calls[0] % nbuf]
            series = {"uamd_token_logprob_f32": lambda i: D.token_logprob_f32(logits(), tok, prm, slot, lp, ent, ws),
                      "uamd_token_logprob_f32_no_entropy": lambda i: D.token_logprob_f32(logits(), tok, prm, slot, lp, None, ws),
                      "uamd_argmax_f32": lambda i: D.argmax_f32(logits(), out=out, ws=aws)}
            for name, v in alternate(series, a.iters, a.warmup, a.burst).items():
                med = statistics.median(v)
                emit(dict(metric="pair", series=name, logits=mode, rows=rows, vocab=V, buffers=nbuf, burst=a.burst, iters=a.iters,
                          **stats(v), bytes_read=nbytes, tb_per_s=round(nbytes / med / 1e9, 3),
                          hbm_peak_fraction=round(nbytes / (med * 1e-3) / HBM_PEAK, 3)))
            del bufs, series
            torch.cuda.empty_cache()


def step(a, model, emit):
    import decode_batch_bench as DB
    start = a.context - a.steps - 8
    for B in (1, 64):
        engines = {"off": DB.engine(model, B, True, a.context, start), "on": DB.engine(model, B, True, a.context, start)}
        engines["on"].track_logprobs(True, entropy=True)

        def round_of(eng):
            def run(_):
                eng.kv_len.fill_(start)
                if eng._lp_slot is not None:
                    eng._lp_slot.zero_()
                for _ in range(a.steps):
                    eng.step(eng.next_tok)
            return run
        for eng in engines.values():                     # capture and warm every launch outside the timed rounds
            eng.kv_len.fill_(start)
            eng.step(torch.zeros(B, dtype=torch.long, device=eng.dev))
        ms = alternate({k: round_of(e) for k, e in engines.items()}, a.iters, a.warmup, 1)
        med = {k: statistics.median(v) / a.steps for k, v in ms.items()}
        for k, v in ms.items():
            emit(dict(metric="step", tracking=k, batch=B, layers=a.layers, context=a.context, first_position=start, steps=a.steps,
                      iters=a.iters, hipgraph=engines[k].use_graph, **stats([t / a.steps for t in v]),
                      on_over_off=round(med["on"] / med["off"], 4) if k == "on" else None))
        del engines
        torch.cuda.empty_cache()


def rollout(a, model, emit):
    from unsloth_amd.models.rl_replacements import get_per_token_logps_and_entropies
    B, T, new = 64, 2048, 256
    ids = torch.randint(0, V, (B, T + new), device="cuda")
    mask = torch.ones_like(ids)

    def run(_):
        with torch.no_grad():
            return get_per_token_logps_and_entropies(model, ids, mask, new, temperature=0.8, compute_entropy=True)
    v = alternate({"forward": run}, 3, 1, 1)["forward"]
    emit(dict(metric="rollout", series="get_per_token_logps_and_entropies", batch=B, prompt=T, completion=new, layers=a.layers,
              iters=3, **stats(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="llama3-8b")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--skip-rollout", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("token_logprob_bench: needs the GPU; nothing is measured without one")
    out = open(a.out, "w") if a.out else None

    def emit(d):
        print(json.dumps(d), flush=True)
        if out:
            out.write(json.dumps(d) + "\n")
            out.flush()
    pair(a, emit)
    import decode_bench
    a.context, ctx = max(a.context, 2048 + 256), a.context          # (the model's rotary tables cover the rollout's rows)
    model = decode_bench.whole_model(a, "cuda")
    a.context = ctx
    step(a, model, emit)
    if not a.skip_rollout:
        rollout(a, model, emit)


if __name__ == "__main__":
    main()
