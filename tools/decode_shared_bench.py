"""Shared-prompt decoding: ms per token step of P prompts x n samples with ONE prompt cache per prompt (DecodeEngine(share_prompt=n),
uamd_attn_decode_shared) against the replicated caches of num_return_sequences (every prompt's K / V copied to its n rows) --
Llama-3-8B shape, NF4, LoRA r = 16, the benchmark's synthetic weights.

A point is (P, n, context): every row attends `context` keys at the end of a round; in the shared layout the last `--suffix` slots
of them are the row's own suffix and the rest is the prompt. Each point runs in a process of its own, started from here under its
own time limit (a point that fails or runs out of time ends the run: nothing more is started on the GPU); inside it the two engines
alternate round by round, every round replays the same positions (the caches hold random keys: the step's traffic does not depend
on their values). One JSON line per (point, route): median / min / max ms per step over the rounds, the bytes of the K / V caches
the engine allocated, and the clocks the device reports.

`--attention`: the attention launches alone at the shape's head geometry, shared (prefix scan, suffix scan, combine) against
replicated (scan, combine), no model; `rocprofv3 --kernel-trace --stats -- python tools/decode_shared_bench.py --attention --one
1x8x2048` (one point, in the profiled process itself) gives the time of each kernel.

    python tools/decode_shared_bench.py [--points 1x8x2048,1x16x2048,2x8x2048,1x16x8192] [--layers 32] [--suffix 256] [--steps 32]
                                        [--rounds 5] [--point-timeout 420] [--out decode_shared.jsonl] [--attention]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MAX_CPUS = 16


def engines(model, P, n, context, suffix):
    from unsloth_amd.models.decode import DecodeEngine
    rep = DecodeEngine(model, max_seq_len=context, batch=P * n, use_graph=True)
    sh = DecodeEngine(model, max_seq_len=context - suffix, batch=P * n, use_graph=True, share_prompt=n, max_new_tokens=suffix)
    assert rep.rows and sh.rows and rep.use_graph and sh.use_graph and sh.S + sh.S_n == rep.S
    for eng in (rep, sh):
        for c in eng.k_cache + eng.v_cache + (eng.pk or []) + (eng.pv or []):
            c.normal_()
    return dict(replicated=rep, shared=sh)


def cache_bytes(eng):
    return sum(c.numel() * c.element_size() for c in eng.k_cache + eng.v_cache + (eng.pk or []) + (eng.pv or []))


def run_round(eng, start, steps):
    """`steps` replayed token steps from total length `start` on; ms per step."""
    eng.kv_len.fill_(start)
    if eng.share_prompt:
        eng.prompt_len.fill_(eng.S)
        eng.new_len.fill_(start - eng.S)
    tok = torch.zeros(eng.B, dtype=torch.long, device=eng.dev)
    eng.step(tok)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.step(eng.next_tok)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def point(a, P, n, context):
    import decode_batch_bench
    import decode_bench
    a.context = context
    model = decode_bench.whole_model(a, "cuda")
    routes = engines(model, P, n, context, a.suffix)
    start = context - a.steps - 8
    assert start > routes["shared"].S
    ms = {k: [] for k in routes}
    for r in range(a.rounds + 1):                        # round 0 captures the graph and warms every launch
        for k, eng in routes.items():
            t = run_round(eng, start, a.steps if r else 3)
            if r:
                ms[k].append(t)
    lines = []
    for k, v in ms.items():
        v = sorted(v)
        eng = routes[k]
        lines.append(dict(metric="decode step, n samples per prompt", prompts=P, samples=n, batch=P * n, route=k, context=context,
                          prompt_keys=eng.S if eng.share_prompt else None, suffix_slots=eng.S_n if eng.share_prompt else None,
                          layers=a.layers, first_position=start, steps=a.steps, rounds=a.rounds, hipgraph=eng.use_graph,
                          ms_per_step=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4),
                          kv_cache_bytes=cache_bytes(eng), **decode_batch_bench.clocks()))
    for d in lines:
        print(json.dumps(d), flush=True)


def attention_only(a, P, n, context):
    """Event-timed launches of uamd_attn_decode_shared and of uamd_attn_decode over the same number of keys per row."""
    import decode_bench
    from unsloth_amd.kernels import decode as Dk
    _, _, _, Hq, Hk, D, _ = decode_bench.SHAPES[a.shape]
    B, S_n, S_p, dt = P * n, a.suffix, context - a.suffix, torch.bfloat16
    rnd = lambda *shape: torch.randn(*shape, device="cuda").to(dt)
    q, pk, pv, sk, sv = rnd(B, Hq * D), rnd(P, Hk, S_p, D), rnd(P, Hk, S_p, D), rnd(B, Hk, S_n, D), rnd(B, Hk, S_n, D)
    kc, vc, out = rnd(B, Hk, context, D), rnd(B, Hk, context, D), torch.empty_like(q)
    new = S_n - a.steps - 8
    plen = torch.full((P,), S_p, dtype=torch.int32, device="cuda")
    nlen = torch.full((B,), new, dtype=torch.int32, device="cuda")
    klen = torch.full((B,), S_p + new, dtype=torch.int32, device="cuda")
    sp = a.split_keys
    part = torch.empty(B, Hq, context // sp, D + 2, dtype=torch.float32, device="cuda")
    routes = dict(shared=lambda: Dk.attn_decode_shared(q, pk, pv, plen, n, sk, sv, nlen, out, part, sp, D ** -0.5),
                  replicated=lambda: Dk.attn_decode(q, kc, vc, klen, out, part, sp, D ** -0.5))
    for k, f in routes.items():
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            f()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="decode attention launches, eager", prompts=P, samples=n, context=context, route=k, split_keys=sp,
                              us_per_call=round(e0.elapsed_time(e1) / 50 * 1e3, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="llama3-8b")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--points", default="1x8x2048,1x16x2048,2x8x2048,1x16x8192", help="PxNxCONTEXT, comma-separated")
    ap.add_argument("--suffix", type=int, default=256, help="slots of a row's own suffix cache (a multiple of 128)")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--point-timeout", type=int, default=420, help="seconds one point may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--attention", action="store_true", help="the attention launches alone, no model")
    ap.add_argument("--split-keys", type=int, default=128, help="--attention: keys per split of both scans (the engine: 128)")
    ap.add_argument("--one", default=None, help="PxNxCONTEXT: measure this one point in this process (what the children run)")
    a = ap.parse_args()
    torch.set_num_threads(min(MAX_CPUS, torch.get_num_threads()))
    if a.one:
        if not torch.cuda.is_available():
            raise SystemExit("decode_shared_bench: needs the GPU; nothing is measured without one")
        return (attention_only if a.attention else point)(a, *[int(x) for x in a.one.split("x")])
    out = open(a.out, "w") if a.out else None
    env = dict(os.environ)
    for var in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[var] = str(min(MAX_CPUS, int(env.get(var) or MAX_CPUS)))
    for pt in a.points.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", pt, "--shape", a.shape, "--layers", str(a.layers), "--suffix",
               str(a.suffix), "--steps", str(a.steps), "--rounds", str(a.rounds)] + (
            ["--attention", "--split-keys", str(a.split_keys)] if a.attention else [])
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.point_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"decode_shared_bench: point {pt} ran past {a.point_timeout} s; nothing more is started")
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"decode_shared_bench: point {pt} ended with status {r.returncode}; nothing more is started")
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()


if __name__ == "__main__":
    main()
