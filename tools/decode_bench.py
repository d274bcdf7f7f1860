"""Single-stream decode throughput of a Llama-shaped QLoRA model (NF4 r=16) with the hipGraph-replayed step
(models/decode.py), and the GEMV and attention kernels alone against the HBM roofline. --shape llama3-8b (default; head_dim
128) or tinyllama (TinyLlama-1.1B: hidden 2048, intermediate 5632, 22 layers, 32 / 4 heads, head_dim 64, vocab 32000).

    python tools/decode_bench.py [--shape llama3-8b] [--layers 32] [--context 2048] [--new 64] [--out decode.jsonl]
    python tools/decode_bench.py --sampler [--out sampler.jsonl]     the device sampler: launch and sampled step
    python tools/decode_bench.py --lookup [--out lookup.jsonl]       prompt-lookup verify replays (K = 2, 4, 8, 15) against the plain step
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8.0e12
# hidden, intermediate, layers, query heads, KV heads, head_dim, vocab
SHAPES = {"llama3-8b": (4096, 14336, 32, 32, 8, 128, 128256), "tinyllama": (2048, 5632, 22, 32, 4, 64, 32000)}


def timeit(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us


def attn_head_dim_ab(context, emit, rounds=7):
    """The fused attention launch at head_dim 64 against head_dim 128 at EQUAL KV heads, batch and context, rounds interleaved
    in one process: the D = 64 launch reads half the cache bytes, so it must not take longer."""
    from unsloth_amd.kernels import decode as D
    dev, bf, Hq, S = "cuda", torch.bfloat16, 32, context
    for Hk in (8, 4):
        fns = {}
        for Dh in (128, 64):
            kc = torch.randn(1, Hk, S, Dh, device=dev, dtype=bf)
            vc = torch.randn(1, Hk, S, Dh, device=dev, dtype=bf)
            qkv = torch.randn(1, (Hq + 2 * Hk) * Dh, device=dev, dtype=bf)
            cos = torch.randn(S, Dh // 2, device=dev, dtype=bf)
            sin = torch.randn(S, Dh // 2, device=dev, dtype=bf)
            kvl = torch.full((1,), S - 1, dtype=torch.int32, device=dev)
            fpart, cnt = D.fused_attn_workspace(1, Hq, Hk, S, Dh, 128, dev)
            ao = torch.empty(1, Hq * Dh, device=dev, dtype=bf)
            fns[Dh] = (lambda t=(qkv, cos, sin, kvl, kc, vc, ao, fpart, cnt), sc=1.0 / Dh ** 0.5:
                       D.attn_decode_fused(*t, 128, sc, Hq))
        us = {128: [], 64: []}
        for _ in range(rounds):
            for Dh in (128, 64):
                us[Dh].append(timeit(fns[Dh], n=50))
        for Dh in (128, 64):
            byts = 2 * S * Hk * Dh * 2
            v = sorted(us[Dh])
            emit(dict(kernel="fused attention, head_dim A/B", head_dim=Dh, kv_heads=Hk, q_heads=Hq, context=S, rounds=rounds,
                      us_median=round(v[len(v) // 2], 2), us_min=round(v[0], 2), us_max=round(v[-1], 2), bytes=byts,
                      frac_hbm=round(byts / (v[len(v) // 2] * 1e-6) / HBM, 3)))


def _spread(us):
    v = sorted(us)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def sampler_ab(V, emit, rounds=7, T=0.8, top_k=50, top_p=0.9, min_p=0.05):
    """The sampler launch against the torch chain generate() ran per token before it (division, filter_logits with its topk and
    full sort, softmax, multinomial -- that chain had no min-p; the launch has it on), [1, V] and [8, V], rounds interleaved in one
    process."""
    from unsloth_amd.kernels import decode as D
    from unsloth_amd.models.decode import filter_logits
    dev = "cuda"
    for rows in (1, 8):
        lg = 4.0 * torch.randn(rows, V, device=dev)
        prm = D.sample_params(dev, T, top_k, top_p, min_p, seed=1)
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        out = torch.empty(rows, dtype=torch.long, device=dev)
        gen = torch.Generator(dev).manual_seed(1)
        fns = dict(kernel=lambda: D.sample_f32(lg, prm, ctr, out=out),
                   torch=lambda: torch.multinomial(torch.softmax(filter_logits(lg / max(T, 1e-6), top_k, top_p), dim=-1), 1,
                                                   generator=gen).view(-1))
        us = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                us[k].append(timeit(fn, n=50))
        emit(dict(kernel="sampler launch against the torch chain", rows=rows, V=V, temperature=T, top_k=top_k, top_p=top_p,
                  min_p_kernel_only=min_p, rounds=rounds, kernel_us=_spread(us["kernel"]), torch_us=_spread(us["torch"]),
                  kernel_is_faster_beyond_the_spread=max(us["kernel"]) < min(us["torch"])))


def sampled_step_ab(eng, emit, steps, rounds=5, T=0.8, top_k=50, top_p=0.9, min_p=0.05):
    """ms per token of the sampled step against the greedy step, both replayed hipGraphs of one engine, rounds interleaved; every
    round starts at the same cache length."""
    kv0 = eng.kv_len.clone()
    tok = torch.zeros(1, dtype=torch.long, device=eng.dev)
    ms = dict(greedy=[], sampled=[])
    for r in range(rounds + 1):                          # round 0 captures and warms both graphs
        for mode in ("greedy", "sampled"):
            if mode == "greedy":
                eng.sampling()
            else:
                eng.sampling(T, top_k, top_p, min_p, seed=r)
            eng.kv_len.copy_(kv0)
            eng.step(tok)
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(steps):
                eng.step(eng.next_tok)
            torch.cuda.synchronize()
            if r:
                ms[mode].append((time.time() - t0) / steps * 1e3)
    eng.sampling()
    g, s = _spread(ms["greedy"]), _spread(ms["sampled"])
    emit(dict(metric="decode ms per token, sampled against greedy step, hipGraph, batch 1", layers=len(eng.core.layers),
              context=int(kv0[0]), steps=steps, rounds=rounds, temperature=T, top_k=top_k, top_p=top_p, min_p=min_p,
              greedy_ms=g, sampled_ms=s, sampled_minus_greedy_us=round((s["median"] - g["median"]) * 1e3, 1)))


def lookup_ab(eng, emit, context, steps, rounds=5, Ks=(2, 4, 8, 15), n_max=2):
    """ms per verify replay of prompt-lookup decoding (K drafts: K + 1 token rows on one pass over the weights) against ms per
    plain fused step, every one a replayed hipGraph of ONE engine, rounds interleaved in one process; every round starts at the
    same cache length. The prompt is random tokens, so hardly a draft is found or accepted and the context stays where it
    started; what a verify step costs does not depend on how many drafts it keeps (rejected rows ran all the same). From the
    costs: the accepted drafts per step at which a verify step breaks even with plain steps, t_K / t_plain - 1, and the
    tokens/s ceiling when every draft is accepted, (K + 1) / t_K."""
    lk = eng._lookup_state()
    kv0 = eng.kv_len.clone()
    st0 = torch.tensor([int(kv0[0]) + 1, 1 << 30, 0, 0], dtype=torch.int32, device=eng.dev)
    lk["hist"][int(kv0[0])] = 1
    tok = torch.zeros(1, dtype=torch.long, device=eng.dev)
    ms = {k: [] for k in ("plain",) + tuple(Ks)}
    accepted = {k: 0 for k in Ks}
    for r in range(rounds + 1):                          # round 0 captures and warms every graph
        for mode in ms:
            eng.kv_len.copy_(kv0)
            if mode == "plain":
                eng.step(tok)
                run = lambda: eng.step(eng.next_tok)
            else:
                lk["state"].copy_(st0)
                lk["stats"].zero_()
                eng._lookup_step(mode + 1, n_max)
                run = lambda: eng._lookup_step(mode + 1, n_max)
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(steps):
                run()
            torch.cuda.synchronize()
            if r:
                ms[mode].append((time.time() - t0) / steps * 1e3)
                if mode != "plain":
                    accepted[mode] += int(lk["stats"][2])
    plain = _spread(ms["plain"])
    emit(dict(metric="decode ms per step: plain fused step, hipGraph, batch 1", layers=len(eng.core.layers), context=context,
              steps=steps, rounds=rounds, ms=plain, tokens_per_s=round(1e3 / plain["median"], 1)))
    for K in Ks:
        v = _spread(ms[K])
        emit(dict(metric="decode ms per verify replay (prompt lookup), hipGraph, batch 1", K=K, rows=K + 1,
                  layers=len(eng.core.layers), context=context, steps=steps, rounds=rounds, ms=v, plain_ms=plain,
                  ratio_to_plain=round(v["median"] / plain["median"], 3),
                  break_even_accepted_per_step=round(v["median"] / plain["median"] - 1.0, 3),
                  tokens_per_s_ceiling_all_accepted=round((K + 1) * 1e3 / v["median"], 1),
                  accepted_while_timing=accepted[K], acceptance_on_real_text="not measured"))


def whole_model(a, dev):
    """The benchmark's synthetic Llama-shaped QLoRA model (NF4, r = 16 on every projection, random B factors)."""
    import bench as B                                   # the benchmark's synthetic Llama-3-8B-shaped config
    from unsloth_amd import FastLanguageModel
    cfg = B.llama3_8b_config(a.layers) if a.shape == "llama3-8b" else B.tinyllama_1b_config(a.layers)
    model, _ = FastLanguageModel.from_pretrained(config=cfg, max_seq_length=a.context, dtype=torch.bfloat16, load_in_4bit=True,
                                                 device=torch.device(dev), random_state=3407, use_gradient_checkpointing=False)
    model = FastLanguageModel.get_peft_model(model, r=16, lora_alpha=16, lora_dropout=0.0, bias="none",
                                             use_gradient_checkpointing=False, random_state=3407)
    gg = torch.Generator(device="cpu").manual_seed(3407)
    for n, p in model.named_parameters():
        if "lora_B" in n:
            p.data.copy_((torch.randn(p.shape, generator=gg) * 0.02).to(p.device))
    model.eval()
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="llama3-8b")
    ap.add_argument("--layers", type=int, default=None, help="default: the shape's own (32 / 22)")
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="whole model, hipGraph step only (for a rocprofv3 kernel trace)")
    ap.add_argument("--attn-ab", action="store_true", help="only the fused attention launch, head_dim 64 against 128")
    ap.add_argument("--sampler", action="store_true",
                    help="only the sampler: its launch against the torch chain, and the sampled against the greedy hipGraph step")
    ap.add_argument("--lookup", action="store_true",
                    help="only prompt-lookup decoding: ms per verify replay at K = 2, 4, 8, 15 against the plain fused step")
    a = ap.parse_args()
    H, I, L0, Hq, Hk, Dh, V = SHAPES[a.shape]
    if a.layers is None:
        a.layers = L0
    QN, KVN = Hq * Dh, Hk * Dh
    out = open(a.out, "w") if a.out else None

    def emit(d):
        print(json.dumps(d), flush=True)
        if out:
            out.write(json.dumps(d) + "\n")

    if a.attn_ab:
        return attn_head_dim_ab(a.context, emit)
    if a.sampler:
        from unsloth_amd.models.decode import DecodeEngine
        sampler_ab(V, emit)
        eng = DecodeEngine(whole_model(a, "cuda"), max_seq_len=a.context, batch=1, use_graph=True)
        eng.prefill(torch.randint(0, 32000, (1, a.context - a.new), device="cuda"))
        return sampled_step_ab(eng, emit, steps=a.new - 4)
    if a.lookup:
        from unsloth_amd.models.decode import DecodeEngine
        steps = 40                                      # replays per timed window; room for 16 new keys per replay behind the context
        eng = DecodeEngine(whole_model(a, "cuda"), max_seq_len=a.context + (steps + 2) * 16, batch=1, use_graph=True)
        ids = torch.randint(0, 32000, (1, a.context), device="cuda")
        eng.prefill(ids)
        eng._lookup_state()["hist"][:a.context].copy_(ids[0])
        return lookup_ab(eng, emit, a.context, steps)
    from unsloth_amd.kernels import decode as D
    from unsloth_amd.nf4 import quantize_nf4
    dev, bf = "cuda", torch.bfloat16
    # ---- GEMV kernels alone (the shape's projections)
    for name, Ns, K in () if a.quick else (("q|k|v", (QN, KVN, KVN), H), ("o", (H,), QN), ("gate|up", (I, I), H),
                        ("down", (H,), I)):
        x = torch.randn(K, device=dev, dtype=bf)
        projs = []
        for N in Ns:
            W = (torch.randn(N, K, device=dev) * 0.02).to(bf)
            packed, qs = quantize_nf4(W, compress_statistics=True)
            qs.dtype = bf
            projs.append((packed, qs, None, None, None))
        outbuf = torch.empty(sum(Ns), device=dev, dtype=bf)
        us = timeit(lambda: D.linear_group(x, projs, out=outbuf))
        byts = sum(Ns) * K * (0.5 + 1 / 64 + 4 / (64 * 256)) + K * 2 + sum(Ns) * 2
        emit(dict(kernel=f"gemv_nf4 {name}", us=round(us, 2), bytes=int(byts), GBps=round(byts / us / 1e3, 1),
                  frac_hbm=round(byts / (us * 1e-6) / HBM, 3)))
    # ---- the five launches of one fused decoder-layer step, each alone (LoRA r=16 on every projection, t = A x inside)
    from unsloth_amd.kernels.decode import attn_decode_fused, attn_decode, rope_kv_append

    def lora_projs(Ns, K):
        ps = []
        for N in Ns:
            W = (torch.randn(N, K, device=dev) * 0.02).to(bf)
            packed, qs = quantize_nf4(W, compress_statistics=True)
            qs.dtype = bf
            ps.append((packed, qs, torch.nn.Parameter(torch.randn(16, K, device=dev) * 0.02),
                       torch.nn.Parameter(torch.randn(N, 16, device=dev) * 0.02), 1.0, None))
        return ps
    resid = torch.randn(H, device=dev, dtype=bf)
    delta = torch.randn(H, device=dev, dtype=bf)
    wn = torch.ones(H, device=dev, dtype=bf)
    hbuf = torch.empty(H, device=dev, dtype=bf)
    for name, Ns, K, fused, xin in () if a.quick else (
            ("q|k|v  (add + RMSNorm in)", (QN, KVN, KVN), H, dict(mode=2, res=resid, norm_w=wn, eps=1e-5, h_out=hbuf), delta),
            ("o", (H,), QN, dict(mode=0), delta[:QN] if QN <= H else torch.randn(QN, device=dev, dtype=bf)),
            ("gate|up (add + RMSNorm in, SwiGLU out)", (I, I), H, dict(mode=2, res=resid, norm_w=wn, eps=1e-5, h_out=hbuf, glu=True), delta),
            ("down", (H,), I, dict(mode=0), torch.randn(I, device=dev, dtype=bf))):
        projs = lora_projs(Ns, K)
        outbuf = torch.empty(Ns[0] if fused.get("glu") else sum(Ns), device=dev, dtype=bf)
        us = timeit(lambda: D.linear_group(xin, projs, out=outbuf, fused=fused))
        us14 = timeit(lambda: D.linear_group(xin, projs))
        byts = sum(Ns) * K * (0.5 + 1 / 64 + 4 / (64 * 256)) + K * 2 + sum(Ns) * 2
        emit(dict(kernel=f"fused gemv_nf4 {name}", us=round(us, 2), separate_t_plus_gemv_us=round(us14, 2), bytes=int(byts),
                  GBps=round(byts / us / 1e3, 1), frac_hbm=round(byts / (us * 1e-6) / HBM, 3)))
    S = a.context if not a.quick else 128
    kc = torch.randn(1, Hk, S, Dh, device=dev, dtype=bf)
    vc = torch.randn(1, Hk, S, Dh, device=dev, dtype=bf)
    qkv = torch.randn(1, (Hq + 2 * Hk) * Dh, device=dev, dtype=bf)
    cos = torch.randn(S, Dh // 2, device=dev, dtype=bf)
    sin = torch.randn(S, Dh // 2, device=dev, dtype=bf)
    kvl = torch.full((1,), S - 1, dtype=torch.int32, device=dev)
    part = torch.empty(1, Hq, S // 128, Dh + 2, dtype=torch.float32, device=dev)
    fpart, cnt = D.fused_attn_workspace(1, Hq, Hk, S, Dh, 128, dev)
    ao = torch.empty(1, Hq * Dh, device=dev, dtype=bf)
    sc = round(1.0 / Dh ** 0.5, 3)                       # 0.088 at head_dim 128
    us = timeit(lambda: attn_decode_fused(qkv, cos, sin, kvl, kc, vc, ao, fpart, cnt, 128, sc, Hq))

    def three():
        rope_kv_append(qkv, cos, sin, kvl, kc, vc, Hq, Hk, Dh)
        attn_decode(qkv[:, :Hq * Dh], kc, vc, kvl, ao, part, 128, sc)
    us3 = timeit(three)
    byts = 2 * S * Hk * Dh * 2
    emit(dict(kernel=f"fused attention (rope + append + split-KV + combine), context {S}", us=round(us, 2),
              three_launches_us=round(us3, 2), bytes=byts, GBps=round(byts / us / 1e3, 1), frac_hbm=round(byts / (us * 1e-6) / HBM, 3)))
    del kc, vc
    K = H
    W = (torch.randn(V, K, device=dev) * 0.02).to(bf)
    x = torch.randn(K, device=dev, dtype=bf)
    us = timeit(lambda: D.gemv(x, [dict(W=W, N=V, y_f32=True)], nf4=False))
    byts = V * K * 2 + V * 4
    if not a.quick:
        emit(dict(kernel="gemv_bf16 lm_head", us=round(us, 2), bytes=byts, GBps=round(byts / us / 1e3, 1),
              frac_hbm=round(byts / (us * 1e-6) / HBM, 3)))
    del W

    # ---- whole model
    from unsloth_amd.models import decode as MD
    from unsloth_amd.models.decode import DecodeEngine
    model = whole_model(a, dev)
    ids = torch.randint(0, 32000, (1, a.context - a.new), device=dev)
    for fused, graph in ((True, True),) if a.quick else ((True, True), (False, True), (True, False), (False, False)):
        MD.FUSED_STEP = fused
        eng = DecodeEngine(model, max_seq_len=a.context, batch=1, use_graph=graph)
        t0 = time.time()
        eng.prefill(ids)
        torch.cuda.synchronize()
        t_prefill = time.time() - t0
        tok = torch.zeros(1, dtype=torch.long, device=dev)
        eng.step(tok)
        eng.step(tok)                                   # warm: the second call replays the graph
        torch.cuda.synchronize()
        n = a.new - 4
        t0 = time.time()
        for _ in range(n):
            eng.step(eng.next_tok)
        torch.cuda.synchronize()
        dt = (time.time() - t0) / n
        # HBM bytes one token must read: NF4 projections + lm_head + KV cache at this context
        cfg = eng.cfg
        nparam = a.layers * (cfg.hidden_size * (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * eng.D
                             + cfg.hidden_size * cfg.num_attention_heads * eng.D + 3 * cfg.hidden_size * cfg.intermediate_size)
        byts = nparam * 0.516 + cfg.vocab_size * cfg.hidden_size * 2 + a.layers * 2 * a.context * cfg.num_key_value_heads * eng.D * 2
        emit(dict(metric="decode tokens/s, batch 1", launches_per_layer=5 if fused else 14, hipgraph=graph, layers=a.layers, context=a.context, ms_per_token=round(dt * 1e3, 3),
                  tokens_per_s=round(1 / dt, 1), prefill_s=round(t_prefill, 3), hbm_bytes_per_token=int(byts),
                  frac_hbm=round(byts / dt / HBM, 3)))
        del eng


if __name__ == "__main__":
    main()
