"""Per-token entropy on the RL log-prob path: what the entropy costs next to the log-probs it rides with.

Three things, event-timed on one GPU in one process. The two kernels alternate A / B / A / B, ... so that drift hits both
alike and each runs behind the other (whatever of the logits the last pass left in the Infinity Cache, both find); the
torch formulation C, which sweeps gigabytes of its own, is timed in a series of its own afterwards:

  A  uamd_cross_entropy_forward    the log-prob-only pass over a [rows, V] bf16 logits chunk (unchanged kernel)
  B  uamd_logprob_entropy_forward  the same pass with the entropy's third running sum
  C  the plain-torch entropy this replaced (kept here as a copy): an fp32 copy of lm_head, an fp32 matmul per 2048
     rows from the hidden states, fp32 logits, their softmax, logsumexp and a reduction. C starts from the hidden states
     because that is where it started in the product; B needs no GEMM of its own -- the chunk already exists for the
     log-probs.

Shapes: [4096, 128256] (row stride 128256: Llama-3's vocabulary, one full chunk) and [2048, 32000], H = 4096. Warm-up
first, then the median of --iters runs. For A and B: bytes read / median time, as a fraction of the 8.0 TB/s HBM peak
(about 6.3 TB/s is what a plain copy reaches). Also `torch.cuda.max_memory_allocated` above the resident inputs for one
call of B and one of C. One JSON line per (shape, series); needs the GPU.

    python tools/logprob_entropy_bench.py [--iters 20] [--warmup 5] [--out profiles/logprob_entropy_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unsloth_amd import _lib                                                                   # noqa: E402
from unsloth_amd.kernels.cross_entropy_loss import _logprob_entropy_forward                    # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = [(4096, 128256), (2048, 32000)]
HIDDEN = 4096


def torch_entropy(rows, lm_head, temperature=1.0):
    """The formulation get_per_token_logps_and_entropies used before the kernel kept a per-row entropy."""
    out = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    with torch.no_grad():
        W = lm_head.float()
        for r0 in range(0, rows.shape[0], 2048):
            lg = rows[r0:r0 + 2048].float() @ W.t()
            lg = lg / temperature
            p = torch.softmax(lg, dim=-1)
            out[r0:r0 + 2048] = torch.logsumexp(lg, dim=-1) - (p * lg).sum(-1)
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def peak_above_resident(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return peak - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprob_entropy_bench: needs the GPU (a CPU run measures nothing)")
    if args.iters < 20:
        raise SystemExit("logprob_entropy_bench: --iters >= 20 (the figures are medians)")
    dev = torch.device("cuda", 0)
    lines = []
    for n_rows, V in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        h = (torch.randn(n_rows, HIDDEN, device=dev, generator=gen) * 0.5).to(torch.bfloat16)
        W = (torch.randn(V, HIDDEN, device=dev, generator=gen) * 0.02).to(torch.bfloat16)
        logits = torch.empty(n_rows, V, dtype=torch.bfloat16, device=dev)
        for r0 in range(0, n_rows, 1024):
            logits[r0:r0 + 1024] = h[r0:r0 + 1024] @ W.t()           # the chunk the log-prob path hands its kernel
        index = torch.randint(0, V, (n_rows,), device=dev, generator=gen)
        # the two kernels through the C entries into outputs allocated once: the events bracket one launch, not the allocator
        o = [torch.empty(n_rows, dtype=torch.float32, device=dev) for _ in range(3)]
        head = (logits, _lib.ptr(logits), logits.stride(0), _lib.ptr(o[0]), _lib.ptr(o[1]))
        tail = (_lib.ptr(index), n_rows, V, 0.0, 0.0, _lib.dtype_code(logits.dtype), _lib.stream_of(logits))
        series = {
            "uamd_cross_entropy_forward": lambda: _lib.call("uamd_cross_entropy_forward", *head, *tail),
            "uamd_logprob_entropy_forward": lambda: _lib.call("uamd_logprob_entropy_forward", *head, _lib.ptr(o[2]), *tail),
            "torch_entropy_from_hidden": lambda: torch_entropy(h, W),
        }
        ms = {k: [] for k in series}
        for group in (("uamd_cross_entropy_forward", "uamd_logprob_entropy_forward"), ("torch_entropy_from_hidden",)):
            for i in range(args.warmup + args.iters):
                for name in group:
                    t, out = timed(series[name])
                    del out
                    if i >= args.warmup:
                        ms[name].append(t)
        # same rows, same quantity: the kernel's entropy against the torch formulation's (fp32 logits, not bf16-rounded ones)
        ent = _logprob_entropy_forward(logits, index, 0.0, 0.0)[2]
        worst = float((ent - torch_entropy(h, W)).abs().max())
        mem = {"uamd_logprob_entropy_forward": peak_above_resident(lambda: _logprob_entropy_forward(logits, index, 0.0, 0.0)),
               "torch_entropy_from_hidden": peak_above_resident(series["torch_entropy_from_hidden"])}
        nbytes = n_rows * V * logits.element_size()
        for name in series:
            med = statistics.median(ms[name])
            rec = dict(series=name, rows=n_rows, vocab=V, row_stride=logits.stride(0), dtype="bf16", iters=args.iters,
                       ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4))
            if name.startswith("uamd_"):
                rec.update(bytes_read=nbytes, tb_per_s=round(nbytes / med / 1e9, 3),
                           hbm_peak_fraction=round(nbytes / (med * 1e-3) / HBM_PEAK, 3))
            else:
                rec.update(hidden=HIDDEN, max_abs_diff_vs_kernel_entropy=round(worst, 5))
            if name in mem:
                rec["peak_bytes_above_inputs"] = mem[name]
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        a = statistics.median(ms["uamd_cross_entropy_forward"])
        b = statistics.median(ms["uamd_logprob_entropy_forward"])
        rec = dict(series="entropy_kernel_over_sibling", rows=n_rows, vocab=V, ratio=round(b / a, 4))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del h, W, logits, index, series, ent, o, head, tail
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
