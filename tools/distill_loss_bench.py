"""Full-vocabulary distillation loss: the HIP kernels against the torch formulation they replace.

Event-timed on one GPU in one process, bf16 logits of student and teacher, beta = 0 (forward KL), 0.5 (JSD) and 1 (reverse
KL), temperature 1. Per (shape, beta) four series; A and B alternate A / B / A / B, ... so that drift hits both alike, then C and D
the same way (a forward-only series does not wait behind a backward that rewrites its input):

  A  uamd_distill_loss_forward     one launch over the two [rows, V] matrices, per-row loss + the two logsumexp
  B  torch forward                 TRL's generalized_jsd_loss as written: two fp32 log_softmax, (mixture,) kl_div, sum
  C  uamd_distill_loss_forward + uamd_distill_loss_backward     loss and d(student logits), written in place
  D  torch forward + autograd backward

and, for context, uamd_cross_entropy_forward over the student logits alone (one stream). Shapes:
[4096, 128256] and [2048, 32000]. Warm-up first, then the median of --iters runs. For the kernels: bytes the algorithm must
move (forward: both matrices read once; backward: both read, the student written) / median time, as a fraction of the 8.0 TB/s
HBM peak; the JSD forward streams both matrices a second time (from L2 / Infinity Cache where they fit), which the byte count
does NOT include. `torch.cuda.max_memory_allocated` above the resident inputs for one call of C and one of D. One JSON line
per (shape, beta, series); needs the GPU.

    python tools/distill_loss_bench.py [--iters 30] [--warmup 5] [--out profiles/distill_loss_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unsloth_amd import _lib                                                                       # noqa: E402
from unsloth_amd.kernels.cross_entropy_loss import _distill_backward_, _distill_forward            # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = [(4096, 128256), (2048, 32000)]
BETAS = [0.0, 0.5, 1.0]


def torch_jsd_rows(student, teacher, beta, temperature=1.0):
    """TRL GKDTrainer.generalized_jsd_loss up to its reduction, summed over the vocabulary: [rows] fp32."""
    s = F.log_softmax(student.float() / temperature, dim=-1)
    t = F.log_softmax(teacher.float() / temperature, dim=-1)
    if beta == 0:
        return F.kl_div(s, t, reduction="none", log_target=True).sum(-1)
    if beta == 1:
        return F.kl_div(t, s, reduction="none", log_target=True).sum(-1)
    b = torch.tensor(beta, dtype=s.dtype, device=s.device)
    m = torch.logsumexp(torch.stack([s + torch.log1p(-b), t + torch.log(b)]), dim=0)
    return b * F.kl_div(m, t, reduction="none", log_target=True).sum(-1) + (1 - b) * F.kl_div(m, s, reduction="none", log_target=True).sum(-1)


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_loss_bench: needs the GPU (a CPU run measures nothing)")
    if args.iters < 20:
        raise SystemExit("distill_loss_bench: --iters >= 20 (the figures are medians)")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    for n_rows, V in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(0)
        student0 = torch.empty(n_rows, V, dtype=torch.bfloat16, device=dev)
        teacher = torch.empty(n_rows, V, dtype=torch.bfloat16, device=dev)
        for r0 in range(0, n_rows, 512):                          # logits-like values without a [rows, V] fp32 temporary
            student0[r0:r0 + 512] = torch.randn(min(512, n_rows - r0), V, device=dev, generator=gen) * 2
            teacher[r0:r0 + 512] = torch.randn(min(512, n_rows - r0), V, device=dev, generator=gen) * 2
        student = student0.clone()                                # the backward writes over it: restored outside the events
        labels = torch.randint(0, V, (n_rows,), device=dev, generator=gen)
        dl = torch.ones(n_rows, dtype=torch.float32, device=dev)
        o = [torch.empty(n_rows, dtype=torch.float32, device=dev) for _ in range(4)]
        nbytes = n_rows * V * student.element_size()
        code, st = _lib.dtype_code(student.dtype), _lib.stream_of(student)

        ce_ms = []
        for i in range(args.warmup + args.iters):
            t, _ = timed(lambda: _lib.call("uamd_cross_entropy_forward", student, _lib.ptr(student), student.stride(0), _lib.ptr(o[0]),
                                           _lib.ptr(o[1]), _lib.ptr(labels), n_rows, V, 0.0, 0.0, code, st))
            if i >= args.warmup:
                ce_ms.append(t)
        med = statistics.median(ce_ms)
        emit(dict(series="uamd_cross_entropy_forward", rows=n_rows, vocab=V, dtype="bf16", iters=args.iters, ms_median=round(med, 4),
                  bytes_moved=nbytes, tb_per_s=round(nbytes / med / 1e9, 3), hbm_peak_fraction=round(nbytes / (med * 1e-3) / HBM_PEAK, 3)))

        for beta in BETAS:
            def k_fwd():
                _lib.call("uamd_distill_loss_forward", student, _lib.ptr(student), student.stride(0), _lib.ptr(teacher),
                          teacher.stride(0), *[_lib.ptr(x) for x in o], _lib.ptr(labels), 1, n_rows, V, beta, 1.0, code, st)

            def k_fwd_bwd():
                k_fwd()
                _lib.call("uamd_distill_loss_backward", student, _lib.ptr(student), student.stride(0), _lib.ptr(teacher),
                          teacher.stride(0), _lib.ptr(dl), 1, _lib.ptr(o[1]), _lib.ptr(o[2]), _lib.ptr(o[3]), _lib.ptr(labels), 1,
                          n_rows, V, beta, 1.0, code, st)

            def t_fwd():
                with torch.no_grad():
                    return torch_jsd_rows(student0, teacher, beta)

            def t_fwd_bwd():
                z = student0.detach().requires_grad_(True)
                torch_jsd_rows(z, teacher, beta).sum().backward()
                return z.grad

            series = {"uamd_distill_forward": k_fwd, "torch_forward": t_fwd, "uamd_distill_forward_backward": k_fwd_bwd,
                      "torch_forward_backward": t_fwd_bwd}
            ms = {k: [] for k in series}
            for group in (("uamd_distill_forward", "torch_forward"), ("uamd_distill_forward_backward", "torch_forward_backward")):
                for i in range(args.warmup + args.iters):
                    for name in group:
                        t, out = timed(series[name])
                        del out
                        if name == "uamd_distill_forward_backward":
                            student.copy_(student0)                                        # outside the events
                        if i >= args.warmup:
                            ms[name].append(t)
            # same rows, same quantity: the kernel's loss and gradient against the torch formulation's
            losses, a, b, c = _distill_forward(student, teacher, None, beta, 1.0)
            worst_loss = float((losses - t_fwd()).abs().max())
            _distill_backward_(student, teacher, dl, a, b, c, None, beta, 1.0)
            worst_grad = float((student.float() - t_fwd_bwd().float()).abs().max())
            student.copy_(student0)

            def k_call():
                out = _distill_forward(student, teacher, None, beta, 1.0)
                _distill_backward_(student, teacher, dl, out[1], out[2], out[3], None, beta, 1.0)
                return out
            mem = {"uamd_distill_forward_backward": peak_above_resident(k_call),
                   "torch_forward_backward": peak_above_resident(t_fwd_bwd)}
            student.copy_(student0)
            moved = {"uamd_distill_forward": 2 * nbytes, "uamd_distill_forward_backward": 5 * nbytes}
            for name in series:
                med = statistics.median(ms[name])
                rec = dict(series=name, rows=n_rows, vocab=V, beta=beta, dtype="bf16", iters=args.iters, ms_median=round(med, 4),
                           ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4))
                if name in moved:
                    rec.update(bytes_moved=moved[name], tb_per_s=round(moved[name] / med / 1e9, 3),
                               hbm_peak_fraction=round(moved[name] / (med * 1e-3) / HBM_PEAK, 3))
                else:
                    rec.update(max_abs_diff_vs_kernel=round(worst_loss if name == "torch_forward" else worst_grad, 6))
                if name in mem:
                    rec["peak_bytes_above_inputs"] = mem[name]
                emit(rec)
            emit(dict(series="torch_over_kernel", rows=n_rows, vocab=V, beta=beta,
                      forward=round(statistics.median(ms["torch_forward"]) / statistics.median(ms["uamd_distill_forward"]), 2),
                      forward_backward=round(statistics.median(ms["torch_forward_backward"]) /
                                             statistics.median(ms["uamd_distill_forward_backward"]), 2)))
        del student, student0, teacher, labels, o, dl
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
