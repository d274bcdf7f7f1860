"""FlatAdamW: torch.optim.AdamW's arithmetic over ONE flat fp32 arena -- one HIP launch per optimizer step.

The reference trains through HF's Trainer with a torch / bitsandbytes optimizer (unsloth/trainer.py:445-623); the
benchmark's step is forward + backward + AdamW on the LoRA factors. torch's fused AdamW needs 52 multi_tensor_apply
launches (2.5 ms) for the 448 factors of Llama-3-8B r=16 -- 168 MB of parameters, 0.2 ms of HBM time. MI355X-first
layout instead: parameters, gradients (dp.LoRAGradArena, which the fused LoRA-gradient kernel ADDS into), exp_avg and
exp_avg_sq are four flat fp32 buffers with the same offsets, `p.data` / `p.grad` / the optimizer state are views into
them, and `uamd_adamw_flat` (csrc/adamw.hip) walks them once -- zeroing the gradient arena in the same pass, which is
the `zero_grad` of the next step.

Interface: a torch.optim.Optimizer (param_groups / state / state_dict / LR schedulers / step hooks work as usual) with
one parameter group. `step(grad_scale=...)` takes the clipping factor; parameters whose gradient is None are skipped
like torch does (all parameters share one step counter: in LoRA training every factor gets a gradient every step). No CPU fallback: the step raises without the HIP library.

`optim_bits=8` (the reference's optim="adamw_8bit", bitsandbytes' block-wise 8-bit AdamW): both moments are one uint8
code per element plus one fp32 absmax per 256-element block (`uamd_adamw8_flat`): 2 B + 8 B / 256 per parameter instead of
8 B. Quant blocks tile the ARENA from element 0 -- they do not restart per parameter, because the offsets belong to
dp.LoRAGradArena and one launch walks the whole arena. Where the 8-bit path differs from torch's skip of parameters without
a gradient: a launch starts and ends on block boundaries, so a block that holds both a parameter with a gradient and one
without is stepped as a whole, the latter with a zero gradient (its moments decay, weight decay applies). It cannot occur
in LoRA training, where every factor gets a gradient every step.
"""
import math

import torch

from . import _lib
from .dp import LoRAGradArena


QBLOCK = 256                  # elements per quantisation block of the 8-bit moments (bitsandbytes' optimizer block size)


def adam8_maps(device):
    """(signed, unsigned) dynamic maps of the 8-bit moments: exp_avg is signed, exp_avg_sq is not."""
    from .nf4 import create_dynamic_map
    return create_dynamic_map(signed=True).to(device), create_dynamic_map(signed=False).to(device)


def adam8_zero_code(code):
    """Index of 0.0 in a map: what a moment that has never been written (or a block whose absmax is 0) stores."""
    return int((code == 0).nonzero()[0, 0])


def adam8_decode(codes, absmax, code, first=0):
    """fp32 values of `codes` (uint8, flat), element i of which is element first + i of the buffer `absmax` belongs to."""
    blk = torch.arange(first, first + codes.numel(), device=codes.device) // QBLOCK
    return code[codes.reshape(-1).long()] * absmax[blk]


def adam8_encode(x, code, signed):
    """Block-wise encode of the flat fp32 `x` (blocks from element 0, the last may be partial): (uint8 codes, absmax).
    absmax = max |x| (signed) or max x; code = nearest map entry to x / absmax (true division; an exact tie takes the lower
    index); a block whose absmax is 0 stores the code of 0.0. The same rule as csrc/adamw.hip adamw8_kernel."""
    n = x.numel()
    xp = torch.nn.functional.pad(x, (0, (-n) % QBLOCK)).view(-1, QBLOCK)
    absmax = (xp.abs() if signed else xp).amax(dim=1).clamp_min(0.0)
    scaled = torch.where(absmax.unsqueeze(1) > 0, xp / absmax.unsqueeze(1), torch.zeros_like(xp))
    mids = (code[:-1] + code[1:]) / 2
    idx = torch.bucketize(scaled.reshape(-1)[:n].contiguous(), mids)
    return idx.to(torch.uint8), absmax


def adam8_step_host(p32, g, m8, v8, absmax_m, absmax_v, code_m, code_v, decays, lr, b1, b2, eps, weight_decay, bc1,
                    bc2_sqrt, grad_scale):
    """One 8-bit AdamW step in torch, in place on (p32, m8, v8, absmax_m, absmax_v): the arithmetic of adamw8_kernel,
    operation by operation in fp32 (constants formed in double and rounded once, no fused multiply-add), so the host branch
    and the kernel are two implementations of one rule. `decays`: bool mask of the elements weight decay applies to."""
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=p32.device)
    m = adam8_decode(m8, absmax_m, code_m)
    v = adam8_decode(v8, absmax_v, code_v)
    gr = g.to(torch.float32) * f(grad_scale)
    p = p32 - torch.where(decays, f(lr * weight_decay), f(0.0)) * p32
    m = f(b1) * m + f(1.0 - b1) * gr
    v = f(b2) * v + f(1.0 - b2) * gr * gr
    denom = v.sqrt() / f(bc2_sqrt) + f(eps)
    p32.copy_(p - f(lr / bc1) * m / denom)
    for dst, src in zip((m8, absmax_m), adam8_encode(m, code_m, True)):
        dst.copy_(src)
    for dst, src in zip((v8, absmax_v), adam8_encode(v, code_v, False)):
        dst.copy_(src)


def _check_bits(optim_bits):
    if optim_bits not in (8, 32):
        raise ValueError(f"optim_bits must be 8 or 32, got {optim_bits!r}")


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, model, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, arena=None, optim_bits=32):
        """`arena`: the dp.LoRAGradArena that already owns the gradients (data-parallel runs); else one is created
        (single rank: no collective is ever issued)."""
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid AdamW hyper-parameters")
        _check_bits(optim_bits)
        self.optim_bits = optim_bits
        if arena is None:
            # two live arenas over the same parameters would both hook gradient accumulation and fight over p.grad and
            # the fused-gradient sinks (the second one's copies racing the first one's collectives): refuse
            for p in model.parameters():
                owner = getattr(p, "_uamd_arena", None)
                if p.requires_grad and owner is not None and owner() is not None:
                    raise RuntimeError("FlatAdamW: these parameters already belong to a live dp.LoRAGradArena; pass it "
                                       "as `arena=` (trainer.make_optimizer(model, arena=arena))")
        self.arena = arena if arena is not None else LoRAGradArena(model)
        self._owns_arena = arena is None
        params = list(self.arena.params)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        g = self.arena.arena
        n = g.numel()
        self.flat_p = torch.empty(n, dtype=torch.float32, device=g.device)
        if optim_bits == 8:
            # zero moments: absmax 0 and the code of 0.0 everywhere
            self.code_m, self.code_v = adam8_maps(g.device)
            self.flat_m = torch.full((n,), adam8_zero_code(self.code_m), dtype=torch.uint8, device=g.device)
            self.flat_v = torch.full((n,), adam8_zero_code(self.code_v), dtype=torch.uint8, device=g.device)
            nblk = (n + QBLOCK - 1) // QBLOCK
            self.absmax_m = torch.zeros(nblk, dtype=torch.float32, device=g.device)
            self.absmax_v = torch.zeros(nblk, dtype=torch.float32, device=g.device)
        else:
            self.flat_m = torch.zeros(n, dtype=torch.float32, device=g.device)
            self.flat_v = torch.zeros(n, dtype=torch.float32, device=g.device)
        self._keys = ("state1", "state2") if optim_bits == 8 else ("exp_avg", "exp_avg_sq")     # (bitsandbytes' names)
        self._views = []                     # (param, offset, numel, grad view)
        self._step_t = torch.zeros((), dtype=torch.float32)
        off = 0
        with torch.no_grad():
            for p in params:
                k = p.numel()
                gv = self.arena._views[id(p)]
                assert gv.data_ptr() == g.data_ptr() + 4 * off, "arena order changed under the optimizer"
                self.flat_p[off:off + k].copy_(p.data.reshape(-1))
                p.data = self.flat_p[off:off + k].view(p.shape)          # the parameter now LIVES in the flat buffer
                self.state[p] = {"step": self._step_t,           # ONE shared host scalar: one increment per step, not 448
                                 self._keys[0]: self.flat_m[off:off + k].view(p.shape),
                                 self._keys[1]: self.flat_v[off:off + k].view(p.shape)}
                self._views.append((p, off, k, gv))
                off += k
        self._t = 0
        self._writes_seen = self.arena.writes    # arena.writes at the moment the arena was last known to be all zeros

    # ------------------------------------------------------------------------------------------
    def _runs(self):
        """Contiguous [start, end) element ranges whose parameters have a gradient; every gradient is (moved) in the
        arena first. One range = the whole arena in a normal LoRA step."""
        runs, cur = [], None
        base = self.flat_p.data_ptr()
        for p, off, k, gv in self._views:
            if p.data_ptr() != base + 4 * off:
                # someone re-pointed p.data (module.to(...), a checkpoint loader that assigns .data): adopt the new
                # values and bring the parameter home again -- stepping a detached copy would silently train nothing
                self.flat_p[off:off + k].copy_(p.data.reshape(-1).to(self.flat_p.dtype))
                p.data = self.flat_p[off:off + k].view(p.shape)
            gr = p.grad
            if gr is None:
                cur = None
                continue
            if gr.data_ptr() != gv.data_ptr():
                gv.copy_(gr)                 # autograd built a fresh tensor (the view had been dropped)
                p.grad = gv
            if cur is not None and cur[1] == off:
                cur[1] = off + k
            else:
                cur = [off, off + k]
                runs.append(cur)
        if self.optim_bits == 8:
            runs = self._whole_blocks(runs)
        return runs

    def _whole_blocks(self, runs):
        """8-bit moments: widen every run outward to quant-block boundaries (a block is re-encoded as a whole) and merge
        what then touches; a parameter without a gradient that a widened run covers is stepped with a zero gradient."""
        n = self.flat_p.numel()
        wide = []
        for s, e in runs:
            s, e = s // QBLOCK * QBLOCK, min((e + QBLOCK - 1) // QBLOCK * QBLOCK, n)
            if wide and s <= wide[-1][1]:
                wide[-1][1] = max(wide[-1][1], e)
            else:
                wide.append([s, e])
        for p, off, k, gv in self._views:
            if p.grad is None and any(s < off + k and off < e for s, e in wide):
                gv.zero_()
        return wide

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grp = self.param_groups[0]
        if len(self.param_groups) != 1:
            raise NotImplementedError("FlatAdamW: one parameter group (use torch.optim.AdamW for per-group settings)")
        b1, b2 = grp["betas"]
        self._t += 1
        t = self._t
        bc1 = 1.0 - b1 ** t
        bc2_sqrt = math.sqrt(1.0 - b2 ** t)
        runs = self._runs()
        _lib.require_gpu(self.flat_p)
        g = self.arena.arena
        L = _lib.lib()
        with _lib.device_ctx(self.flat_p):
            hyper = (float(grp["lr"]), float(b1), float(b2), float(grp["eps"]), float(grp["weight_decay"]), bc1, bc2_sqrt,
                     float(grad_scale), 1, _lib.stream_of(self.flat_p))
            for s, e in runs:
                # (a run that does not start on a 16-byte boundary cannot happen for LoRA factors: every numel is a
                # multiple of 4; the C side checks. 8-bit runs start on a quant-block boundary.)
                if self.optim_bits == 8:
                    rc = L.uamd_adamw8_flat(self.flat_p.data_ptr() + 4 * s, g.data_ptr() + 4 * s, self.flat_m.data_ptr() + s,
                                            self.flat_v.data_ptr() + s, self.absmax_m.data_ptr() + 4 * (s // QBLOCK),
                                            self.absmax_v.data_ptr() + 4 * (s // QBLOCK), self.code_m.data_ptr(),
                                            self.code_v.data_ptr(), e - s, *hyper)
                else:
                    rc = L.uamd_adamw_flat(self.flat_p.data_ptr() + 4 * s, g.data_ptr() + 4 * s,
                                           self.flat_m.data_ptr() + 4 * s, self.flat_v.data_ptr() + 4 * s, e - s, *hyper)
                _lib.check(rc, "uamd_adamw8_flat" if self.optim_bits == 8 else "uamd_adamw_flat")
        self._step_t += 1                    # (shared by every parameter's state entry)
        # every range that had a gradient is zero again; ranges without one were never written
        self._writes_seen = self.arena.writes
        return loss

    def zero_grad(self, set_to_none=True):
        """The step already zeroed the arena in its own pass; the gradient views stay attached (the fused LoRA-gradient
        kernel adds into them). Called without a step in between (gradients thrown away): one fill."""
        if self.arena.writes != self._writes_seen:
            self.arena.arena.zero_()
            self._writes_seen = self.arena.writes
        self.arena.reset_arrivals()                  # (arrival bookkeeping of the exchange: a new accumulation starts)
        for p, _, _, gv in self._views:
            p.grad = gv

    def grad_norm(self):
        return self.arena.arena.norm()

    def moments(self, p):
        """fp32 (exp_avg, exp_avg_sq) of parameter `p`, decoded from the codes and block scales with 8-bit state."""
        off, k = next((off, k) for q, off, k, _ in self._views if q is p)
        if self.optim_bits == 32:
            return self.flat_m[off:off + k].view(p.shape), self.flat_v[off:off + k].view(p.shape)
        return (adam8_decode(self.flat_m[off:off + k], self.absmax_m, self.code_m, off).view(p.shape),
                adam8_decode(self.flat_v[off:off + k], self.absmax_v, self.code_v, off).view(p.shape))

    def moment_bytes(self):
        """Bytes both moments take, block scales included."""
        extra = 4 * (self.absmax_m.numel() + self.absmax_v.numel()) if self.optim_bits == 8 else 0
        return (self.flat_m.numel() + self.flat_v.numel()) * self.flat_m.element_size() + extra

    def state_dict(self):
        sd = super().state_dict()
        if self.optim_bits == 8:
            # a snapshot: codes and step count are copied together with the scales (live views next to copied scales
            # would stop decoding to the saved moments at the next step)
            sd["state"] = {i: {k: v.clone() for k, v in st.items()} for i, st in sd["state"].items()}
            sd["uamd_flat8"] = dict(blocksize=QBLOCK, absmax1=self.absmax_m.clone(), absmax2=self.absmax_v.clone())
        return sd

    def load_state_dict(self, state_dict):
        saved_bits = 8 if "uamd_flat8" in state_dict or any("state1" in st for st in state_dict["state"].values()) else 32
        if saved_bits != self.optim_bits:
            raise ValueError(f"FlatAdamW: the state was saved with optim_bits={saved_bits} ({saved_bits}-bit moments), this "
                             f"optimizer has optim_bits={self.optim_bits}: the two do not convert into each other")
        q8 = state_dict.get("uamd_flat8")
        if self.optim_bits == 8:
            if q8 is None or q8["blocksize"] != QBLOCK or q8["absmax1"].numel() != self.absmax_m.numel():
                raise ValueError("FlatAdamW: 8-bit state without matching block scales (key 'uamd_flat8')")
            self.absmax_m.copy_(q8["absmax1"])
            self.absmax_v.copy_(q8["absmax2"])
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "uamd_flat8"})
        # torch replaced the state tensors by copies: move them back into the flat buffers and re-attach the views.
        # The step counter becomes the LOADED one (loading an earlier checkpoint into an optimizer that has already
        # stepped must restart the bias correction there); a parameter the checkpoint has no state for (saved before the
        # first step) starts from zero moments. All parameters share one step counter -- a parameter that received no
        # gradient on some steps is bias-corrected with the run's step count, not its own (torch counts per parameter;
        # in LoRA training every factor gets a gradient every step, so the two agree).
        loaded_t = None
        with torch.no_grad():
            for p, off, k, _ in self._views:
                st = self.state.get(p, None)
                km, kv = self._keys
                if not st or km not in st:
                    # (8-bit: the code of 0.0; such a parameter's blocks keep the loaded scales of their neighbours)
                    self.flat_m[off:off + k].fill_(adam8_zero_code(self.code_m) if self.optim_bits == 8 else 0)
                    self.flat_v[off:off + k].fill_(adam8_zero_code(self.code_v) if self.optim_bits == 8 else 0)
                    st = self.state[p] = {}
                else:
                    # (8-bit: torch's loader turned the uint8 codes into the parameter's dtype; 0 .. 255 come back exactly)
                    self.flat_m[off:off + k].copy_(st[km].reshape(-1))
                    self.flat_v[off:off + k].copy_(st[kv].reshape(-1))
                    if "step" in st:
                        t = int(st["step"])
                        loaded_t = t if loaded_t is None else max(loaded_t, t)
                st[km] = self.flat_m[off:off + k].view(p.shape)
                st[kv] = self.flat_v[off:off + k].view(p.shape)
                st["step"] = self._step_t
            self._t = 0 if loaded_t is None else loaded_t
            self._step_t.fill_(float(self._t))

    def close(self):
        if self._owns_arena:
            self.arena.close()
