"""Helpers of the fused linear + cross-entropy edge tests (tests/test_linear_ce_inputs.py on the host,
tests/test_gpu_linear_ce_edges.py on the GPU): a table of small cases that put `unsloth_fused_ce_loss`
(unsloth_amd/kernels/cross_entropy_loss.py) on the vocabulary, vector, row-chunk and dW-scaling edges, inputs whose softmax mass
sits on those edges, an fp64 truth, a model of what a correct 16-bit implementation rounds away, the wrong variants that model
can be turned into, an error per token row of d(hidden) / vocabulary row of dW, and a bound per row loss. Nothing here runs a
kernel or imports the product.

Every case is B = 2 sequences of L = 97 tokens at H = 256: T = 194 rows, with chunk_rows = 64 the row chunks 64 | 64 | 64 | 2.
A gradient is judged slice by slice: err(kernel, truth64) <= factor x err(rounding model, truth64), both on the same slice, so
the bound is a multiple of the reference side's own error and one wrong row or column shows at full size."""
import functools
import math
import zlib

import torch

B, L, H = 2, 97, 256
T = B * L
CHUNK = 64
UPSTREAM = 1.0 / 3.0                            # (loss / 3).backward(): an upstream scale bf16 does not hold
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# half an ulp relative to the power of two below: bf16 keeps 8 significant bits, fp16 11
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
LOSS_FP32 = 2e-5                                # tests/test_gpu_elementwise.py test_cross_entropy's figure for the fp32 CE forward

# short names of the library entry points the route assertions speak of
GEMM = {"uamd_gemm_nt": "nt", "uamd_gemm_nt_256": "nt_256", "uamd_gemm_nn_256": "nn_256", "uamd_gemm_tn_256": "tn_256",
        "uamd_gemm_nt_nf4": "nt_nf4"}
CE = {"uamd_cross_entropy_forward": "ce_fwd", "uamd_cross_entropy_backward": "ce_bwd"}
ENTRIES = tuple(GEMM) + tuple(CE)

# Token rows (r = b L + l; its label is labels[b, l + 1]). EDGE_ROWS carry the edge columns: on and beside the chunk edges
# 63 | 64, 127 | 128, 191 | 192 (192 is the only live row of the last chunk: 193 is a last position) and interior rows.
EDGE_ROWS = (63, 64, 65, 127, 128, 191, 192, 11, 40, 83, 101, 150, 170, 185, 23, 140)
PAD_ROW = 129                                   # the pad-sensitive row of a padded vocabulary
INTERIOR_ROWS = (50, 120)                       # two ordinary rows whose loss is checked alone, too
DEAD_ROWS = (0, 1, 2, 62, 66, 126, 190)         # label -100 by the data (beside the -100 of both last positions, 96 and 193)
_SPECIAL = set(EDGE_ROWS) | {PAD_ROW} | set(INTERIOR_ROWS)
MASKED_ROWS = tuple(r for r in range(T) if (r % 9 == 4 or r in (61, 67, 188)) and r not in _SPECIAL)

CASES = {}


def padded(V):
    return (V + 7) // 8 * 8


def routes_of(mode, V):
    """(logits GEMM, d(hidden) GEMM, is W^T built) as the host code decides them -- kernels/utils.py `_launch_gemm` /
    `_use_gemm256` with GEMM256_MODE forced "on" or "off", kernels/cross_entropy_loss.py `_nn_ok` / `_dhidden`:
      logits     h [rows, H] @ W^T: the 256-tile NT kernel when the mode is "on" and the contraction H is a multiple of 64
      d(hidden)  the NN form over W in place when V % 64 == 0 (and H % 8 == 0) on the 256-tile family; else the NT form over the
                 cached W^T [H, Vp], on the 256-tile kernel only when ITS contraction Vp is a multiple of 64
    (dW is uamd_gemm_tn_256 whatever the mode: utils.dense_dw.)"""
    assert mode in ("on", "off")
    on = mode == "on"
    logits = "nt_256" if on and H % 64 == 0 else "nt"
    nn = V % 64 == 0 and H % 8 == 0 and on
    dh = "nn_256" if nn else ("nt_256" if on and padded(V) % 64 == 0 else "nt")
    return logits, dh, not nn


def _case(name, V, mode, logits, dh, wt, *, dtype="bf16", softcap=0, scale=0, chunk_rows=CHUNK, n_items=None, mask=False,
          view=False):
    """One row of the table. `mode`: utils.GEMM256_MODE for the case. What the case means to reach, asserted exactly by the GPU
    test: `logits` / `dh` the GEMM entry points (short names of GEMM), `wt` whether the transposed head is built.
    `n_items`: None (counted), an int, or ("tensor", value) for a 0-dim GPU tensor. `mask`: MASKED_ROWS are removed by the
    `mask` argument. `view`: the hidden states are the [..., :H] view of a [B, L, H + 8] buffer."""
    assert name not in CASES
    CASES[name] = dict(name=name, V=V, mode=mode, logits=logits, dh=dh, wt=wt, dtype=dtype, softcap=softcap, scale=scale,
                       chunk_rows=chunk_rows, n_items=n_items, mask=mask, view=view)


_case("v1000", 1000, "off", "nt", "nt", True)                                          # plain; n_items counted
_case("v1000-scale", 1000, "off", "nt", "nt", True, scale=0.5)
# padded row stride 1008, scalar tail of the vector CE kernels, the [:, V:] padding
_case("v1003-cap", 1003, "off", "nt", "nt", True, softcap=30.0, n_items=160)
_case("v1003-cap-256", 1003, "on", "nt_256", "nt", True, softcap=30.0)
_case("v1003-cap-fp16", 1003, "off", "nt", "nt", True, softcap=30.0, dtype="fp16")
_case("v1024-256-nn", 1024, "on", "nt_256", "nn_256", False)                           # d(hidden) over W in place: no W^T
# column 8191 | 8192: two blocks of ce_bwd_kernel; row 8191 | 8192 of dW: the _DW_SCALE_ROWS boundary
_case("v8200-256", 8200, "on", "nt_256", "nt", True)
_case("v8200-fp16", 8200, "off", "nt", "nt", True, dtype="fp16")
_case("v8197-cap-256", 8197, "on", "nt_256", "nt", True, softcap=30.0)
# other entry arguments
_case("v1000-one-chunk", 1000, "off", "nt", "nt", True, chunk_rows=256)
_case("v1003-nitems-tensor", 1003, "off", "nt", "nt", True, n_items=("tensor", 100.0))
_case("v1024-cap-scale-mask-view-nn", 1024, "on", "nt_256", "nn_256", False, softcap=30.0, scale=0.5, n_items=150, mask=True,
      view=True)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def edge_columns(V):
    """0 | 7 | 8 (the first 16-byte vector of bf16 / fp16 and the one after), the last column of the last whole vector, the
    first column of the scalar tail (V % 8 != 0), the last column, and 8191 | 8192 where a row has them."""
    Vw = V // 8 * 8
    cols = [0, 7, 8, Vw - 1] + ([Vw] if V % 8 else []) + [V - 1] + ([8191, 8192] if V > 8192 else [])
    return list(dict.fromkeys(cols))


def edge_uses(V):
    """[(column e, row, is e the row's label)]: every edge column twice, once as a label and once beside another label."""
    out = []
    for k, e in enumerate(edge_columns(V)):
        out += [(e, EDGE_ROWS[2 * k], True), (e, EDGE_ROWS[2 * k + 1], False)]
    return out


def n_items_value(c, live_count):
    n = c["n_items"]
    if n is None:
        return float(live_count)
    return float(n[1]) if isinstance(n, tuple) else float(n)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(hidden [T, H], W [V, H], labels [B, L] int64, mask [B, L] bool or None) of a case, seeded, on the CPU, hidden and W in
    the activation dtype. Shared and never written to.

    h ~ 0.7 N(0, 1), W ~ 0.05 N(0, 1). For each use (e, r) of an edge column W[e] gets about c h_r / |h_r|^2 added, which sets
    the logit of row r at column e to c = (ln V + 1) / logit_scaling: ln V + 1 before the soft cap, whatever the scale, so
    that column e holds a good share of the row's softmax (e / (e + 1.2) of it without a cap). With a padded vocabulary one
    row is pad-sensitive: every row of W has 1.5 u subtracted (u a unit vector: a constant per token row, the softmax does not
    see it) and hidden[PAD_ROW] has 8 u added, which puts all of that row's logits near -12 -- a zero padding column counted
    into its logsumexp would take the mass."""
    c = CASES[name]
    V, dt = c["V"], DTYPES[c["dtype"]]
    h = 0.7 * torch.randn(T, H, generator=_gen("h", name), dtype=torch.float64)
    W = 0.05 * torch.randn(V, H, generator=_gen("W", name), dtype=torch.float64)
    bump = (math.log(V) + 1.0) / (c["scale"] or 1.0)
    labels = torch.randint(16, V // 8 * 8 - 8, (B, L), generator=_gen("labels", name))
    edges = set(edge_columns(V))
    for e in edge_columns(V):
        # both rows of the column at once: W[e] += sum_i a_i h_ri with (h_ri . h_rj) a = bump (a_i ~ bump / |h_ri|^2: the rows
        # are nearly orthogonal), and the random part of W[e] taken out along them, so that each row's logit at e is `bump` and
        # not bump + N(0, 0.56^2) -- at the low end of that the column held 0.15 of its row
        rs = [r for e2, r, _ in edge_uses(V) if e2 == e]
        hr = h[rs]
        W[e] += torch.linalg.solve(hr @ hr.t(), bump - hr @ W[e]) @ hr
    for e, r, is_label in edge_uses(V):
        b, l = divmod(r, L)
        if is_label:
            labels[b, l + 1] = e
        else:
            while int(labels[b, l + 1]) in edges:
                labels[b, l + 1] += 1
    for r in DEAD_ROWS:
        b, l = divmod(r, L)
        labels[b, l + 1] = -100
    if V % 8:
        u = torch.randn(H, generator=_gen("u", name), dtype=torch.float64)
        u /= u.norm()
        # (the random components along u taken out first: every logit of the row is then h_perp . W_v - 12, sigma 0.56)
        W -= (W @ u)[:, None] * u + 1.5 * u
        h[PAD_ROW] += (8.0 - h[PAD_ROW] @ u) * u
    mask = None
    if c["mask"]:
        mask = torch.ones(T, dtype=torch.bool)
        mask[list(MASKED_ROWS)] = False
        mask = mask.view(B, L)
    return h.to(dt), W.to(dt), labels, mask


# ---- the fp64 truth, the rounding model and its wrong variants ------------------------------------------------------------------
def shifted(labels, mask=None, shift=True):
    """The label of every token row, [T]: labels moved one position to the left, -100 at each sequence's last position, -100
    where `mask` is False."""
    s = torch.full_like(labels, -100)
    if shift:
        s[:, :-1] = labels[:, 1:]
    else:
        s.copy_(labels)
    if mask is not None:
        s = torch.where(mask, s, torch.full_like(s, -100))
    return s.reshape(-1)


def _compute(name, rounded, mutant=None):
    c = CASES[name]
    V, cap, scale = c["V"], c["softcap"], c["scale"]
    dt = DTYPES[c["dtype"]]
    rnd = (lambda x: x.to(dt).double()) if rounded else (lambda x: x)
    assert mutant is None or (rounded and mutant in mutants(name)), mutant
    h, W, labels, mask = case_inputs(name)
    h, W = h.double(), W.double()
    lab = shifted(labels, None if mutant == "mask_ignored" else mask, shift=mutant != "no_shift")
    live = lab != -100
    if mutant == "label_plus1":
        lab = torch.where(live, (lab + 1) % V, lab)
    n = float(live.sum()) if mutant == "n_items_ignored" else n_items_value(c, int(live.sum()))

    z = rnd(h @ W.t())                                             # 1. the logits, in the activation dtype
    t, dtdz = z, torch.ones_like(z)
    if scale:
        t = scale * t
        if mutant != "scale_factor_missing":
            dtdz = dtdz * scale
    if cap:
        th = torch.tanh(t / cap)
        t = cap * th
        if mutant != "no_cap_deriv":
            dtdz = dtdz * (1.0 - th * th)
    if mutant == "drop_last_col":
        lse = torch.logsumexp(t[:, :-1], dim=1)
    else:
        lse = torch.logsumexp(t, dim=1)
    if mutant == "pad_counted":
        lse = torch.logaddexp(lse, torch.full_like(lse, math.log(padded(V) - V)))
    p = torch.exp(t - lse[:, None])
    if mutant == "drop_last_col":
        p[:, -1] = 0.0
    onehot = torch.zeros_like(p)
    rows = torch.nonzero(live).flatten()
    onehot[rows, lab[rows]] = 1.0
    row_loss = torch.where(live, lse - t[torch.arange(T), lab.clamp(min=0)], torch.zeros_like(lse))
    livef = live.double()[:, None]
    dlog = rnd((p - onehot) * livef * dtdz / n)                    # 2. dlogits with 1 / n_items, in the activation dtype
    if mutant == "chunk_last_row":
        dlog[CHUNK - 1] = 0.0
    dh = rnd(dlog @ W)                                             # 3. d(hidden), one rounding
    dW = torch.zeros(V, H, dtype=torch.float64)
    for r0 in range(0, T, c["chunk_rows"]):                        # 4. dW, rounded after each chunk's accumulation
        part = dlog[r0:r0 + c["chunk_rows"]].t() @ h[r0:r0 + c["chunk_rows"]]
        dW = rnd(part if mutant == "dw_overwrite" else dW + part)
    dh = rnd(dh * UPSTREAM)                                        # 5. the upstream scale, one more rounding
    if mutant == "dw_tail_unscaled":
        dW = torch.cat([rnd(dW[:8192] * UPSTREAM), dW[8192:]])
    else:
        dW = rnd(dW * UPSTREAM)
    res = dict(dh=dh, dW=dW, row_loss=row_loss, loss=row_loss.sum() / n, live=live, n=n)
    if not rounded:
        # what each row's loss would be were it live (the single-row calls of the GPU test ignore the case's own mask) and how
        # far one ulp of every logit can move it: b_r = sum_v |p_v - y_v| |dt/dz_v| 2u |z_v| + LOSS_FP32. u is HALF an ulp; one
        # half comes from rounding the logits, the other from the GEMM's fp32 sum landing on the other side of a rounding
        # boundary.
        lab0 = shifted(labels)
        live0 = lab0 != -100
        y0 = torch.zeros_like(p)
        r0 = torch.nonzero(live0).flatten()
        y0[r0, lab0[r0]] = 1.0
        res["row_loss_unmasked"] = torch.where(live0, lse - t[torch.arange(T), lab0.clamp(min=0)], torch.zeros_like(lse))
        res["live_unmasked"] = live0
        res["b"] = ((p - y0).abs() * dtdz.abs() * 2 * U16[c["dtype"]] * z.abs()).sum(1) + LOSS_FP32
        res["p"] = p
    return res


def truth64(name):
    """Everything in fp64, nothing rounded: label shift, mask, scale then soft cap, n_items; `row_loss` [T] (0 on dead rows),
    `loss`, `dh` [T, H] and `dW` [V, H] with the upstream scale, `live` [T]; and for the row-loss checks `row_loss_unmasked` /
    `live_unmasked` (the case's mask not applied), the bound `b` [T] and the softmax `p` [T, V]."""
    return _compute(name, rounded=False)


def rounding_model(name, mutant=None):
    """The same computation in fp64 with the product's rounding points (numbered in `_compute`): the logits, dlogits including
    1 / n_items, d(hidden) = round(dlogits @ W), dW after each chunk's accumulation following the case's chunking, and both
    gradients once more after the upstream scale. The yardstick of the GPU tests, not a model of any kernel's schedule.
    `mutant`: None or one of `mutants(name)`."""
    return _compute(name, rounded=True, mutant=mutant)


def mutants(name):
    """The wrong variants of the rounding model that the checks must reject on this case:
      drop_last_col         the softmax without the last vocabulary column
      pad_counted           the zero padding columns counted into the logsumexp (V % 8 != 0)
      label_plus1, no_shift the label one column / one position off
      chunk_last_row        row 63, the last of the first chunk, gets no gradient (more than one chunk)
      dw_overwrite          dW holds the last chunk alone (more than one chunk)
      dw_tail_unscaled      rows >= 8192 of dW without the upstream scale (V > 8192)
      no_cap_deriv          1 - tanh^2 missing (soft cap)          scale_factor_missing   the factor missing (logit scaling)
      mask_ignored          (mask cases)                           n_items_ignored        the live rows counted (n_items given)"""
    c = CASES[name]
    out = ["drop_last_col", "label_plus1", "no_shift"]
    if c["V"] % 8:
        out.append("pad_counted")
    if c["chunk_rows"] < T:
        out += ["chunk_last_row", "dw_overwrite"]
    if c["V"] > 8192:
        out.append("dw_tail_unscaled")
    if c["softcap"]:
        out.append("no_cap_deriv")
    if c["scale"]:
        out.append("scale_factor_missing")
    if c["mask"]:
        out.append("mask_ignored")
    if c["n_items"] is not None:
        out.append("n_items_ignored")
    return out


# ---- the error and the verdict ----------------------------------------------------------------------------------------------
def row_err(got, ref):
    """The L2 norm of got - ref per row, fp64 [rows]: a token row of d(hidden), a vocabulary row of dW."""
    d = got.detach().double().cpu().reshape(ref.shape) - ref
    return d.norm(dim=1)


BOUND_FACTOR = 4        # the project's figure (tests/_attn_edges.py, tests/_lora_blocks.py)
MAX_FACTOR = 8          # no per-tensor exception goes beyond this; a ratio above it is a finding
FACTORS = {}            # tensor name -> factor, where a healthy route needs more than BOUND_FACTOR (with the measured reason)
TENSORS = ("dh", "dW")


@functools.lru_cache(maxsize=None)
def build_case(name):
    """A case computed once per process and shared by every test that reads it (nothing in it is written to)."""
    truth, model = truth64(name), rounding_model(name)
    err = {t: row_err(model[t], truth[t]) for t in TENSORS}
    return dict(CASES[name], truth=truth, model=model, model_err=err)


def judge(case, tensor, got):
    """(err per row of `got` against the fp64 truth, the rounding model's, the worst ratio, the verdict). A row passes when its
    error is at most the tensor's factor x the model's error on that row; a row whose truth is exactly zero (an ignored or
    masked token: the model is exact there too) therefore has to be exactly zero. 0 / 0 counts as ratio 0."""
    c = case if isinstance(case, dict) else build_case(case)
    ref, model = c["truth"][tensor], c["model_err"][tensor]
    err = row_err(got, ref)
    zero = ref.norm(dim=1) == 0
    assert not bool((model[zero] != 0).any()), "the rounding model is not exact where the truth is zero"
    ratio = torch.where(err == 0, torch.zeros_like(err), err / model)
    factor = FACTORS.get(tensor, BOUND_FACTOR)
    assert BOUND_FACTOR <= factor <= MAX_FACTOR
    return err, model, float(ratio.max()), bool((err <= factor * model).all())


def checked_rows(name):
    """The rows whose loss the GPU test takes alone: every edge row in use, the pad-sensitive row, two interior rows."""
    V = CASES[name]["V"]
    return [r for _, r, _ in edge_uses(V)] + ([PAD_ROW] if V % 8 else []) + list(INTERIOR_ROWS)
