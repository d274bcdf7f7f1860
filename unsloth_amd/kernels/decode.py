"""Single-token decode launchers (csrc/decode.hip); mirror of the decode half of unsloth/kernels/utils.py.

`fast_gemv` / the bsz == 1 branch of `fast_linear_forward` (utils.py:872-977, :1082-1125) become ONE `uamd_gemv`
launch per group of projections that share the token (q|k|v, gate|up), plus one small `uamd_gemv` over the LoRA A rows
that share it. NF4 weights are read in bitsandbytes' format straight from the `Params4bit` storage: nothing is
dequantised to memory. The token rows of a batch of 2 .. 64 sequences share one pass over the weights: `uamd_gemv_rows`
up to 16 rows, `uamd_gemv_rows64` above (`gemv_rows`, `gemv_rows64`, `linear_group_rows`), where utils.py:1095-1097
dequantises and calls matmul.
"""
import ctypes

import torch

from .. import _lib
from .._lib import GemvGroup, GemvPrologue

MAX_GROUPS = 4
HEAD_DIMS = (64, 128)                 # the head dims the attention kernels are instantiated for


def block_keys(D):
    """Keys one block-load of the decode attention kernels covers (4 waves x 64 lanes x 16 B over D 16-bit values per key):
    `split_keys` must be a multiple of it."""
    assert D in HEAD_DIMS
    return 2048 // D
_SYNC = {}


class HandOff:
    """Device workspace + tag source of the in-launch hand-offs (uamd_gemv_fused's t = A x, uamd_attn_decode_fused's partials).
    Every launch on a workspace needs a tag no earlier launch on it used:
      * eager launches: `next_tag()`, a host counter (step_dev None);
      * launches captured in a hipGraph: a per-launch-SITE constant `site` (1 .. TAG_STRIDE - 1) plus TAG_STRIDE x the value of
        the device counter `step_dev` (int32 [1]), which the owner advances once per replay (DecodeEngine: with the position).
    Launches that share a HandOff must be ordered (one stream / one graph)."""

    def __init__(self, dev, nbytes=None, step_dev=None):
        self.ws = torch.zeros(((nbytes or _lib.GEMV_SYNC_BYTES) + 3) // 4, dtype=torch.int32, device=dev)
        self.step_dev = step_dev
        self._host = 0

    def next_tag(self):
        # below 2^31 so that host tags and step tags (step * TAG_STRIDE + site, step >= 1) of one workspace cannot meet early; on
        # wrap-around the workspace is cleared
        self._host += 1
        if self._host >= (1 << 31):
            self.ws.zero_()
            self._host = 1
        return self._host

    def tags(self, site=None):
        """(tag, tag_dev pointer or None) for one launch."""
        if site is None or self.step_dev is None:
            return self.next_tag(), None
        assert 0 < site < _lib.TAG_STRIDE
        return int(site), self.step_dev


def sync_workspace(dev):
    """The default HandOff of a device, for eager launches on the current stream; a caller that decodes on several streams at
    once, or under a hipGraph, owns its own (`fused["sync"]`, as DecodeEngine does)."""
    key = (dev.type, dev.index)
    ws = _SYNC.get(key)
    if ws is None:
        ws = _SYNC[key] = HandOff(dev)
    return ws


def _nf4_fields(qs):
    """(absmax_u8, absmax_f32, code2, absmax2, offset, blocksize2) of a quant state; python floats cached on it."""
    if getattr(qs, "quant_type", "nf4") not in ("nf4", None):
        raise NotImplementedError(f"uamd_gemv decodes NF4 only (quant_type {qs.quant_type!r})")
    if qs.nested:
        off = getattr(qs, "_offset_float", None)
        if off is None:
            off = qs._offset_float = float(qs.offset)          # one host sync per weight, outside any graph capture
        return qs.absmax, None, qs.state2.code, qs.state2.absmax, off, int(qs.state2.blocksize)
    return None, qs.absmax, None, None, 0.0, 0


def lora_a_rows(A_list, dtype):
    """[sum R_i, K] activation-dtype copy of the LoRA A factors that share an input, cached on the first Parameter
    (the reference caches `lora_A._fast_lora = lora_A.to(dtype)`, utils.py:1104-1106; weights are frozen at inference)."""
    from .utils import _stamp
    key = A_list[0]
    ent = getattr(key, "_uamd_fast_lora_rows", None)
    # validity = kernels/utils._stamp, the rule of every factor cache: _version alone is not enough -- the fused optimizers
    # (optim.FlatAdamW's raw HIP kernel, torch's fused AdamW) update parameters WITHOUT bumping it, so the global
    # optimizer-step / model-forward epoch and the storage address are part of the key (generate -> train -> generate
    # must not multiply the trained B by the pre-training A)
    vers = tuple(_stamp(a) for a in A_list)
    stamps, rows, shapes = ent if ent is not None else (None, None, None)
    if stamps != vers or rows.dtype != dtype:
        was, shapes = shapes, [a.shape[0] for a in A_list]
        if (rows is not None and rows.dtype == dtype and was == shapes and rows.shape[1] == A_list[0].shape[1]
                and rows.device == A_list[0].device):
            # refresh IN PLACE: a captured hipGraph of the token step holds this buffer's address
            r0 = 0
            with torch.no_grad():
                for a in A_list:
                    rows[r0:r0 + a.shape[0]].copy_(a.detach())
                    r0 += a.shape[0]
        else:
            rows = torch.cat([a.detach().to(dtype) for a in A_list], dim=0).contiguous()
        key._uamd_fast_lora_rows = (vers, rows, shapes)
    return rows


def gemv(x, groups, nf4, blocksize=64, pro=None):
    """One launch. x: [K] (contiguous, 16-bit). groups: list of dicts with W, N and optionally qs (quant state),
    y, y_f32, lora_t, lora_b, lora_scale, R, bias. Returns the list of outputs.
    `pro` (uamd_gemv_fused): dict(mode=0|1|2, x2=, res=, norm_w=, eps=, h_out=, a_rows=, t_off=[per group], sync=HandOff, site=,
    glu=) -- the
    token is produced inside the launch (SwiGLU of x and x2 / residual add + RMSNorm; x may be None in mode 2), the LoRA
    t = A x is computed once by the launch's first workgroups from the stacked A rows (handed over through `sync`) instead
    of arriving from a launch of its own, and with glu=True the two groups (gate, up) leave ONE output h = SwiGLU(gate, up)."""
    ref = x if x is not None else pro["res"]
    _lib.require_gpu(ref)
    K = ref.numel()
    dtype, dev = ref.dtype, ref.device
    assert 1 <= len(groups) <= MAX_GROUPS
    arr = (GemvGroup * len(groups))()
    outs, keep = [], []
    for i, g in enumerate(groups):
        N = g["N"]
        y_f32 = bool(g.get("y_f32", False))
        y = g.get("y")
        if y is None:
            y = torch.empty(N, dtype=torch.float32 if y_f32 else dtype, device=dev)
        outs.append(y)
        W = g["W"]
        e = arr[i]
        e.W = W.data_ptr()
        if nf4:
            a_u8, a_f32, code2, absmax2, off, bs2 = _nf4_fields(g["qs"])
            e.absmax_u8 = a_u8.data_ptr() if a_u8 is not None else None
            e.absmax_f32 = a_f32.data_ptr() if a_f32 is not None else None
            e.code2 = code2.data_ptr() if code2 is not None else None
            e.absmax2 = absmax2.data_ptr() if absmax2 is not None else None
            e.offset, e.blocksize2, e.ldw = off, bs2, 0
        else:
            assert W.dim() == 2 and W.stride(1) == 1 and W.dtype == dtype and W.shape[1] == K
            e.ldw = W.stride(0)
        e.y = y.data_ptr()
        t = g.get("lora_t")
        if t is not None or (pro is not None and pro.get("a_rows") is not None and g.get("lora_b") is not None):
            B = g["lora_b"]
            assert (t is None or t.dtype == torch.float32) and B.stride(1) == 1
            e.lora_t = t.data_ptr() if t is not None else None
            e.lora_b, e.ld_lb = B.data_ptr(), B.stride(0)
            e.lora_scale, e.R = float(g["lora_scale"]), int(g["R"])
            e.lora_b_f32 = int(B.dtype == torch.float32)
            assert B.dtype in (torch.float32, dtype)
            keep += [t, B]
        bias = g.get("bias")
        e.bias = bias.data_ptr() if bias is not None else None
        e.N, e.y_f32 = N, int(y_f32)
    if pro is None:
        _lib.call("uamd_gemv", ref, _lib.ptr(x), K, arr, len(groups), int(bool(nf4)), int(blocksize), _lib.dtype_code(dtype),
                  _lib.stream_of(ref))
        return outs
    P = GemvPrologue()
    P.mode = int(pro.get("mode", 0))
    P.glu = int(bool(pro.get("glu", False)))
    for name in ("x2", "res", "norm_w", "h_out", "a_rows"):
        tns = pro.get(name)
        setattr(P, name, tns.data_ptr() if tns is not None else None)
        keep.append(tns)
    if P.mode == 1:
        assert pro["x2"].dtype == dtype and pro["x2"].numel() == K and pro["x2"].is_contiguous()
    if P.mode == 2:
        w = pro["norm_w"]
        assert w.numel() == K and w.is_contiguous() and w.dtype in (dtype, torch.float32) and pro["res"].is_contiguous()
        P.w_f32 = int(w.dtype == torch.float32 and dtype != torch.float32)
        P.eps = float(pro["eps"])
    a_rows = pro.get("a_rows")
    if a_rows is not None:
        assert a_rows.dtype == dtype and a_rows.stride(1) == 1 and a_rows.shape[1] == K
        P.Rt, P.ld_a = int(a_rows.shape[0]), int(a_rows.stride(0))
        for i, off in enumerate(pro["t_off"]):
            P.t_off[i] = int(off)
        ho = pro.get("sync")
        if ho is None:
            ho = sync_workspace(dev)
        assert isinstance(ho, HandOff) and ho.ws.numel() * 4 >= _lib.GEMV_SYNC_BYTES and ho.ws.device == dev
        tag, tag_dev = ho.tags(pro.get("site"))
        P.sync, P.tag = ho.ws.data_ptr(), tag
        P.tag_dev = tag_dev.data_ptr() if tag_dev is not None else None
        keep += [ho.ws, tag_dev]
    _lib.call("uamd_gemv_fused", ref, _lib.ptr(x) if x is not None else None, K, arr, len(groups), int(bool(nf4)),
              int(blocksize), _lib.dtype_code(dtype), _lib.stream_of(ref), ctypes.byref(P))
    return outs


def linear_group(x, projs, out=None, fused=None):
    """y_i = W_i x + s_i B_i (A_i x) (+ bias_i) for projections sharing the token x [K]: at most two launches (the A rows
    of all members, then the weights). projs: (W, quant_state, A, B, s[, bias]) as get_lora_parameters(_bias) returns
    them. `out`: optional preallocated [sum N_i] row the outputs are written into back to back. Returns the views.
    `fused` (dict: mode / x2 / res / norm_w / eps / h_out / sync / site / glu, see gemv): ONE launch -- the token is produced inside it
    (x may be None in mode 2), the A x products are computed by the launch's own first workgroups, and with glu=True the two
    projections (gate, up) return ONE vector h = SwiGLU(gate, up) of N entries."""
    if fused is not None:
        return _linear_group_fused(x, projs, out, fused)
    x = x.reshape(-1)
    dtype = x.dtype
    nf4 = projs[0][1] is not None
    assert all((p[1] is not None) == nf4 for p in projs), "a launch is all-NF4 or all-16-bit"
    Ns = [int(p[1].shape[0]) if p[1] is not None else int(p[0].shape[0]) for p in projs]
    if out is None:
        out = torch.empty(sum(Ns), dtype=dtype, device=x.device)
    with_lora = [p for p in projs if p[2] is not None]
    t_all = None
    if with_lora:
        A_rows = lora_a_rows([p[2] for p in with_lora], dtype)
        (t_all,) = gemv(x, [dict(W=A_rows, N=A_rows.shape[0], y_f32=True)], nf4=False)
    groups, col, r0 = [], 0, 0
    for p, N in zip(projs, Ns):
        W, qs, A, B, s = p[:5]
        g = dict(W=W, N=N, qs=qs, y=out[col:col + N], bias=p[5] if len(p) > 5 else None)
        if A is not None:
            R = A.shape[0]
            g.update(lora_t=t_all[r0:r0 + R], lora_b=B.detach(), lora_scale=s, R=R)
            r0 += R
        groups.append(g)
        col += N
    blocksize = int(projs[0][1].blocksize) if nf4 else 64
    ys = []
    for i in range(0, len(groups), MAX_GROUPS):
        ys += gemv(x, groups[i:i + MAX_GROUPS], nf4=nf4, blocksize=blocksize)
    return ys


MAX_ROWS = 16                         # token rows of one uamd_gemv_rows launch
MAX_ROWS_WIDE = 64                    # token rows of one uamd_gemv_rows64 launch


def gemv_rows(x, groups, nf4, blocksize=64, M=None):
    """One uamd_gemv_rows launch: x [M, K] (unit stride along K, any row stride that is a multiple of 8; M <= 16) against the
    groups of `gemv`. A group's `y` is an [M, N] view whose rows may be strided (all groups of a launch share the row stride:
    adjacent column ranges of one buffer) and is allocated when absent; `lora_t` is fp32 [M, R] (a column range of the t
    buffer, one row stride for all groups). `M` < x.shape[0] launches the first M rows only. Returns the outputs."""
    return _rows_launch("uamd_gemv_rows", x, groups, nf4, blocksize, M)


def gemv_rows64(x, groups, nf4, blocksize=64, M=None):
    """`gemv_rows` for M <= 64 token rows: one uamd_gemv_rows64 launch, still one pass over the weights. Every output row has
    the bits `gemv_rows` gives that token row (a 64-row launch equals four 16-row launches on its slices)."""
    return _rows_launch("uamd_gemv_rows64", x, groups, nf4, blocksize, M)


def _rows_launch(symbol, x, groups, nf4, blocksize, M):
    _lib.require_gpu(x)
    assert x.dim() == 2 and x.stride(1) == 1
    M = x.shape[0] if M is None else int(M)
    K = x.shape[1]
    dtype, dev = x.dtype, x.device
    assert 1 <= len(groups) <= MAX_GROUPS
    arr = (GemvGroup * len(groups))()
    outs, keep, ldy, ldt, f32 = [], [], None, 0, None
    for i, g in enumerate(groups):
        N = g["N"]
        y_f32 = bool(g.get("y_f32", False))
        y = g.get("y")
        if y is None:
            y = torch.empty(x.shape[0], N, dtype=torch.float32 if y_f32 else dtype, device=dev)
        assert y.dim() == 2 and y.shape[1] == N and y.stride(1) == 1 and y.dtype == (torch.float32 if y_f32 else dtype)
        assert y.shape[0] >= M and (M == 1 or ldy in (None, y.stride(0))), "the groups of a launch share the row stride of y"
        assert f32 in (None, y_f32), "a launch stores 16-bit or fp32 rows, not both"
        ldy, f32 = (y.stride(0) if M > 1 else N), y_f32         # (one row: the stride is never used)
        outs.append(y)
        W = g["W"]
        e = arr[i]
        e.W = W.data_ptr()
        if nf4:
            a_u8, a_f32, code2, absmax2, off, bs2 = _nf4_fields(g["qs"])
            e.absmax_u8 = a_u8.data_ptr() if a_u8 is not None else None
            e.absmax_f32 = a_f32.data_ptr() if a_f32 is not None else None
            e.code2 = code2.data_ptr() if code2 is not None else None
            e.absmax2 = absmax2.data_ptr() if absmax2 is not None else None
            e.offset, e.blocksize2, e.ldw = off, bs2, 0
        else:
            assert W.dim() == 2 and W.stride(1) == 1 and W.dtype == dtype and W.shape[1] == K
            e.ldw = W.stride(0)
        e.y = y.data_ptr()
        t = g.get("lora_t")
        if t is not None:
            B = g["lora_b"]
            assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and B.stride(1) == 1
            assert B.dtype in (torch.float32, dtype)
            assert t.shape[0] >= M and (M == 1 or ldt in (0, t.stride(0)))
            ldt = t.stride(0) if M > 1 else t.shape[1]
            e.lora_t, e.lora_b, e.ld_lb = t.data_ptr(), B.data_ptr(), B.stride(0)
            e.lora_scale, e.R, e.lora_b_f32 = float(g["lora_scale"]), int(g["R"]), int(B.dtype == torch.float32)
            keep += [t, B]
        bias = g.get("bias")
        e.bias = bias.data_ptr() if bias is not None else None
        e.N, e.y_f32 = N, int(y_f32)
    _lib.call(symbol, x, _lib.ptr(x), x.stride(0) if M > 1 else K, M, K, arr, len(groups),
              int(ldy), int(ldt), int(bool(nf4)), int(blocksize), _lib.dtype_code(dtype), _lib.stream_of(x))
    return outs


def linear_group_rows(x2d, projs, out=None, y_f32=False, t_buf=None):
    """`linear_group` for M = 1 .. 64 token rows x2d [M, K] that share one pass over the weights (uamd_gemv_rows up to 16 rows,
    uamd_gemv_rows64 above; the same bits per row either way): at most two
    launches per four projections (the stacked A rows of all members -> t fp32 [M, sum R], then the weights). `out`: an
    [M, sum N_i] buffer (rows may be strided) the outputs are written into side by side -- q|k|v land in the fused row with no
    concatenation; `t_buf`: an fp32 [M, >= sum R] buffer to reuse under a hipGraph. Returns the [M, N_i] views. The value of a
    row depends on that row and the weights alone (the kernel's row-independence contract)."""
    assert x2d.dim() == 2 and 1 <= x2d.shape[0] <= MAX_ROWS_WIDE
    M, dtype = x2d.shape[0], x2d.dtype
    launch = gemv_rows if M <= MAX_ROWS else gemv_rows64
    nf4 = projs[0][1] is not None
    assert all((p[1] is not None) == nf4 for p in projs), "a launch is all-NF4 or all-16-bit"
    Ns = [int(p[1].shape[0]) if p[1] is not None else int(p[0].shape[0]) for p in projs]
    if out is None:
        out = torch.empty(M, sum(Ns), dtype=torch.float32 if y_f32 else dtype, device=x2d.device)
    assert out.shape == (M, sum(Ns))
    with_lora = [p for p in projs if p[2] is not None]
    t_all = None
    if with_lora:
        A_rows = lora_a_rows([p[2] for p in with_lora], dtype)
        Rt = A_rows.shape[0]
        t_all = t_buf[:M, :Rt] if t_buf is not None else torch.empty(M, Rt, dtype=torch.float32, device=x2d.device)
        launch(x2d, [dict(W=A_rows, N=Rt, y=t_all, y_f32=True)], nf4=False)
    groups, col, r0 = [], 0, 0
    for p, N in zip(projs, Ns):
        W, qs, A, B, s = p[:5]
        g = dict(W=W, N=N, qs=qs, y=out[:, col:col + N], y_f32=y_f32, bias=p[5] if len(p) > 5 else None)
        if A is not None:
            R = A.shape[0]
            g.update(lora_t=t_all[:, r0:r0 + R], lora_b=B.detach(), lora_scale=s, R=R)
            r0 += R
        groups.append(g)
        col += N
    blocksize = int(projs[0][1].blocksize) if nf4 else 64
    ys = []
    for i in range(0, len(groups), MAX_GROUPS):
        ys += launch(x2d, groups[i:i + MAX_GROUPS], nf4=nf4, blocksize=blocksize)
    return ys


def _linear_group_fused(x, projs, out, fused):
    ref = x if x is not None else fused["res"]
    if x is not None:
        x = x.reshape(-1)
    dtype, dev = ref.dtype, ref.device
    nf4 = projs[0][1] is not None
    assert all((p[1] is not None) == nf4 for p in projs), "a launch is all-NF4 or all-16-bit"
    assert len(projs) <= MAX_GROUPS
    Ns = [int(p[1].shape[0]) if p[1] is not None else int(p[0].shape[0]) for p in projs]
    glu = bool(fused.get("glu", False))
    if glu:
        assert len(projs) == 2 and Ns[0] == Ns[1], "glu: gate and up of one MLP"
    if out is None:
        out = torch.empty(Ns[0] if glu else sum(Ns), dtype=dtype, device=dev)
    with_lora = [p for p in projs if p[2] is not None]
    pro = dict(fused)
    pro.setdefault("mode", 0)
    t_off = [0] * len(projs)
    if with_lora:
        pro["a_rows"] = lora_a_rows([p[2] for p in with_lora], dtype)
    groups, col, r0 = [], 0, 0
    for i, (p, N) in enumerate(zip(projs, Ns)):
        W, qs, A, B, s = p[:5]
        g = dict(W=W, N=N, qs=qs, y=out[:N] if glu else out[col:col + N], bias=p[5] if len(p) > 5 else None)
        if A is not None:
            R = A.shape[0]
            g.update(lora_b=B.detach(), lora_scale=s, R=R)
            t_off[i] = r0
            r0 += R
        groups.append(g)
        col += N
    pro["t_off"] = t_off
    blocksize = int(projs[0][1].blocksize) if nf4 else 64
    ys = gemv(x, groups, nf4=nf4, blocksize=blocksize, pro=pro)
    return ys[:1] if glu else ys


def rope_kv_append(qkv, cos, sin, kv_len, k_cache, v_cache, Hq, Hk, D, rope_pos=None):
    """In place on qkv [B, (Hq + 2 Hk) D]; k_cache / v_cache [B, Hk, S_max, D]; kv_len int32 [B] on the device."""
    B = qkv.shape[0]
    assert qkv.stride(1) == 1 and k_cache.is_contiguous() and v_cache.is_contiguous() and kv_len.dtype == torch.int32
    assert cos.stride(1) == 1 and sin.stride() == cos.stride() and cos.dtype == qkv.dtype
    _lib.call("uamd_rope_kv_append", qkv, _lib.ptr(qkv), qkv.stride(0), _lib.ptr(cos), _lib.ptr(sin), cos.stride(0),
              _lib.ptr(kv_len), _lib.ptr(rope_pos) if rope_pos is not None else None, _lib.ptr(k_cache), _lib.ptr(v_cache),
              k_cache.stride(0), k_cache.stride(1), B, Hq, Hk, D, k_cache.shape[2], _lib.dtype_code(qkv.dtype),
              _lib.stream_of(qkv))


def attn_decode(q, k_cache, v_cache, kv_len, out, partials, split_keys, scale, len_add=1, window=0):
    """q [B, Hq*D] (a view into the fused qkv row is fine), out [B, Hq*D]; partials fp32 [B, Hq, nsplit, D + 2]."""
    B, Hk, S_max, D = k_cache.shape
    Hq = partials.shape[1]
    nsplit = partials.shape[2]
    assert nsplit * split_keys >= S_max and q.stride(1) == 1 and out.stride(1) == 1
    _lib.call("uamd_attn_decode", q, _lib.ptr(q), q.stride(0), _lib.ptr(k_cache), _lib.ptr(v_cache), k_cache.stride(0),
              k_cache.stride(1), _lib.ptr(kv_len), int(len_add), _lib.ptr(partials), _lib.ptr(out), out.stride(0), B, Hq, Hk, D,
              nsplit, int(split_keys), int(window), float(scale), _lib.dtype_code(q.dtype), _lib.stream_of(q))
    return out


MAX_SHARE = 16                        # samples per prompt of one uamd_attn_decode_shared launch (n * G <= 128 query rows)


def attn_decode_shared(q, pk, pv, prompt_len, n_share, sk, sv, new_len, out, partials, split_keys, scale, len_add=1, window=0):
    """`attn_decode` for P groups of `n_share` adjacent rows that share their prompt's keys (uamd_attn_decode_shared): q, out
    [P * n, Hq*D]; pk / pv [P, Hk, S_p, D] with prompt_len int32 [P]; sk / sv [P * n, Hk, S_n, D] with new_len int32 [P * n];
    partials fp32 [P * n, Hq, S_p / split_keys + S_n / split_keys, D + 2]. Row r attends the last `window` keys (0: all) of
    prompt r // n followed by its own new_len[r] + len_add suffix keys."""
    _lib.require_gpu(q)
    P, Hk, S_p, D = pk.shape
    B, _, S_n, _ = sk.shape
    Hq = partials.shape[1]
    nsp, nsn = S_p // split_keys, S_n // split_keys
    assert pv.shape == pk.shape and sv.shape == sk.shape and tuple(sk.shape[1::2]) == (Hk, D) and B == P * int(n_share)
    assert S_p % split_keys == 0 and S_n % split_keys == 0 and tuple(partials.shape) == (B, Hq, nsp + nsn, D + 2)
    assert partials.is_contiguous() and partials.dtype == torch.float32
    assert q.stride(1) == 1 and out.stride(1) == 1 and q.shape[0] == B and out.shape[0] == B
    assert pk.stride()[2:] == (D, 1) and pv.stride() == pk.stride() and sk.stride()[2:] == (D, 1) and sv.stride() == sk.stride()
    assert pk.dtype == pv.dtype == sk.dtype == sv.dtype == q.dtype == out.dtype
    assert prompt_len.dtype == torch.int32 and new_len.dtype == torch.int32 and prompt_len.numel() == P and new_len.numel() == B
    assert prompt_len.is_contiguous() and new_len.is_contiguous()
    _lib.call("uamd_attn_decode_shared", q, _lib.ptr(q), q.stride(0), _lib.ptr(pk), _lib.ptr(pv), pk.stride(0), pk.stride(1),
              _lib.ptr(prompt_len), int(n_share), _lib.ptr(sk), _lib.ptr(sv), sk.stride(0), sk.stride(1), _lib.ptr(new_len),
              int(len_add), _lib.ptr(partials), _lib.ptr(out), out.stride(0), P, Hq, Hk, D, nsp, nsn, int(split_keys),
              int(window), float(scale), _lib.dtype_code(q.dtype), _lib.stream_of(q))
    return out


MAX_SPAN = 16                         # token rows per sequence of one span step (uamd_gemv_rows' 16 rows; R * G <= 128 query rows)
MAX_EOS = 8                           # eos ids uamd_accept_greedy compares against


def rope_kv_append_span(qkv, cos, sin, kv_len, k_cache, v_cache, R, Hq, Hk, D):
    """`rope_kv_append` for R new tokens per sequence (uamd_rope_kv_append_span): in place on qkv [B * R, (Hq + 2 Hk) D], row
    b * R + j at RoPE position and cache slot kv_len[b] + j; kv_len is not advanced. The bits of R successive appends."""
    B = k_cache.shape[0]
    assert qkv.shape[0] == B * int(R) and qkv.stride(1) == 1 and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert kv_len.dtype == torch.int32 and kv_len.numel() >= B
    assert cos.stride(1) == 1 and sin.stride() == cos.stride() and cos.dtype == qkv.dtype
    _lib.call("uamd_rope_kv_append_span", qkv, _lib.ptr(qkv), qkv.stride(0), _lib.ptr(cos), _lib.ptr(sin), cos.stride(0),
              _lib.ptr(kv_len), _lib.ptr(k_cache), _lib.ptr(v_cache), k_cache.stride(0), k_cache.stride(1), B, int(R), Hq, Hk, D,
              k_cache.shape[2], _lib.dtype_code(qkv.dtype), _lib.stream_of(qkv))


def attn_decode_span(q, k_cache, v_cache, kv_len, R, out, partials, split_keys, scale, window=0):
    """Attention of the R tokens per sequence that `rope_kv_append_span` has just appended (uamd_attn_decode_span): q, out
    [B * R, Hq*D] (q may be a view into the fused qkv rows); partials fp32 [B * R, Hq, nsplit, D + 2]. Row (b, j) attends keys
    [max(0, t - window), t), t = kv_len[b] + j + 1, of sequence b's cache, which holds kv_len[b] + R keys by now."""
    _lib.require_gpu(q)
    B, Hk, S_max, D = k_cache.shape
    Hq, nsplit = partials.shape[1], partials.shape[2]
    assert tuple(partials.shape) == (B * int(R), Hq, nsplit, D + 2) and partials.is_contiguous() and partials.dtype == torch.float32
    assert nsplit * split_keys >= S_max and q.stride(1) == 1 and out.stride(1) == 1
    assert q.shape[0] == B * int(R) and out.shape[0] == B * int(R)
    assert k_cache.stride()[2:] == (D, 1) and v_cache.stride() == k_cache.stride() and v_cache.shape == k_cache.shape
    assert k_cache.dtype == v_cache.dtype == q.dtype == out.dtype and kv_len.dtype == torch.int32 and kv_len.numel() >= B
    _lib.call("uamd_attn_decode_span", q, _lib.ptr(q), q.stride(0), _lib.ptr(k_cache), _lib.ptr(v_cache), k_cache.stride(0),
              k_cache.stride(1), _lib.ptr(kv_len), int(R), _lib.ptr(partials), _lib.ptr(out), out.stride(0), B, Hq, Hk, D,
              nsplit, int(split_keys), int(window), float(scale), _lib.dtype_code(q.dtype), _lib.stream_of(q))
    return out


def ngram_draft(hist, hist_len, K, n_max, tok, n_draft):
    """The prompt-lookup draft of one sequence (uamd_ngram_draft; the rule is stated in include/unsloth_amd.h): hist int64 [cap],
    hist_len int32 [1] -> tok int64 [K + 1] = (last token, the draft, zeros), n_draft int32 [1]. Everything on the device."""
    _lib.require_gpu(hist)
    assert hist.dtype == torch.long and hist.is_contiguous() and tok.dtype == torch.long and tok.is_contiguous()
    assert tok.numel() >= int(K) + 1 and hist_len.dtype == torch.int32 and n_draft.dtype == torch.int32
    _lib.call("uamd_ngram_draft", hist, _lib.ptr(hist), _lib.ptr(hist_len), hist.numel(), int(n_max), int(K), _lib.ptr(tok),
              _lib.ptr(n_draft), _lib.stream_of(hist))


def accept_greedy(tok, amax, K, eos, hist, hist_len, kv_len, remaining, done, n_draft, stats):
    """The verdict of a greedy verify step (uamd_accept_greedy; the rule is stated in include/unsloth_amd.h): tok, amax int64
    [K + 1]; eos int64 [<= 8] or None; hist int64 [cap]; hist_len, kv_len, remaining, done, n_draft int32 [1]; stats int64 [4]
    (steps, drafted, accepted, tokens). Everything on the device, updated in place."""
    _lib.require_gpu(tok)
    n_eos = 0 if eos is None else eos.numel()
    assert n_eos <= MAX_EOS and (eos is None or (eos.dtype == torch.long and eos.is_contiguous()))
    assert tok.dtype == amax.dtype == hist.dtype == stats.dtype == torch.long and stats.numel() >= 4
    assert tok.numel() >= int(K) + 1 and amax.numel() >= int(K) + 1
    assert all(t.dtype == torch.int32 for t in (hist_len, kv_len, remaining, done, n_draft))
    assert all(t.is_contiguous() for t in (tok, amax, hist, stats))
    _lib.call("uamd_accept_greedy", tok, _lib.ptr(tok), _lib.ptr(amax), int(K), _lib.ptr(eos), n_eos, _lib.ptr(hist),
              hist.numel(), _lib.ptr(hist_len), _lib.ptr(kv_len), _lib.ptr(remaining), _lib.ptr(done), _lib.ptr(n_draft),
              _lib.ptr(stats), _lib.stream_of(tok))


def _fp8_cache(codes, scales):
    """Asserts the layout of one FP8 cache (include/unsloth_amd.h): codes uint8 [B, Hk, S_max, D] and scales fp32 [B, Hk, S_max];
    the batch stride is free (every n-th row of a cache is a cache), the rest is dense. Returns (B, Hk, S_max, D)."""
    B, Hk, S_max, D = codes.shape
    assert D in HEAD_DIMS and codes.dtype == torch.uint8 and scales.dtype == torch.float32 and scales.device == codes.device
    assert tuple(scales.shape) == (B, Hk, S_max)
    assert codes.stride()[1:] == (S_max * D, D, 1) and scales.stride()[1:] == (S_max, 1)
    assert codes.stride(0) == scales.stride(0) * D and codes.stride(0) >= Hk * S_max * D
    return B, Hk, S_max, D


def kv_store_fp8(x, codes, scales):
    """x [B, Hk, T, D] (16-bit, unit stride along D, any other strides that are multiples of 8: the transposed view of prefill)
    -> positions [0, T) of the FP8 cache `codes` (uint8 [B, Hk, S_max, D]) / `scales` (fp32 [B, Hk, S_max])
    (uamd_kv_store_fp8; the format is defined in include/unsloth_amd.h)."""
    _lib.require_gpu(x)
    B, Hk, S_max, D = _fp8_cache(codes, scales)
    assert x.dim() == 4 and tuple(x.shape[:2]) == (B, Hk) and x.shape[3] == D and x.stride(3) == 1 and x.shape[2] <= S_max
    assert codes.device == x.device
    _lib.call("uamd_kv_store_fp8", x, _lib.ptr(x), x.stride(0), x.stride(1), x.stride(2), _lib.ptr(codes), _lib.ptr(scales),
              codes.stride(0), codes.stride(1), B, Hk, x.shape[2], D, S_max, _lib.dtype_code(x.dtype), _lib.stream_of(x))


def rope_kv_append_fp8(qkv, cos, sin, kv_len, k_codes, v_codes, k_scales, v_scales, Hq, Hk, D, rope_pos=None):
    """`rope_kv_append` with an FP8 cache: in place on qkv [B, (Hq + 2 Hk) D]; the rotated k and the raw v are stored at
    kv_len[b] as codes + scale."""
    B = qkv.shape[0]
    assert _fp8_cache(k_codes, k_scales) == _fp8_cache(v_codes, v_scales) == (B, Hk, k_codes.shape[2], D)
    assert k_codes.stride() == v_codes.stride()
    assert qkv.stride(1) == 1 and kv_len.dtype == torch.int32
    assert cos.stride(1) == 1 and sin.stride() == cos.stride() and cos.dtype == qkv.dtype
    _lib.call("uamd_rope_kv_append_fp8", qkv, _lib.ptr(qkv), qkv.stride(0), _lib.ptr(cos), _lib.ptr(sin), cos.stride(0),
              _lib.ptr(kv_len), _lib.ptr(rope_pos) if rope_pos is not None else None, _lib.ptr(k_codes), _lib.ptr(v_codes),
              _lib.ptr(k_scales), _lib.ptr(v_scales), k_codes.stride(0), k_codes.stride(1), B, Hq, Hk, D, k_codes.shape[2],
              _lib.dtype_code(qkv.dtype), _lib.stream_of(qkv))


def attn_decode_fp8(q, k_codes, v_codes, k_scales, v_scales, kv_len, out, partials, split_keys, scale, len_add=1, window=0):
    """`attn_decode` over an FP8 cache: q [B, Hq*D] and out [B, Hq*D] 16-bit, partials fp32 [B, Hq, nsplit, D + 2]."""
    B, Hk, S_max, D = _fp8_cache(k_codes, k_scales)
    assert _fp8_cache(v_codes, v_scales) == (B, Hk, S_max, D) and k_codes.stride() == v_codes.stride()
    Hq = partials.shape[1]
    nsplit = partials.shape[2]
    assert nsplit * split_keys >= S_max and q.stride(1) == 1 and out.stride(1) == 1 and kv_len.dtype == torch.int32
    _lib.call("uamd_attn_decode_fp8", q, _lib.ptr(q), q.stride(0), _lib.ptr(k_codes), _lib.ptr(v_codes), _lib.ptr(k_scales),
              _lib.ptr(v_scales), k_codes.stride(0), k_codes.stride(1), _lib.ptr(kv_len), int(len_add), _lib.ptr(partials),
              _lib.ptr(out), out.stride(0), B, Hq, Hk, D, nsplit, int(split_keys), int(window), float(scale),
              _lib.dtype_code(q.dtype), _lib.stream_of(q))
    return out


def fused_attn_workspace(B, Hq, Hk, S_max, D, split_keys, device, step_dev=None):
    """(HandOff holding the partials as granules, counters) of uamd_attn_decode_fused for a cache of S_max positions, zeroed
    here, once."""
    nsplit = (S_max + split_keys - 1) // split_keys
    ho = HandOff(device, nbytes=B * Hq * nsplit * (D + 2) * 8, step_dev=step_dev)
    ho.nsplit = nsplit
    return ho, torch.zeros(B * Hk, dtype=torch.int32, device=device)


def attn_decode_fused(qkv, cos, sin, kv_len, k_cache, v_cache, out, partials, counters, split_keys, scale, Hq, window=0,
                      rope_pos=None, site=None):
    """RoPE on the new token's q / k, append of k / v at kv_len[b], split-KV attention over kv_len[b] + 1 keys and the
    combine, ONE launch (uamd_attn_decode_fused). qkv [B, (Hq + 2 Hk) D] is the raw q|k|v row and is left untouched; out
    [B, Hq * D]; (partials, counters) from `fused_attn_workspace`, owned by ONE stream of launches; `site`: the launch-site
    constant when the launch is captured in a hipGraph (HandOff)."""
    B, Hk, S_max, D = k_cache.shape
    nsplit = partials.nsplit
    assert nsplit * split_keys >= S_max and qkv.stride(1) == 1 and out.stride(1) == 1
    assert partials.ws.numel() * 4 >= B * Hq * nsplit * (D + 2) * 8
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and kv_len.dtype == torch.int32
    assert counters.dtype == torch.int32 and counters.numel() >= B * Hk
    assert cos.stride(1) == 1 and sin.stride() == cos.stride() and cos.dtype == qkv.dtype
    tag, tag_dev = partials.tags(site)
    _lib.call("uamd_attn_decode_fused", qkv, _lib.ptr(qkv), qkv.stride(0), _lib.ptr(cos), _lib.ptr(sin), cos.stride(0),
              _lib.ptr(kv_len), _lib.ptr(rope_pos) if rope_pos is not None else None, _lib.ptr(k_cache), _lib.ptr(v_cache),
              k_cache.stride(0), k_cache.stride(1), partials.ws.data_ptr(), _lib.ptr(counters), _lib.ptr(out), out.stride(0),
              B, Hq, Hk, D, S_max, nsplit, int(split_keys), int(window), float(scale), tag,
              tag_dev.data_ptr() if tag_dev is not None else None, _lib.dtype_code(qkv.dtype), _lib.stream_of(qkv))
    return out


def argmax_f32(logits, out=None, ws=None):
    """Greedy next token: argmax over the last dimension of contiguous fp32 logits [rows, n] -> int64 [rows] (uamd_argmax_f32).
    `ws` = (float32 [rows * 64], int64 [rows * 64]) workspaces to reuse under a hipGraph."""
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    rows, n = logits.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.long, device=logits.device)
    if ws is None:
        ws = (torch.empty(rows * 64, dtype=torch.float32, device=logits.device),
              torch.empty(rows * 64, dtype=torch.long, device=logits.device))
    _lib.call("uamd_argmax_f32", logits, _lib.ptr(logits), rows, n, _lib.ptr(ws[0]), _lib.ptr(ws[1]), _lib.ptr(out),
              _lib.stream_of(logits))
    return out


SAMPLE_MAX_V = 1 << 18                # uamd_sample_f32: 2^18 fixed-point masses cannot overflow 64 bits


def sample_params(device=None, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=None, out=None):
    """The device parameter block of `sample_f32` (uamd_sample_params: fp32 temperature, int32 top_k, fp32 top_p, fp32 min_p,
    uint64 seed) as an int32 [6] tensor; `out` updates an existing block in place, so a launch captured in a hipGraph follows
    the new settings. `seed`: a python int (any 64 bits), an int64 tensor of one element on any device (copied without a
    sync when it is on the block's device), or None = leave the seed as it is (0 in a new block)."""
    import numpy as np
    if not float(temperature) > 0.0:
        raise ValueError(f"temperature must be positive (got {temperature})")
    if out is None:
        out = torch.zeros(6, dtype=torch.int32, device=device)
    host = np.zeros(1, dtype=np.dtype([("t", "<f4"), ("k", "<i4"), ("p", "<f4"), ("m", "<f4")]))
    host[0] = (float(temperature), int(top_k or 0), float(1.0 if top_p is None else top_p), float(min_p or 0.0))
    out[:4].copy_(torch.from_numpy(host.view(np.int32)))
    if seed is not None:
        if not torch.is_tensor(seed):
            s = int(seed) & ((1 << 64) - 1)
            seed = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64)
        out.view(torch.int64)[2:3].copy_(seed.view(1))
    return out


def sample_f32(logits, params, ctr, out=None, ws=None, kept_out=None, thresh_out=None, u_out=None, u_in=None):
    """Sampled next token (uamd_sample_f32): temperature -> top-k -> top-p -> min-p -> one draw per row, one launch.
    logits fp32 [rows, V] with unit stride along V (row stride 0, an expanded row, is fine); `params` from `sample_params`;
    `ctr` int64 [1] on the device, the draw counter (read only -- the caller advances it). Returns int64 [rows] (`out` is
    reused when given). Optional outputs: kept_out int32 [rows] (size of the kept set), thresh_out fp32 [rows] (its smallest
    scaled logit), u_out fp32 [rows] (the uniform number used); u_in fp32 [rows] replaces the generator. `ws` is accepted for
    the calling convention of `argmax_f32` and unused: the launch needs no device workspace."""
    _lib.require_gpu(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and (logits.shape[1] == 1 or logits.stride(1) == 1)
    rows, V = logits.shape
    ld = logits.stride(0) if rows > 1 else V
    assert ld == 0 or ld >= V
    dev = logits.device
    assert params.dtype == torch.int32 and params.numel() >= 6 and params.device == dev and params.is_contiguous()
    assert u_in is not None or (ctr is not None and ctr.dtype == torch.int64 and ctr.device == dev)
    if out is None:
        out = torch.empty(rows, dtype=torch.long, device=dev)
    for t, dt in ((out, torch.long), (kept_out, torch.int32), (thresh_out, torch.float32), (u_out, torch.float32),
                  (u_in, torch.float32)):
        assert t is None or (t.dtype == dt and t.numel() >= rows and t.is_contiguous() and t.device == dev)
    _lib.call("uamd_sample_f32", logits, _lib.ptr(logits), ld, rows, V, _lib.ptr(params), _lib.ptr(ctr), _lib.ptr(u_in),
              _lib.ptr(out), _lib.ptr(kept_out), _lib.ptr(thresh_out), _lib.ptr(u_out), _lib.stream_of(logits))
    return out
