"""-m gpu: the key range of the split-KV decode attention (csrc/decode.hip: attn_decode_kernel + attn_decode_combine_kernel, and the
single launch attn_decode_fused_kernel) with the softmax mass placed ON its two ends.

The other decode attention tests feed randn, where a key too many or too few at `first` or at `len` moves a row by |v| / n_keys,
or compare the single launch with the three launches, which compute `first`, the split's end and `valid` with the same
expressions. Here (tests/_decode_edges.py) the oldest allowed key, the new token or a key in the middle holds most of a row's mass
and the forbidden slot beside it -- an older key under a window, a stale key of an earlier prompt behind `len` -- would hold more.
Both paths are judged row by row against an fp64 reference over a plain slice of the cache; the bound is 4 x the error of that
reference rounded once to the 16-bit type. tests/test_decode_edge_inputs.py shows on the host that every off-by-one range moves
the rows that watch it by at least 0.5, more than 20 x the bound. The measured ratios go to decode_edge_report.json in the directory
UAMD_REPORT_DIR names (default: test_reports/ in the repository root, git-ignored); profiles/decode_edge_report.json is a committed
copy of one MI355X run."""
import json
import os

import pytest
import torch

from tests import _decode_edges as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}

CASE_DTYPE = [(n, d) for n in E.CASES for d in E.DTYPES]
# the cases of test_stale_slots_are_never_used: no window, and window 1
STALE_CASES = [n for n, c in E.CASES.items() if c[4] in (0, 1)]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_edge_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _rope_tables(D, S, dtype):
    """The real tables; row 0 is cos = 1, sin = 0 exactly."""
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(S).float()[:, None] * inv[None, :]
    return (torch.cat([ang.cos(), ang.cos()], dim=1).to(dtype).to(DEV), torch.cat([ang.sin(), ang.sin()], dim=1).to(dtype).to(DEV))


def _forbidden(c):
    """(k_bad [B, Hk, D], v_bad [B, Hk, D]): for every KV head a key that every query head of its group scores far above its
    edge key (the sum of the group's queries: q . q is 2.75 D for a role head, q . code is D), and a value no reference row uses."""
    B, Hq, Hk, D = c["B"], c["Hq"], c["Hk"], c["D"]
    k_bad = c["q"].float().view(B, Hk, Hq // Hk, D).sum(2).to(c["dtype"])
    v_bad = (3.0 + torch.randn(B, Hk, D, generator=torch.Generator().manual_seed(77))).to(c["dtype"])
    return k_bad, v_bad


def _hold(c, name, dtype_name, path, got):
    assert torch.isfinite(got.float()).all(), (path, "not finite")
    err, model, ok = E.judge(c, got)
    ratio = err / model if model > 0 else (0.0 if err == 0 else float("inf"))       # (one key: the model is exact)
    REPORT[f"{name}/{dtype_name}/{path}"] = dict(kernel=err, model=model, ratio=ratio)
    print(f"{name}/{dtype_name}/{path}: err {err:.3e} model_err {model:.3e} ratio {ratio:.2f}")
    assert ok, (path, err, model, ratio)


def _three_launches(c, kc, vc):
    """uamd_attn_decode with len_add = 1 on caches that already hold the new token: out [B, Hq * D] on the host."""
    from unsloth_amd.kernels import decode as Dk
    B, Hq, D = c["B"], c["Hq"], c["D"]
    kv_len = torch.tensor([L - 1 for L in c["lens"]], dtype=torch.int32, device=DEV)
    part = torch.empty(B, Hq, E.S_MAX // c["split_keys"], D + 2, dtype=torch.float32, device=DEV)
    out = torch.full((B, Hq * D), float("nan"), dtype=c["dtype"], device=DEV)
    Dk.attn_decode(c["q"].to(DEV), kc, vc, kv_len, out, part, c["split_keys"], c["scale"], len_add=1, window=c["window"])
    return out.cpu()


def _single_launch(c, kc, vc):
    """uamd_attn_decode_fused on the raw q|k|v row whose k and v are the case's key and value of slot len - 1 (kc / vc hold
    whatever the caller left in that slot), rope_pos = 0: the rotation is the identity. Returns (out on the host, raw row before,
    raw row after, counters)."""
    from unsloth_amd.kernels import decode as Dk
    B, Hq, Hk, D = c["B"], c["Hq"], c["Hk"], c["D"]
    rows = torch.arange(B)
    last = torch.tensor([L - 1 for L in c["lens"]])
    raw = torch.cat([c["q"], c["kc"][rows, :, last].flatten(1), c["vc"][rows, :, last].flatten(1)], dim=1).to(DEV)
    keep = raw.clone()
    cos, sin = _rope_tables(D, E.S_MAX, c["dtype"])
    assert bool((cos[0] == 1).all()) and bool((sin[0] == 0).all())
    kv_len = last.to(torch.int32).to(DEV)
    part, cnt = Dk.fused_attn_workspace(B, Hq, Hk, E.S_MAX, D, c["split_keys"], DEV)
    out = torch.full((B, Hq * D), float("nan"), dtype=c["dtype"], device=DEV)
    Dk.attn_decode_fused(raw, cos, sin, kv_len, kc, vc, out, part, cnt, c["split_keys"], c["scale"], Hq, window=c["window"],
                         rope_pos=torch.zeros(B, dtype=torch.int32, device=DEV))
    return out.cpu(), keep, raw, cnt


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_attn_decode_edges_match_fp64(name, dtype_name):
    c = E.build_case(name, dtype_name)
    got = _three_launches(c, c["kc"].to(DEV), c["vc"].to(DEV))
    _hold(c, name, dtype_name, "three_launches", got)


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_attn_decode_fused_edges_match_fp64(name, dtype_name):
    """Before the launch, slot len - 1 of the cache holds a key that scores far above every edge key and an unrelated value: a
    kernel that took the new token from the cache instead of its LDS copy would return that value."""
    c = E.build_case(name, dtype_name)
    kc, vc = c["kc"].to(DEV), c["vc"].to(DEV)
    k_bad, v_bad = _forbidden(c)
    for b, L in enumerate(c["lens"]):
        kc[b, :, L - 1] = k_bad[b].to(DEV)
        vc[b, :, L - 1] = v_bad[b].to(DEV)
    got, keep, raw, cnt = _single_launch(c, kc, vc)
    _hold(c, name, dtype_name, "single_launch", got)
    assert torch.equal(raw, keep)                                    # the raw row is left alone
    # slot len - 1 now holds the raw k and v (identity rotation: the case's own rows), and no other slot changed
    assert torch.equal(kc.cpu(), c["kc"]) and torch.equal(vc.cpu(), c["vc"])
    assert int(cnt.abs().sum()) == 0                                 # arrival counters back at zero


@pytest.mark.parametrize("path", ["three_launches", "single_launch"])
@pytest.mark.parametrize("dtype_name", list(E.DTYPES))
@pytest.mark.parametrize("name", STALE_CASES)
def test_stale_slots_are_never_used(name, dtype_name, path):
    """The slots >= len hold an earlier prompt's keys (DecodeEngine rewinds kv_len and keeps its caches). The same launch on two
    contents of those slots -- finite keys that every head scores above its edge key, then NaN in both caches -- gives the same
    finite output, bit for bit; for the single launch slot len - 1, which it overwrites, is part of those contents. The slots
    below `first` stay finite in both runs: this sequence wrote them, and a masked lane may load one with weight zero.

    len = 1 on the single launch is the case to look at: its masked lanes load row `safe` = 0, the slot the same workgroup appends
    to, and give it weight zero -- NaN if they still see the old content. On an MI355X both contents gave equal, finite outputs at
    len = 1 (both types, both head dims): the appended row is what those lanes load, and no kernel was changed."""
    c = E.build_case(name, dtype_name)
    k_bad, v_bad = _forbidden(c)
    outs = []
    for poison in (False, True):
        kc, vc = c["kc"].to(DEV), c["vc"].to(DEV)
        for b, L in enumerate(c["lens"]):
            lo = L - 1 if path == "single_launch" else L
            if poison:
                kc[b, :, lo:] = float("nan")
                vc[b, :, lo:] = float("nan")
            else:
                kc[b, :, lo:] = k_bad[b].to(DEV)[:, None]
                vc[b, :, lo:] = v_bad[b].to(DEV)[:, None]
        outs.append(_three_launches(c, kc, vc) if path == "three_launches" else _single_launch(c, kc, vc)[0])
    assert torch.isfinite(outs[0].float()).all() and torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])
    assert E.judge(c, outs[0])[2], E.judge(c, outs[0])


def _rope_rows(x, cos, sin, pos, D):
    """rope_pair of csrc/decode.hip on rows x [B, H, D] at table rows pos [B], on the host: every product and the sum / difference
    rounded to the 16-bit type T, r1 = T(T(x1 c) - T(x2 s)), r2 = T(T(x2 c) + T(x1 s)). The products of two 16-bit values are exact
    in fp32, so each step is one rounding, as on the device."""
    T = x.dtype
    half = D // 2
    x1, x2 = x[..., :half].float(), x[..., half:].float()
    c, s = cos[pos.long(), :half].float()[:, None], sin[pos.long(), :half].float()[:, None]

    def r(t):
        return t.to(T).float()
    return torch.cat([(r(x1 * c) - r(x2 * s)).to(T), (r(x2 * c) + r(x1 * s)).to(T)], dim=-1)


@pytest.mark.parametrize("dtype_name", list(E.DTYPES))
@pytest.mark.parametrize("D", [64, 128])
def test_rope_pos_overrides_the_cache_position(D, dtype_name):
    """rope_pos, the optional position array of uamd_rope_kv_append and uamd_attn_decode_fused (the HF-style batch path of
    models/decode.py: left-padded rows whose position is not their cache slot): the rotation reads table row rope_pos[b], the
    append still goes to slot kv_len[b]. Rotated q and k, the appended cache rows of both launchers: bit-equal to a host
    emulation of rope_pair that calls no kernel."""
    from unsloth_amd.kernels import decode as Dk
    dtype = E.DTYPES[dtype_name]
    B, Hq, Hk, S, split_keys = 3, 8, 2, 512, 128
    gen = torch.Generator().manual_seed(31 + D)
    qkv = torch.randn(B, (Hq + 2 * Hk) * D, generator=gen).to(dtype)
    kc0 = torch.randn(B, Hk, S, D, generator=gen).to(dtype)
    vc0 = torch.randn(B, Hk, S, D, generator=gen).to(dtype)
    lens, pos = (5, 17, 200), torch.tensor([0, 300, 3])
    cos, sin = _rope_tables(D, S, dtype)
    want_q = _rope_rows(qkv[:, :Hq * D].view(B, Hq, D), cos.cpu(), sin.cpu(), pos, D)
    want_k = _rope_rows(qkv[:, Hq * D:(Hq + Hk) * D].view(B, Hk, D), cos.cpu(), sin.cpu(), pos, D)
    want_v = qkv[:, (Hq + Hk) * D:].view(B, Hk, D)
    assert torch.equal(want_q[0], qkv[0, :Hq * D].view(Hq, D))             # position 0: the identity
    assert not torch.equal(want_k[1], _rope_rows(qkv[1:2, Hq * D:(Hq + Hk) * D].view(1, Hk, D), cos.cpu(), sin.cpu(),
                                                 torch.tensor([17]), D)[0])  # position 300 is not position kv_len = 17
    want_kc, want_vc = kc0.clone(), vc0.clone()
    for b, L in enumerate(lens):
        want_kc[b, :, L], want_vc[b, :, L] = want_k[b], want_v[b]
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rope_pos = pos.to(torch.int32).to(DEV)
    scale = D ** -0.5

    kc1, vc1, row1 = kc0.to(DEV), vc0.to(DEV), qkv.to(DEV)
    Dk.rope_kv_append(row1, cos, sin, kv_len, kc1, vc1, Hq, Hk, D, rope_pos=rope_pos)
    assert torch.equal(row1[:, :Hq * D].cpu().view(B, Hq, D), want_q)
    assert torch.equal(row1[:, Hq * D:(Hq + Hk) * D].cpu().view(B, Hk, D), want_k)
    assert torch.equal(row1[:, (Hq + Hk) * D:].cpu(), qkv[:, (Hq + Hk) * D:])
    assert torch.equal(kc1.cpu(), want_kc) and torch.equal(vc1.cpu(), want_vc)
    part1 = torch.empty(B, Hq, S // split_keys, D + 2, dtype=torch.float32, device=DEV)
    out1 = torch.full((B, Hq * D), float("nan"), dtype=dtype, device=DEV)
    Dk.attn_decode(row1[:, :Hq * D], kc1, vc1, kv_len, out1, part1, split_keys, scale, len_add=1)

    kc2, vc2, row2 = kc0.to(DEV), vc0.to(DEV), qkv.to(DEV)
    part2, cnt = Dk.fused_attn_workspace(B, Hq, Hk, S, D, split_keys, DEV)
    out2 = torch.full((B, Hq * D), float("nan"), dtype=dtype, device=DEV)
    Dk.attn_decode_fused(row2, cos, sin, kv_len, kc2, vc2, out2, part2, cnt, split_keys, scale, Hq, rope_pos=rope_pos)
    assert torch.equal(row2.cpu(), qkv)
    assert torch.equal(kc2.cpu(), want_kc) and torch.equal(vc2.cpu(), want_vc)
    assert int(cnt.abs().sum()) == 0
    # the single launch's output against the three launches on the rotated row: the bound of
    # test_attn_decode_fused_is_the_three_launches (tests/test_gpu_decode.py)
    assert torch.isfinite(out1.float()).all() and torch.isfinite(out2.float()).all()
    err = (out2.float() - out1.float()).abs().max().item()
    assert err <= (1.6e-2 if dtype == torch.bfloat16 else 2e-3) * max(out1.float().abs().max().item(), 1e-3), err
