"""-m gpu: shared-prompt decoding -- uamd_attn_decode_shared (csrc/decode.hip: attn_decode_prefix_kernel over the prompt cache that
the n samples of a prompt share, attn_decode_kernel over every row's own suffix, one combine) and DecodeEngine(share_prompt=n).

The kernel is judged row by row against an fp64 reference over the keys [first, total) of prompt | suffix (tests/_decode_shared.py)
with the softmax mass placed on the ends of that range and on the seam between the two caches; the bound is 4 x the error of a host
model that makes the roundings the kernel documents. tests/test_decode_shared_host.py shows on the host that every wrong range
moves the rows that watch it by more than twice that bound. The measured ratios go to decode_shared_edge_report.json in the
directory UAMD_REPORT_DIR names (default: test_reports/ in the repository root, git-ignored); profiles/decode_shared_edge_report.json
is a committed copy of one MI355X run. The engine runs the tiny model of tests/_decode_batched.py against the replicated engine
(bits, where the code is the same) and against the training-path forward (logits)."""
import json
import os

import pytest
import torch

from tests import _decode_shared as H
from tests._decode_batched import DEV, Recorder, full_logits, g, left_padded, tiny

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}

CASE_DTYPE = [(n, d) for n in H.CASES for d in H.DTYPES]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_shared_edge_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _shared(c, pk, pv, sk, sv, q=None, n=None, lens=None, news=None):
    """uamd_attn_decode_shared with len_add = 1 on suffix caches that already hold the new token: out [B, Hq * D] on the host."""
    from unsloth_amd.kernels import decode as Dk
    B, Hq, D, sp = c["B"], c["Hq"], c["D"], c["split_keys"]
    q = (c["q"] if q is None else q).to(DEV)
    prompt_len = torch.tensor(c["lens"] if lens is None else lens, dtype=torch.int32, device=DEV)
    new_len = torch.tensor([m - 1 for m in (c["news"] if news is None else news)], dtype=torch.int32, device=DEV)
    part = torch.full((B, Hq, H.S_P // sp + H.S_N // sp, D + 2), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((B, Hq * D), float("nan"), dtype=c["dtype"], device=DEV)
    Dk.attn_decode_shared(q, pk.to(DEV), pv.to(DEV), prompt_len, c["n"] if n is None else n, sk.to(DEV), sv.to(DEV), new_len, out,
                          part, sp, c["scale"], len_add=1, window=c["window"])
    return out.cpu()


def _hold(c, key, got):
    assert torch.isfinite(got.float()).all(), (key, "not finite")
    err, model, ok = H.judge(c, got)
    ratio = err / model if model > 0 else (0.0 if err == 0 else float("inf"))       # (one key: the model is exact)
    REPORT[key] = dict(kernel=err, model=model, ratio=ratio)
    print(f"{key}: err {err:.3e} model_err {model:.3e} ratio {ratio:.2f}")
    assert ok, (key, err, model, ratio)


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_shared_edges_match_fp64(name, dtype_name):
    c = H.build_case(name, dtype_name)
    got = _shared(c, c["pk"], c["pv"], c["sk"], c["sv"])
    _hold(c, f"{name}/{dtype_name}/shared", got)


def _forbidden(c):
    """(per prompt and KV head, per row and KV head): keys that the heads of the group score far above their edge keys -- the sum
    of the queries that read the slot (q . q is 2.75 D for a role head, q . code is D): all n G of a prompt slot, the row's G of a
    suffix slot -- and a value no reference row uses."""
    P, n, B, Hq, Hk, D = c["P"], c["n"], c["B"], c["Hq"], c["Hk"], c["D"]
    per_row = c["q"].float().view(B, Hk, Hq // Hk, D).sum(2)
    k_row = per_row.to(c["dtype"])
    k_prompt = per_row.view(P, n, Hk, D).sum(1).to(c["dtype"])
    gen = torch.Generator().manual_seed(77)
    v_prompt = (3.0 + torch.randn(P, Hk, D, generator=gen)).to(c["dtype"])
    v_row = (3.0 + torch.randn(B, Hk, D, generator=gen)).to(c["dtype"])
    return k_prompt, v_prompt, k_row, v_row


def _has_stale_slots(case):
    _, _, _, rows_L, news, ranges = H.geometry(case)
    return any(L < H.S_P for L in rows_L) or any(m < H.S_N for m in news) or any(f > 0 for f, _ in ranges)


# (the two cases that fill both caches to their last slots have no slot outside the range)
STALE_CASE_DTYPE = [(n, d) for n, c in H.CASES.items() if _has_stale_slots(c) for d in H.DTYPES]
assert len(STALE_CASE_DTYPE) == len(CASE_DTYPE) - 4


@pytest.mark.parametrize("name,dtype_name", STALE_CASE_DTYPE)
def test_stale_slots_are_never_read(name, dtype_name):
    """Prompt slots >= L_p and below the oldest key any row of the group attends, suffix slots >= new and below the suffix's first
    key, filled with keys that would take the mass: the output is the clean run's, bit for bit, and within the bound."""
    c = H.build_case(name, dtype_name)
    clean = _shared(c, c["pk"], c["pv"], c["sk"], c["sv"])
    k_prompt, v_prompt, k_row, v_row = _forbidden(c)
    pk, pv, sk, sv = (c[t].clone() for t in ("pk", "pv", "sk", "sv"))
    n = c["n"]
    for p, L in enumerate(c["lens"]):
        first = min(f for f, _ in c["ranges"][p * n:(p + 1) * n])
        pk[p, :, L:], pv[p, :, L:] = k_prompt[p][:, None], v_prompt[p][:, None]
        pk[p, :, :min(first, L)], pv[p, :, :min(first, L)] = k_prompt[p][:, None], v_prompt[p][:, None]
    for r, (first, total) in enumerate(c["ranges"]):
        new, lo = c["news"][r], max(0, first - c["rows_L"][r])
        sk[r, :, new:], sv[r, :, new:] = k_row[r][:, None], v_row[r][:, None]
        sk[r, :, :lo], sv[r, :, :lo] = k_row[r][:, None], v_row[r][:, None]
    assert not (torch.equal(pk, c["pk"]) and torch.equal(sk, c["sk"]))
    got = _shared(c, pk, pv, sk, sv)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, clean)
    assert H.judge(c, got)[2], H.judge(c, got)


@pytest.mark.parametrize("dtype_name", list(H.DTYPES))
@pytest.mark.parametrize("name", ["d128_r21_split_seam", "d128_suffix129", "d64_g7_r21", "d128_rows_differ"])
def test_a_row_does_not_depend_on_the_others(name, dtype_name):
    """Row r with every other row's query and suffix replaced, and every other prompt's caches: bit-equal. A NaN query in one row:
    every other row finite and bit-equal."""
    c = H.build_case(name, dtype_name)
    base = _shared(c, c["pk"], c["pv"], c["sk"], c["sv"])
    B, n = c["B"], c["n"]
    gen = torch.Generator().manual_seed(5)
    for r in (0, B // 2, B - 1):
        q, pk, pv, sk, sv = (c[t].clone() for t in ("q", "pk", "pv", "sk", "sv"))
        others = [x for x in range(B) if x != r]
        q[others] = torch.randn(len(others), q.shape[1], generator=gen).to(c["dtype"])
        sk[others] = (torch.randint(0, 2, sk[others].shape, generator=gen) * 2 - 1).to(c["dtype"])
        sv[others] = torch.randn(sv[others].shape, generator=gen).to(c["dtype"])
        for p in range(c["P"]):
            if p != r // n:
                pk[p] = (torch.randint(0, 2, pk[p].shape, generator=gen) * 2 - 1).to(c["dtype"])
                pv[p] = torch.randn(pv[p].shape, generator=gen).to(c["dtype"])
        got = _shared(c, pk, pv, sk, sv, q=q)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got[r], base[r]), r
        assert not torch.equal(got[others[0]], base[others[0]])
        q = c["q"].clone()
        q[r] = float("nan")
        got = _shared(c, c["pk"], c["pv"], c["sk"], c["sv"], q=q)
        assert torch.isfinite(got[others].float()).all() and torch.equal(got[others], base[others]), r


@pytest.mark.parametrize("name,dtype_name", CASE_DTYPE)
def test_the_replicated_kernel_agrees_within_the_bound(name, dtype_name):
    """The same keys, every row's prompt | suffix in a cache of its own, through uamd_attn_decode: both outputs within the bound of
    the fp64 reference (no equality: the summation orders differ)."""
    from unsloth_amd.kernels import decode as Dk
    c = H.build_case(name, dtype_name)
    B, Hq, Hk, D, sp = c["B"], c["Hq"], c["Hk"], c["D"], c["split_keys"]
    S = H.S_P + H.S_N
    kc = torch.zeros(B, Hk, S, D, dtype=c["dtype"])
    vc = torch.zeros_like(kc)
    for r in range(B):
        L, p = c["rows_L"][r], c["rows_p"][r]
        kc[r, :, :L], vc[r, :, :L] = c["pk"][p, :, :L], c["pv"][p, :, :L]
        kc[r, :, L:L + H.S_N], vc[r, :, L:L + H.S_N] = c["sk"][r], c["sv"][r]
    kv_len = torch.tensor([t - 1 for _, t in c["ranges"]], dtype=torch.int32, device=DEV)
    part = torch.empty(B, Hq, S // sp, D + 2, dtype=torch.float32, device=DEV)
    out = torch.full((B, Hq * D), float("nan"), dtype=c["dtype"], device=DEV)
    Dk.attn_decode(c["q"].to(DEV), kc.to(DEV), vc.to(DEV), kv_len, out, part, sp, c["scale"], len_add=1, window=c["window"])
    _hold(c, f"{name}/{dtype_name}/replicated", out.cpu())
    assert H.judge(c, _shared(c, c["pk"], c["pv"], c["sk"], c["sv"]))[2]


def test_more_than_16_samples_are_refused_before_any_launch():
    from unsloth_amd.kernels import decode as Dk
    c = H.build_case("d128_r2_new1", "bf16")
    Hk, D = c["Hk"], c["D"]
    for n in (1, 17):
        B = n
        sk = torch.zeros(B, Hk, H.S_N, D, dtype=c["dtype"], device=DEV)
        part = torch.full((B, c["Hq"], H.S_P // 128 + H.S_N // 128, D + 2), 7.0, dtype=torch.float32, device=DEV)
        out = torch.full((B, c["Hq"] * D), 7.0, dtype=c["dtype"], device=DEV)
        q = torch.zeros(B, c["Hq"] * D, dtype=c["dtype"], device=DEV)
        with pytest.raises(RuntimeError, match="uamd_attn_decode_shared"):
            Dk.attn_decode_shared(q, c["pk"][:1].to(DEV), c["pv"][:1].to(DEV), torch.ones(1, dtype=torch.int32, device=DEV), n, sk, sk,
                                  torch.zeros(B, dtype=torch.int32, device=DEV), out, part, 128, c["scale"])
        torch.cuda.synchronize()
        assert bool((part == 7.0).all()) and bool((out == 7.0).all())          # nothing ran


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def _prompts(P, padded, seed):
    """(ids [P, 9] on the device, mask or None, the unpadded prompts)."""
    if padded:
        ids, mask, rows = left_padded((4, 9)[:P], 9, seed=seed)
        return ids.to(DEV), mask.to(DEV), [r.to(DEV) for r in rows]
    ids = torch.randint(1, 1000, (P, 9), generator=g(seed)).to(DEV)
    return ids, None, [ids[p] for p in range(P)]


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("P,n", [(2, 3), (1, 16)])
def test_engine_against_the_replicated_engine_and_the_training_path(P, n, padded, monkeypatch):
    from unsloth_amd import _lib
    from unsloth_amd.models.decode import DecodeEngine
    monkeypatch.setenv("UNSLOTH_RETURN_LOGITS", "1")
    model = tiny(True)
    B = P * n
    ids, mask, rows = _prompts(P, padded, seed=31)
    lens = [len(r) for r in rows]

    def allocated(make):
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        e = make()
        torch.cuda.synchronize()
        return e, torch.cuda.memory_allocated() - m0
    rep, rep_bytes = allocated(lambda: DecodeEngine(model, max_seq_len=256, batch=B))
    sh, sh_bytes = allocated(lambda: DecodeEngine(model, max_seq_len=256, batch=B, share_prompt=n, max_new_tokens=128))
    sh_e = DecodeEngine(model, max_seq_len=256, batch=B, share_prompt=n, max_new_tokens=128, use_graph=False)
    print(f"P = {P}, n = {n}: engine allocations {sh_bytes} bytes shared, {rep_bytes} replicated")
    assert sh_bytes < rep_bytes
    assert sh.use_graph and sh.rows and sh.share_prompt == n and (sh.S, sh.S_n) == (256, 128)
    Hk, D = sh.Hk, sh.D
    assert all(t.shape == (P, Hk, 256, D) for t in sh.pk + sh.pv)                    # one prompt cache per prompt ...
    assert all(t.shape == (B, Hk, 128, D) for t in sh.k_cache + sh.v_cache)          # ... and only suffixes per row
    lg_r = rep.prefill(ids, mask, repeat=n).clone()
    lg = sh.prefill(ids, mask, repeat=n).clone()
    lg_e = sh_e.prefill(ids, mask, repeat=n).clone()
    assert torch.equal(lg, lg_r) and torch.equal(lg_e, lg_r)                         # the prefill code is the same
    assert sh.prompt_len.tolist() == lens and sh.kv_len.tolist() == [lens[r // n] for r in range(B)]
    assert sh.new_len.tolist() == [0] * B
    for p, L in enumerate(lens):
        assert torch.equal(sh.pk[0][p, :, :L], rep.k_cache[0][p * n, :, :L])
        assert torch.equal(sh.pv[0][p, :, :L], rep.v_cache[0][p * n, :, :L])
        assert float(sh.pk[0][p, :, L:].float().abs().sum()) == 0.0
    assert all(float(t.float().abs().sum()) == 0.0 for t in sh.k_cache + sh.v_cache)  # no replica copies anywhere
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    seqs = [rows[r // n].view(1, -1) for r in range(B)]
    shift = torch.arange(B, device=DEV)
    for step in range(7):                                            # prefill + six steps
        for p in range(P):                                           # (the rows of a prompt are equally long: one forward)
            full = full_logits(model, torch.cat(seqs[p * n:(p + 1) * n], dim=0))
            for i in range(n):
                scale = full[i].abs().max().item()
                err = (lg[p * n + i] - full[i]).abs().max().item()
                assert err < 4e-2 * scale, (step, p, i, err, scale)
        if step == 6:
            break
        nxt = (torch.argmax(lg, dim=-1) + shift) % 1000              # every row its own token: the rows of a group differ
        seqs = [torch.cat([s, nxt[r].view(1, 1)], dim=1) for r, s in enumerate(seqs)]
        names.clear()
        lg_e = sh_e.step(nxt).clone()
        assert "uamd_attn_decode_shared" in names and "uamd_attn_decode" not in names, names
        lg = sh.step(nxt).clone()
        assert torch.equal(lg, lg_e), f"graph replay differs from the eager step at step {step}"
        if step == 0:                                                # layer 0's K / V do not depend on attention
            rep.step(nxt)
            for r in range(B):
                L = lens[r // n]
                assert torch.equal(sh.k_cache[0][r, :, 0], rep.k_cache[0][r, :, L])
                assert torch.equal(sh.v_cache[0][r, :, 0], rep.v_cache[0][r, :, L])
    assert sh._graph is not None
    for e in (sh, sh_e):
        assert e.kv_len.tolist() == [lens[r // n] + 6 for r in range(B)] and e.new_len.tolist() == [6] * B
        assert e.prompt_len.tolist() == lens
    # the sampled step is a capture of its own and agrees with the eager one too
    outs = [e.generate(ids, attention_mask=mask, max_new_tokens=5, do_sample=True, temperature=1.3, top_k=50,
                       num_return_sequences=n, generator=torch.Generator(DEV).manual_seed(5)) for e in (sh, sh_e)]
    assert sh._graph_s is not None and torch.equal(outs[0], outs[1])


def test_generate_with_share_prompt_cache():
    from unsloth_amd import FastLanguageModel
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True, fresh=True)
    FastLanguageModel.for_inference(model)
    rec = Recorder(ret="hf")
    model._old_generate = rec
    ids = torch.randint(0, 1000, (2, 9), generator=g(23)).to(DEV)
    gen = lambda: torch.Generator(DEV).manual_seed(7)
    kw = dict(max_new_tokens=5, do_sample=True, temperature=2.0, top_k=0)
    out = model.generate(input_ids=ids, num_return_sequences=3, share_prompt_cache=True, generator=gen(), **kw)
    assert out.shape == (6, 14) and not rec.calls
    assert torch.equal(out[:, :9], ids.repeat_interleave(3, 0))
    eng = model._uamd_decode_engine
    assert eng.share_prompt == 3 and eng.pk[0].shape[0] == 2 and eng.S >= 9 and eng.S_n >= 5
    again = model.generate(input_ids=ids, num_return_sequences=3, share_prompt_cache=True, generator=gen(), **kw)
    assert torch.equal(out, again) and model._uamd_decode_engine is eng
    want = DecodeEngine(model, max_seq_len=128, batch=6, share_prompt=3).generate(ids, num_return_sequences=3, generator=gen(), **kw)
    assert torch.equal(out, want)
    for b in range(2):                                               # replicas draw differently
        trio = out[3 * b:3 * b + 3, 9:]
        assert not (torch.equal(trio[0], trio[1]) and torch.equal(trio[1], trio[2])), trio
    # one sequence per prompt: the keyword does nothing; without it: the replicated engine again
    one = model.generate(input_ids=ids, share_prompt_cache=True, max_new_tokens=5)
    assert one.shape == (2, 14) and model._uamd_decode_engine.share_prompt is None
    # recorded on the model by for_inference
    FastLanguageModel.for_inference(model, share_prompt_cache=True)
    marked = model.generate(input_ids=ids, num_return_sequences=3, generator=gen(), **kw)
    assert torch.equal(marked, out) and model._uamd_decode_engine.share_prompt == 3 and not rec.calls
    with pytest.raises(NotImplementedError, match="share_prompt"):
        DecodeEngine(model, max_seq_len=128, batch=6, share_prompt=3, kv_cache_dtype="fp8")


def test_a_second_generate_ignores_the_stale_slots():
    """A longer prompt and more new tokens first, then a shorter call on the same engine: the tokens of a fresh engine, although
    the prompt caches and the suffixes still hold the first call's keys behind the new lengths."""
    from unsloth_amd.models.decode import DecodeEngine
    model = tiny(True)
    gen = lambda: torch.Generator(DEV).manual_seed(9)
    kw = dict(do_sample=True, temperature=1.5, top_k=0, num_return_sequences=3)
    long_ids = torch.randint(1, 1000, (2, 40), generator=g(51)).to(DEV)
    ids, mask, _ = left_padded((4, 9), 9, seed=52)
    ids, mask = ids.to(DEV), mask.to(DEV)
    eng = DecodeEngine(model, max_seq_len=128, batch=6, share_prompt=3, max_new_tokens=32)
    eng.generate(long_ids, max_new_tokens=20, generator=gen(), **kw)
    assert float(eng.pk[0][:, :, 9:40].float().abs().sum()) > 0 and float(eng.k_cache[0][:, :, 5:19].float().abs().sum()) > 0
    got = eng.generate(ids, attention_mask=mask, max_new_tokens=6, generator=gen(), **kw)
    fresh = DecodeEngine(model, max_seq_len=128, batch=6, share_prompt=3, max_new_tokens=32)
    want = fresh.generate(ids, attention_mask=mask, max_new_tokens=6, generator=gen(), **kw)
    assert got.shape == (6, 15) and torch.equal(got, want)
    assert eng.prompt_len.tolist() == [4, 9] and eng.new_len.tolist() == [5] * 6
