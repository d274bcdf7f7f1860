"""-m gpu: uamd_token_logprob_f32 (csrc/token_logprob.hip) against fp64 log_softmax / entropy on the CPU, and the decode engine that
calls it behind every choice of a token.

Tolerance: torch's own fp32 log_softmax / entropy on the same scaled logits has an error e against fp64 (worst row of the case);
the kernel must be within 4 e + 1e-6 (its sums run in another order). Both errors are printed. Measured on an MI355X over the
cases below: worst kernel error 1.51e-6 (log-prob; torch fp32 5.3e-6 there) and 5.2e-7 (entropy; torch fp32 up to 2.4e-5), never
above 0.25 of the bound."""
import pytest
import torch

from tests import _decode_batched as H

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _scaled(x, T):
    """z = x * (1 / T) in fp32, the kernel's own expression (T None: the NULL block, temperature 1)."""
    return x if T is None else x * (torch.ones((), dtype=torch.float32) / torch.tensor(T, dtype=torch.float32))


def _lp_ent(z, tok):
    """(log-prob at tok, entropy) per row in z's precision; a -inf logit weighs 0."""
    ls = torch.log_softmax(z, dim=-1)
    return ls.gather(1, tok[:, None])[:, 0], -(ls.exp() * torch.where(ls > -float("inf"), ls, torch.zeros_like(ls))).sum(-1)


def _check(got, z, tok, what):
    """got = (lp, ent) of the kernel for fp32 scaled logits z (CPU): within 4 x torch's fp32 error + 1e-6 of fp64."""
    for name, g, r32, r64 in zip(("log-prob", "entropy"), got, _lp_ent(z, tok), _lp_ent(z.double(), tok)):
        assert torch.isfinite(r32).all(), f"{what}: torch's fp32 {name} is not finite on this input"
        e_torch, e_kernel = float((r32.double() - r64).abs().max()), float((g.double().cpu() - r64).abs().max())
        print(f"{what} {name}: kernel error {e_kernel:.3e}, torch fp32 error {e_torch:.3e}")
        assert torch.isfinite(g).all() and e_kernel <= 4 * e_torch + 1e-6, (what, name, e_kernel, e_torch)


def _rows(kind, V, rows):
    """(logits [rows, V] fp32, tok [rows]) of one kind of row."""
    from unsloth_amd.kernels.decode import token_logprob_split
    x = 4.0 * torch.randn(rows, V, generator=H.g(V + rows))
    r = torch.arange(rows)
    span = token_logprob_split(V)[1]
    if kind == "first":
        tok = 0 * r
    elif kind == "last":
        tok = 0 * r + V - 1
    elif kind == "boundary":                       # the first logit of the second slice, then the last ones of the first
        tok = min(span, V - 1) - r
    elif kind == "half_inf":                       # row 0: whole slices of -inf; the others: every second logit
        x[0, V // 2:] = -float("inf")
        x[1:, ::2] = -float("inf")
        tok = 1 + 2 * r
    elif kind == "one_hot":
        x, tok = torch.zeros(rows, V), 7 + 300 * r
        x[r, tok] = 30.0
    else:                                          # "equal": lp = -ln V, H = ln V
        x, tok = torch.full((rows, V), 1.5), 3 + r
    return x, tok


def _launch(x, tok, T, slot=0, cap=3):
    """The kernel on x laid out with a row stride of V + 13 floats from an address 4 bytes off a 16-byte boundary."""
    from unsloth_amd.kernels import decode as D
    rows, V = x.shape
    buf = torch.zeros(rows * (V + 13) + 1, device=DEV)
    view = buf[1:].view(rows, V + 13)[:, :V]
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and (rows == 1 or view.stride(0) == V + 13)
    lp, ent = torch.full((rows, cap), -7.0, device=DEV), torch.full((rows, cap), -7.0, device=DEV)
    prm = None if T is None else D.sample_params(DEV, temperature=T, top_k=5, top_p=0.5)     # (the filters must not matter)
    D.token_logprob_f32(view, tok.to(DEV), prm, torch.tensor([slot], dtype=torch.int32, device=DEV), lp, ent)
    return lp, ent


@pytest.mark.parametrize("kind", ["first", "last", "boundary", "half_inf", "one_hot", "equal"])
@pytest.mark.parametrize("T", [None, 1.0, 0.7])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("V", [1000, 1001, 70000])         # one slice, an odd tail, 64 slices
def test_kernel_against_fp64(V, rows, T, kind):
    x, tok = _rows(kind, V, rows)
    lp, ent = _launch(x, tok, T, slot=1)
    _check((lp[:, 1], ent[:, 1]), _scaled(x, T), tok, f"V={V} rows={rows} T={T} {kind}")
    assert bool((lp[:, ::2] == -7.0).all() & (ent[:, ::2] == -7.0).all()), "a column other than *slot was written"
    if kind == "equal":
        assert torch.allclose(lp[:, 1].cpu(), -torch.log(torch.tensor(float(V))).expand(rows), atol=1e-6, rtol=0)


def test_slot_and_block_are_read_on_the_device():
    """slot.add_(1) between two calls fills adjacent columns; ONE captured launch follows the temperature in the block and the
    slot over several replays, bit-equal to eager launches; a token outside [0, V) gives NaN, not a wild read."""
    from unsloth_amd.kernels import decode as D
    x, tok = 4.0 * torch.randn(2, 3000, generator=H.g(5)), torch.tensor([17, 2999])
    xd, tokd = x.to(DEV), tok.to(DEV)
    prm, slot, ws = D.sample_params(DEV, temperature=1.0), torch.zeros(1, dtype=torch.int32, device=DEV), torch.empty(2 * 192, device=DEV)
    lp, ent = torch.full((2, 6), -7.0, device=DEV), torch.full((2, 6), -7.0, device=DEV)
    for _ in range(2):
        D.token_logprob_f32(xd, tokd, prm, slot, lp, ent, ws)
        slot.add_(1)
    assert torch.equal(lp[:, 0], lp[:, 1]) and torch.equal(ent[:, 0], ent[:, 1]) and bool((lp[:, 2:] == -7.0).all())
    _check((lp[:, 1], ent[:, 1]), x, tok, "slot 1")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        D.token_logprob_f32(xd, tokd, prm, slot, lp, ent, ws)
    for col, T in ((2, 0.5), (3, 1.0), (4, 0.5), (5, 1.3)):
        D.sample_params(temperature=T, out=prm)
        slot.fill_(col)
        graph.replay()
        eager = torch.empty(2, 1, device=DEV), torch.empty(2, 1, device=DEV)
        D.token_logprob_f32(xd, tokd, prm, torch.zeros(1, dtype=torch.int32, device=DEV), *eager)
        assert torch.equal(lp[:, col], eager[0][:, 0]) and torch.equal(ent[:, col], eager[1][:, 0]), (col, T)
        _check((lp[:, col], ent[:, col]), _scaled(x, T), tok, f"replay T={T}")
    assert not torch.equal(lp[:, 2], lp[:, 3]) and torch.equal(lp[:, 2], lp[:, 4])
    bad = _launch(x, torch.tensor([-1, 3000]), 1.0)
    assert bool(torch.isnan(bad[0][:, 0]).all() & torch.isfinite(bad[1][:, 0]).all())


GREEDY, SAMPLED = dict(), dict(do_sample=True, temperature=0.7, top_k=40, top_p=0.9)
ENGINES = {"one": (dict(batch=1), 1, [11]),                          # the fused single-sequence step
           "padded": (dict(batch=3), 1, [5, 12, 9]),                 # left-padded rows on the batched step
           "shared": (dict(batch=2, share_prompt=2, max_new_tokens=8), 2, [10])}      # two samples on one prompt cache


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("name", list(ENGINES))
def test_engine_scores_the_tokens_it_chooses(name, sampled):
    """6 new tokens: the sequences are those of the call without the keywords; graph and eager engines agree bit for bit; the
    log-probs / entropies are those of each step's logits in eager, teacher-forced stepping; a row that ends early holds 0.0
    behind its end-of-sequence token. ("shared" needs sampling for its two rows: its greedy variant samples with top_k = 1.)"""
    from unsloth_amd.models.decode import DecodeEngine
    model = H.tiny()
    ekw, n, lens = ENGINES[name]
    ids, mask, _ = H.left_padded(lens, max(lens), seed=70)
    T = max(lens)
    kw = dict(SAMPLED if sampled else (dict(do_sample=True, top_k=1) if n > 1 else GREEDY), max_new_tokens=6, attention_mask=mask,
              num_return_sequences=n)
    gen = lambda e, **more: e.generate(ids, generator=torch.Generator(DEV).manual_seed(3) if kw.get("do_sample") else None, **kw, **more)
    eng, eng_e = DecodeEngine(model, max_seq_len=128, **ekw), DecodeEngine(model, max_seq_len=128, use_graph=False, **ekw)
    plain = gen(eng)
    seq, lp, ent = gen(eng, output_logprobs=True, output_entropies=True)
    assert torch.equal(seq, plain) and lp.shape == ent.shape == (eng.B, 6) and eng.use_graph
    seq_e, lp_e, ent_e = gen(eng_e, output_logprobs=True, output_entropies=True)
    assert torch.equal(seq_e, seq) and torch.equal(lp_e, lp) and torch.equal(ent_e, ent), "graph and eager disagree"
    assert torch.equal(gen(eng), plain) and eng._lp_slot is None, "a call without the keywords still tracks"
    from unsloth_amd.models.decode import unsloth_fast_generate                 # what model.generate is after for_inference
    pub = unsloth_fast_generate(model, ids, generator=torch.Generator(DEV).manual_seed(3) if kw.get("do_sample") else None,
                                share_prompt_cache=n > 1, output_logprobs=True, output_entropies=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(pub, (seq, lp, ent))) and len(pub) == 3
    temp = kw.get("temperature") if sampled else None
    logits = eng_e.prefill(ids, mask, repeat=n).clone()
    for i in range(6):
        tok = seq[:, T + i]
        _check((lp[:, i], ent[:, i]), _scaled(logits.cpu(), temp), tok.cpu(), f"{name} sampled={sampled} token {i}")
        logits = eng_e.step(tok).clone()
    # the third new token of row 0 as the end-of-sequence id: row 0 ends where that id first appears
    eos = int(seq[0, T + 2])
    end = [int((seq[b, T:] == eos).nonzero()[0]) if bool((seq[b, T:] == eos).any()) else 5 for b in range(eng.B)]
    seq2, lp2, ent2 = gen(eng, output_logprobs=True, output_entropies=True, eos_token_id=eos)
    for b in range(eng.B):
        live = min(end[b] + 1, lp2.shape[1])
        assert torch.equal(lp2[b, :live], lp[b, :live]) and torch.equal(ent2[b, :live], ent[b, :live])
        assert bool((lp2[b, live:] == 0).all() & (ent2[b, live:] == 0).all()), "scores behind a row's end"


def test_prompt_lookup_with_logprobs_is_refused_before_any_launch():
    from unsloth_amd.models.decode import DecodeEngine
    eng = DecodeEngine(H.tiny(), max_seq_len=128)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        eng.generate(torch.randint(1, 1000, (1, 9), generator=H.g(1)), max_new_tokens=6, prompt_lookup_num_tokens=3, output_logprobs=True)
    assert eng.logits is None and eng._lp_slot is None and eng._fed == 0
