"""-m gpu: the device sampler (csrc/sampler.hip, uamd_sample_f32) against the fp64 host reference of tests/_sampler_ref.py, and the
decode engine that draws with it inside the (captured) token step.

The kept set is exact: its size and its smallest scaled logit equal the reference's bit for bit on inputs whose boundaries sit at
least 1e-4 away from the nearest token (tests/test_sampler_ref_host.py asserts that on the host). The token is judged against
the fp64 CDF: with [a_j, b_j) the interval of the returned token, u may miss it by at most (ceil(V / 256) + 16) * 2^-24 -- the worst
case of an fp32 sum with at least 256 lanes per row plus exp at 2 ulp. The worst miss per case goes to sampler_report.json in the
directory UAMD_REPORT_DIR names (default: test_reports/ in the repository root, git-ignored); profiles/sampler_report.json is a
committed copy of one MI355X run."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}

U_ROWS = np.array([(r + 0.5) / 64 for r in range(64)] + [0.0, 1.0 - 2.0 ** -24], np.float32)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield REPORT
    try:
        out = os.environ.get("UAMD_REPORT_DIR") or os.path.join(ROOT, "test_reports")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "sampler_report.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _params(c, seed=None):
    from unsloth_amd.kernels import decode as D
    return D.sample_params(DEV, c["T"], c["top_k"], c["top_p"], c["min_p"], seed=seed)


def _ctr(v=0):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def _launch(x, prm, rows=None, u_in=None, ctr=None):
    """(tokens, kept, thresh, u) as numpy; x: numpy [V] (expanded to `rows` rows at stride 0) or a device tensor [rows, V]."""
    from unsloth_amd.kernels import decode as D
    lg = torch.from_numpy(np.array(x)).to(DEV)[None].expand(rows, -1) if isinstance(x, np.ndarray) else x
    n = lg.shape[0]
    kept = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    thresh = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    u = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    tok = D.sample_f32(lg, prm, ctr if ctr is not None else _ctr(), kept_out=kept, thresh_out=thresh, u_out=u,
                       u_in=None if u_in is None else torch.from_numpy(u_in).to(DEV))
    return tok.cpu().numpy(), kept.cpu().numpy(), thresh.cpu().numpy(), u.cpu().numpy()


def _miss(c, tok, u):
    """max over rows of the distance of u from the fp64 interval of the returned token; every token must be kept."""
    a, b = R.cdf_intervals(c["z"], c["keep"])
    assert ((tok >= 0) & (tok < c["V"])).all() and c["keep"][tok].all(), "a token outside the kept set"
    ud = u.astype(np.float64)
    return float(np.maximum(np.maximum(a[tok] - ud, ud - b[tok]), 0.0).max())


# "crowded": one first radix digit for 70,000 entries -- the selections' path without the gather into LDS (V carries top_k, si m)
ALL_CASES = ([("grid", V, si) for V, si in R.CASES] + [("tiny", V, 0) for V in R.TINY]
             + [("crowded", k, m) for k, m in R.CROWDED])


def _case(kind, V, si):
    return R.case(V, si) if kind == "grid" else R.tiny_case(V) if kind == "tiny" else R.crowded_case(V, si)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("kind,V,si", ALL_CASES)
def test_kept_set_is_exact(kind, V, si, rows):
    """kept_out = the reference's count, thresh_out = its smallest kept z bit for bit; row r holds the logits rolled by 17 r
    places (the same values at other indices, rows at a real stride)."""
    c = _case(kind, V, si)
    x = torch.from_numpy(np.stack([np.roll(c["x"], 17 * r) for r in range(rows)])).to(DEV)
    tok, kept, thresh, _ = _launch(x, _params(c, seed=5))
    want = np.float32(c["z"][c["keep"]].min())
    assert kept.tolist() == [int(c["keep"].sum())] * rows
    assert thresh.view(np.uint32).tolist() == [int(want.view(np.uint32))] * rows
    for r in range(rows):
        assert np.roll(c["keep"], 17 * r)[tok[r]]


@pytest.mark.parametrize("kind,V,si", ALL_CASES)
def test_token_follows_the_fp64_cdf(kind, V, si):
    c = _case(kind, V, si)
    tok, kept, _, u = _launch(c["x"], _params(c), rows=66, u_in=U_ROWS)
    assert np.array_equal(u, U_ROWS) and (kept == int(c["keep"].sum())).all()
    d = _miss(c, tok, u)
    REPORT[f"{kind}-V{V}-{si}"] = dict(worst_miss=d, bound=R.bound(c["V"]), kept=int(kept[0]))
    print(f"{kind} V={V} settings={si} kept={int(kept[0])} worst miss {d:.3e} bound {R.bound(c['V']):.3e}")
    assert d <= R.bound(c["V"])
    assert tok[64] == int(np.nonzero(c["keep"])[0][0]), "u = 0 must give the lowest kept index"


def test_ties_across_the_top_k_boundary_all_stay():
    z = np.full(5000, -3.0, np.float32)
    z[1234:1244] = 2.0
    z[77] = 4.0
    c = dict(V=5000, x=z, T=1.0, top_k=4, top_p=1.0, min_p=0.0, z=R.scaled(z, 1.0))
    c["keep"] = R.kept_set(c["z"], 4)
    tok, kept, thresh, u = _launch(z, _params(c), rows=66, u_in=U_ROWS)
    assert c["keep"].sum() == 11 and (kept == 11).all() and (thresh == 2.0).all()
    assert _miss(c, tok, u) <= R.bound(5000)


@pytest.mark.parametrize("top_p,n", [(0.75, 5), (0.45, 1)])
def test_a_tied_group_across_the_top_p_boundary_stays_whole(top_p, n):
    p = np.array([0.01] * 4 + [0.1, 0.5, 0.1, 0.1] + [0.01] * 6 + [0.1])
    x = np.log(p).astype(np.float32)
    c = dict(V=15, x=x, T=1.0, top_k=0, top_p=top_p, min_p=0.0, z=R.scaled(x, 1.0))
    c["keep"] = R.kept_set(c["z"], 0, top_p)
    tok, kept, thresh, u = _launch(x, _params(c), rows=66, u_in=U_ROWS)
    assert c["keep"].sum() == n and (kept == n).all() and (thresh == c["z"][c["keep"]].min()).all()
    assert _miss(c, tok, u) <= R.bound(15)


def test_special_values_are_never_returned():
    from unsloth_amd.kernels import decode as D
    V = 3001
    x = (4.0 * np.random.RandomState(3).standard_normal(V)).astype(np.float32)
    x[::3] = -np.inf
    x[1::7] = np.nan
    x[int(np.nanargmax(np.where(np.isfinite(x), x, -1e30)))] = np.nan            # the would-be winner too
    for T, k, p, mp in ((1.0, 0, 1.0, 0.0), (0.7, 40, 0.9, 0.0), (1.0, 0, 1.0, 0.05), (1.3, 3000, 0.5, 0.01)):
        c = dict(V=V, x=x, T=T, top_k=k, top_p=p, min_p=mp, z=R.scaled(x, T))
        c["keep"] = R.kept_set(c["z"], k, p, mp)
        tok, kept, thresh, u = _launch(x, _params(c), rows=66, u_in=U_ROWS)
        assert (kept == int(c["keep"].sum())).all() and np.isfinite(x[tok]).all()
        assert _miss(c, tok, u) <= R.bound(V)
    dead = torch.full((2, 500), float("-inf"), device=DEV)
    dead[1, 5] = float("nan")
    tok, kept, _, _ = _launch(dead, D.sample_params(DEV, 1.0, 10, 0.9, 0.1, seed=1))
    assert tok.tolist() == [0, 0] and kept.tolist() == [0, 0]


def test_rejects_bad_arguments_before_any_launch():
    from unsloth_amd.kernels import decode as D
    prm = D.sample_params(DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        D.sample_f32(torch.zeros(1, (1 << 18) + 1, device=DEV), prm, _ctr())
    with pytest.raises(ValueError):
        D.sample_params(DEV, temperature=0.0)


@pytest.mark.parametrize("seed,draw", [(0, 0), (1, 1), (0xFEDCBA9876543210, 7), (12345, (1 << 32) + 3),
                                       (0x8000000000000001, (1 << 40) + 11)])
def test_generator_is_philox(seed, draw):
    """u_out = the helper's Philox4x32-10 at (seed, draw counter, row), bit for bit; also a draw counter above 2^32 and a seed
    with its high bits set."""
    from unsloth_amd.kernels import decode as D
    rows = 5
    x = torch.randn(rows, 300, device=DEV)
    prm = D.sample_params(DEV, seed=seed)
    _, _, _, u = _launch(x, prm, ctr=_ctr(draw))
    assert u.tolist() == [float(R.uniform(seed, draw, r)) for r in range(rows)]
    # the seed as a device tensor (what generate() hands over) is the same seed
    s = seed - (1 << 64) if seed >= (1 << 63) else seed
    D.sample_params(seed=torch.tensor([s], device=DEV), out=prm)
    assert _launch(x, prm, ctr=_ctr(draw))[3].tolist() == u.tolist()


def test_launches_are_bit_reproducible():
    """V = 128256 with top-p and min-p on, 20 launches into fresh outputs and 20 through reused buffers: one result."""
    from unsloth_amd.kernels import decode as D
    c = R.case(128256, 7)
    lg = torch.from_numpy(c["x"].copy()).to(DEV)[None].expand(8, -1)
    prm = D.sample_params(DEV, 0.8, 0, c["top_p"], 0.02, seed=99)
    ctr = _ctr(4)
    first = None
    for _ in range(20):
        got = _launch(lg, prm, ctr=ctr)
        first = first or got
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(got, first))
    out = torch.empty(8, dtype=torch.long, device=DEV)
    ws = (torch.empty(8 * 64, dtype=torch.float32, device=DEV), torch.empty(8 * 64, dtype=torch.long, device=DEV))
    for _ in range(20):
        assert D.sample_f32(lg, prm, ctr, out=out, ws=ws) is out
        assert np.array_equal(out.cpu().numpy(), first[0])
    assert len(set(first[0].tolist())) > 1, "eight rows, eight streams: not one token"


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def g(seed):
    return torch.Generator().manual_seed(seed)


def _tiny(load_in_4bit=True, r=8):
    """The tiny Llama of tests/test_gpu_decode.py."""
    from transformers import LlamaConfig
    from unsloth_amd import FastLanguageModel
    cfg = LlamaConfig(hidden_size=512, intermediate_size=1408, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=128, vocab_size=1000, rms_norm_eps=1e-5, max_position_embeddings=512,
                      rope_parameters={"rope_type": "default", "rope_theta": 5e5}, tie_word_embeddings=False)
    model, _ = FastLanguageModel.from_pretrained(config=cfg, max_seq_length=256, load_in_4bit=load_in_4bit, device=DEV,
                                                 random_state=3407, use_gradient_checkpointing=False)
    model = FastLanguageModel.get_peft_model(model, r=r, lora_alpha=2 * r, use_gradient_checkpointing=False, random_state=3407)
    gg = torch.Generator().manual_seed(11)
    for n, p in model.named_parameters():
        if "lora_B" in n:
            p.data.copy_((torch.randn(p.shape, generator=gg) * 0.05).to(DEV))
    model.eval()
    return model


@pytest.fixture(scope="module")
def tiny():
    return _tiny()


SET = dict(temperature=0.8, top_k=20, top_p=0.9, min_p=0.05)
SEED = 0x9E3779B97F4A7C15


def _check_draw(logits, tok, seed, draw):
    """Every row's token lies in the reference kept set of its logits and its CDF interval holds u(seed, draw, row)."""
    lg = logits.float().cpu().numpy()
    for row in range(lg.shape[0]):
        z = R.scaled(lg[row], SET["temperature"])
        c = dict(V=z.shape[0], z=z, keep=R.kept_set(z, SET["top_k"], SET["top_p"], SET["min_p"]))
        u = np.array([R.uniform(seed, draw, row)])
        assert _miss(c, tok.cpu().numpy()[row:row + 1], u) <= R.bound(c["V"]), (draw, row)


@pytest.mark.parametrize("batch", [1, 2])
def test_engine_steps_draw_inside_the_step(tiny, batch):
    """prefill, one eager draw, then 6 steps with the sampler on (batch 1: replayed hipGraph, batch 2: the plain step): the token
    of draw i follows the reference at u(seed, i, row) -- the counter advances inside the step, every row has its own stream --
    and an engine without the graph draws the same tokens bit for bit."""
    from unsloth_amd.models.decode import DecodeEngine
    ids = torch.randint(0, 1000, (batch, 13), generator=g(41)).to(DEV)
    eng = DecodeEngine(tiny, max_seq_len=128, batch=batch, use_graph=True)
    eng_e = DecodeEngine(tiny, max_seq_len=128, batch=batch, use_graph=False)
    toks = []
    for e in (eng, eng_e):
        lg = e.prefill(ids).clone()
        e.sampling(seed=SEED, **SET)
        seq = [e.draw().clone()]
        _check_draw(lg, seq[0], SEED, 0)
        for i in range(1, 7):
            lg = e.step(seq[-1]).clone()
            seq.append(e.next_tok.clone())
            _check_draw(lg, seq[-1], SEED, i)
        assert int(e._draw_ctr[0]) == 7
        toks.append(torch.stack(seq))
    assert torch.equal(toks[0], toks[1]), "the captured step and the eager step drew different tokens"


def test_generate_is_reproducible_and_leaves_greedy_alone(tiny):
    from unsloth_amd.models.decode import DecodeEngine
    ids = torch.randint(0, 1000, (1, 9), generator=g(42)).to(DEV)
    eng = DecodeEngine(tiny, max_seq_len=128)
    kw = dict(max_new_tokens=12, do_sample=True, **SET)
    greedy = eng.generate(ids, max_new_tokens=12)
    s1 = eng.generate(ids, generator=torch.Generator(DEV).manual_seed(3), **kw)
    s2 = eng.generate(ids, generator=torch.Generator(DEV).manual_seed(3), **kw)
    s3 = eng.generate(ids, generator=torch.Generator(DEV).manual_seed(4), **kw)
    assert s1.shape == (1, 21) and torch.equal(s1, s2) and not torch.equal(s1, s3)
    assert torch.equal(eng.generate(ids, max_new_tokens=12), greedy), "a sampled call changed the greedy one after it"
    assert torch.equal(DecodeEngine(tiny, max_seq_len=128, use_graph=False).generate(ids, max_new_tokens=12), greedy)


def test_settings_change_on_a_live_capture(tiny):
    """The captured sampled step reads its settings from the device: a second call at another temperature equals a fresh engine's."""
    from unsloth_amd.models.decode import DecodeEngine
    ids = torch.randint(0, 1000, (1, 9), generator=g(43)).to(DEV)
    eng = DecodeEngine(tiny, max_seq_len=128)
    gen = lambda e, T: e.generate(ids, max_new_tokens=12, do_sample=True, temperature=T, top_k=50, top_p=0.95,
                                  generator=torch.Generator(DEV).manual_seed(8))
    hot = gen(eng, 1.5)
    assert eng._graph_s is not None
    cold = gen(eng, 0.05)
    assert torch.equal(cold, gen(DecodeEngine(tiny, max_seq_len=128), 0.05))
    assert torch.equal(hot, gen(DecodeEngine(tiny, max_seq_len=128), 1.5)) and not torch.equal(hot, cold)


def test_min_p_stays_on_the_engine_through_for_inference():
    from unsloth_amd import FastLanguageModel
    model = _tiny()
    FastLanguageModel.for_inference(model)
    ids = torch.randint(0, 1000, (1, 9), generator=g(44)).to(DEV)
    greedy = model.generate(input_ids=ids, max_new_tokens=6)
    calls = []
    model._old_generate = lambda *a, **k: (calls.append(k), greedy)[1]
    out = model.generate(input_ids=ids, max_new_tokens=6, do_sample=True, min_p=0.1, generator=torch.Generator(DEV).manual_seed(1))
    assert not calls and out.shape == greedy.shape
    only = model.generate(input_ids=ids, max_new_tokens=6, do_sample=True, min_p=1.0, generator=torch.Generator(DEV).manual_seed(1))
    assert not calls and torch.equal(only, greedy)
    base = model.get_base_model()
    base.generation_config.do_sample, base.generation_config.min_p = True, 1.0
    model.generation_config = base.generation_config
    assert torch.equal(model.generate(input_ids=ids, max_new_tokens=6), greedy) and not calls
