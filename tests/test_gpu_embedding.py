"""-m gpu: the token-embedding kernels (csrc/embedding.hip) through unsloth_amd.kernels.fast_embedding.
  * forward: the bits of torch.nn.functional.embedding, also on padded row strides; an id == V gives a zero row
  * backward: every element of dW against an fp64 index_add_ of the same dY, within
        |dW - ref| <= u |ref| + c 2^-23 sum_run |dY|,   u = 2^-8 (bf16) / 2^-11 (fp16),  c = run length (+ 1 when accumulating)
    (one rounding to 16 bits behind at most c fp32 additions); rows nobody references are exactly 0 (overwrite) or keep their
    bits (accumulate); two launches give the same bits
  * a 2-layer Llama under full fine-tuning: the embedding gradient of each of two micro-batches lands in the flat bucket
    within the same bound, on top of the lm_head gradient when the two are tied."""
import pytest
import torch
import torch.nn.functional as F

from unsloth_amd.kernels import fast_embedding
from unsloth_amd.kernels.embedding import embedding_bwd, embedding_fwd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float16]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
NS, HS, V = [1, 63, 65, 257], [64, 200, 1024], 37


def _ref64(ids, dY, vocab, pad=None):
    """(sum, sum of magnitudes, run length) per vocabulary row in float64, over the ids that count."""
    keep = (ids >= 0) & (ids < vocab) & (ids != (-1 if pad is None else pad))
    z = torch.zeros(vocab, dY.shape[1], dtype=torch.float64, device=dY.device)
    d = dY[keep].double()
    return z.index_add(0, ids[keep], d), z.index_add(0, ids[keep], d.abs()), torch.bincount(ids[keep], minlength=vocab)


def _assert_within(got, base, ids, dY, vocab, pad=None):
    """`got` against base + sum (base None: overwrite mode, untouched rows exactly 0; else they keep base's bits)."""
    s, mag, cnt = _ref64(ids, dY, vocab, pad)
    ref = s if base is None else base.double() + s
    c = (cnt + (0 if base is None else 1)).double().unsqueeze(1)
    over = (got.double() - ref).abs() - (U[got.dtype] * ref.abs() + c * 2.0 ** -23 * mag)
    assert not bool((over[cnt > 0] > 0).any()), float(over[cnt > 0].max())
    idle = cnt == 0
    assert torch.equal(got[idle], torch.zeros_like(got[idle]) if base is None else base[idle])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_forward_is_torch_embedding_bit_for_bit(n, H, dtype):
    g = torch.Generator().manual_seed(n + H)
    W = torch.randn(V, H, generator=g).to(dtype).to(DEV)
    ids = torch.randint(0, V, (n,), generator=g).to(DEV)
    assert torch.equal(fast_embedding(ids, W), F.embedding(ids, W))
    assert torch.equal(fast_embedding(ids.view(1, n), W, padding_idx=3), F.embedding(ids.view(1, n), W, padding_idx=3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_padded_row_strides_and_an_id_past_the_table(dtype):
    n, H = 65, 200
    g = torch.Generator().manual_seed(5)
    Wp = torch.randn(V, H + 8, generator=g).to(dtype).to(DEV)
    ids = torch.randint(0, V, (n,), generator=g).to(DEV)
    ids[17] = V
    outp = torch.full((n, H + 16), 7.0, dtype=dtype, device=DEV)
    embedding_fwd(ids, Wp[:, :H], out=outp[:, 8:8 + H])
    want = F.embedding(ids.clamp(max=V - 1), Wp[:, :H])
    want[17] = 0
    assert torch.equal(outp[:, 8:8 + H], want)
    assert bool((outp[:, :8] == 7).all()) and bool((outp[:, 8 + H:] == 7).all())          # nothing outside the rows' H columns


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("pattern", ["distinct", "equal", "runs5", "padding"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("n", NS)
def test_backward_against_fp64_and_deterministic(n, H, dtype, pattern, accumulate):
    g = torch.Generator().manual_seed(n * 7 + H)
    vocab, pad = {"distinct": n + 3, "runs5": 5}.get(pattern, V), None
    if pattern == "distinct":
        ids = torch.randperm(vocab, generator=g)[:n]
    elif pattern == "equal":
        ids = torch.full((n,), 7)
    else:
        ids = torch.randint(0, vocab, (n,), generator=g)
    if pattern == "padding":
        pad = int(ids[n // 2])
    ids = ids.to(DEV)
    dY = torch.randn(n, H + 8, generator=g).to(dtype).to(DEV)[:, 8:]                      # a strided column slice
    base = torch.randn(vocab, H, generator=g).to(dtype).to(DEV) if accumulate else None
    runs = []
    for _ in range(2):
        out = base.clone() if accumulate else torch.full((vocab, H), float("nan"), dtype=dtype, device=DEV)
        runs.append(embedding_bwd(ids, dY, vocab, pad, out=out, accumulate=accumulate))
    _assert_within(runs[0], base, ids, dY, vocab, pad)
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_returns_the_gradient_or_writes_it_into_the_callers_view(dtype):
    n, H = 257, 200
    g = torch.Generator().manual_seed(11)
    W = torch.randn(V, H, generator=g).to(dtype).to(DEV).requires_grad_(True)
    ids = torch.randint(0, V, (3, n), generator=g).to(DEV)
    ids[0, :4] = torch.tensor([-1, V, V + 5, -9], device=DEV)                             # ids outside the table are skipped
    dY = torch.randn(3, n, H, generator=g).to(dtype).to(DEV)
    fast_embedding(ids, W, padding_idx=2).backward(dY)
    _assert_within(W.grad, None, ids.view(-1), dY.view(-1, H), V, 2)
    bucket = torch.randn(V * H + 8, generator=g).to(dtype).to(DEV)
    view, before = bucket[8:].view(V, H), bucket[8:].view(V, H).clone()
    W.grad = None
    fast_embedding(ids, W, padding_idx=2, grad_out=view, accumulate=True).backward(dY)
    assert W.grad is None
    _assert_within(view, before, ids.view(-1), dY.view(-1, H), V, 2)
    frozen = fast_embedding(ids, W.detach())                                              # no backward without a trainable table
    assert not frozen.requires_grad


@pytest.mark.parametrize("tie", [False, True])
def test_full_finetune_embedding_gradient_lands_in_the_bucket(tie, monkeypatch):
    from transformers import LlamaConfig
    import unsloth_amd.models.llama as llama
    from unsloth_amd import FastLanguageModel, _lib
    from unsloth_amd.full_finetune import ShardedAdamW
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                      head_dim=128, vocab_size=512, rms_norm_eps=1e-5, max_position_embeddings=256,
                      rope_parameters={"rope_type": "default", "rope_theta": 5e5}, tie_word_embeddings=tie)
    model, _ = FastLanguageModel.from_pretrained(config=cfg, max_seq_length=128, full_finetuning=True, load_in_4bit=True,
                                                 device=DEV, random_state=3407, use_gradient_checkpointing=False)
    W = model.get_input_embeddings().weight
    assert (model.get_output_embeddings().weight is W) == tie
    opt = ShardedAdamW(model, lr=1e-3)
    B = opt.buckets
    names, real, seen = [], _lib.call, []
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def spy(ids, weight, *a, **k):          # dY of the lookup, and what the bucket held when it arrived (None: nothing yet)
        out = fast_embedding(ids, weight, *a, **k)
        out.register_hook(lambda d: seen.append((ids.reshape(-1), d.reshape(-1, d.shape[-1]).clone(),
                                                 None if B.first_write(W) else B.grad_view(W).clone())))
        return out
    monkeypatch.setattr(llama, "fast_embedding", spy)
    g = torch.Generator().manual_seed(4)
    for step in range(2):                   # one optimizer step, two micro-batches
        ids = torch.randint(0, 40 if step else 512, (2, 96), generator=g).to(DEV)        # (the second: long runs)
        pos = torch.arange(96, dtype=torch.int32, device=DEV).unsqueeze(0).expand(2, 96).contiguous()
        if step == 0:
            with B.no_sync():
                model(input_ids=ids, labels=ids, position_ids=pos).loss.backward()
        else:
            model(input_ids=ids, labels=ids, position_ids=pos).loss.backward()
        tok, dY, base = seen[step]
        assert (base is None) == (step == 0 and not tie)          # untied: the first micro-batch overwrites
        _assert_within(B.grad_view(W), base, tok, dY, 512, model.get_input_embeddings().padding_idx)
    B.finish()
    assert names.count("uamd_embedding_bwd") == 2 and names.count("uamd_embedding_fwd") == 2
    assert W.grad.data_ptr() == B.grad_view(W).data_ptr()
    opt.step()
    opt.zero_grad()
    B.close()
