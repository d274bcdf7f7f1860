"""Helpers of the batched-decode tests (test_gpu_decode_batched.py, test_decode_batch_host.py)."""
import torch

DEV = "cuda"


def g(seed):
    return torch.Generator().manual_seed(seed)


_MODELS = {}


def tiny(load_in_4bit=True, r=8, fresh=False):
    """The tiny model of tests/test_gpu_decode.py::_tiny: hidden 512, 2 layers, 4 / 2 heads, head_dim 128, vocab 1000, LoRA r = 8
    with lora_B randomised. One instance per precision is shared by the tests that only read it (`fresh`: a model of the
    caller's own, for tests that rebind its generate)."""
    key = (load_in_4bit, r)
    if not fresh and key in _MODELS:
        return _MODELS[key]
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
    if not fresh:
        _MODELS[key] = model
    return model


def left_padded(lengths, T, seed, pad_id=0):
    """(ids [B, T], mask [B, T], rows: the unpadded prompts) of left-padded random prompts."""
    rows = [torch.randint(1, 1000, (L,), generator=g(seed + i)) for i, L in enumerate(lengths)]
    ids = torch.full((len(lengths), T), pad_id, dtype=torch.long)
    mask = torch.zeros(len(lengths), T, dtype=torch.long)
    for b, row in enumerate(rows):
        ids[b, T - len(row):] = row
        mask[b, T - len(row):] = 1
    return ids, mask, rows


def full_logits(model, seq):
    """fp32 last-position logits of the training-path forward over one unpadded sequence [1, L] (UNSLOTH_RETURN_LOGITS set)."""
    with torch.no_grad():
        return model(input_ids=seq).logits[:, -1].float()


class Recorder:
    """Stands in for `model._old_generate`: records the calls and returns a fixed tensor."""

    def __init__(self, ret=None):
        self.calls, self.ret = [], ret

    def __call__(self, *a, **k):
        self.calls.append((a, k))
        return self.ret


class StubEngine:
    """A DecodeEngine for the routing tests on the host: the attributes unsloth_fast_generate looks at, and a generate that
    records its keyword arguments."""

    def __init__(self, B, S):
        self.B, self.S, self.calls = B, S, []

    def generate(self, input_ids, **kw):
        self.calls.append(kw)
        n = kw.get("num_return_sequences", 1)
        return torch.zeros(input_ids.shape[0] * n, input_ids.shape[1] + kw["max_new_tokens"], dtype=torch.long)
