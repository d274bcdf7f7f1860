"""KV-cache decode path; counterpart of the inference half of unsloth/models/llama.py.

Reference: LlamaAttention_fast_forward_inference (:352-569), fast_swiglu_inference (:572-606),
fast_rms_layernorm_inference (:609-632), LlamaModel_fast_forward_inference (:1249-1364) and unsloth_fast_generate
(:2167-2259): a Python loop of ~25 small torch / bitsandbytes calls per layer per token, with a KV cache that grows by
KV_CACHE_INCREMENT re-allocations and host syncs for the rotary length.

MI355X design: one `DecodeEngine` per (model, max_seq_len, batch):
  * the KV cache is allocated ONCE at [layers][B, Hk, S_max, D] (288 GB of HBM: no growth, no copies);
  * a token step of one sequence is FIVE launches per layer -- q|k|v GEMV (residual add + RMSNorm inside), attention (RoPE,
    cache append, split-KV attention and its combine inside), o GEMV, gate|up GEMV (residual add + RMSNorm in, SwiGLU out),
    down GEMV; every LoRA `A x` is computed once inside the GEMV launch that needs it (uamd_gemv_fused) -- that read the
    position from DEVICE memory, so the whole step -- all layers, final norm, lm_head GEMV, greedy argmax (or, when sampling,
    the temperature / top-k / top-p / min-p draw of uamd_sample_f32 and its draw counter), position increment -- is captured
    once as a hipGraph and replayed per token. (Rounds 2-3: 14 launches per layer, ~450 kernels
    of ~9 us for ~0.6 ms of HBM traffic; still the batch > 1 path and `UNSLOTH_AMD_DECODE_FUSED=0`.);
  * prefill runs the training-path kernels (flash attention over the prompt) and writes K (post-RoPE) / V into the cache.
Batches of 2 .. 64 sequences run the 14-launch step with every linear on uamd_gemv_rows (17 rows and up: uamd_gemv_rows64, the
same bits per row) -- ONE pass over the weights for all token rows, LoRA term and bias inside the launch, q|k|v written straight into the fused row -- captured and replayed as a
hipGraph like the single-sequence step (`BATCH_ROWS`); a row's logits do not depend on its companions. Larger batches decode
through the fused NF4 GEMM (as the reference does, utils.py:1095-1097), eager. Prompts of different lengths arrive LEFT-padded
with their attention_mask: prefill treats the padding as documents, counts RoPE positions from each row's first real token
and stores row b's keys at cache positions [0, L_b); the step works per row from kv_len[b] and needs nothing else.
`kv_cache_dtype="fp8"` (opt-in): the cache holds e4m3 codes and one fp32 scale per key (include/unsloth_amd.h; uamd_kv_store_fp8,
uamd_rope_kv_append_fp8, uamd_attn_decode_fp8) at (D + 4) / (2 D) of the bytes -- for batches and long contexts; one sequence
leaves the 5-launch step for it.
`share_prompt=n` (opt-in, 16-bit cache): rows p n .. p n + n - 1 are n samples of prompt p (num_return_sequences; GRPO's n
completions of one prompt). The prompt's K / V are stored once per prompt and each row keeps only the keys it appended; the step's
attention (uamd_attn_decode_shared) scores the n x G query rows of a (prompt, KV head) against one fetch of every prompt key.
`generate(..., prompt_lookup_num_tokens=K)` (opt-in, one greedy sequence, 16-bit cache): every step verifies the last token and K
drafts found in the sequence's own context as K + 1 token rows on one pass over the weights (uamd_ngram_draft, uamd_gemv_rows,
uamd_rope_kv_append_span, uamd_attn_decode_span, uamd_accept_greedy), a third captured graph beside the greedy and the sampled step.
"""
import math
import os

import torch

from ..kernels import decode as _dk
from ..kernels.rms_layernorm import add_rms_fwd, rms_fwd
from ..kernels.rope_embedding import fast_rope_embedding
from ..kernels.swiglu import swiglu_fg_kernel
from ..kernels.utils import get_lora_parameters_bias, matmul_lora

SPLIT_KEYS = 128


def _base(model):
    m = model.get_base_model() if hasattr(model, "get_base_model") else model
    return m


# UNSLOTH_AMD_DECODE_FUSED=0: one token of one sequence as the 14 separate launches per layer of rounds 2-3 instead of 5.
# (Round 3's first fused step -- 7 launches, every workgroup recomputing the norm AND t = A x, up to 48 rows x K from L2 --
# measured slower than the 14, 4.97 vs 4.13 ms per token, profiles/r03r_decode_fused_ab.jsonl; t is now computed once per
# launch and handed over through a device workspace, RoPE / append / combine ride in the attention launch and SwiGLU in the
# gate|up epilogue.)
FUSED_STEP = True
# Batches of 2 .. 64 sequences: every linear of the token step through uamd_gemv_rows / uamd_gemv_rows64 (one pass over the
# weights for all rows, LoRA term and bias inside the launch) and the step captured as a hipGraph, against the 128 x 128-tile NF4 GEMM + separate
# LoRA / bias launches, eager (False: the route of every larger batch). Read when an engine is built; only tests and
# tools/decode_batch_bench.py flip it (profiles/decode_batch_bench.jsonl and decode_batch64_bench.jsonl are the A/B).
BATCH_ROWS = True


def left_pad_lengths(attention_mask):
    """Lengths [B] (int64, on the mask's device) of a LEFT-padded key mask [B, T] -- every row `[zeros | ones]` with at least
    one real token (a row of all ones included) -- or None for anything else: right padding, holes, an empty row. One host
    sync."""
    m = attention_mask != 0
    if m.dim() != 2 or m.shape[1] == 0:
        return None
    n = m.sum(1)
    T = m.shape[1]
    tail = torch.arange(T, device=m.device)[None, :] >= (T - n)[:, None]
    if not bool(((n > 0).all()) & ((m == tail).all())):
        return None
    return n


def kv_cache_kind(kv_cache_dtype):
    """The cache type of an engine: None (`None` / "auto": the cache holds the activation type) or "fp8" (e4m3 codes + one fp32
    scale per key, include/unsloth_amd.h). Anything else: ValueError."""
    if kv_cache_dtype is None or kv_cache_dtype == "auto":
        return None
    if kv_cache_dtype == "fp8":
        return "fp8"
    raise ValueError(f"kv_cache_dtype: None, 'auto' or 'fp8' (got {kv_cache_dtype!r})")


class DecodeEngine:
    """Greedy / sampled generation for a (PEFT-wrapped) Llama-family causal LM loaded by unsloth_amd."""

    def __init__(self, model, max_seq_len=2048, batch=1, use_graph=True, kv_cache_dtype=None, share_prompt=None,
                 max_new_tokens=None):
        from . import llama as _ll
        self.model = model
        self.lm = _base(model)                    # LlamaForCausalLM
        self.core = self.lm.model                 # LlamaModel
        cfg = self.lm.config
        self.cfg = cfg
        self.dtype = _ll._model_dtype(self.core)
        self.dev = self.core.embed_tokens.weight.device
        self.B = batch
        self.S = int(math.ceil(max_seq_len / SPLIT_KEYS) * SPLIT_KEYS)
        self.Hq, self.Hk = cfg.num_attention_heads, cfg.num_key_value_heads
        self.D = getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads
        if self.D not in _dk.HEAD_DIMS:
            raise NotImplementedError(f"decode attention kernels: head_dim 64 or 128 only (got {self.D})")
        if getattr(cfg, "hidden_act", "silu") != "silu":
            raise NotImplementedError("decode path: SwiGLU MLP only")
        self.window = int(getattr(cfg, "sliding_window", None) or 0)
        self.scale = 1.0 / math.sqrt(self.D)
        self.rows = bool(BATCH_ROWS) and 2 <= batch <= _dk.MAX_ROWS_WIDE      # the batched step on uamd_gemv_rows / _rows64
        self.use_graph = bool(use_graph) and (batch == 1 or self.rows)
        L = len(self.core.layers)
        # "fp8": the caches hold e4m3 codes (uint8) and one fp32 scale per (sequence, KV head, position) beside them -- (D + 4) /
        # (2 D) of the 16-bit cache's bytes. For batches and long contexts, where the cache is most of what a step reads; one
        # sequence leaves the single-launch step for it (_step_body) and a short one is slower that way.
        self.kv_cache_dtype = kv_cache_kind(kv_cache_dtype)
        kw = dict(dtype=torch.uint8 if self.kv_cache_dtype == "fp8" else self.dtype, device=self.dev)
        # share_prompt = n >= 2: rows p n .. p n + n - 1 are the n samples of prompt p. The prompt's K / V are stored ONCE, in
        # pk / pv [P, Hk, S, D] (S: the prompt capacity, `max_seq_len`), and k_cache / v_cache [P n, Hk, S_n, D] hold only what
        # each row appended after it (S_n: `max_new_tokens`, default max_seq_len). prompt_len [P] is fixed by prefill, new_len
        # [P n] counts the suffix keys and kv_len stays the total; the step reads every counter from device memory.
        self.share_prompt = None if share_prompt is None else int(share_prompt)
        self.S_n = self.S
        self.pk = self.pv = self.prompt_len = self.new_len = None
        if self.share_prompt is not None:
            n = self.share_prompt
            if n < 2 or batch % n:
                raise ValueError(f"share_prompt: n >= 2 samples per prompt and a batch of P * n rows (got n = {n}, batch = {batch})")
            if n > _dk.MAX_SHARE:
                raise NotImplementedError(f"uamd_attn_decode_shared takes up to {_dk.MAX_SHARE} samples per prompt (got {n})")
            if self.kv_cache_dtype == "fp8":
                raise NotImplementedError("share_prompt together with kv_cache_dtype='fp8': the shared FP8 prompt cache is not built")
            self.S_n = int(math.ceil((max_new_tokens or max_seq_len) / SPLIT_KEYS) * SPLIT_KEYS)
            self.pk = [torch.zeros(batch // n, self.Hk, self.S, self.D, **kw) for _ in range(L)]
            self.pv = [torch.zeros(batch // n, self.Hk, self.S, self.D, **kw) for _ in range(L)]
            self.prompt_len = torch.zeros(batch // n, dtype=torch.int32, device=self.dev)
        self.k_cache = [torch.zeros(batch, self.Hk, self.S_n, self.D, **kw) for _ in range(L)]
        self.v_cache = [torch.zeros(batch, self.Hk, self.S_n, self.D, **kw) for _ in range(L)]
        self.k_scale = self.v_scale = None
        if self.kv_cache_dtype == "fp8":
            # (codes 0, scale 1: what the quantiser makes of the zero rows a 16-bit cache starts with)
            self.k_scale = [torch.ones(batch, self.Hk, self.S, dtype=torch.float32, device=self.dev) for _ in range(L)]
            self.v_scale = [torch.ones(batch, self.Hk, self.S, dtype=torch.float32, device=self.dev) for _ in range(L)]
        # [kv_len per sequence ..., step counter]: ONE add_(1) per token advances both. The step counter (never reset) is the
        # device half of the hand-off tags of the fused kernels (kernels/decode.HandOff): unlike the position it cannot repeat
        # when a new prompt is prefilled or a caller rewinds kv_len
        # (a shared prompt: [kv_len ..., new_len ..., step counter] -- the same add_(1) advances the suffix count)
        npos = batch * (2 if self.share_prompt else 1)
        self._pos = torch.zeros(npos + 1, dtype=torch.int32, device=self.dev)
        self._pos[npos] = 1
        self.kv_len = self._pos[:batch]
        self._lens = self._pos[:npos]                 # every length counter: what a capture's warm-up has to put back
        if self.share_prompt:
            self.new_len = self._pos[batch:npos]
        self.step_ctr = self._pos[npos:]
        self._steps = 1                               # host mirror of step_ctr (no sync): wrap-around guard
        nsplit = self.S // SPLIT_KEYS + (self.S_n // SPLIT_KEYS if self.share_prompt else 0)      # prompt splits, then suffix splits
        self.partials = torch.empty(batch, self.Hq, nsplit, self.D + 2, dtype=torch.float32, device=self.dev)
        # the fused attention's splits: 128 keys each (64 keys = 256 workgroups at context 2048 measured 3.5 % slower per token,
        # profiles/r04_decode_split_keys_ab.txt), longer ones where 128 would mean more than 256 workgroups -- up to 256 of them
        # combine through granules, a larger launch pays the 21 us fence + arrival-counter tail: 256 keys at context 8192 with 8 KV
        # heads, 1024 at 32768
        bk = _dk.block_keys(self.D)                   # a split is whole block-loads of the kernel: 16 keys at D = 128, 32 at D = 64
        self.fsplit = max(SPLIT_KEYS, int(math.ceil(self.S * self.Hk * batch / 256 / bk) * bk))
        self.fpartials, self.counters = _dk.fused_attn_workspace(batch, self.Hq, self.Hk, self.S, self.D, self.fsplit, self.dev,
                                                                  step_dev=self.step_ctr)
        self.sync = _dk.HandOff(self.dev, step_dev=self.step_ctr)                             # uamd_gemv_fused hand-off
        self.tok = torch.zeros(batch, 1, dtype=torch.long, device=self.dev)
        self.next_tok = torch.zeros(batch, dtype=torch.long, device=self.dev)
        self.logits = None
        tables = _ll._rope_tables(self.core)
        self.cos, self.sin = tables.get(self.S + (self.S_n if self.share_prompt else 0), self.dev, self.dtype)
        self._graph = None
        assert 5 * L + 1 < 1024, "hand-off tag sites: 5 per layer below UAMD_TAG_STRIDE"
        self._params = [self._layer_params(l) for l in self.core.layers]
        self._head = self.lm.lm_head.weight
        # sampling: None = the steps pick next_tok greedily; otherwise (`sampling()`) they draw it with uamd_sample_f32 from the
        # DEVICE parameter block and draw counter below -- settings, seed and counter change in place, so the captured sampled
        # step (a capture of its own beside the greedy one) follows them. The counter is the engine's and starts at 0 in every
        # generate(): the hand-off step counter never resets and would make equal seeds give different tokens
        self._sample = None
        self._sparams = _dk.sample_params(self.dev)
        self._draw_ctr = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._graph_s = None
        # prompt-lookup decoding (generate(prompt_lookup_num_tokens=K)): the verify step of R = K + 1 token rows, one capture
        # per (R, n-gram size); its device state (`_lookup_state`) is allocated by the first call that asks for it
        self._graph_l = {}
        self._lk = None
        self.lookup_stats = None

    # ---- per-layer parameter tuples, read once (adapters must not be switched under a live engine) -------------------
    @staticmethod
    def _layer_params(layer):
        a, m = layer.self_attn, layer.mlp
        g = get_lora_parameters_bias
        return dict(qkv=[g(a.q_proj), g(a.k_proj), g(a.v_proj)], o=[g(a.o_proj)],
                    gu=[g(m.gate_proj), g(m.up_proj)], down=[g(m.down_proj)],
                    ln1=(layer.input_layernorm.weight, _eps(layer.input_layernorm)),
                    ln2=(layer.post_attention_layernorm.weight, _eps(layer.post_attention_layernorm)))

    # ---- prefill: prompt through the training-path kernels, K / V into the cache -----------------------------------------
    @torch.no_grad()
    def prefill(self, input_ids, attention_mask=None, repeat=1):
        """The prompt(s) [B, T] through the training-path kernels; K / V into the cache, next-token logits out.
        `attention_mask`: a LEFT-padded key mask (`left_pad_lengths`); row b's L_b real tokens get RoPE positions 0 .. L_b - 1
        and cache positions [0, L_b), pad positions never enter the cache, kv_len[b] = L_b. `repeat` = n: the engine's batch is
        B * n and every prompt's cache rows and logits are replicated to n adjacent rows (num_return_sequences)."""
        from . import llama as _ll
        from ..kernels import attention as _flash
        B, T = input_ids.shape
        assert B * repeat == self.B and T <= self.S
        assert self.share_prompt is None or repeat == self.share_prompt, "an engine with share_prompt = n prefills with repeat = n"
        lens = pad = seq_info = rope_pos = None
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            attention_mask = attention_mask.to(self.dev)
            lens = left_pad_lengths(attention_mask)
            if lens is None or attention_mask.shape != (B, T):
                raise ValueError("DecodeEngine.prefill: the attention_mask must be left-padded ([zeros | ones] rows, none empty)")
            pad = (T - lens)
            seq_info = (_flash.padding_mask_documents(attention_mask), None, None)
            ar = torch.arange(T, device=self.dev)
            rope_pos = (ar[None, :] - pad[:, None]).clamp_min(0).to(torch.int32).reshape(-1)
            src = (ar[None, :] + pad[:, None]).clamp_max(T - 1)                         # cache position j <- column pad_b + j
            src = src[:, None, :, None].expand(B, self.Hk, T, self.D)
            live = (ar[None, :] < lens[:, None])[:, None, :, None]
        # parameters were updated since the token step was captured (an optimizer stepped, a training forward ran): the
        # graph holds pointers to activation-dtype copies of the LoRA factors that are stale now -- capture again
        from ..kernels.utils import _CAST_EPOCH
        if getattr(self, "_epoch", None) != _CAST_EPOCH[0]:
            self._epoch = _CAST_EPOCH[0]
            # (a) the activation-dtype copies of the LoRA A factors are refreshed IN PLACE (the captured graph keeps
            # their addresses); (b) if a parameter's storage moved (optim.FlatAdamW adopts the parameters into its flat
            # arena, module.to(...)) the graph's pointers to the fp32 B factors dangle: capture again
            sig = []
            for P in self._params:
                for grp in ("qkv", "o", "gu", "down"):
                    As = [pr[2] for pr in P[grp] if pr[2] is not None]
                    if As:
                        _dk.lora_a_rows(As, self.dtype)
                    sig += [t.data_ptr() for pr in P[grp] for t in pr[:4] if torch.is_tensor(t)]
            sig = tuple(sig)
            if getattr(self, "_ptr_sig", None) != sig:
                self._graph = self._graph_s = None
                self._graph_l = {}
                self._ptr_sig = sig
        core = self.core
        h = core.embed_tokens(input_ids.to(self.dev)).to(self.dtype)
        cos, sin = self.cos, self.sin
        resid, delta = h, None
        for li, layer in enumerate(core.layers):
            w1, e1 = self._params[li]["ln1"]
            if delta is None:
                x = rms_fwd(resid, w1, e1)[0].view(B, T, -1)
            else:
                resid, x, _ = add_rms_fwd(delta, resid, w1, e1)
                resid, x = resid.view(B, T, -1), x.view(B, T, -1)
            attn = layer.self_attn
            Q, K, V = attn.apply_qkv(attn, x)
            Q = Q.view(B, T, self.Hq, self.D).transpose(1, 2)
            K = K.view(B, T, self.Hk, self.D).transpose(1, 2)
            V = V.view(B, T, self.Hk, self.D).transpose(1, 2)
            Q, K = fast_rope_embedding(Q, K, cos, sin, rope_pos)
            Kc, Vc = K, V
            if lens is not None:
                zero = torch.zeros((), dtype=self.dtype, device=self.dev)
                Kc, Vc = torch.where(live, K.gather(2, src), zero), torch.where(live, V.gather(2, src), zero)
            if self.kv_cache_dtype == "fp8":
                # quantise each prompt once, into the first of its `repeat` rows; the replicas are copies of codes and scales
                for rows_, codes, scales in ((Kc, self.k_cache[li], self.k_scale[li]), (Vc, self.v_cache[li], self.v_scale[li])):
                    _dk.kv_store_fp8(rows_, codes[::repeat], scales[::repeat])
                    if repeat > 1:
                        c5, s4 = codes.view(B, repeat, self.Hk, self.S, self.D), scales.view(B, repeat, self.Hk, self.S)
                        c5[:, 1:, :, :T].copy_(c5[:, :1, :, :T])
                        s4[:, 1:, :, :T].copy_(s4[:, :1, :, :T])
            elif self.share_prompt:                 # once per prompt: no replicas
                self.pk[li][:, :, :T].copy_(Kc)
                self.pv[li][:, :, :T].copy_(Vc)
            else:
                if repeat > 1:
                    Kc, Vc = Kc.repeat_interleave(repeat, 0), Vc.repeat_interleave(repeat, 0)
                self.k_cache[li][:, :, :T].copy_(Kc)
                self.v_cache[li][:, :, :T].copy_(Vc)
            A = _ll._attention(Q, K, V, seq_info, None, self.window or None)
            o = attn.apply_o(attn, A)
            w2, e2 = self._params[li]["ln2"]
            resid, x, _ = add_rms_fwd(o, resid, w2, e2)
            resid, x = resid.view(B, T, -1), x.view(B, T, -1)
            delta = layer.mlp(x)
        wn, en = core.norm.weight, _eps(core.norm)
        _, xn, _ = add_rms_fwd(delta[:, -1:], resid[:, -1:], wn, en)
        if lens is None:
            self.kv_len.fill_(T)
        else:
            self.kv_len.copy_(lens.repeat_interleave(repeat, 0))
        if self.share_prompt:
            self.prompt_len.copy_(self.kv_len[::repeat])
            self.new_len.zero_()
        xn = xn.view(B, -1)
        self.logits = self._lm_head(xn if repeat == 1 else xn.repeat_interleave(repeat, 0))
        return self.logits

    def _greedy(self):
        """next_tok = argmax of the step's logits, inside the captured step."""
        lg = self.logits
        if lg.dtype == torch.float32 and lg.is_contiguous():
            if getattr(self, "_amax_ws", None) is None:
                self._amax_ws = (torch.empty(self.B * 64, dtype=torch.float32, device=self.dev),
                                 torch.empty(self.B * 64, dtype=torch.long, device=self.dev))
            _dk.argmax_f32(lg, out=self.next_tok, ws=self._amax_ws)
        else:
            self.next_tok.copy_(torch.argmax(lg, dim=-1))

    def sampling(self, temperature=None, top_k=0, top_p=1.0, min_p=0.0, seed=None):
        """`sampling()`: greedy steps. `sampling(temperature, top_k, top_p, min_p, seed)`: from now on `draw()` and every step
        sample next_tok -- HF's warpers in HF's order, then one Philox draw per row at (seed, draw counter, row) -- and the
        draw counter starts over at 0. `seed`: python int or int64 device tensor of one element (no sync); None keeps it."""
        if temperature is None:
            self._sample = None
            return
        V = self._head.shape[0]
        if V > _dk.SAMPLE_MAX_V:
            raise NotImplementedError(f"uamd_sample_f32 samples vocabularies up to {_dk.SAMPLE_MAX_V} entries (got {V})")
        _dk.sample_params(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed, out=self._sparams)
        self._draw_ctr.zero_()
        self._sample = True

    def draw(self):
        """next_tok ~ the current logits (of `prefill` or of the last step) at the current draw counter, which advances by one.
        The step bodies call it where the greedy step calls `_greedy()`; generate() calls it once, eagerly, after prefill."""
        lg = self.logits
        assert lg.dtype == torch.float32 and lg.stride(-1) == 1
        _dk.sample_f32(lg, self._sparams, self._draw_ctr, out=self.next_tok)
        self._draw_ctr.add_(1)
        return self.next_tok

    def _lm_head(self, x):                       # x [B, H] -> fp32 logits [B, V]
        W = self._head
        if self.B == 1 and W.dtype == x.dtype and W.shape[1] <= 16384:
            (y,) = _dk.gemv(x.reshape(-1), [dict(W=W, N=W.shape[0], y_f32=True)], nf4=False)
            return y.view(1, -1)
        if self.rows and W.dtype == x.dtype and W.shape[1] <= 16384:
            launch = _dk.gemv_rows if self.B <= _dk.MAX_ROWS else _dk.gemv_rows64
            (y,) = launch(x, [dict(W=W, N=W.shape[0], y_f32=True)], nf4=False)
            return y
        return (x @ W.t().to(x.dtype)).float()

    # ---- one token ----------------------------------------------------------------------------------------------------------
    def _linear(self, x, projs):
        """x [B, K] -> list of [B, N_i]."""
        if self.B == 1:
            return [y.view(1, -1) for y in _dk.linear_group(x, projs)]
        if self.rows:
            return _dk.linear_group_rows(x, projs)
        outs = []
        for p in projs:                           # batch > 1: the fused small-M NF4 GEMM (utils.py:1095-1097 does dequant + matmul)
            y = matmul_lora(x, p[0], p[1], p[2], p[3], p[4])
            if len(p) > 5 and p[5] is not None:
                y = y + p[5]
            outs.append(y)
        return outs

    @torch.no_grad()
    def _step_body(self):
        if self.B == 1 and FUSED_STEP and self.kv_cache_dtype is None:       # (the single-launch attention reads a 16-bit cache)
            return self._step_body_fused()
        return self._step_body_plain()

    @torch.no_grad()
    def _step_body_fused(self):
        """One token of one sequence, 5 launches per decoder layer: q|k|v (residual add + RMSNorm inside), attention (RoPE,
        cache append and the split combine inside), o, gate|up (add + RMSNorm in, SwiGLU out), down; every LoRA `A x` inside
        the GEMV launch that consumes it."""
        H = self.cfg.hidden_size
        core = self.core
        resid = core.embed_tokens(self.tok).to(self.dtype).view(H)
        delta = None
        I = self.cfg.intermediate_size
        kw = dict(dtype=self.dtype, device=self.dev)
        nf4 = self._params[0]["gu"][0][1] is not None
        glu_ok = H <= (8192 if nf4 else 4096)            # a wave needs the gate row and the up row of an n in one trip
        for li in range(len(core.layers)):
            P = self._params[li]
            qkv = torch.empty(1, (self.Hq + 2 * self.Hk) * self.D, **kw)
            h = torch.empty_like(resid) if delta is not None else None
            site = 5 * li + 1                       # launch-site constants of the hand-off tags: 5 per layer
            _dk.linear_group(delta, P["qkv"], out=qkv.view(-1), fused=dict(mode=2, res=resid, norm_w=P["ln1"][0], eps=P["ln1"][1],
                                                                           h_out=h, sync=self.sync, site=site))
            if h is not None:
                resid = h
            a_out = torch.empty(1, self.Hq * self.D, **kw)
            _dk.attn_decode_fused(qkv, self.cos, self.sin, self.kv_len, self.k_cache[li], self.v_cache[li], a_out,
                                  self.fpartials, self.counters, self.fsplit, self.scale, self.Hq, window=self.window,
                                  site=site + 1)
            (o,) = _dk.linear_group(a_out.view(-1), P["o"], fused=dict(mode=0, sync=self.sync, site=site + 2))
            h = torch.empty_like(resid)
            pre = dict(mode=2, res=resid, norm_w=P["ln2"][0], eps=P["ln2"][1], h_out=h, sync=self.sync, site=site + 3)
            if glu_ok:
                (hmid,) = _dk.linear_group(o, P["gu"], fused=dict(pre, glu=True))
                (delta,) = _dk.linear_group(hmid, P["down"], fused=dict(mode=0, sync=self.sync, site=site + 4))
            else:
                gu = torch.empty(2 * I, **kw)
                _dk.linear_group(o, P["gu"], out=gu, fused=pre)
                (delta,) = _dk.linear_group(gu[:I], P["down"], fused=dict(mode=1, x2=gu[I:], sync=self.sync, site=site + 4))
            resid = h
        W = self._head
        if W.dtype == self.dtype and W.shape[1] <= 16384:
            (y,) = _dk.gemv(delta, [dict(W=W, N=W.shape[0], y_f32=True)], nf4=False,
                            pro=dict(mode=2, res=resid, norm_w=core.norm.weight, eps=_eps(core.norm), h_out=None))
            self.logits = y.view(1, -1)
        else:
            _, xn, _ = add_rms_fwd(delta.view(1, H), resid.view(1, H), core.norm.weight, _eps(core.norm))
            self.logits = self._lm_head(xn)
        self._pos.add_(1)                                   # positions and the step counter
        if self._sample is None:
            self._greedy()
        else:
            self.draw()
        return self.logits

    @torch.no_grad()
    def _step_body_plain(self):
        B, H = self.B, self.cfg.hidden_size
        core = self.core
        h = core.embed_tokens(self.tok).to(self.dtype).view(B, H)
        resid, delta = h, None
        for li in range(len(core.layers)):
            P = self._params[li]
            if delta is None:
                x = rms_fwd(resid, *P["ln1"])[0]
            else:
                resid, x, _ = add_rms_fwd(delta, resid, *P["ln1"])
            if B == 1:
                qkv = torch.empty(1, (self.Hq + 2 * self.Hk) * self.D, dtype=self.dtype, device=self.dev)
                _dk.linear_group(x, P["qkv"], out=qkv.view(-1))
            elif self.rows:                       # q | k | v straight into the fused row
                qkv = torch.empty(B, (self.Hq + 2 * self.Hk) * self.D, dtype=self.dtype, device=self.dev)
                _dk.linear_group_rows(x, P["qkv"], out=qkv)
            else:
                qkv = torch.cat(self._linear(x, P["qkv"]), dim=1)
            a_out = torch.empty(B, self.Hq * self.D, dtype=self.dtype, device=self.dev)
            if self.kv_cache_dtype == "fp8":
                _dk.rope_kv_append_fp8(qkv, self.cos, self.sin, self.kv_len, self.k_cache[li], self.v_cache[li],
                                       self.k_scale[li], self.v_scale[li], self.Hq, self.Hk, self.D)
                _dk.attn_decode_fp8(qkv[:, :self.Hq * self.D], self.k_cache[li], self.v_cache[li], self.k_scale[li],
                                    self.v_scale[li], self.kv_len, a_out, self.partials, SPLIT_KEYS, self.scale, len_add=1,
                                    window=self.window)
            elif self.share_prompt:                 # slot new_len[b] of the row's suffix, RoPE position = the total length
                _dk.rope_kv_append(qkv, self.cos, self.sin, self.new_len, self.k_cache[li], self.v_cache[li],
                                   self.Hq, self.Hk, self.D, rope_pos=self.kv_len)
                _dk.attn_decode_shared(qkv[:, :self.Hq * self.D], self.pk[li], self.pv[li], self.prompt_len, self.share_prompt,
                                       self.k_cache[li], self.v_cache[li], self.new_len, a_out, self.partials, SPLIT_KEYS,
                                       self.scale, len_add=1, window=self.window)
            else:
                _dk.rope_kv_append(qkv, self.cos, self.sin, self.kv_len, self.k_cache[li], self.v_cache[li],
                                   self.Hq, self.Hk, self.D)
                _dk.attn_decode(qkv[:, :self.Hq * self.D], self.k_cache[li], self.v_cache[li], self.kv_len, a_out,
                                self.partials, SPLIT_KEYS, self.scale, len_add=1, window=self.window)
            (o,) = self._linear(a_out, P["o"])
            resid, x, _ = add_rms_fwd(o, resid, *P["ln2"])
            gate, up = self._linear(x, P["gu"])
            hmid = swiglu_fg_kernel(gate.view(B, 1, -1), up.view(B, 1, -1)).view(B, -1)
            (delta,) = self._linear(hmid, P["down"])
        _, xn, _ = add_rms_fwd(delta, resid, core.norm.weight, _eps(core.norm))
        self.logits = self._lm_head(xn)
        self._pos.add_(1)                                   # positions and the step counter
        if self._sample is None:
            self._greedy()
        else:
            self.draw()
        return self.logits

    def step(self, token_ids):
        """Feed one token per sequence ([B] or [B, 1]); returns fp32 logits [B, V] for the next position."""
        self.tok.copy_(token_ids.view(self.B, 1))
        self._steps += 1
        if self._steps >= (1 << 22) - 8:                     # step * TAG_STRIDE would wrap: start the tags over on clean workspaces
            self.sync.ws.zero_()
            self.fpartials.ws.zero_()
            self.step_ctr.fill_(1)
            self._steps = 1
        if not self.use_graph:
            return self._step_body()
        # the greedy step and the sampled step are two captures (argmax against the draw and its counter); which one replays
        # follows `sampling()`, what the sampled one draws with follows the device parameter block
        g, gl = ("_graph", "_graph_logits") if self._sample is None else ("_graph_s", "_graph_s_logits")
        if getattr(self, g) is None:
            # eager warm-up (first-use attribute calls, allocator growth), with the position restored afterwards
            kv0, ctr0 = self._lens.clone(), self._draw_ctr.clone()
            self._step_body()
            self._lens.copy_(kv0)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._step_body()
            setattr(self, g, graph)
            setattr(self, gl, self.logits)       # the graph's static output buffer (prefill() rebinds self.logits)
            self._lens.copy_(kv0)                # the capture itself does not execute
            self._draw_ctr.copy_(ctr0)
        getattr(self, g).replay()
        self.logits = getattr(self, gl)
        return self.logits

    # ---- prompt-lookup decoding: K drafts from the sequence's own context, verified in one pass over the weights ----------------
    def _lookup_fallback(self, K, T, max_new_tokens, do_sample, attention_mask, eos):
        """Why a call with prompt_lookup_num_tokens = K runs the plain token steps instead (None: it takes the lookup path)."""
        if self.B != 1:
            return "more than one sequence"
        if do_sample:
            return "sampling"
        if self.kv_cache_dtype is not None:
            return "fp8 KV cache"
        if self.share_prompt is not None:
            return "shared prompt cache"
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            return "padded prompt"
        if not 1 <= K <= _dk.MAX_SPAN - 1:
            return f"prompt_lookup_num_tokens outside 1 .. {_dk.MAX_SPAN - 1}"
        if (K + 1) * (self.Hq // self.Hk) > 128:
            return "more than 128 query rows per KV head"
        if self.S < T + max_new_tokens + K:
            return "cache capacity below prompt + max_new_tokens + prompt_lookup_num_tokens"
        if eos is not None and len(eos) > _dk.MAX_EOS:
            return f"more than {_dk.MAX_EOS} eos ids"
        if self._head.dtype != self.dtype or self._head.shape[1] > 16384:
            return "lm_head outside uamd_gemv_rows"
        return None

    def _lookup_state(self):
        """Device state of the lookup path: hist [S] the sequence, state = (hist_len, remaining, done, n_draft), stats = (steps,
        drafted, accepted, tokens), tok / amax the token rows of a step and the arg-max of their logits, eos (-1: no id)."""
        if self._lk is None:
            R = _dk.MAX_SPAN
            z = lambda *shape, dtype=torch.long: torch.zeros(*shape, dtype=dtype, device=self.dev)
            self._lk = dict(hist=z(self.S), state=z(4, dtype=torch.int32), stats=z(4), tok=z(R), amax=z(R),
                            eos=torch.full((_dk.MAX_EOS,), -1, dtype=torch.long, device=self.dev),
                            partials=torch.empty(R, self.Hq, self.S // SPLIT_KEYS, self.D + 2, dtype=torch.float32, device=self.dev),
                            amax_ws=(torch.empty(R * 64, dtype=torch.float32, device=self.dev), z(R * 64)))
        return self._lk

    @torch.no_grad()
    def _lookup_body(self, R, n_max):
        """One verify step: draft -> the R token rows through every layer on ONE pass over the weights (uamd_gemv_rows; the span
        append and the span attention put row j at position kv_len + j) -> fp32 logits [R, V] -> arg-max per row -> accept.
        Everything it reads and advances is on the device."""
        lk, core = self._lk, self.core
        st = lk["state"]
        kw = dict(dtype=self.dtype, device=self.dev)
        _dk.ngram_draft(lk["hist"], st[0:1], R - 1, n_max, lk["tok"], st[3:4])
        resid, delta = core.embed_tokens(lk["tok"][:R]).to(self.dtype), None
        part = lk["partials"][:R]
        for li in range(len(core.layers)):
            P = self._params[li]
            if delta is None:
                x = rms_fwd(resid, *P["ln1"])[0]
            else:
                resid, x, _ = add_rms_fwd(delta, resid, *P["ln1"])
            qkv = torch.empty(R, (self.Hq + 2 * self.Hk) * self.D, **kw)
            _dk.linear_group_rows(x, P["qkv"], out=qkv)
            a_out = torch.empty(R, self.Hq * self.D, **kw)
            _dk.rope_kv_append_span(qkv, self.cos, self.sin, self.kv_len, self.k_cache[li], self.v_cache[li], R,
                                    self.Hq, self.Hk, self.D)
            _dk.attn_decode_span(qkv[:, :self.Hq * self.D], self.k_cache[li], self.v_cache[li], self.kv_len, R, a_out, part,
                                 SPLIT_KEYS, self.scale, window=self.window)
            (o,) = _dk.linear_group_rows(a_out, P["o"])
            resid, x, _ = add_rms_fwd(o, resid, *P["ln2"])
            gate, up = _dk.linear_group_rows(x, P["gu"])
            hmid = swiglu_fg_kernel(gate.view(R, 1, -1), up.view(R, 1, -1)).view(R, -1)
            (delta,) = _dk.linear_group_rows(hmid, P["down"])
        _, xn, _ = add_rms_fwd(delta, resid, core.norm.weight, _eps(core.norm))
        W = self._head
        (logits,) = _dk.gemv_rows(xn.view(R, -1), [dict(W=W, N=W.shape[0], y_f32=True)], nf4=False)
        _dk.argmax_f32(logits, out=lk["amax"][:R], ws=lk["amax_ws"])
        _dk.accept_greedy(lk["tok"], lk["amax"], R - 1, lk["eos"], lk["hist"], st[0:1], self.kv_len, st[1:2], st[2:3], st[3:4],
                          lk["stats"])
        self.step_ctr.add_(1)

    def _lookup_step(self, R, n_max):
        """`_lookup_body`, eagerly or as the replay of its capture (one per (R, n_max))."""
        self._steps += 1
        if not self.use_graph:
            return self._lookup_body(R, n_max)
        graph = self._graph_l.get((R, n_max))
        if graph is None:
            # eager warm-up, with every counter put back afterwards (the K / V it appended sit behind kv_len again)
            lk = self._lk
            saved = [(t, t.clone()) for t in (self._lens, lk["state"], lk["stats"])]
            self._lookup_body(R, n_max)
            for t, v in saved:
                t.copy_(v)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._lookup_body(R, n_max)
            self._graph_l[(R, n_max)] = graph
            for t, v in saved:                  # the capture itself does not execute
                t.copy_(v)
        graph.replay()

    @torch.no_grad()
    def _generate_lookup(self, input_ids, logits, max_new_tokens, eos, K, n_max):
        """The greedy tokens of the plain steps, several per pass over the weights where the drafts hit. hist = prompt + first
        token; every iteration is one verify step and ONE host read (done flag, hist_len)."""
        T = input_ids.shape[1]
        lk = self._lookup_state()
        hist, st = lk["hist"], lk["state"]
        first = torch.argmax(logits, dim=-1)                         # the first token: from the prefill logits, as today
        hist[:T].copy_(input_ids[0])
        hist[T:T + 1].copy_(first)
        lk["eos"].fill_(-1)
        if eos:
            lk["eos"][:len(eos)].copy_(torch.tensor(eos, device=self.dev))
        lk["stats"].zero_()
        done0 = torch.isin(first, lk["eos"]).to(torch.int32).view(1) if max_new_tokens > 1 else torch.ones(1, dtype=torch.int32, device=self.dev)
        st.copy_(torch.cat([torch.tensor([T + 1, max_new_tokens - 1], dtype=torch.int32, device=self.dev), done0, done0 * 0]))
        while True:
            hist_len, _, done, _ = st.tolist()                       # the loop's one sync per step
            if done:
                break
            self._lookup_step(K + 1, n_max)
        steps, drafted, accepted, tokens = lk["stats"].tolist()
        self.lookup_stats = dict(steps=steps, drafted=drafted, accepted=accepted, tokens=tokens, fallback=None)
        return hist[:hist_len].clone().view(1, -1)

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens=32, eos_token_id=None, do_sample=False, temperature=1.0, top_k=0,
                 generator=None, pad_token_id=None, top_p=1.0, min_p=0.0, attention_mask=None, num_return_sequences=1,
                 prompt_lookup_num_tokens=None, max_matching_ngram_size=2):
        """Greedy (default) or temperature / top-k / top-p / min-p sampling. Returns [B, T + new] token ids. Rows that have
        produced an end-of-sequence token keep emitting `pad_token_id` (default: the first eos id), like HF's generate.
        `attention_mask`: left-padded prompts (see `prefill`); the padded prompt is returned in front of the new tokens.
        `num_return_sequences` = n > 1 (sampling only): the engine's batch is B * n, every prompt is prefilled once and decoded
        as n adjacent rows that draw differently (the draw is keyed on the row) -- the tokens of the same call on
        input_ids.repeat_interleave(n, 0). An engine built with share_prompt = n takes exactly that n, and at most its suffix
        capacity of new tokens.
        Sampling happens on the device (uamd_sample_f32): one 64-bit seed per call is drawn from `generator` (the default
        generator of its device when None) without a sync, the first token is drawn from the prefill logits at draw 0 and every
        later one inside the token step, so equally seeded generators give equal tokens.
        `prompt_lookup_num_tokens` = K (1 .. 15; HF's keyword, with `max_matching_ngram_size`): one greedy sequence is decoded by
        verify steps -- the last token and K drafts that followed the latest earlier occurrence of the sequence's last n-gram
        go through the layers as K + 1 token rows on one pass over the weights, and the longest prefix of the drafts the model
        agrees with is kept (uamd_ngram_draft, uamd_attn_decode_span, uamd_accept_greedy). The tokens are those of the plain
        steps up to the rounding of a batched step against a single one; `lookup_stats` = steps / drafted / accepted / tokens of
        the call. A call outside the path's scope (`_lookup_fallback`) runs the plain steps and says why in
        `lookup_stats["fallback"]`; `lookup_stats` is None after a call without the keyword."""
        input_ids = input_ids.to(self.dev)
        n = int(num_return_sequences or 1)
        if n > 1 and not do_sample:
            raise ValueError("greedy decoding returns one sequence per prompt: num_return_sequences > 1 needs do_sample=True")
        eos = None if eos_token_id is None else sorted(set(eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id]))
        self.lookup_stats = None
        K = int(prompt_lookup_num_tokens or 0)
        if K:
            why = self._lookup_fallback(K, input_ids.shape[1], max_new_tokens, do_sample or n > 1, attention_mask, eos)
            if why is None and max_new_tokens < 1:
                why = "no new tokens"
            if why is None:
                logits = self.prefill(input_ids, attention_mask)
                self.sampling()
                return self._generate_lookup(input_ids, logits, int(max_new_tokens), eos, K, max(1, int(max_matching_ngram_size or 2)))
            self.lookup_stats = dict(steps=0, drafted=0, accepted=0, tokens=0, fallback=why)
        logits = self.prefill(input_ids, attention_mask, repeat=n)
        if n > 1:
            input_ids = input_ids.repeat_interleave(n, 0)
        if do_sample:
            gdev = generator.device if generator is not None else self.dev
            seed = torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64, device=gdev, generator=generator)
            self.sampling(max(temperature, 1e-6), top_k, top_p, min_p, seed=seed)
            self.draw()
        else:
            self.sampling()
        out = [input_ids]
        eos_t = None if eos is None else torch.tensor(eos, device=self.dev)
        pad = pad_token_id if pad_token_id is not None else (eos[0] if eos else 0)
        done = torch.zeros(self.B, dtype=torch.bool, device=self.dev)
        room = self.S_n if self.share_prompt else self.S - input_ids.shape[1]      # (a shared prompt: the suffix caches' slots)
        # a hand-off inside the fused decode launches that times out (csrc/decode.hip: a workgroup polled 2^18 times for a granule
        # that never came) poisons its output with NaN on purpose; NaN logits would otherwise turn into plausible-looking token ids
        # through argmax / multinomial. One element per row and token is accumulated (NaN * 0 = NaN) and looked at ONCE, after
        # the loop: no sync per token, and no silently wrong text.
        poison = torch.zeros(self.B, dtype=torch.float32, device=self.dev)
        for i in range(min(max_new_tokens, room)):
            poison += logits[:, 0].float() * 0.0
            if do_sample:
                nxt = self.next_tok.clone()                  # drawn from `logits` already: after prefill, or inside the step
            else:
                nxt = torch.argmax(logits, dim=-1)
            if eos_t is not None:
                nxt = torch.where(done, torch.full_like(nxt, pad), nxt)      # finished rows: padding from here on
            out.append(nxt.view(self.B, 1))
            if eos_t is not None:
                done |= torch.isin(nxt, eos_t)
                if bool(done.all()):
                    break
            if i + 1 < min(max_new_tokens, room):
                logits = self.step(nxt)
        self.sampling()
        if bool(torch.isnan(poison).any()):
            raise RuntimeError("unsloth_amd decode: non-finite logits -- an in-launch hand-off of the fused decode step timed out "
                               "(not every workgroup of a launch was resident: a CU-masked / shared GPU?) or the model produced "
                               "NaN / inf. UNSLOTH_AMD_DECODE_FUSED=0 runs the 14-launch step without hand-offs.")
        return torch.cat(out, dim=1)


def filter_logits(logits, top_k=0, top_p=1.0, min_p=0.0):
    """HF's warper order and rules (generation/logits_process.py TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper) on
    [B, V] logits: keep the top_k largest (ties with the k-th stay), then the smallest set of most probable tokens whose mass
    reaches top_p -- a token goes when the cumulative probability of it and everything LESS likely is <= 1 - top_p; the most
    likely token always stays -- then the tokens whose probability is at least min_p times the largest one. Everything else
    becomes -inf. The host statement of what uamd_sample_f32 keeps (the engine samples on the device and does not call this)."""
    if top_k and top_k < logits.shape[-1]:
        kth = torch.topk(logits, int(top_k), dim=-1).values[..., -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p is not None and top_p < 1.0:
        ascending, order = torch.sort(logits, descending=False, dim=-1)
        drop = ascending.softmax(dim=-1).cumsum(dim=-1) <= (1.0 - float(top_p))
        drop[..., -1:] = False
        logits = logits.masked_fill(drop.scatter(-1, order, drop), float("-inf"))
    if min_p is not None and min_p > 0.0:
        probs = logits.softmax(dim=-1)
        drop = probs < float(min_p) * probs.max(dim=-1, keepdim=True).values
        drop.scatter_(-1, logits.argmax(dim=-1, keepdim=True), False)
        logits = logits.masked_fill(drop, float("-inf"))
    return logits


def _eps(norm):
    return float(getattr(norm, "variance_epsilon", getattr(norm, "eps", 1e-6)))


# generate() arguments the decode engine implements itself; anything else a caller passes changes what HF's generate would
# return, so such calls go to the original `generate` (kept as `model._old_generate` by for_inference) instead of being
# silently ignored
_ENGINE_KWARGS = {"max_new_tokens", "max_length", "eos_token_id", "pad_token_id", "do_sample", "temperature", "top_k", "top_p",
                  "min_p", "attention_mask", "use_cache", "generator", "max_seq_len", "return_dict_in_generate", "output_scores",
                  "generation_config", "tokenizer", "num_return_sequences", "kv_cache_dtype", "share_prompt_cache",
                  "prompt_lookup_num_tokens", "max_matching_ngram_size"}


# generation_config fields the engine reads (below the explicit keywords, above the model's own generation config)
_CONFIG_FIELDS = ("max_new_tokens", "max_length", "eos_token_id", "pad_token_id", "do_sample", "temperature", "top_k", "top_p",
                  "min_p", "num_return_sequences", "prompt_lookup_num_tokens", "max_matching_ngram_size")
_NEUTRAL = {"repetition_penalty": (None, 1.0), "num_beams": (None, 1), "streamer": (None,), "num_return_sequences": (None, 1),
            "min_new_tokens": (None, 0), "return_dict_in_generate": (None, False), "output_scores": (None, False),
            "generation_config": (None,)}


def _config_fields(gc):
    """(fields the engine reads, names of the other fields that are set to something else than the class default) of a
    `generation_config=` object."""
    def public(o):
        d = o.to_dict() if hasattr(o, "to_dict") else dict(vars(o))
        return {k: v for k, v in d.items() if not k.startswith("_") and k != "transformers_version"}
    have = public(gc)
    try:
        base = public(type(gc)())
    except Exception:
        base = {}
    other = [k for k, v in have.items() if k not in _CONFIG_FIELDS and k not in ("use_cache",) and v != base.get(k, None)
             and not (k in _NEUTRAL and v in _NEUTRAL[k])]
    return {k: have[k] for k in _CONFIG_FIELDS if have.get(k, None) is not None}, other


def route_generate(model, input_ids, max_new_tokens, kwargs):
    """Where a `generate` call goes: ("old", reasons) -- HF's own generate -- or ("engine", settings): the keyword arguments of
    DecodeEngine.generate plus `batch` (rows the engine decodes: B x num_return_sequences) and `need` (padded prompt + new
    tokens). A left-padded attention_mask is the engine's when its masked positions hold the pad token (or no pad token is
    known). Explicit keywords win over `generation_config=`'s fields, those over the model's generation config. No GPU work:
    one host sync when an attention_mask with zeros has to be classified."""
    attention_mask = kwargs.get("attention_mask", None)
    lens = None
    reasons = []
    call_cfg, cfg_other = {}, []
    if kwargs.get("generation_config", None) is not None:
        call_cfg, cfg_other = _config_fields(kwargs["generation_config"])
    gen_cfg = getattr(model, "generation_config", None)
    if gen_cfg is None:
        gen_cfg = getattr(_base(model), "generation_config", None)
    eos, pad = kwargs.get("eos_token_id", None), kwargs.get("pad_token_id", None)
    for cfg in (call_cfg, gen_cfg):
        if eos is None and cfg is not None:
            eos = cfg.get("eos_token_id") if isinstance(cfg, dict) else getattr(cfg, "eos_token_id", None)
        if pad is None and cfg is not None:
            pad = cfg.get("pad_token_id") if isinstance(cfg, dict) else getattr(cfg, "pad_token_id", None)
    if attention_mask is not None and not bool(torch.all(attention_mask != 0)):
        # The engine takes PADDING: rows `[zeros | ones]` whose masked positions hold the pad token, as a tokenizer with
        # padding_side="left" writes them (no pad token known anywhere: the mask's word is taken). A mask that hides other
        # tokens is not padding; such calls stay with HF's generate, as every mask with a zero did before the engine had a
        # padded prefill.
        lens = left_pad_lengths(attention_mask)
        if lens is None or tuple(attention_mask.shape) != tuple(input_ids.shape):
            reasons.append("attention_mask that is not left-padded")
        elif isinstance(pad, int) and not bool((input_ids[(attention_mask == 0).to(input_ids.device)] == pad).all()):
            reasons.append("attention_mask that hides tokens other than the pad token")
            lens = None
    reasons += [k for k, v in kwargs.items()
                if (k not in _ENGINE_KWARGS and not (k in _NEUTRAL and v in _NEUTRAL[k]))
                or (k in ("return_dict_in_generate", "output_scores") and v)]
    reasons += [f"generation_config.{k}" for k in cfg_other]
    if reasons:
        return "old", reasons

    # Sampling defaults come from the model's generation_config like in HF's generate (a checkpoint that ships
    # do_sample=True / temperature / top_k / top_p / min_p -- Llama-3-Instruct's does -- samples without the caller saying so);
    # a generation_config= of the call stands above it, explicit keywords win.
    def gen_default(name, fallback):
        if name in kwargs and kwargs[name] is not None:
            return kwargs[name]
        if name in call_cfg:
            return call_cfg[name]
        v = getattr(gen_cfg, name, None) if (gen_cfg is not None and not call_cfg) else None
        return fallback if v is None else v
    if max_new_tokens is None:
        max_length = kwargs.get("max_length", None)
        if max_length is not None:
            max_new_tokens = max(int(max_length) - input_ids.shape[1], 0)
        else:
            max_new_tokens = call_cfg.get("max_new_tokens") or getattr(gen_cfg, "max_new_tokens", None) or 32
    do_sample = bool(gen_default("do_sample", False))
    n = int(kwargs.get("num_return_sequences", None) or call_cfg.get("num_return_sequences", None) or 1)
    if n > 1 and not do_sample:
        raise ValueError("greedy decoding returns one sequence per prompt: num_return_sequences > 1 needs do_sample=True")
    # prompt-lookup drafts (HF's two keywords / generation_config fields; None / 0: off): the engine verifies them for ONE greedy
    # sequence; anything else keeps HF's own assisted generation
    lookup = {}
    K = int(gen_default("prompt_lookup_num_tokens", 0) or 0)
    if K:
        if do_sample or input_ids.shape[0] * n > 1:
            return "old", ["prompt_lookup_num_tokens with " + ("do_sample" if do_sample else "more than one sequence")]
        lookup = dict(prompt_lookup_num_tokens=K, max_matching_ngram_size=int(gen_default("max_matching_ngram_size", 2) or 2))
    return "engine", dict(max_new_tokens=int(max_new_tokens), eos_token_id=eos, pad_token_id=pad, do_sample=do_sample,
                          temperature=float(gen_default("temperature", 1.0)),
                          top_k=int(gen_default("top_k", 0) or 0) if do_sample else 0,
                          top_p=float(gen_default("top_p", 1.0)) if do_sample else 1.0,
                          min_p=float(gen_default("min_p", 0.0) or 0.0) if do_sample else 0.0,
                          generator=kwargs.get("generator", None), attention_mask=attention_mask if lens is not None else None,
                          num_return_sequences=n, batch=input_ids.shape[0] * n,
                          need=input_ids.shape[1] + int(max_new_tokens) + K, **lookup)


def wanted_kv_cache(model, kv_cache_dtype=None):
    """The cache type a `generate` call decodes with: its `kv_cache_dtype=` keyword, else what `from_pretrained(...,
    float8_kv_cache=True)` / `for_inference(model, float8_kv_cache=True)` recorded on the model, else None (the activation
    type). An unknown string raises ValueError."""
    if kv_cache_dtype is not None:
        return kv_cache_kind(kv_cache_dtype)
    for m in (model, _base(model)):
        mark = getattr(m, "_uamd_float8_kv_cache", None)
        if mark is not None:
            return "fp8" if mark else None
    return None


def wanted_share_prompt(model, share_prompt_cache=None):
    """Whether a `generate` call with num_return_sequences = n > 1 keeps ONE prompt cache for the n samples of a prompt: its
    `share_prompt_cache=` keyword, else what `from_pretrained(..., share_prompt_cache=True)` / `for_inference(model,
    share_prompt_cache=True)` recorded on the model, else False."""
    if share_prompt_cache is not None:
        return bool(share_prompt_cache)
    for m in (model, _base(model)):
        mark = getattr(m, "_uamd_share_prompt_cache", None)
        if mark is not None:
            return bool(mark)
    return False


def unsloth_fast_generate(model, input_ids=None, max_new_tokens=None, max_seq_len=None, **kwargs):
    """llama.py:2167-2259 counterpart: `model.generate(...)` after `FastLanguageModel.for_inference(model)`.
    The reference forwards every keyword to HF's generate; the engine covers greedy / temperature / top-k / top-p / min-p
    decoding of unpadded and LEFT-padded batches (pad tokens under the mask's zeros), `num_return_sequences` when sampling, a `generation_config=` object
    whose other fields are at their defaults, and `prompt_lookup_num_tokens` / `max_matching_ngram_size` for one greedy sequence
    (DecodeEngine.generate; the engine's capacity grows by the K draft slots). Calls outside that (repetition_penalty, beams, streamers, logits processors, a
    right-padded or holey attention_mask, ...) are handed to HF's own generate (`model._old_generate`) -- or raise when it is
    unavailable. `share_prompt_cache=True` (the keyword, or the model's record: `wanted_share_prompt`) with
    num_return_sequences = n > 1: the engine is built with share_prompt = n -- one prompt cache for the n samples of a prompt;
    with n = 1 it does nothing."""
    input_ids = kwargs.pop("inputs", input_ids)
    kind = wanted_kv_cache(model, kwargs.pop("kv_cache_dtype", None))       # (the engine's own keyword: HF's generate has none)
    share = wanted_share_prompt(model, kwargs.pop("share_prompt_cache", None))      # (likewise)
    where, what = route_generate(model, input_ids, max_new_tokens, kwargs)
    if where == "old":
        old = getattr(model, "_old_generate", None)
        if old is None:
            raise NotImplementedError(f"unsloth_fast_generate: unsupported arguments {what}")
        return old(input_ids, max_new_tokens=max_new_tokens, **kwargs) if max_new_tokens is not None else old(input_ids, **kwargs)
    batch, need = what.pop("batch"), what.pop("need")
    eng = getattr(model, "_uamd_decode_engine", None)
    n = what["num_return_sequences"]
    if share and n > 1:
        # one prompt cache for the n samples of a prompt: prompt capacity >= T, suffix capacity >= the call's new tokens
        if kind == "fp8":
            raise NotImplementedError("share_prompt_cache together with kv_cache_dtype='fp8': the shared FP8 prompt cache is not built")
        T, new = input_ids.shape[1], need - input_ids.shape[1]
        if (eng is None or eng.B != batch or getattr(eng, "share_prompt", None) != n or eng.S < T or eng.S_n < new
                or getattr(eng, "kv_cache_dtype", None) is not None):
            eng = DecodeEngine(model, max_seq_len=max(T, max_seq_len or 0), batch=batch, share_prompt=n, max_new_tokens=max(new, 1))
            model._uamd_decode_engine = eng
        return eng.generate(input_ids, **what)
    if (eng is None or eng.B != batch or eng.S < need or getattr(eng, "kv_cache_dtype", None) != kind
            or getattr(eng, "share_prompt", None) is not None):
        # (kwargs only when asked for: the default engine is built exactly as before)
        eng = DecodeEngine(model, max_seq_len=max(need, max_seq_len or 0), batch=batch, **(dict(kv_cache_dtype=kind) if kind else {}))
        model._uamd_decode_engine = eng
    return eng.generate(input_ids, **what)


# ---- the reference's function names, for code written against unsloth/models/llama.py ----------------------------------------
def fast_rms_layernorm_inference(self, X, XX=None, XX2=None, variance=None):
    """llama.py:609-632 (the scratch arguments are accepted and unused: one kernel, statistics in registers)."""
    return rms_fwd(X, self.weight, _eps(self))[0].view(X.shape)


def fast_swiglu_inference(self, X, temp_gate=None, temp_up=None, gate_multiplier=None, down_multiplier=None):
    """llama.py:572-606: down(silu(gate(X)) * up(X)) for one token per sequence; gate | up are one grouped launch."""
    from ..kernels.utils import fast_linear_forward
    bsz, q_len, _ = X.shape
    if bsz == 1 and q_len == 1:
        gate, up = _dk.linear_group(X.reshape(-1), [get_lora_parameters_bias(self.gate_proj),
                                                    get_lora_parameters_bias(self.up_proj)])
        gate, up = gate.view(1, 1, -1), up.view(1, 1, -1)
    else:
        gate, up = fast_linear_forward(self.gate_proj, X), fast_linear_forward(self.up_proj, X)
    if gate_multiplier is not None:
        gate = gate * gate_multiplier
    h = swiglu_fg_kernel(gate, up)
    down = fast_linear_forward(self.down_proj, h)
    return down * down_multiplier if down_multiplier is not None else down


def LlamaAttention_fast_forward_inference(self, hidden_states, past_key_value, position_ids, do_prefill=False,
                                          attention_mask=None, rotary_seq_len=None):
    """llama.py:352-569: one new token per sequence against the KV cache. `past_key_value` = (K, V) [B, Hk, S, D] seeds the
    module's cache when `do_prefill` (allocated once at the model's max_seq_length instead of growing by
    KV_CACHE_INCREMENT); returns (attention output [B, 1, hidden], (K, V) views of the cache incl. the new token).
    Key-padding masks are not supported here (the training path handles them through SDPA)."""
    from . import llama as _ll
    from ..kernels.utils import fast_linear_forward
    if attention_mask is not None:
        raise NotImplementedError("decode attention takes no padding mask; left-pad-free batches only")
    cfg = self.config
    bsz = hidden_states.shape[0]
    Hq, Hk, D = cfg.num_attention_heads, cfg.num_key_value_heads, self.head_dim
    dev, dtype = hidden_states.device, hidden_states.dtype
    K1, V1 = past_key_value
    seq_len = K1.shape[-2]
    st = getattr(self, "_uamd_kv", None)
    if do_prefill or st is None or st["k"].shape[0] != bsz:
        S = int(math.ceil(max(getattr(self, "max_seq_length", 0) or 0, seq_len + 1, 2048) / SPLIT_KEYS) * SPLIT_KEYS)
        st = dict(k=torch.zeros(bsz, Hk, S, D, dtype=dtype, device=dev), v=torch.zeros(bsz, Hk, S, D, dtype=dtype, device=dev),
                  len=torch.zeros(bsz, dtype=torch.int32, device=dev),
                  part=torch.empty(bsz, Hq, S // SPLIT_KEYS, D + 2, dtype=torch.float32, device=dev))
        st["k"][:, :, :seq_len].copy_(K1)
        st["v"][:, :, :seq_len].copy_(V1)
        self._uamd_kv = st
    st["len"].fill_(seq_len)
    qkv = torch.cat([fast_linear_forward(p, hidden_states).view(bsz, -1) for p in (self.q_proj, self.k_proj, self.v_proj)], dim=1) \
        if bsz != 1 else torch.empty(1, (Hq + 2 * Hk) * D, dtype=dtype, device=dev)
    if bsz == 1:
        _dk.linear_group(hidden_states.reshape(-1), [get_lora_parameters_bias(p) for p in (self.q_proj, self.k_proj, self.v_proj)],
                         out=qkv.view(-1))
    if position_ids.dim() == 1:
        position_ids = position_ids[:, None]
    pos = position_ids[:, -1].to(device=dev, dtype=torch.int32).contiguous()
    tables = getattr(self, "_uamd_rope", None)
    if tables is None:
        tables = self._uamd_rope = _ll.RopeTables(cfg)
    cos, sin = tables.get(max(seq_len + 1, st["k"].shape[2]), dev, dtype)
    _dk.rope_kv_append(qkv, cos, sin, st["len"], st["k"], st["v"], Hq, Hk, D, rope_pos=pos)
    out = torch.empty(bsz, Hq * D, dtype=dtype, device=dev)
    _dk.attn_decode(qkv[:, :Hq * D], st["k"], st["v"], st["len"], out, st["part"], SPLIT_KEYS, 1.0 / math.sqrt(D),
                    len_add=1, window=int(getattr(cfg, "sliding_window", None) or 0))
    A = fast_linear_forward(self.o_proj, out.view(bsz, 1, Hq * D))
    return A, (st["k"][:, :, :seq_len + 1], st["v"][:, :, :seq_len + 1])
