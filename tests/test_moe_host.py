"""The MoE expert block without a GPU: the patched Qwen3MoeExperts.forward leaves CPU tensors to the original, and the kernel
path refuses them like every other kernel."""
import pytest
import torch

from unsloth_amd.kernels import moe_experts_forward, patch_moe_experts
from unsloth_amd.models.llama import unpatch_all


def _experts_and_inputs():
    from transformers.models.qwen3_moe.configuration_qwen3_moe import Qwen3MoeConfig
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts
    cfg = Qwen3MoeConfig(hidden_size=64, moe_intermediate_size=64, num_experts=4, num_experts_per_tok=2, hidden_act="silu")
    cfg._experts_implementation = "eager"
    torch.manual_seed(0)
    experts = Qwen3MoeExperts(cfg).requires_grad_(False)
    for p in experts.parameters():
        p.copy_(torch.randn_like(p) / 8)
    idx = torch.stack([torch.randperm(4)[:2] for _ in range(10)])
    return experts, torch.randn(10, 64), idx, torch.rand(10, 2)


def test_patched_forward_on_cpu_tensors_is_the_original():
    experts, x, idx, w = _experts_and_inputs()
    want = experts(x, idx, w)
    try:
        patch_moe_experts()
        got = experts(x, idx, w)
    finally:
        unpatch_all()
    assert torch.equal(got, want)


def test_kernel_path_refuses_cpu_tensors():
    experts, x, idx, w = _experts_and_inputs()
    with pytest.raises(RuntimeError, match="MI355X"):
        moe_experts_forward(x.bfloat16(), experts.gate_up_proj.bfloat16(), experts.down_proj.bfloat16(), idx, w.bfloat16())
