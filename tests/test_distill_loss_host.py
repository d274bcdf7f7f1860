"""CPU: the distillation loss is declared at every layer -- the C header and the ctypes table carry the two entry points with
matching argument counts -- and its Python entries check their scalars and refuse to run without a GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,n_args", [("uamd_distill_loss_forward", 16), ("uamd_distill_loss_backward", 17)])
def test_header_and_ctypes_table_declare_the_entry(name, n_args):
    from unsloth_amd import _lib
    src = open(os.path.join(ROOT, "include", "unsloth_amd.h")).read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", src, flags=re.M)
    assert m, f"include/unsloth_amd.h does not declare {name}"
    res, args = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(args) == len([a for a in m.group(1).split(",") if a.strip()]) == n_args


@pytest.mark.parametrize("kw", [dict(beta=-0.1), dict(beta=1.5), dict(temperature=0.0), dict(temperature=-1.0),
                                dict(temperature=float("inf"))])
def test_scalars_out_of_range_raise(kw):
    from unsloth_amd.kernels import Fast_DistillationLoss, fast_generalized_jsd_loss
    from unsloth_amd.models.rl_replacements import chunked_hidden_states_distillation_loss
    x = torch.randn(2, 3, 16)
    with pytest.raises(ValueError):
        fast_generalized_jsd_loss(x, x.clone(), **kw)
    with pytest.raises(ValueError):
        Fast_DistillationLoss.apply(x[0], x[1], None, kw.get("beta", 0.5), kw.get("temperature", 1.0))
    with pytest.raises(ValueError):
        chunked_hidden_states_distillation_loss(x, x.clone(), torch.randn(8, 16), torch.randn(8, 16), **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_cpu_fallback():
    from unsloth_amd.kernels import fast_generalized_jsd_loss
    from unsloth_amd.models.rl_replacements import chunked_hidden_states_distillation_loss
    x = torch.randn(2, 3, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        fast_generalized_jsd_loss(x, x.clone())
    with pytest.raises(RuntimeError, match="MI355X"):
        chunked_hidden_states_distillation_loss(x, x.clone(), torch.randn(8, 16), torch.randn(8, 16))
