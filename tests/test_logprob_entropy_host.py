"""CPU: the per-token entropy of the RL log-prob path is declared at every layer -- the C header and the ctypes table carry
`uamd_logprob_entropy_forward`, the two Python entry points take `return_entropy` (default off), and the driver no longer
holds the plain-torch entropy branch (an fp32 copy of lm_head and a torch softmax over fp32 logits)."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_ctypes_table_declare_the_entry():
    from unsloth_amd import _lib
    src = open(os.path.join(ROOT, "include", "unsloth_amd.h")).read()
    m = re.search(r"^int\s+uamd_logprob_entropy_forward\s*\(([^;]*)\)\s*;", src, flags=re.M)
    assert m, "include/unsloth_amd.h does not declare uamd_logprob_entropy_forward"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert "uamd_logprob_entropy_forward" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["uamd_logprob_entropy_forward"]
    assert res is _lib.c_int and len(args) == n_args == 12
    # the cross-entropy forward's arguments plus one output pointer (the entropy) after the logsumexp
    fwd = _lib.SIGNATURES["uamd_cross_entropy_forward"][1]
    assert args == fwd[:4] + [_lib.c_void_p] + fwd[4:]


def test_python_entry_points_take_return_entropy_default_off():
    from unsloth_amd.kernels import cross_entropy_loss as ce
    from unsloth_amd.models import rl_replacements as rl
    for fn in (rl.chunked_hidden_states_selective_log_softmax, rl.chunked_selective_log_softmax):
        p = inspect.signature(fn).parameters
        assert "return_entropy" in p and p["return_entropy"].default is False, fn.__name__
    assert list(inspect.signature(ce._logprob_entropy_forward).parameters) == ["logits2d", "index", "softcap", "scale"]


def test_driver_holds_no_torch_entropy_branch():
    src = open(os.path.join(ROOT, "unsloth_amd", "models", "rl_replacements.py")).read()
    assert "lm_head.float()" not in src and "torch.softmax" not in src and ".softmax(" not in src
