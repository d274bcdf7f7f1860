"""Host checks of the fused linear + cross-entropy edge cases (tests/_linear_ce.py; the GPU side is
tests/test_gpu_linear_ce_edges.py).

The GPU tests hold every token row of d(hidden) and every vocabulary row of dW to `err <= BOUND_FACTOR x the rounding model's
err` against an fp64 truth, and every checked row loss to the bound b_r. Here the reference side alone is shown to carry that:
the inputs put the softmax mass on the edge columns and make one row pad-sensitive, the truth agrees with fp64 autograd, the
rounding model's error has the size of 16-bit rounding on every slice and is exactly zero where the truth is, its own row
losses stay inside b_r, and every wrong variant (tests/_linear_ce.py `mutants`) is rejected by the very checks the GPU test
applies. These are conditions on the CASES and the yardstick -- a case that misses one is changed, never the mutant list or a
factor."""
import math

import pytest
import torch

from tests import _linear_ce as C

ALL = list(C.CASES)
EDGE_MASS_MIN = 0.2
# The rounding model's error per slice, relative to the slice's norm, measured on the CPU over the whole table (printed by the
# test): d(hidden) rows 1.9e-3 .. 1.7e-2 in bf16 and 3.2e-4 .. 2.8e-3 in fp16, dW rows 1.9e-3 .. 9.6e-3 in bf16 and 2.6e-4 ..
# 3.2e-2 in fp16 (dlogits / n_items of an ordinary column at V = 8200 is a SUBNORMAL fp16 number: 2^-24 absolute steps, and
# a dW row is a sum of such numbers that nearly cancels). The band: from a tenth of the relative error of one rounding
# (2^-9 / 2^-12) to 16 (bf16) / 256 (fp16) of them.
BAND = {"bf16": (0.1 * 2.0 ** -9, 16 * 2.0 ** -9), "fp16": (0.1 * 2.0 ** -12, 256 * 2.0 ** -12)}


def test_the_table_covers_what_it_has_to():
    cs = list(C.CASES.values())
    assert {1000, 1003, 1024, 8200, 8197} <= {c["V"] for c in cs}
    for V in (8200, 1003):
        assert {"bf16", "fp16"} <= {c["dtype"] for c in cs if c["V"] == V}
    assert {"on", "off"} <= {c["mode"] for c in cs if c["V"] == 1003 and c["softcap"]}
    assert any(c["scale"] and not c["softcap"] for c in cs) and any(c["V"] == 8197 and c["softcap"] for c in cs)
    assert any(c["chunk_rows"] >= C.T for c in cs) and any(isinstance(c["n_items"], tuple) for c in cs)
    assert any(c["mask"] and c["view"] for c in cs) and any(c["n_items"] is None for c in cs)
    assert any(c["dh"] == "nn_256" and not c["wt"] for c in cs)
    for c in cs:
        assert (c["logits"], c["dh"], c["wt"]) == C.routes_of(c["mode"], c["V"]), c["name"]
    # the chunks 64 | 64 | 64 | 2, the edge rows on and beside their edges, no special row used twice or dead
    assert [min(C.CHUNK, C.T - r) for r in range(0, C.T, C.CHUNK)] == [64, 64, 64, 2]
    assert {63, 64, 65, 127, 128, 191, 192} <= set(C.EDGE_ROWS)
    special = list(C.EDGE_ROWS) + [C.PAD_ROW] + list(C.INTERIOR_ROWS)
    dead = set(C.DEAD_ROWS) | set(C.MASKED_ROWS) | {C.L - 1, C.T - 1}
    assert len(set(special)) == len(special) and not set(special) & dead and len(C.MASKED_ROWS) >= 10
    assert C.edge_columns(1003) == [0, 7, 8, 999, 1000, 1002] and C.edge_columns(1024) == [0, 7, 8, 1023]
    assert C.edge_columns(8200) == [0, 7, 8, 8199, 8191, 8192] and C.edge_columns(8197) == [0, 7, 8, 8191, 8192, 8196]


@pytest.mark.parametrize("name", ALL)
def test_the_mass_sits_on_the_edges(name):
    """In the fp64 truth every edge column holds at least EDGE_MASS_MIN of its row's softmax, as a label and beside one; the
    pad-sensitive row has every logit below -9, so that zero padding columns would take nearly all of its mass; dead rows are
    the two last positions, the -100 labels and the masked rows."""
    c = C.build_case(name)
    tr = c["truth"]
    h, W, labels, mask = C.case_inputs(name)
    lab = C.shifted(labels, mask)
    mass = {}
    for e, r, is_label in C.edge_uses(c["V"]):
        assert bool(tr["live"][r]) and (int(lab[r]) == e) == is_label, (e, r)
        mass[(e, r)] = float(tr["p"][r, e])
    print(name, "edge mass:", {k: round(v, 2) for k, v in mass.items()})
    assert min(mass.values()) >= EDGE_MASS_MIN, mass
    if c["V"] % 8:
        z = h[C.PAD_ROW].double() @ W.double().t()
        s = c["scale"] or 1.0
        t = c["softcap"] * torch.tanh(s * z / c["softcap"]) if c["softcap"] else s * z
        stolen = (c["V"] + 7) // 8 * 8 - c["V"]
        share = stolen / (stolen + float(t.exp().sum()))
        print(name, "pad row: max logit", float(t.max()), "share of the padding if counted", share)
        assert float(t.max()) < -9.0 and share > 0.9
    dead = ~tr["live"]
    want = set(C.DEAD_ROWS) | {C.L - 1, C.T - 1} | (set(C.MASKED_ROWS) if c["mask"] else set())
    assert set(torch.nonzero(dead).flatten().tolist()) == want
    assert float(tr["dh"][dead].abs().max()) == 0.0 and float(tr["dh"][~dead].norm(dim=1).min()) > 0.0


@pytest.mark.parametrize("name", ["v1000-scale", "v1003-cap", "v1024-cap-scale-mask-view-nn"])
def test_truth64_agrees_with_fp64_autograd(name):
    """The hand-written gradient formulas of the truth against torch.autograd on F.cross_entropy in fp64."""
    c = C.build_case(name)
    h, W, labels, mask = C.case_inputs(name)
    h64, W64 = h.double().requires_grad_(True), W.double().requires_grad_(True)
    z = h64 @ W64.t()
    if c["scale"]:
        z = c["scale"] * z
    if c["softcap"]:
        z = c["softcap"] * torch.tanh(z / c["softcap"])
    lab = C.shifted(labels, mask)
    rows = torch.nn.functional.cross_entropy(z, lab, ignore_index=-100, reduction="none")
    loss = rows.sum() / C.n_items_value(c, int((lab != -100).sum()))
    (loss * C.UPSTREAM).backward()
    tr = c["truth"]
    assert abs(float(loss.detach()) - float(tr["loss"])) <= 1e-12 * abs(float(tr["loss"]))
    assert float((rows.detach() - tr["row_loss"]).abs().max()) <= 1e-12
    for t, g in (("dh", h64.grad), ("dW", W64.grad)):
        assert float((g - tr[t]).norm()) <= 1e-12 * float(tr[t].norm()), t


@pytest.mark.parametrize("name", ALL)
def test_the_yardstick_is_usable(name):
    """The rounding model's error per slice: exactly zero where the truth is zero, positive elsewhere and within BAND x the
    slice's norm; its own row losses within b_r."""
    c = C.build_case(name)
    tr, lo_hi = c["truth"], BAND[c["dtype"]]
    for t in C.TENSORS:
        assert c["model"][t].shape == tr[t].shape and bool(torch.isfinite(c["model"][t]).all())
        err, norm = c["model_err"][t], tr[t].norm(dim=1)
        assert bool((err[norm == 0] == 0).all()), t
        rel = err[norm > 0] / norm[norm > 0]
        print(name, t, "model error / ||slice||: %.2e .. %.2e" % (float(rel.min()), float(rel.max())))
        assert lo_hi[0] <= float(rel.min()) and float(rel.max()) <= lo_hi[1], (t, float(rel.min()), float(rel.max()))
    live = tr["live"]
    d = (c["model"]["row_loss"] - tr["row_loss"]).abs()
    frac = d[live] / tr["b"][live]
    half = d[live] / ((tr["b"][live] - C.LOSS_FP32) / 2 + C.LOSS_FP32)
    print(name, "model row loss: worst %.2f of b_r, %.2f of the half-ulp bound" % (float(frac.max()), float(half.max())))
    assert float(frac.max()) <= 1.0
    assert bool((c["model"]["row_loss"][~live] == 0).all())
    assert abs(float(c["model"]["loss"] - tr["loss"])) <= float(tr["b"][live].sum()) / tr["n"]


def _rejected(c, res):
    """By which of the GPU test's checks a result is rejected, [] when it passes them all (MAX_FACTOR for the gradients: the
    largest factor any tensor may ever be given)."""
    tr, why = c["truth"], {}
    for t in C.TENSORS:
        ratio = C.judge(c, t, res[t])[2]
        if ratio > C.MAX_FACTOR:
            why[t] = ratio
    live = tr["live"]
    frac = (res["row_loss"] - tr["row_loss"]).abs()[live] / tr["b"][live]
    if float(frac.max()) > 1.0:
        why["row_loss"] = float(frac.max())
    if bool((res["row_loss"][~live] != 0).any()):
        why["dead_row_loss"] = math.inf
    return why


@pytest.mark.parametrize("name", ALL)
def test_every_mutant_is_rejected(name):
    c = C.build_case(name)
    assert not _rejected(c, c["model"])
    seen = {m: _rejected(c, C.rounding_model(name, m)) for m in C.mutants(name)}
    print(name, {m: {k: round(v, 1) for k, v in w.items()} for m, w in seen.items()})
    for m, why in seen.items():
        assert why, m


def test_mutants_apply_where_they_should():
    ms = {n: set(C.mutants(n)) for n in ALL}
    assert all({"drop_last_col", "label_plus1", "no_shift"} <= m for m in ms.values())
    for n, c in C.CASES.items():
        assert ("pad_counted" in ms[n]) == bool(c["V"] % 8) and ("dw_tail_unscaled" in ms[n]) == (c["V"] > 8192)
        assert ("chunk_last_row" in ms[n]) == ("dw_overwrite" in ms[n]) == (c["chunk_rows"] < C.T)
        assert ("no_cap_deriv" in ms[n]) == bool(c["softcap"]) and ("scale_factor_missing" in ms[n]) == bool(c["scale"])
        assert ("mask_ignored" in ms[n]) == c["mask"] and ("n_items_ignored" in ms[n]) == (c["n_items"] is not None)
    assert set().union(*ms.values()) == {"drop_last_col", "pad_counted", "label_plus1", "no_shift", "chunk_last_row",
                                         "dw_overwrite", "dw_tail_unscaled", "no_cap_deriv", "scale_factor_missing",
                                         "mask_ignored", "n_items_ignored"}


def test_judge_on_hand_written_rows():
    c = C.build_case("v1000")
    for t in C.TENSORS:
        err, model, ratio, ok = C.judge(c, t, c["model"][t])
        assert ok and ratio <= 1.0 and torch.equal(err, model)
    dead = C.DEAD_ROWS[0]
    assert float(c["truth"]["dh"][dead].abs().max()) == 0.0 and float(c["model"]["dh"][dead].abs().max()) == 0.0
    dust = c["model"]["dh"].clone()
    dust[dead, 0] = 1e-30
    assert not C.judge(c, "dh", dust)[3] and C.judge(c, "dh", dust)[2] == float("inf")
    assert C.row_err(torch.tensor([[3.0, 4.0], [0.0, 1.0]]), torch.zeros(2, 2, dtype=torch.float64)).tolist() == [5.0, 1.0]
