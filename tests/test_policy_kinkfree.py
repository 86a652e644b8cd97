"""te_policy_ppo_grad_shaped and te_policy_act_shaped held to fp64, per packed tensor, on inputs that have no kink.

tests/test_policy_grad.py and tests/test_policy_grad_shapes.py allow every tensor 1e-4 ||g||_inf + 1e-6 + 0.02 / B against fp32 autograd; the
last term, one row's share of the gradient at a ReLU kink, exceeds the norm of a third of the tensors at B = 33 and of nearly all at B = 1.
Here the inputs are built so that there is no kink to excuse (tests/_kinkfree.py): the bias of every ReLU unit is moved into the widest
gap of its own pre-activations over the rows of the case, so no row lies near 0 and about half the units stay active, and old_logp is
set so that the ratios are e^-0.5, e^-0.05, e^0.05, e^0.5 in turn, on both sides of the clip and at least 0.149 from 0.8 and 1.2.  The
conditions (CPU, fp64 on the fp32-rounded weights and inputs, test_fixture_conditions): every |pre-activation| >= 1e-4 (>= 2e-5 at
2 081 rows), 25 % to 75 % of every layer active, every ratio >= 0.1 from either threshold.

The bound comes from a pair of CPU references and never from the kernel.  g64 is autograd through the module in fp64, g32 in fp32, both
on the same fp32 values and with the same (mean, std) of the advantage as constants.  Per packed tensor t:
    E_t = max |g32 - g64|,  bound_t = 16 max(E_t, 2^-23 ||g64_t||_inf),  |kernel - g64| <= bound_t for every element;
a tensor whose fp64 gradient is identically zero must be exactly zero; pg, vl and ent by the same rule as scalars; clip_frac must be the
fp64 count of clipped rows over B (to the two roundings of an fp32 mean).  16: the kernel's order (sequential k inside the MFMA, split-K
partials) differs from both references, the device's tanhf and expf are a little less exact than the host's, and a maximum over up to
10^6 elements is heavy-tailed; the floor keeps four-element tensors from being judged against a lucky E_t.
test_the_reference_pair_agrees holds a third evaluation, fp32 with the units of every hidden layer permuted, to half of that bound.
Two places where that rule, taken by the letter, contradicts a CPU reference, and what holds instead (both found on the CPU pair or
reproduced there, neither fitted to the kernel):
  * pg is what is left of terms of both signs, so its floor is 2^-23 of the mean |term| and not of |pg|: the permuted reference sat at
    9 x E of the literal rule (default, C = 3, B = 16), beyond the half it must keep to.  vl's and ent's terms have one sign: no change.
  * The sums that run over the rows alone (every bias, log_std, pg, vl, ent) the kernel forms as the ones-column of its split-K GEMM,
    one fp32 accumulator per slice of 2 048 rows, row after row; PyTorch's CPU sums are cascaded.  A fourth reference sums the fp32
    per-row terms in exactly that order (tests/_kinkfree.py _strict_row_sums), and E_t of these tensors is the larger of its gap and
    g32's.  test_strict_row_order_needs_its_room: at 2 081 rows the strict sum of the rows' equal entropies is 41 x the literal rule's
    max(E, floor) from fp64, and value.bias 25 to 73 x; at 33 rows it needs no room.  The weight tensors keep g32's E_t alone.
test_the_bound_bites_where_the_old_one_does_not puts on record what the old bound let through.
The forward (mu, value of te_policy_act_shaped) by the same rule, with E over both outputs of the case and the floor 2^-23 of the
largest |output|.

Cases (FusedPolicy.ppo_grad, all three served shapes): C = 3 at B = 1, 16, 17, 32, 33, 33 of 80 stored rows through an index with
duplicates, and 2 081 (two split-K slices for the one-position layers, 13 for conv1); C = 2 at 17 and 33.

Measured on the MI355X (profiles/policy_kinkfree.json), the worst gap / max(E_t, floor) over the cases of a shape, against the 16 allowed:
  gradient and statistics: default 8.7 (value.bias, C = 3, B = 33; weight tensors 4.6), reference BO 6.2 (value.weight, B = 1), reference
  learn 5.6 (pi.4.weight, B = 1); forward: default 5.2, reference BO 7.3, reference learn 6.4.  Under the literal rule the same run missed
  only at 2 081 rows, in all three shapes: ent at 40.9 x (exactly the strict row order's CPU figure) and value.bias at 19 to 47 x.

TE_POLICY_KINKFREE_RECORD=<path>: every GPU case appends one JSON line (the case, the fixture's margins, per tensor E_t, bound_t and
the kernel's largest gap, the worst ratio)."""
import json
import os

import pytest

from tests import _kinkfree as K
from tests._policy_cases import _gpu

CASES = {3: [(1, None), (16, None), (17, None), (32, None), (33, None), (33, 80), (2081, None)], 2: [(17, None), (33, None)]}
INSTANCES = [(name, c) for name in K.SHAPES for c in (3, 2)]
OLD_REL, OLD_ABS, OLD_KINK = 1e-4, 1e-6, 0.02      # tests/test_policy_grad.py


def _label(fx):
    c = fx["case"]
    return f"{c['shape']} C={c['C']} B={c['B']}" + (f" of {c['stored']} stored" if c["stored"] else "")


# ---------------------------------------------------------------------------------------------------------- no GPU needed
@pytest.mark.parametrize("name,c", INSTANCES)
def test_fixture_conditions(name, c):
    """What "kink-free" rests on, before anything runs on a GPU."""
    for rows, stored in CASES[c]:
        fx = K.fixture(name, c, rows, stored)
        m = fx["margins"]
        print(f"\n{_label(fx)}: {json.dumps(m)}")
        assert m["min_abs_preactivation"] >= (1e-4 if rows <= 33 else 2e-5), (_label(fx), m)
        assert 0.25 <= m["active_share_min"] and m["active_share_max"] <= 0.75, (_label(fx), m)
        assert m["ratio_distance"] >= 0.1, (_label(fx), m)
        if rows >= 16:
            assert 0.25 <= m["clip_frac"] <= 0.75, (_label(fx), m)                  # both clip branches
            assert fx["ms"] is not None and fx["ms"].dtype.is_floating_point and fx["ms"].element_size() == 4
        else:
            assert m["clip_frac"] == 0.0 and fx["ms"] is None and float(fx["g64"][-3].abs().max()) > 0.0      # mu.weight: not clipped away
        if stored:
            assert fx["index"].unique().numel() < rows                                # duplicates
        assert all(s > 0.0 for s in fx["scale"]), _label(fx)                          # no tensor's gradient vanishes


@pytest.mark.parametrize("name,c", INSTANCES)
def test_the_reference_pair_agrees(name, c):
    """The margin is sane: the same function in fp32 in another summation order (hidden units permuted, gradient un-permuted) stays
    within bound_t / 2 of g64, and E_t is a rounding error, not a disagreement."""
    import torch
    for rows, stored in CASES[c]:
        fx = K.fixture(name, c, rows, stored)
        gp, sp = K.permuted(name, c, rows, stored)
        half = dict(fx, bound=[b / 2 for b in fx["bound_pair"]], stat_bound=[b / 2 for b in fx["stat_bound_pair"]])       # of g32's own E_t
        bad, rec, worst = K.judge(half, gp, sp.float())
        rel = max(e / s for e, s in zip(fx["E"], fx["scale"]))
        print(f"\n{_label(fx)}: permuted fp32 at most {worst:.2f} x max(E_t, floor); largest E_t / ||g64_t|| {rel:.2e}")
        assert not bad, (_label(fx), bad)
        assert 0.0 < rel < 1e-4, (_label(fx), rel)
        assert any(not torch.equal(a, b) for a, b in zip(gp, fx["g32"])), _label(fx)      # it is another order


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_strict_row_order_needs_its_room(name):
    """Why E_t of the biases, log_std and the means also takes the strict row order's gap (tests/_kinkfree.py _strict_row_sums): at
    2 081 rows an fp32 sum of the rows' equal entropies, one addition per row in slices of 2 048, is further from fp64 than 16 x max(g32's
    gap, floor), on the CPU, before any kernel is asked.  At 33 rows it needs no room worth the name, so the bound stays what g32 sets."""
    at = K.fixture(name, 3, 33)["names"].index("value.bias")
    for rows, least, most in ((2081, 16.0, 64.0), (33, 0.0, 8.0)):
        fx = K.fixture(name, 3, rows)
        ratio = lambda strict, pair, scale: strict / max(pair, K.EPS32 * scale)
        ent = ratio(fx["stat_E_strict"][2], fx["stat_E_pair"][2], fx["stat_scale"][2])
        vb = ratio(fx["E_strict"][at], fx["E_pair"][at], fx["scale"][at])
        print(f"\n{_label(fx)}: strict row order / max(g32's gap, floor): ent {ent:.1f}, value.bias {vb:.1f}")
        assert least < ent < most, (_label(fx), ent)
        assert all((e is None) == (n.endswith(".weight")) for n, e in zip(fx["names"], fx["E_strict"]))      # weights keep g32's E_t alone


def _old_bound_accepts(fx, grads):
    rows = fx["case"]["B"]
    return all(float((k.double() - r).abs().max()) <= OLD_REL * float(r.abs().max()) + OLD_ABS + OLD_KINK / rows for k, r in zip(grads, fx["g32"]))


def test_the_bound_bites_where_the_old_one_does_not():
    """Three wrong gradients (reference BO, C = 3, B = 33) that the bound of tests/test_policy_grad.py accepts and this one rejects."""
    import torch
    fx = K.fixture("BO", 3, 33)
    clean = lambda: [g.float() for g in fx["g64"]]            # what a perfect fp32 kernel would return
    at = fx["names"].index
    bad, _, worst = K.judge(fx, clean(), fx["s64"].float())
    assert not bad and worst <= 1.0, (bad, worst)
    assert _old_bound_accepts(fx, clean())

    one = clean()                                             # one element at the tensor's median magnitude, zeroed
    t = one[at("inertial.0.weight")]
    i = t.abs().flatten().argsort()[t.numel() // 2]
    assert float(t.flatten()[i].abs()) > 0.0
    t.view(-1)[i] = 0.0
    rows = clean()                                            # two rows swapped
    t = rows[at("final.0.weight")]
    t[[3, 200]] = t[[200, 3]]
    cols = clean()                                            # a slice of columns off by 1e-4 of itself
    cols[at("pi.2.weight")][:, -16:] *= 1.0 + 1e-4
    for what, name, grads in (("element zeroed", "inertial.0.weight", one), ("rows swapped", "final.0.weight", rows), ("columns scaled", "pi.2.weight", cols)):
        bad, rec, _ = K.judge(fx, grads, fx["s64"].float())
        print(f"\n{what}: {name} gap {rec[name]['gap']:.3e}, bound_t {rec[name]['bound']:.3e}, old bound "
              f"{OLD_REL * fx['scale'][at(name)] + OLD_ABS + OLD_KINK / 33:.3e}, ||g|| {fx['scale'][at(name)]:.3e}")
        assert len(bad) == 1 and bad[0].startswith(name + ":"), (what, bad)
        assert _old_bound_accepts(fx, grads), what
    zeros = clean()                                           # and the issue's example: whole tensors returned as zeros pass the old bound
    for n in ("inertial.0.weight", "action.0.weight", "vf.0.weight"):
        zeros[at(n)].zero_()
    assert _old_bound_accepts(fx, zeros) and len(K.judge(fx, zeros, fx["s64"].float())[0]) == 3


# ---------------------------------------------------------------------------------------------------------- MI355X
def _record(rec):
    print("\n" + json.dumps(rec))
    if os.environ.get("TE_POLICY_KINKFREE_RECORD"):
        with open(os.environ["TE_POLICY_KINKFREE_RECORD"], "a") as f:
            f.write(json.dumps(rec) + "\n")


def _fused(torch, fx):
    import copy
    from dronechase_amd.ppo import FusedPolicy
    return FusedPolicy(copy.deepcopy(fx["policy"]).to("cuda:0"))


def _dev(d):
    return {k: v.to("cuda:0").contiguous() for k, v in d.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", INSTANCES)
def test_gradient_against_fp64(name, c):
    torch = _gpu()
    failures = []
    for rows, stored in CASES[c]:
        fx = K.fixture(name, c, rows, stored)
        fused = _fused(torch, fx)
        obs, ro = _dev(fx["obs"]), _dev(fx["ro"])
        index = None if fx["index"] is None else fx["index"].to("cuda:0")
        ms = None if fx["ms"] is None else fx["ms"].to("cuda:0")
        grad = torch.full_like(fused.params, float("nan"))
        stats = torch.full((4,), float("nan"), device="cuda:0")
        fused.ppo_grad(obs, index, ro["action"], ro["old_logp"], ro["adv"], ro["ret"], ms, K.CLIP, K.VF_COEF, K.ENT_COEF, grad, stats)
        torch.cuda.synchronize()
        bad, rec, worst = K.judge(fx, K.split(fx["policy"], grad.cpu()), stats.cpu())
        _record({"kernel": "te_policy_ppo_grad_shaped", "case": fx["case"], "margins": fx["margins"], "tensors": rec, "worst_gap_over_max_E_floor": worst})
        failures += [f"{_label(fx)}: {b}" for b in bad]
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("name,c", INSTANCES)
def test_forward_against_fp64(name, c):
    """mu and value of te_policy_act_shaped on the gathered rows of the same fixtures."""
    torch = _gpu()
    failures = []
    for rows, stored in CASES[c]:
        fx = K.fixture(name, c, rows, stored)
        sel = (lambda t: t) if fx["index"] is None else (lambda t: t[fx["index"]])
        mu, value = _fused(torch, fx).forward(_dev({k: sel(v) for k, v in fx["obs"].items()}))
        torch.cuda.synchronize()
        gap_mu, gap_v = (mu.cpu().double() - fx["mu64"]).abs().max(), (value.cpu().double() - fx["v64"]).abs().max()
        gap = float(torch.maximum(gap_mu, gap_v))
        floor = max(fx["out_E"], K.EPS32 * fx["out_scale"])
        _record({"kernel": "te_policy_act_shaped", "case": fx["case"], "margins": fx["margins"], "E": fx["out_E"], "bound": fx["out_bound"],
                 "gap_mu": float(gap_mu), "gap_value": float(gap_v), "largest_output": fx["out_scale"], "worst_gap_over_max_E_floor": gap / floor})
        if not gap <= fx["out_bound"]:
            failures.append(f"{_label(fx)}: |kernel - fp64| mu {float(gap_mu):.3e}, value {float(gap_v):.3e} > {fx['out_bound']:.3e}")
    assert not failures, "\n".join(failures)
