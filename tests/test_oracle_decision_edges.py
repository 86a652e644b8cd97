"""The crafted decision states of tests/_decision_states.py, checked WITHOUT a GPU, and the bound that tests/test_gpu_decision_edges.py holds the
step kernels to: the oracle's float32 / float64 pair on the same blobs.  Per (shape, family):
  * the float64 oracle decides as the sign of the numpy margin says (who is disarmed or respawned, done, info, the command words of a search, the
    reward term of a reward-only threshold); at margin 0 it takes the strict side: < for the ranges, > for the dome;
  * threshold families: state_margins() (margins() for the reward-only ones) equals the numpy margin of the env to 1e-12: the crafted decision
    is the env's least decidable one.  Tie and integer families: both are above 0.05 m;
  * no env advanced its round or ended for a reason other than the decision under test;
  * G of the case is printed; the pair agrees on every exact and integer env; at least 0.6 of the envs are held (margin above M, or exact);
  * each reward-only jump is at least 0.1 and at least 100 x the reward bar;
  * the fixture is identical when built twice."""
import numpy as np
import pytest

from dronechase_amd import config as K
from tests import _decision_states as S
from tests._blob import Blob

CASES = [(shape, family) for shape in S.SHAPES for family in S.families(shape)]


def _killed(before, after, e, j):
    """Slot j was disarmed by the step (stage02 re-arms it at a fresh position before the step ends)."""
    return not after.i(e, j, "ARMED") or not np.array_equal(after.f(e, j, "POS", 3), before.f(e, j, "POS", 3))


@pytest.mark.parametrize("shape,family", CASES)
def test_the_float64_oracle_decides_as_numpy_says(shape, family):
    r = S.reference(shape, family)
    c, out = r["case"], r["f64"]
    N, D, ctx = c["N"], c["D"], c["ctx"]
    fig = S.figures(c, r["pair_differs"])
    print(f"{shape}/{family}: N = {N}, G = {r['G']:.3g} m (family: {S.family_G(family):.3g} m), M <= {fig['M']:.3g} m, held = {fig['held_share']:.3f}, "
          f"the pair differs in {fig['disagreeing']} envs up to {fig['largest_disagreeing_margin']:.3g} m, agrees down to {fig['smallest_agreeing_margin']}")
    assert N % 64 != 0 and N <= 700 and c["real"].sum() >= 190
    assert not (r["pair_differs"] & c["exact"]).any(), "the oracle's two builds disagree on an exact or integer env"
    assert np.isfinite(r["G"]) and not fig["unexcused"] and fig["held_share"] >= 0.6
    assert fig["M"] < 3e-5, "M has reached the rungs that the 0.6 share counts on: add rungs, do not raise the factor"
    before, after = Blob(c["blob"], N, D), Blob(out["state"], N, D)
    sm, am = out["state_margins"], out["margins"]
    if family == "central":
        assert (am <= sm).all()
        return
    # (a rung of 0.1 or 0.3 m is larger than the 0.05 m that everything else keeps: there the oracle's figure is only known to be at least 0.05)
    small = np.array([len(w["under"]) > 0 for w in c["want"]]) & (c["margin"] < S.CLEAR)
    if family in S.THRESHOLD_FAMILIES:
        assert np.abs(sm[small] - c["margin"][small]).max(initial=0.0) < 1e-12 and small.sum() >= (0.5 * N if ctx.origin_rule or family != "origin_rim" else 0)
        assert (sm[~small] >= S.CLEAR).all() and (am >= np.minimum(sm, S.CLEAR)).all()
    elif family == "reward_edges":
        assert np.abs(am[small] - c["margin"][small]).max() < 1e-12 and small.sum() >= 0.5 * N and (sm >= S.CLEAR).all() and (am[~small] >= S.CLEAR).all()
    else:       # ties, integers: the oracle notes no margin for a search, and nothing else is near
        assert (sm >= S.CLEAR).all() and (am >= S.CLEAR).all()
    for e, w in enumerate(c["want"]):
        label = (e, w["tag"], c["margin"][e])
        for j, armed in w["want_armed"].items():
            assert _killed(before, after, e, j) == (not armed), label
        if w["want_done"] is not None:
            assert out["done"][e] == w["want_done"], label
        elif family in ("shoot_rim", "origin_rim", "catch_rim", "reward_edges") or w["tag"] == "quiet":
            assert out["done"][e] == 0, label
        if w["want_info"] is not None:
            assert tuple(out["info"][e]) == w["want_info"], label
        if not w.get("round_may_advance"):
            assert after.ei(e, "ROUND") == before.ei(e, "ROUND"), label
        elif not w["want_done"]:
            assert after.ei(e, "ROUND") == before.ei(e, "ROUND") + 1, label
        if w["want_dir"] is not None:        # the command words: set-point (vx, vy, 0, vz) = speed x the unit vector at the target
            slot, target = w["want_dir"]
            sp = after.f(e, slot, "SETPOINT", 4).astype(np.float64)
            u = (w["pos"][target] - w["pos"][slot]) / np.linalg.norm(w["pos"][target] - w["pos"][slot])
            got = np.array([sp[0], sp[1], sp[3]])
            assert got @ u / np.linalg.norm(got) > 0.9999, label
        if w["want_reward"] is not None:
            assert abs(float(out["reward"][e]) - w["want_reward"][0]) < 1e-3, label
    if family == "reward_edges":
        bar = S.REWARD_ATOL + S.REWARD_RTOL * float(np.abs(out["reward"]).max())
        assert c["jumps"] and all(j >= 0.1 and j >= 100 * bar for j in c["jumps"].values()), (c["jumps"], bar)
        for tag in c["jumps"]:       # both sides of every jump are there
            on = [w["want_reward"][1] for w in c["want"] if w["tag"] == tag]
            assert 0.3 < np.mean(on) < 0.7, tag
    # at margin 0 the strict side: d == range is no hit, |p| == dome_radius is inside
    for e in np.flatnonzero(c["rim_exact"]):
        w = c["want"][e]
        assert c["margin"][e] == 0.0, (e, w["tag"])
        if ctx.kind == "s02" and "/empty" in w["tag"]:      # (stage02's suicide rule removes the target of an empty gun inside SHOOT range)
            continue
        assert all(armed == 1 for armed in w["want_armed"].values()) and not w["want_done"] and (w["want_info"] is None or w["want_info"][0] == 0)


def test_the_ladder_reaches_both_sides_and_the_exact_cases():
    c = S.case("exp03", "shoot_rim")
    hit = np.array([w["want_armed"][c["P"]] == 0 for w in c["want"] if w["real"]])
    assert 0.4 < hit.mean() < 0.6
    assert c["rim_exact"].sum() >= 12 and c["exact"].sum() == c["rim_exact"].sum() + (~c["real"]).sum()
    m = c["margin"][c["real"] & ~c["exact"]]
    assert m.min() < 1e-6 and m.max() > 0.29
    t = S.case("exp03", "ties")
    mirrors = [e for e, w in enumerate(t["want"]) if w["tag"].endswith("/mirror")]
    assert len(mirrors) >= 24 and (t["margin"][mirrors] == 0.0).all() and t["exact"][mirrors].all()


def test_the_fixture_is_identical_when_built_twice():
    for shape, family in (("exp03", "ties"), ("stage02", "shoot_rim"), ("stage01", "dome_rim"), ("level5_c1", "reward_edges"), ("evaluation", "central")):
        a = S.case(shape, family)
        b = S.case.__wrapped__(shape, family)
        assert a is not b and np.array_equal(a["blob"], b["blob"]) and np.array_equal(a["margin"], b["margin"]) and np.array_equal(a["tag"], b["tag"])
        assert a["cfg"].n_envs == b["cfg"].n_envs and bytes(a["cfg"]) == bytes(b["cfg"])
