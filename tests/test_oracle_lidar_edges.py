"""The bound that tests/test_gpu_lidar_edges.py holds the step kernels to, worked out WITHOUT a GPU: the oracle's float32 / float64 pair on the
crafted LIDAR geometry of tests/_lidar_states.py.  Per family G is the largest decision margin (metres) at which the two builds disagree on
which cells are hit or on who won a cell, pooled over the shapes (L.family_G says why), and the kernel's bound is M = 4 G.  Asserted here:
  * above M the pair itself agrees (by construction of G) and M leaves every asserted rung of the ladder in: M < 3e-4 m;
  * at least two thirds of every family's targets have a margin above M (or are exact cases);
  * the exact cases (signed zeros at the seam, x = y = 0 at the poles, a coincident drone, bitwise identical positions) agree exactly in the pair:
    no disagreeing cell lies in the neighbourhood of one;
  * the margins mean what they say: in the edge, seam, pole and rim families a target's margin is never larger than the offset it was placed with."""
import numpy as np
import pytest

from tests import _lidar_states as L


CASES = [(t, o, n, f) for t, o, n in L.SHAPES for f in L.FAMILIES + (("crowd",) if dict(o).get("n_pursuers") == 5 else ())]   # crowd: 13 other drones


@pytest.mark.parametrize("task,over,limit,family", CASES)
def test_the_pair_sets_the_bound(task, over, limit, family):
    r = L.reference(task, family, 0, over, limit)
    c = r["case"]
    bad = L.mismatch(r["f32"], r["f64"])
    M = L.bound(family)
    fig = L.figures(r, bad, M)
    print(f"{task}{dict(over)} {family}: N = {c['N']}, targets = {fig['targets']}, G = {r['G']:.3g} m (family: {L.family_G(family):.3g} m), M = {M:.3g} m, "
          f"held = {fig['kept_share']:.3f}, disagreeing cells = {fig['disagreeing_cells']}, smallest agreeing margin = {fig['smallest_agreeing_margin']}")
    assert c["N"] % 64 != 0 and c["N"] <= 1024 and len(c["env"]) > 0
    assert np.isfinite(r["G"]), "the pair disagrees next to an exact case, or in a cell that no target's neighbourhood covers"
    assert fig["largest_disagreeing_margin"] <= L.family_G(family) and M == 4 * L.family_G(family)     # above M the pair itself agrees
    assert M < min(L.LADDER), "4 G has reached the asserted rungs: add rungs at the top, do not raise the factor"
    assert fig["kept_share"] >= 2.0 / 3.0
    if family not in ("ties", "crowd", "central"):   # (two ranges 1e-6 m apart may round to ONE float32 position: decidable, no tie margin)
        placed = (c["delta"] > 0) & ~c["exact"]
        # a level observer: the float32 rounding of the positions (4e-6 m at 38 m).  A tilted one: its quaternion is moved by up to 1e-6 per component to
        # be unit in float32 (tests/_flight_states.py) and its Euler angles are float32 words: 4e-6 rad at 30 m, 2e-4 m with the positions
        slack = np.where(c["env"] % 3 == 2, 2e-4, 4e-6)
        assert (r["margin"][placed] <= c["delta"][placed] * (1 + 1e-3) + slack[placed]).all()
    if family == "seam":
        # the signed zeros (level observer at the origin, x < 0): y = +0.0 is phi = +pi, column 25; y = -0.0 is phi = -pi, column 0, but only below
        # the horizon: the quaternion rotation of the reframe adds a product 0 * z to y, which is +0 for z >= 0 and turns -0.0 into +0.0 (-0 + +0 = +0);
        # for z < 0 it is -0 and the sign survives.  Both oracle builds do this alike; the kernels are held to it.
        pos = L.poses(c)[0]
        zeros = np.flatnonzero(c["exact"])
        assert len(zeros) == 24
        for i in zeros:
            x, y, z = pos[c["env"][i], c["slot"][i]]
            want = 0 if (np.signbit(y) and z < 0) else 25
            assert x < 0 and y == 0 and r["cell"][i] % 26 == want, (x, y, z, r["cell"][i])
            assert (r["f32"][c["env"][i], 0, r["cell"][i] // 26, want] < 1.0)


def test_per_env_margins_are_the_smallest_per_target_margin():
    """OracleEnv.lidar_margins() (opt-in) after a step = the minimum of own_sphere_margins over the env's targets, on the oracle's own IMU read."""
    from oracle import te_oracle as O
    r = L.reference("exp03", "theta_edge", 0, (), 700)
    c = r["case"]
    orc = O.OracleEnv(c["cfg"], "f64")
    orc.set_state(c["blob"])
    with pytest.raises(AssertionError):
        orc.lidar_margins()
    orc.set_lidar_margins(True)
    orc.step(np.zeros((c["N"], 4), np.float32))
    got = orc.lidar_margins()
    orc.close()
    want = np.full(c["N"], 1e30)
    np.minimum.at(want, c["env"], r["margin"])
    has = want < 1e29
    # the env-level figure is taken on the unrounded float64 IMU read, the per-target one on its float32 rounding: 1.2e-7 rad at up to 30 m
    assert has.sum() > 300 and np.abs(got[has] - want[has]).max() < 1e-5
    assert (got[~has] > 1.0).all()
