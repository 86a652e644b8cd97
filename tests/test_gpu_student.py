"""te_sphere_encode (csrc/te_sphere.hpp), StudentDriver(fused_encoder=True) and evaluate_policy on the stacked observation, on the
MI355X.  References: the fp64 conv stack of the reference's SphereCNN (tests/golden/student_flia.npz) and FLIAStudent's own conv blocks
on the CPU; tolerance |d| <= 1e-4 + 1e-4 |ref| (tests/_student_cases.py) wherever the comparison is not bitwise."""
import ctypes as C

import numpy as np
import pytest

from tests import _student_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 1792


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def encode(params, stacked, mask=None, fill=float("nan")):
    """te_sphere_encode on device tensors -> [n_rows, n_spheres, 1792]; the output buffer starts full of `fill`."""
    import torch
    from dronechase_amd import _lib
    n_rows, n_spheres = stacked.shape[:2]
    out = torch.full((n_rows, n_spheres, F), fill, dtype=torch.float32, device=DEV)
    _lib.call_on(torch.device(DEV), "te_sphere_encode", params.data_ptr(), 3, n_rows, n_spheres, stacked.data_ptr(),
                 None if mask is None else mask.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def pack(w1, b1, w2, b2):
    import torch
    return torch.from_numpy(np.concatenate([np.asarray(a, np.float32).ravel() for a in (w1, b1, w2, b2)])).to(DEV)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(S.FIXTURE))


@pytest.fixture(scope="module")
def student():
    """The recipe's student on the CPU (the reference side of every comparison)."""
    import torch
    from dronechase_amd.student import load_flia_student
    w = S.recipe_weights(S.keys_and_shapes())
    return load_flia_student({k: torch.from_numpy(v).float() for k, v in w.items()})


@pytest.fixture(scope="module")
def params(student):
    need_gpu()
    cnn = student.sphere_cnn
    return pack(*(t.detach().numpy() for t in (cnn.block1[0].conv.weight, cnn.block1[0].conv.bias, cnn.block2[0].conv.weight, cnn.block2[0].conv.bias)))


@pytest.fixture(scope="module")
def pool(fx, student):
    """88 spheres (11 rows of 8): the fixture's four CONV_SPHERES first, seeded LIDAR-like cells behind them; and the module's own
    conv blocks on them in fp32 on the CPU.  Computed once, never written."""
    import torch
    rng = np.random.default_rng(S.SEED + 3)
    x = rng.uniform(0.0, 1.0, (88, 3, 13, 26)).astype(np.float32)
    for i, (r, s) in enumerate(fx["conv_spheres"]):
        x[i] = fx["stacked_spheres"][r, s]
    with torch.no_grad():
        ref = student.sphere_cnn.conv_stack(torch.from_numpy(x)).numpy()
    x.setflags(write=False); ref.setflags(write=False)
    return x, ref


# ---------------------------------------------------------------------- geometry, bitwise
def _ramp():
    """[3, 13, 26], every cell distinct, below the padding's 1.0 and exact in float32."""
    return ((np.arange(3 * 13 * 26, dtype=np.float64) + 1.0) / 2048.0).reshape(3, 13, 26).astype(np.float32)


def _hybrid_pad(x, p):
    x = np.concatenate([x[..., -p:], x, x[..., :p]], axis=-1)                      # circular in W
    return np.pad(x, [(0, 0)] * (x.ndim - 2) + [(p, p), (0, 0)], constant_values=1.0)   # then 1.0 in H, the corners included


def test_geometry_is_the_references_padding_and_stride_bitwise():
    """One weight of each layer is 1, all else 0: the output is a shifted, padded copy of the input, exactly.
    conv1: each of the 25 taps of (co, ci) = (5, tap % 3) behind conv2's centre tap (which reads conv1's even positions);
    conv2: each of the 9 taps of (co, ci) = (7, 5) behind conv1's centre tap, which copies the input's even cells: that shows the
    wrap of the feature map's columns and its 1.0 rows."""
    import torch
    need_gpu()
    x = _ramp()
    xin = torch.from_numpy(x).to(DEV).reshape(1, 1, 3, 13, 26).contiguous()
    xp = _hybrid_pad(x, 2)                                  # [3, 17, 30]
    assert xp.shape == (3, 17, 30) and xp[0, 1, 0] == 1.0 and xp[0, 2, 0] == x[0, 0, 24] and xp[0, 2, 29] == x[0, 0, 1]
    cases = [("conv1", t, 1, 1) for t in range(25)] + [("conv2", 12, kh, kw) for kh in range(3) for kw in range(3)]
    for which, tap, kh2, kw2 in cases:
        ci, kh, kw = (tap % 3 if which == "conv1" else 1), tap // 5, tap % 5
        w1, w2 = np.zeros((32, 3, 5, 5), np.float32), np.zeros((64, 32, 3, 3), np.float32)
        w1[5, ci, kh, kw] = 1.0
        w2[7, 5, kh2, kw2] = 1.0
        got = encode(pack(w1, np.zeros(32), w2, np.zeros(64)), xin).cpu().numpy().reshape(64, 4, 7)
        c1 = xp[ci, kh:kh + 13:2, kw:kw + 25:2]             # conv1 channel 5: [7, 13]
        assert c1.shape == (7, 13)
        c1p = _hybrid_pad(c1, 1)                            # [9, 15]
        want = np.zeros((64, 4, 7), np.float32)
        want[7] = c1p[kh2:kh2 + 7:2, kw2:kw2 + 13:2]
        assert np.array_equal(got, want), (which, tap, kh2, kw2, np.argwhere(got != want)[:5])


# ---------------------------------------------------------------------- parity
@pytest.mark.parametrize("n_spheres", [1, 6, 8])
@pytest.mark.parametrize("n_rows", [1, 5, 11])
def test_parity_with_the_fp64_fixture_and_the_modules_conv_blocks(fx, params, pool, n_rows, n_spheres):
    """Measured on the MI355X: see the printed gaps (max |d| and its share of the bound); DESIGN.md section 7 records them."""
    import torch
    x, ref = pool
    n = n_rows * n_spheres
    stacked = torch.from_numpy(x[:n].copy()).to(DEV).reshape(n_rows, n_spheres, 3, 13, 26)
    got = encode(params, stacked).cpu().numpy().reshape(n, F)
    ok, gap, ratio = S.within(got, ref[:n])
    print(f"[{n_rows} x {n_spheres}] against the module in fp32: max |d| {gap:.3g}, {ratio:.3g} of the bound")
    assert ok, (gap, ratio)
    k = min(n, 4)
    ok, gap, ratio = S.within(got[:k], fx["conv"][:k])
    print(f"[{n_rows} x {n_spheres}] against the fp64 fixture ({k} spheres): max |d| {gap:.3g}, {ratio:.3g} of the bound")
    assert ok, (gap, ratio)


# ---------------------------------------------------------------------- skipping
def test_spheres_that_do_not_count_are_skipped_and_zeroed(fx, params, student):
    import torch
    mask = fx["validity_mask"]
    counts = S.counting(mask)
    x = fx["stacked_spheres"].astype(np.float32)
    with torch.no_grad():
        ref = student.sphere_cnn.conv_stack(torch.from_numpy(x).reshape(48, 3, 13, 26)).numpy().reshape(8, 6, F)
    poisoned = x.copy()
    poisoned[~counts] = np.nan
    got = encode(params, torch.from_numpy(poisoned).to(DEV), torch.from_numpy(mask).to(DEV)).cpu().numpy()
    assert np.all(got[~counts] == 0.0) and not np.signbit(got[~counts]).any()        # exact zeros, written over the buffer's NaN
    ok, gap, ratio = S.within(got[counts], ref[counts])
    print(f"counting spheres: max |d| {gap:.3g}, {ratio:.3g} of the bound")
    assert ok, (gap, ratio)
    for i, (r, s) in enumerate(fx["conv_spheres"]):
        if counts[r, s]:
            assert S.within(got[r, s], fx["conv"][i])[0]
    assert counts[0, 0] and not mask[0, 0] and (got[0, 0] != 0).any()                # sphere 0 of the all-zero row is encoded
    # a bool mask's bytes are the same mask
    as_bool = encode(params, torch.from_numpy(poisoned).to(DEV), torch.from_numpy(mask).to(DEV).bool().view(torch.uint8)).cpu().numpy()
    assert np.array_equal(as_bool, got)
    # mask = NULL: every sphere is encoded
    everything = encode(params, torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert S.within(everything, ref)[0]
    assert np.array_equal(everything[counts], got[counts])


# ---------------------------------------------------------------------- placement independence
def test_a_spheres_features_do_not_depend_on_where_it_is(params, pool):
    import torch
    x, _ = pool
    base = encode(params, torch.from_numpy(x[:66].copy()).to(DEV).reshape(11, 6, 3, 13, 26)).cpu().numpy().reshape(66, F)
    perm = np.random.default_rng(4).permutation(66)
    shuffled = encode(params, torch.from_numpy(x[perm].copy()).to(DEV).reshape(11, 6, 3, 13, 26)).cpu().numpy().reshape(66, F)
    assert np.array_equal(shuffled, base[perm])
    alone = encode(params, torch.from_numpy(x[:6].copy()).to(DEV).reshape(1, 6, 3, 13, 26)).cpu().numpy().reshape(6, F)
    assert np.array_equal(alone, base[:6])
    wide = encode(params, torch.from_numpy(x[:88].copy()).to(DEV).reshape(11, 8, 3, 13, 26)).cpu().numpy().reshape(88, F)
    assert np.array_equal(wide[:66], base)
    # ... nor on the mask of the others
    mask = (np.random.default_rng(5).uniform(size=(11, 6)) < 0.5).astype(np.uint8)
    masked = encode(params, torch.from_numpy(x[:66].copy()).to(DEV).reshape(11, 6, 3, 13, 26), torch.from_numpy(mask).to(DEV)).cpu().numpy()
    counts = S.counting(mask)
    assert 0 < counts.sum() < 66
    assert np.array_equal(masked[counts], base.reshape(11, 6, F)[counts]) and np.all(masked[~counts] == 0.0)


def test_more_spheres_than_workgroups(params, pool):
    """2 048 spheres: more than one per compute unit, so the persistent workgroups loop; a repeat of the pool, bitwise per sphere."""
    import torch
    x, _ = pool
    idx = np.arange(2048) % 88
    mask = (np.random.default_rng(6).uniform(size=(256, 8)) < 0.6).astype(np.uint8)
    base = encode(params, torch.from_numpy(x.copy()).to(DEV).reshape(11, 8, 3, 13, 26)).cpu().numpy().reshape(88, F)
    got = encode(params, torch.from_numpy(x[idx]).to(DEV).reshape(256, 8, 3, 13, 26), torch.from_numpy(mask).to(DEV)).cpu().numpy()
    counts = S.counting(mask)
    assert np.array_equal(got[counts], base[idx].reshape(256, 8, F)[counts]) and np.all(got[~counts] == 0.0)


def test_byte_offsets_past_two_to_the_32(params, pool):
    """75 000 rows of 8 spheres: the input is 2.4 GB (past 2^31 bytes), the output 4.3 GB (past 2^32).  The pool repeated, on the
    device; every sphere bitwise its small-batch result, the masked ones zeros."""
    import torch
    x, _ = pool
    n_rows, n_spheres, n = 75_000, 8, 600_000
    assert n * F * 4 > 1 << 32 and n * 3 * 13 * 26 * 4 > 1 << 31
    base = encode(params, torch.from_numpy(x.copy()).to(DEV).reshape(11, 8, 3, 13, 26)).reshape(88, F)
    gen = torch.Generator(device=DEV).manual_seed(7)
    idx = torch.randint(0, 88, (n,), device=DEV, generator=gen)
    mask = (torch.rand((n_rows, n_spheres), device=DEV, generator=gen) < 0.7).to(torch.uint8)
    stacked = torch.from_numpy(x.copy()).to(DEV)[idx].reshape(n_rows, n_spheres, 3, 13, 26)
    got = encode(params, stacked, mask).reshape(n, F)
    counts = (mask != 0)
    counts[:, 0] |= ~counts.any(dim=1)
    counts = counts.reshape(n)
    for a in range(0, n, 100_000):
        want = base[idx[a:a + 100_000]] * counts[a:a + 100_000, None]
        assert torch.equal(got[a:a + 100_000], want), a
    assert torch.equal(got[-1], base[idx[-1]] * counts[-1])


# ---------------------------------------------------------------------- the driver
def _gpu_student(student):
    import copy
    return copy.deepcopy(student).to(DEV).requires_grad_(False)


def _gpu_obs(fx):
    import torch
    return {"stacked_spheres": torch.from_numpy(fx["stacked_spheres"]).float().to(DEV), "validity_mask": torch.from_numpy(fx["validity_mask"]).to(DEV),
            "inertial_data": torch.from_numpy(fx["inertial_data"]).float().to(DEV), "last_action": torch.from_numpy(fx["last_action"]).float().to(DEV)}


def test_driver_with_the_fused_encoder_agrees_with_the_module(fx, student):
    import torch
    from dronechase_amd.student import StudentDriver
    need_gpu()
    net = _gpu_student(student)
    obs = _gpu_obs(fx)
    plain, fused = StudentDriver(net), StudentDriver(net, fused_encoder=True)
    a0, a1 = plain.predict(obs)[0].cpu().numpy(), fused.predict(obs)[0].cpu().numpy()
    ok, gap, ratio = S.within(a1, a0)
    print(f"fused against unfused actions: max |d| {gap:.3g}, {ratio:.3g} of the bound")
    assert ok, (gap, ratio)
    want = np.clip(fx["out"], [-1, -1, -1, 0], 1)
    assert S.within(a1, want)[0] and S.within(a0, want)[0]
    assert np.array_equal(fused.predict(dict(obs, validity_mask=obs["validity_mask"].bool()))[0].cpu().numpy(), a1)
    # a changed conv weight flies after refresh()
    with torch.no_grad():
        net.sphere_cnn.block1[0].conv.weight.mul_(1.5)
        net.sphere_cnn.block2[0].conv.bias.add_(0.05)
    fused.refresh()
    b0, b1 = plain.predict(obs)[0].cpu().numpy(), fused.predict(obs)[0].cpu().numpy()
    assert np.abs(b0 - a0).max() > 100 * S.ATOL
    ok, gap, ratio = S.within(b1, b0)
    print(f"after refresh(): max |d| {gap:.3g}, {ratio:.3g} of the bound")
    assert ok, (gap, ratio)


# ---------------------------------------------------------------------- evaluation
def _env(task, n, **kw):
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    return BatchedEnv(default_config(task, n_envs=n, max_step=20, seed=7, **kw), DEV)


def test_evaluate_policy_flies_the_student_on_level5_c1(student):
    """Episodes are capped by max_step = 20.  The task's time limit is the reference's `step > max_step` (csrc/te_logic.hpp, pinned
    by the oracle tests), so a capped episode ends on its 21st step: the bound on the lengths is max_step + 1, not max_step.  Measured
    on the MI355X: all 100 episodes of either encoder setting are 21 steps long."""
    from dronechase_amd.monitor import evaluate_policy
    from dronechase_amd.pipeline import ReinforcementLearningPipeline as RLP
    from dronechase_amd.student import StudentDriver
    need_gpu()
    net = _gpu_student(student)
    first = []
    for driver in (net, StudentDriver(net, fused_encoder=True)):
        env = _env("level5_c1", 64)
        env.reset()
        obs = env.observe_stacked()
        who = driver if isinstance(driver, StudentDriver) else StudentDriver(driver)
        first.append(who.predict(dict(zip(("stacked_spheres", "validity_mask", "inertial_data", "last_action"), obs)))[0].cpu().numpy())
        ret, length = evaluate_policy(driver, env, n_eval_episodes=100)
        print(f"lengths {length.min()} .. {length.max()}, returns {ret.min():.1f} .. {ret.max():.1f}")
        assert ret.shape == (100,) and length.shape == (100,) and np.isfinite(ret).all() and (length >= 1).all()
        assert (length <= int(env.cfg.max_step) + 1).all()
        env.close()
    ok, gap, ratio = S.within(first[1], first[0])
    print(f"first step's actions, fused against unfused: max |d| {gap:.3g}, {ratio:.3g} of the bound")
    assert ok, (gap, ratio)
    env = _env("level5_c1", 64)
    avg, std, n, rewards = RLP.evaluate(net, env, n_eval_episodes=70)
    assert n == 70 and rewards.shape == (70,) and np.isfinite(avg)
    env.close()


def test_evaluate_policy_says_which_policy_fits(student):
    import torch
    from dronechase_amd.monitor import evaluate_policy
    from dronechase_amd.ppo import LidarInertialActionPolicy
    need_gpu()
    net = _gpu_student(student)
    env = _env("level5_c1", 64)
    with pytest.raises(ValueError, match="stacked.*FLIAStudent or a StudentDriver"):
        evaluate_policy(LidarInertialActionPolicy().to(DEV), env, n_eval_episodes=4)
    env.close()
    env = _env("stage03", 64)
    with pytest.raises(ValueError, match="FLIAStudent / StudentDriver reads the stacked.*LidarInertialActionPolicy"):
        evaluate_policy(net, env, n_eval_episodes=4)
    env.close()
    env = _env("level5_dumb", 64)
    with pytest.raises(ValueError, match="'level5_dumb' has no agent"):
        evaluate_policy(net, env, n_eval_episodes=4)
    env.close()
    torch.cuda.synchronize()
