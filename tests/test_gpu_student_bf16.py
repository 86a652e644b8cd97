"""te_sphere_encode_bf16 (csrc/te_sphere_bf16.hpp), te_sphere_pack_bf16 and StudentDriver(encoder_precision="bf16") on the MI355X.
The reference is E64 of tests/_student_bf16_ref.py (the numerics contract on the CPU with float64 sums) under that module's two
conditions: at most 1 % of the elements further than NEAR = 1e-5 (1 + |E64|) from E64, and every element within NEAR + 2 B[o] (B: what
one block1 value on the other side of a bf16 rounding boundary can move the output by).  Everything else is bitwise.

Measured on the MI355X: pool spheres max |d| 6.5e-6 .. 3.05e-4, share 0 .. 0.104 %, worst ratio 0.0007 .. 0.045; the fixture's 48 spheres
max |d| 2.95e-4, share 0.121 % (0.305 % of its 19 counting ones), ratio 0.038, the figures of the CPU pair E32 / E64."""
import numpy as np
import pytest

from tests import _student_bf16_ref as R
from tests import _student_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 1792


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def pack(w1, b1, w2, b2):
    """(the fp32 parameter buffer, te_sphere_pack_bf16's buffer for it) on the device"""
    import torch
    from dronechase_amd import _lib
    params = torch.from_numpy(np.concatenate([np.asarray(a, np.float32).ravel() for a in (w1, b1, w2, b2)])).to(DEV)
    wb = torch.from_numpy(np.full(R.WORDS, 0x7FC0, np.uint16).view(np.int16)).to(DEV)   # NaN patterns: every element has to be written
    _lib.call_on(torch.device(DEV), "te_sphere_pack_bf16", params.data_ptr(), 3, wb.data_ptr())
    torch.cuda.synchronize()
    return params, wb


def encode(packed, stacked, mask=None, fill=float("nan")):
    """te_sphere_encode_bf16 on device tensors -> [n_rows, n_spheres, 1792]; the output buffer starts full of `fill`."""
    import torch
    from dronechase_amd import _lib
    n_rows, n_spheres = stacked.shape[:2]
    out = torch.full((n_rows, n_spheres, F), fill, dtype=torch.float32, device=DEV)
    _lib.call_on(torch.device(DEV), "te_sphere_encode_bf16", packed[0].data_ptr(), packed[1].data_ptr(), 3, n_rows, n_spheres, stacked.data_ptr(),
                 None if mask is None else mask.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


def on_device(x, n_rows, n_spheres):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).reshape(n_rows, n_spheres, 3, 13, 26)


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
def packed(student):
    need_gpu()
    return pack(*(t.numpy() for t in R.conv_tensors(student)))


def _reference(student, x):
    import torch
    conv = R.conv_tensors(student)
    e64, y1 = R.encode(conv, torch.from_numpy(np.array(x)), torch.float64)
    e64, allowance = e64.numpy(), R.flip_allowance(conv, y1).numpy()
    e64.setflags(write=False); allowance.setflags(write=False)
    return e64, allowance


@pytest.fixture(scope="module")
def pool(fx, student):
    """88 spheres (11 rows of 8), te_sphere_encode's test pool: the fixture's four CONV_SPHERES first, seeded LIDAR-like cells behind
    them; E64 and the flip allowance B of each.  Computed once, never written."""
    rng = np.random.default_rng(S.SEED + 3)
    x = rng.uniform(0.0, 1.0, (88, 3, 13, 26)).astype(np.float32)
    for i, (r, s) in enumerate(fx["conv_spheres"]):
        x[i] = fx["stacked_spheres"][r, s]
    x.setflags(write=False)
    return (x,) + _reference(student, x)


@pytest.fixture(scope="module")
def rows(student):
    """The fixture's 8 rows of 6 spheres with its eight masks, E64 and B."""
    inputs = S.fixture_inputs()
    x = inputs["stacked_spheres"].astype(np.float32).reshape(48, 3, 13, 26)
    x.setflags(write=False)
    return (x, inputs["validity_mask"]) + _reference(student, x)


@pytest.fixture(scope="module")
def base(packed, pool):
    """The pool encoded a few at a time (11 launches of one row of 8), on the device."""
    import torch
    return torch.cat([encode(packed, on_device(pool[0][a:a + 8], 1, 8)).reshape(8, F) for a in range(0, 88, 8)])


def _hold(what, got, e64, allowance):
    gap, share, ratio = R.figures(got, e64, allowance)
    print(f"{what}: max |d| {gap:.3g}, share past NEAR {100 * share:.3g} %, worst |d| / (NEAR + 2 B) {ratio:.3g}")
    assert np.isfinite(got).all() and share <= R.SHARE_CAP and ratio <= 1.0, (what, gap, share, ratio)


# ---------------------------------------------------------------------- the pack kernel
def test_pack_is_the_rounded_weights_at_the_documented_offsets(student, packed):
    want, pad = R.packed_weights(R.conv_tensors(student))
    got = packed[1].cpu().numpy().view(np.uint16)
    assert got.shape == (R.WORDS,) and want.shape == (R.WORDS,) and packed[1].data_ptr() % 16 == 0
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert pad.size == 32 * 128 - 32 * 75 and not got[pad].any()              # conv1's pad columns: kw >= 5 and k >= 120
    assert got[:R.W2_AT].reshape(32, 128)[:, 120:].max() == 0 and got[R.W2_AT:].size == 64 * 288


# ---------------------------------------------------------------------- parity with E64
@pytest.mark.parametrize("n_spheres", [1, 6, 8])
@pytest.mark.parametrize("n_rows", [1, 5, 11])
def test_parity_with_the_contract_in_float64(packed, pool, n_rows, n_spheres):
    """Measured on the MI355X: see the printed figures; DESIGN.md section 7 records them."""
    x, e64, allowance = pool
    n = n_rows * n_spheres
    got = encode(packed, on_device(x[:n], n_rows, n_spheres)).cpu().numpy().reshape(n, F)
    _hold(f"[{n_rows} x {n_spheres}]", got, e64[:n], allowance[:n])


def test_parity_under_the_fixtures_eight_masks(packed, rows):
    import torch
    x, mask, e64, allowance = rows
    counts = S.counting(mask.copy()).reshape(48)
    got = encode(packed, on_device(x, 8, 6), torch.from_numpy(mask).to(DEV)).cpu().numpy().reshape(48, F)
    assert np.all(got[~counts] == 0.0)
    _hold("the fixture's rows, counting spheres", got[counts], e64[counts], allowance[counts])
    _hold("the fixture's rows, no mask", encode(packed, on_device(x, 8, 6)).cpu().numpy().reshape(48, F), e64, allowance)


# ---------------------------------------------------------------------- exact arithmetic, bitwise
def _hybrid_pad(x, p):
    x = np.concatenate([x[..., -p:], x, x[..., :p]], axis=-1)                      # circular in W
    return np.pad(x, [(0, 0)] * (x.ndim - 2) + [(p, p), (0, 0)], constant_values=1.0)   # then 1.0 in H, the corners included


def _conv64(x, w, b, k):
    """hybrid padding, conv k x k stride 2 and ReLU in float64 -> (the result, the same sum over absolute values)"""
    xp = _hybrid_pad(x, (k - 1) // 2)
    ho, wo = (xp.shape[1] - k) // 2 + 1, (xp.shape[2] - k) // 2 + 1
    win = np.stack([xp[:, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2] for kh in range(k) for kw in range(k)], axis=1)   # [ci, k k, ho, wo]
    y = np.einsum("ctyx,oct->oyx", win, w.reshape(w.shape[0], w.shape[1], k * k)) + b[:, None, None]
    mass = np.einsum("ctyx,oct->oyx", np.abs(win), np.abs(w).reshape(w.shape[0], w.shape[1], k * k)) + np.abs(b)[:, None, None]
    return np.maximum(y, 0.0), mass


def test_exact_arithmetic_is_bitwise_the_float64_reference():
    """Cells in {0, 1/2, 1}, sparse weights that are small multiples of 1/4, biases of 1/16: every block1 sum is a multiple of 1/16
    below 8 (a bf16 value: 7 bits), every block2 partial sum a multiple of 1/64 far below 2^24 / 64 (exact in fp32 in any order).  The
    properties are asserted on the CPU first; then no rounding happens anywhere and the kernel must give the float64 result bitwise."""
    import torch
    need_gpu()
    rng = np.random.default_rng(S.SEED + 11)
    x = rng.integers(0, 3, (5, 3, 13, 26)).astype(np.float64) / 2.0
    w1 = np.where(rng.uniform(size=(32, 3, 5, 5)) < 0.06, rng.integers(-3, 4, (32, 3, 5, 5)), 0).astype(np.float64) / 4.0
    w2 = np.where(rng.uniform(size=(64, 32, 3, 3)) < 0.04, rng.integers(-3, 4, (64, 32, 3, 3)), 0).astype(np.float64) / 4.0
    b1, b2 = np.full(32, 1.0 / 16.0), np.full(64, 1.0 / 16.0)
    assert (w1 != 0).sum() > 100 and (w2 != 0).sum() > 500
    want = np.empty((5, F), np.float32)
    for i in range(5):
        y1, mass1 = _conv64(x[i], w1, b1, 5)
        assert mass1.max() < 8.0 and np.array_equal(y1 * 16.0, np.round(y1 * 16.0))
        assert np.array_equal(R.q(torch.from_numpy(y1)).numpy(), y1)                 # every block1 output is a bf16 value
        y2, mass2 = _conv64(y1, w2, b2, 3)
        assert mass2.max() < 2.0 ** 17 and np.array_equal(y2 * 64.0, np.round(y2 * 64.0))   # every partial sum is exact in fp32
        assert np.array_equal(y2.astype(np.float32).astype(np.float64), y2) and (y2 > 0).sum() > 200
        want[i] = y2.reshape(F)
    got = encode(pack(w1, b1, w2, b2), on_device(x.astype(np.float32), 1, 5)).cpu().numpy().reshape(5, F)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def _bf16_ramp():
    """[3, 13, 26], every cell a distinct bf16 value below the padding's 1.0: the 1014 bf16 values next below 1."""
    bits = (0x3F80 - 1 - np.arange(3 * 13 * 26)).astype(np.uint32) << 16
    x = bits.view(np.float32).reshape(3, 13, 26)
    assert np.unique(x).size == x.size and 0.0 < x.min() and x.max() < 1.0
    return x


def test_geometry_is_the_references_padding_and_stride_bitwise():
    """te_sphere_encode's geometry test on a ramp of bf16 values: one weight of each layer is 1, all else 0, so the output is a
    shifted, padded copy of the input, exactly.  conv1: each of the 25 taps of (co, ci) = (5, tap % 3) behind conv2's centre tap;
    conv2: each of the 9 taps of (co, ci) = (7, 5) behind conv1's centre tap: the wrap of the feature map's columns and its 1.0 rows."""
    need_gpu()
    x = _bf16_ramp()
    xin = on_device(x, 1, 1)
    xp = _hybrid_pad(x, 2)
    assert xp.shape == (3, 17, 30) and xp[0, 1, 0] == 1.0 and xp[0, 2, 0] == x[0, 0, 24] and xp[0, 2, 29] == x[0, 0, 1]
    cases = [("conv1", t, 1, 1) for t in range(25)] + [("conv2", 12, kh, kw) for kh in range(3) for kw in range(3)]
    for which, tap, kh2, kw2 in cases:
        ci, kh, kw = (tap % 3 if which == "conv1" else 1), tap // 5, tap % 5
        w1, w2 = np.zeros((32, 3, 5, 5), np.float32), np.zeros((64, 32, 3, 3), np.float32)
        w1[5, ci, kh, kw] = 1.0
        w2[7, 5, kh2, kw2] = 1.0
        got = encode(pack(w1, np.zeros(32), w2, np.zeros(64)), xin).cpu().numpy().reshape(64, 4, 7)
        c1 = xp[ci, kh:kh + 13:2, kw:kw + 25:2]             # conv1 channel 5: [7, 13]
        want = np.zeros((64, 4, 7), np.float32)
        want[7] = _hybrid_pad(c1, 1)[kh2:kh2 + 7:2, kw2:kw2 + 13:2]
        assert np.array_equal(got, want), (which, tap, kh2, kw2, np.argwhere(got != want)[:5])


# ---------------------------------------------------------------------- skipping
def test_spheres_that_do_not_count_are_skipped_and_zeroed(packed, rows):
    import torch
    x, mask, _, _ = rows
    counts = S.counting(mask.copy())
    m = torch.from_numpy(mask).to(DEV)
    clean = encode(packed, on_device(x, 8, 6), m).cpu().numpy()
    poisoned = x.reshape(8, 6, 3, 13, 26).copy()
    poisoned[~counts] = np.nan
    got = encode(packed, on_device(poisoned, 8, 6), m).cpu().numpy()
    assert np.all(got[~counts] == 0.0) and not np.signbit(got[~counts]).any()        # exact zeros, written over the buffer's NaN
    assert np.array_equal(got, clean) and np.isfinite(got).all()                     # the NaN input changes nothing anywhere
    assert counts[0, 0] and not mask[0, 0] and (got[0, 0] != 0).any()                # sphere 0 of the all-zero row is encoded
    everything = encode(packed, on_device(x, 8, 6)).cpu().numpy()                    # mask = NULL: every sphere is encoded
    assert np.array_equal(everything[counts], got[counts]) and (everything[~counts] != 0).any()
    as_bool = encode(packed, on_device(poisoned, 8, 6), m.bool().view(torch.uint8)).cpu().numpy()
    assert np.array_equal(as_bool, got)


# ---------------------------------------------------------------------- placement independence
def test_a_spheres_features_do_not_depend_on_where_it_is(packed, pool, base):
    import torch
    x = pool[0]
    base = base.cpu().numpy()
    rows6 = encode(packed, on_device(x[:66], 11, 6)).cpu().numpy().reshape(66, F)
    assert np.array_equal(rows6, base[:66])                                           # another slot, another n_rows
    assert np.array_equal(encode(packed, on_device(x[:66], 11, 6)).cpu().numpy().reshape(66, F), rows6)   # a second call
    perm = np.random.default_rng(4).permutation(66)
    shuffled = encode(packed, on_device(x[perm], 11, 6)).cpu().numpy().reshape(66, F)
    assert np.array_equal(shuffled, base[perm])
    alone = encode(packed, on_device(x[7:8], 1, 1)).cpu().numpy().reshape(1, F)
    assert np.array_equal(alone, base[7:8])
    mask = (np.random.default_rng(5).uniform(size=(11, 6)) < 0.5).astype(np.uint8)    # ... nor on the mask of the others
    masked = encode(packed, on_device(x[:66], 11, 6), torch.from_numpy(mask).to(DEV)).cpu().numpy()
    counts = S.counting(mask.copy())
    assert 0 < counts.sum() < 66
    assert np.array_equal(masked[counts], base[:66].reshape(11, 6, F)[counts]) and np.all(masked[~counts] == 0.0)


def test_more_spheres_than_workgroups(packed, pool, base):
    """1 200 spheres: more than two per compute unit, so the persistent workgroups loop; a repeat of the pool, bitwise per sphere."""
    import torch
    x = pool[0]
    idx = np.random.default_rng(8).integers(0, 88, 1200)
    mask = (np.random.default_rng(6).uniform(size=(150, 8)) < 0.6).astype(np.uint8)
    got = encode(packed, on_device(x[idx], 150, 8), torch.from_numpy(mask).to(DEV)).cpu().numpy()
    counts = S.counting(mask.copy())
    want = base.cpu().numpy()[idx].reshape(150, 8, F)
    assert np.array_equal(got[counts], want[counts]) and np.all(got[~counts] == 0.0)
    assert np.array_equal(encode(packed, on_device(x[idx], 150, 8)).cpu().numpy(), want)


def test_byte_offsets_past_two_to_the_32(packed, pool, base):
    """75 000 rows of 8 spheres: the input is 2.4 GB (past 2^31 bytes), the output 4.3 GB (past 2^32).  The pool repeated, on the
    device; every sphere bitwise its small-batch result, the masked ones zeros."""
    import torch
    x = pool[0]
    n_rows, n_spheres, n = 75_000, 8, 600_000
    assert n * F * 4 > 1 << 32 and n * 3 * 13 * 26 * 4 > 1 << 31
    gen = torch.Generator(device=DEV).manual_seed(7)
    idx = torch.randint(0, 88, (n,), device=DEV, generator=gen)
    mask = (torch.rand((n_rows, n_spheres), device=DEV, generator=gen) < 0.7).to(torch.uint8)
    stacked = torch.from_numpy(x.copy()).to(DEV)[idx].reshape(n_rows, n_spheres, 3, 13, 26)
    got = encode(packed, stacked, mask).reshape(n, F)
    counts = (mask != 0)
    counts[:, 0] |= ~counts.any(dim=1)
    counts = counts.reshape(n)
    for a in range(0, n, 100_000):
        want = base[idx[a:a + 100_000]] * counts[a:a + 100_000, None]
        assert torch.equal(got[a:a + 100_000], want), a
    assert torch.equal(got[-1], base[idx[-1]] * counts[-1])


def test_nothing_is_written_past_the_output(packed, pool):
    """The output sits between two guard bands of a larger buffer; with and without a mask the bands keep their pattern."""
    import torch
    from dronechase_amd import _lib
    x = pool[0]
    guard = 4096
    for n_rows, n_spheres, masked in ((1, 1, False), (3, 5, True), (11, 8, True), (11, 8, False)):
        n = n_rows * n_spheres
        buf = torch.full((2 * guard + n * F,), -7.25, dtype=torch.float32, device=DEV)
        out = buf[guard:guard + n * F]
        assert out.data_ptr() % 16 == 0
        mask = torch.from_numpy((np.random.default_rng(n).uniform(size=(n_rows, n_spheres)) < 0.5).astype(np.uint8)).to(DEV) if masked else None
        _lib.call_on(torch.device(DEV), "te_sphere_encode_bf16", packed[0].data_ptr(), packed[1].data_ptr(), 3, n_rows, n_spheres,
                     on_device(x[:n], n_rows, n_spheres).data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert bool((buf[:guard] == -7.25).all()) and bool((buf[guard + n * F:] == -7.25).all()), (n_rows, n_spheres, masked)
        assert bool((out != -7.25).all())                                             # and every element inside is written


# ---------------------------------------------------------------------- the driver
def _gpu_student(student):
    import copy
    return copy.deepcopy(student).to(DEV).requires_grad_(False)


def _gpu_obs(fx):
    import torch
    return {"stacked_spheres": torch.from_numpy(fx["stacked_spheres"]).float().to(DEV), "validity_mask": torch.from_numpy(fx["validity_mask"]).to(DEV),
            "inertial_data": torch.from_numpy(fx["inertial_data"]).float().to(DEV), "last_action": torch.from_numpy(fx["last_action"]).float().to(DEV)}


def _clamped(a):
    import torch
    return torch.max(torch.min(a, torch.ones_like(a)), torch.tensor([-1.0, -1.0, -1.0, 0.0], device=a.device))


def test_driver_flies_the_bf16_encoder_and_refresh_repacks_in_place(fx, student, rows):
    import torch
    from dronechase_amd.student import StudentDriver
    need_gpu()
    net = _gpu_student(student).eval()
    obs = _gpu_obs(fx)
    drv = StudentDriver(net, fused_encoder=True, encoder_precision="bf16")
    assert drv.weights_bf16.dtype == torch.int16 and drv.weights_bf16.numel() == R.WORDS and drv.weights_bf16.data_ptr() % 16 == 0
    a = drv.predict(obs)[0]
    encoded = drv.encode(obs["stacked_spheres"], obs["validity_mask"]).clone()
    with torch.no_grad():
        assert torch.equal(a, _clamped(net(obs, encoded)))                             # the module fed with encode()'s own output, bitwise
    x, mask, e64, allowance = rows
    counts = S.counting(mask.copy()).reshape(48)
    _hold("the driver's encode()", encoded.cpu().numpy().reshape(48, F)[counts], e64[counts], allowance[counts])
    fp32 = StudentDriver(net, fused_encoder=True)
    gap = (a - fp32.predict(obs)[0]).abs().max().item()
    print(f"actions, bf16 against fp32 fused encoder: max |d| {gap:.3g} (recorded, not bounded)")
    assert fp32.weights_bf16 is None and np.isfinite(gap)
    # a changed conv weight flies after refresh(), from the same two buffers
    at = (drv.params.data_ptr(), drv.weights_bf16.data_ptr())
    with torch.no_grad():
        net.sphere_cnn.block1[0].conv.weight.mul_(1.5)
        net.sphere_cnn.block2[0].conv.bias.add_(0.05)
    assert torch.equal(drv.predict(obs)[0], a)                                         # not before
    drv.refresh()
    torch.cuda.synchronize()
    assert (drv.params.data_ptr(), drv.weights_bf16.data_ptr()) == at
    conv = [t.cpu() for t in R.conv_tensors(net)]
    assert np.array_equal(drv.weights_bf16.cpu().numpy().view(np.uint16), R.packed_weights(conv)[0])
    assert np.array_equal(drv.params.cpu().numpy(), np.concatenate([t.numpy().ravel() for t in conv]))
    b = drv.predict(obs)[0]
    assert (b - a).abs().max().item() > 1e-2
    e64b, y1 = R.encode(conv, torch.from_numpy(np.array(x)), torch.float64)
    _hold("after refresh()", drv.encode(obs["stacked_spheres"], obs["validity_mask"]).cpu().numpy().reshape(48, F)[counts], e64b.numpy()[counts],
          R.flip_allowance(conv, y1).numpy()[counts])


def test_evaluate_policy_flies_the_bf16_driver_on_level5_c1(student):
    """64 level5_c1 envs capped at max_step = 20: a capped episode ends on its 21st step (the reference's `step > max_step`)."""
    from dronechase_amd import default_config
    from dronechase_amd.batched_env import BatchedEnv
    from dronechase_amd.monitor import evaluate_policy
    from dronechase_amd.student import OBS_KEYS, StudentDriver
    need_gpu()
    net = _gpu_student(student)
    first = []
    for precision in ("fp32", "bf16"):
        env = BatchedEnv(default_config("level5_c1", n_envs=64, max_step=20, seed=7), DEV)
        env.reset()
        driver = StudentDriver(net, fused_encoder=True, encoder_precision=precision)
        first.append(driver.predict(dict(zip(OBS_KEYS, env.observe_stacked())))[0].cpu().numpy())
        if precision == "bf16":
            ret, length = evaluate_policy(driver, env, n_eval_episodes=100)
            print(f"lengths {length.min()} .. {length.max()}, returns {ret.min():.1f} .. {ret.max():.1f}")
            assert ret.shape == (100,) and length.shape == (100,) and np.isfinite(ret).all() and (length >= 1).all()
            assert (length <= int(env.cfg.max_step) + 1).all()
        env.close()
    gap = np.abs(first[1] - first[0]).max()
    print(f"first step's actions, bf16 against fp32 fused encoder: max |d| {gap:.3g} (recorded, not bounded)")
    assert np.isfinite(first[1]).all()
