"""te_dataset_append / te_dataset_gather (csrc/te_dataset.hpp), imitation.ImitationDataset and StudentTrainer.fit on the MI355X.
Reference: the numpy restatement in tests/_dataset_cases.py.  Everything is compared bitwise except the Gaussian branch of
last_action, held to 4e-6 absolute against the float64 restatement: the noise is at most 0.2 * 5.8 = 1.15, logf / sqrtf / sinf / cosf
and the product with the fp32 angle are a few ulp of it, and the sum rounds once.

Source rows are synthetic: every float encodes (row, position), the rows that are not kept are full of NaN."""
import copy

import numpy as np
import pytest

from tests import _dataset_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = {"stacked": "stacked_spheres", "mask": "validity_mask", "inertial": "inertial_data", "last_action": "last_action"}
NOISE_ATOL = 4e-6


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


@pytest.fixture(scope="module")
def pool():
    """2 100 synthetic rows on the host, shared and never written."""
    p = D.rows(range(2100))
    for v in p.values():
        v.setflags(write=False)
    return p


def to_dev(r, active=None):
    import torch
    t = {k: torch.tensor(v).to(DEV) for k, v in r.items()}          # a copy: the pool is read-only
    obs = {name: t[k] for k, name in KEYS.items()}
    return obs, t["teacher"], None if active is None else torch.tensor(active).to(DEV)


def dataset(capacity, max_append_rows, n_spheres=6):
    from dronechase_amd.imitation import ImitationDataset
    return ImitationDataset(capacity, DEV, max_append_rows, n_spheres)


def ring_of(ds):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(ds, k).cpu().numpy() for k in D.FIELDS}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_rings_equal(got, want, what=""):
    for k in D.FIELDS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


def patterns(n, pool):
    """name -> (rows, active) for every keep pattern the append is held to, on the first n pool rows."""
    p = {k: v[:n] for k, v in pool.items()}
    rng = np.random.default_rng(n)
    rand = rng.random(n) < 0.5
    out = {"all": D.with_pattern(p, np.ones(n, bool)), "none": D.with_pattern(p, np.zeros(n, bool)), "random": D.with_pattern(p, rand)}
    drop = np.flatnonzero(~rand)
    if len(drop):
        out["inactive_but_valid"] = D.with_pattern(p, rand, inactive_but_valid=drop[::2])
        out["active_but_empty"] = D.with_pattern(p, rand, active_but_empty=drop[::2])
    return out


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 2100])
def test_append_is_bitwise_the_kept_rows_in_order(pool, n_rows):
    need_gpu()
    for name, (r, active) in patterns(n_rows, pool).items():
        keep = D.keep_rule(r["mask"], active)
        if name == "random" and n_rows > 1:
            assert 0 < keep.sum() < n_rows
        ds = dataset(2200, 2100)
        obs, teacher, act = to_dev(r, active)
        ds.append(obs, teacher, act)
        got = ring_of(ds)
        assert ds.total() == ds.size() == keep.sum(), name
        for k in D.FIELDS:
            assert np.array_equal(bits(got[k][:keep.sum()]), bits(r[k][keep])), (name, k)
            assert not got[k][keep.sum():].any(), (name, k)
        if name == "all":           # active=None is every row active
            ds2 = dataset(2200, 2100)
            ds2.append(obs, teacher, None)
            assert_rings_equal(ring_of(ds2), got, "active=None")
            assert ds2.total() == n_rows


@pytest.mark.parametrize("n_spheres", [5, 8])
def test_append_and_gather_with_other_sphere_counts(n_spheres):
    """An odd sphere count leaves a row 8 bytes off 16: the copy's other width."""
    need_gpu()
    import torch
    r, active = D.with_pattern(D.rows(range(70), n_spheres), np.random.default_rng(n_spheres).random(70) < 0.6)
    ring = D.Ring(64, n_spheres)
    ds = dataset(64, 35, n_spheres)
    for at in (0, 35):
        part = {k: v[at:at + 35] for k, v in r.items()}
        ring.append(part, active[at:at + 35])
        ds.append(*to_dev(part, active[at:at + 35]))
    assert ds.total() == ring.total > 0
    assert_rings_equal(ring_of(ds), ring.a)
    idx = torch.arange(ring.size - 1, -1, -1, device=DEV)
    obs, teacher = ds.batch(ring.size, index=idx)
    assert np.array_equal(bits(obs["stacked_spheres"].cpu().numpy()), bits(ring.a["stacked"][:ring.size][::-1]))
    assert np.array_equal(bits(teacher.cpu().numpy()), bits(ring.a["teacher"][:ring.size][::-1]))


@pytest.mark.parametrize("prefill", [False, True])
def test_ring_wrap(pool, prefill):
    need_gpu()
    ring, ds = D.Ring(32), dataset(32, 21)
    if prefill:
        ds.buf.fill_(255)
        ds.clear()
    for a in range(4):
        part = {k: v[100 * a:100 * a + 21] for k, v in pool.items()}
        keep = np.ones(21, bool)
        keep[np.random.default_rng(a).choice(21, 6, replace=False)] = False
        r, active = D.with_pattern(part, keep)
        ring.append(r, active)
        ds.append(*to_dev(r, active))
    assert ds.total() == ring.total == 60 and ds.size() == 32
    assert_rings_equal(ring_of(ds), ring.a)


def test_offsets_past_4_gib(pool):
    need_gpu()
    import torch
    capacity = 180000
    ds = dataset(capacity, 21)
    assert ds.buf.numel() > 2 ** 32 and ds.offsets.mask > 2 ** 32
    ds._total.fill_(capacity - 10)
    r = {k: v[500:521] for k, v in pool.items()}
    ds.append(*to_dev(r))
    assert ds.total() == capacity + 11 and ds.size() == capacity
    for k in D.FIELDS:
        ring = getattr(ds, k)
        assert np.array_equal(bits(ring[capacity - 10:].cpu().numpy()), bits(r[k][:10])), k
        assert np.array_equal(bits(ring[:11].cpu().numpy()), bits(r[k][10:])), k
        assert not bool(ring[11:13].any()) and not bool(ring[capacity - 12:capacity - 10].any()), k
    obs, teacher, used = ds.batch(3, index=torch.tensor([capacity - 1, 0, capacity + 5], device=DEV), return_index=True)
    assert used.tolist() == [capacity - 1, 0, capacity - 1]
    assert np.array_equal(bits(obs["stacked_spheres"].cpu().numpy()), bits(r["stacked"][[9, 10, 9]]))


@pytest.fixture(scope="module")
def filled(pool):
    """A ring of 96 slots holding 80 pool rows (ids 1000 .. 1079), and the same on the host."""
    need_gpu()
    r = {k: v[1000:1080] for k, v in pool.items()}
    ring, ds = D.Ring(96), dataset(96, 80)
    ring.append(r)
    ds.append(*to_dev(r))
    assert ds.size() == 80
    return ds, ring


def batch_np(out):
    obs, teacher = out[0], out[1]
    return {"stacked": obs["stacked_spheres"].cpu().numpy(), "mask": obs["validity_mask"].cpu().numpy(), "inertial": obs["inertial_data"].cpu().numpy(),
            "last_action": obs["last_action"].cpu().numpy(), "teacher": teacher.cpu().numpy()}


def test_gather_by_index_repeats_unsorted_and_clamped(filled):
    import torch
    ds, ring = filled
    index = np.array([5, 5, 79, 0, 33, 5, 95, -1, -2 ** 40, 96, 2 ** 40, 17], np.int64)
    want = np.clip(index, 0, 95)
    for mode in ("keep", "random", "noise"):
        out = ds.batch(len(index), index=torch.from_numpy(index).to(DEV), last_action_mode=mode, seed=3, draw=4, return_index=True)
        got = batch_np(out)
        assert out[2].tolist() == want.tolist()
        for k in D.FIELDS:
            if k != "last_action" or mode == "keep":        # nothing but last_action is ever perturbed
                assert np.array_equal(bits(got[k]), bits(ring.a[k][want])), (mode, k)
        assert out[0]["stacked_spheres"].is_contiguous() and out[0]["validity_mask"].dtype == torch.uint8


def test_gather_draws_its_slots_on_the_device(filled):
    ds, ring = filled
    seed, draw = 0xDEADBEEF12345678, (7 << 32) | 9
    out = ds.batch(1000, seed=seed, draw=draw, return_index=True)
    slots = D.philox_slots(1000, 80, seed, draw)
    assert np.array_equal(out[2].cpu().numpy(), slots) and len(np.unique(slots)) == 80
    got = batch_np(out)
    for k in D.FIELDS:
        assert np.array_equal(bits(got[k]), bits(ring.a[k][slots])), k
    again = batch_np(ds.batch(1000, seed=seed, draw=draw))
    assert_rings_equal(again, got, "same (seed, draw)")
    other = ds.batch(1000, seed=seed, draw=draw + 1, return_index=True)
    assert not np.array_equal(other[2].cpu().numpy(), slots)


def test_gather_from_an_empty_ring_is_zeros():
    need_gpu()
    ds = dataset(16, 4)
    for mode in ("keep", "random", "noise"):
        out = ds.batch(5, last_action_mode=mode, seed=1, draw=1, return_index=True)
        assert out[2].tolist() == [-1] * 5
        for k, v in batch_np(out).items():
            assert not v.any(), (mode, k)


def test_random_last_action_is_bitwise_the_restatement(filled):
    ds, ring = filled
    seed, draw = 77, 2 ** 33 + 1
    got = batch_np(ds.batch(4096, last_action_mode="random", seed=seed, draw=draw))
    f32, _ = D.la_random(4096, seed, draw)
    assert np.array_equal(bits(got["last_action"]), bits(f32))
    slots = D.philox_slots(4096, 80, seed, draw)
    assert np.array_equal(bits(got["teacher"]), bits(ring.a["teacher"][slots]))


def test_noisy_last_action_against_the_float64_restatement(filled):
    ds, ring = filled
    seed, draw = 123456789, 5
    got = batch_np(ds.batch(8192, last_action_mode="noise", seed=seed, draw=draw))
    slots = D.philox_slots(8192, 80, seed, draw)
    want = D.la_noise(ring.a["last_action"][slots], seed, draw)
    err = np.abs(got["last_action"].astype(np.float64) - want).max()
    print("noisy last_action: max |kernel - float64| =", err)
    assert err <= NOISE_ATOL
    # the stored values are +-[0.5, 1): both clamps are reached, and exactly
    hi, lo = want == 1.0, want == -1.0
    assert hi.sum() > 100 and lo.sum() > 100
    inside = np.abs(want) < 1.0 - NOISE_ATOL
    assert (np.abs(got["last_action"]) <= 1.0).all() and (np.abs(got["last_action"][inside]) < 1.0).all()
    edge = np.abs(np.abs(ring.a["last_action"][slots].astype(np.float64) + 0.2 * D.normals(8192, seed, draw)) - 1.0) < 1e-5
    assert (got["last_action"][hi & ~edge] == 1.0).all() and (got["last_action"][lo & ~edge] == -1.0).all()
    again = batch_np(ds.batch(8192, last_action_mode="noise", seed=seed, draw=draw))
    assert np.array_equal(bits(again["last_action"]), bits(got["last_action"]))
    other = batch_np(ds.batch(8192, last_action_mode="noise", seed=seed, draw=draw + 1))
    assert not np.array_equal(bits(other["last_action"]), bits(got["last_action"]))


def test_noise_has_the_mean_and_std_asked_for(pool):
    need_gpu()
    r = {k: v[:8].copy() for k, v in pool.items()}
    r["last_action"][:] = 0.0
    ds = dataset(8, 8)
    ds.append(*to_dev(r))
    noise = batch_np(ds.batch(8192, last_action_mode="noise", seed=2024, draw=0))["last_action"].astype(np.float64)
    n = noise.size
    assert n == 8192 * 4 and np.abs(noise).max() <= 0.2 * 5.8 + NOISE_ATOL
    assert np.abs(noise - D.la_noise(np.zeros((8192, 4), np.float32), 2024, 0)).max() <= NOISE_ATOL
    print("noise mean", noise.mean(), "std", noise.std())
    assert abs(noise.mean()) < 5 * 0.2 / np.sqrt(n) and abs(noise.std() - 0.2) < 5 * 0.2 / np.sqrt(2 * n)


class _Recorded:
    """An env whose step_students keeps a host copy of what it returned."""

    def __init__(self, env):
        self.env, self.steps = env, []

    def step_students(self):
        out = self.env.step_students()
        self.steps.append([t.cpu().numpy() for t in out[:5]])
        return out


def test_collect_keeps_what_the_collector_keeps(tmp_path):
    need_gpu()
    from dronechase_amd import default_config, dump
    from dronechase_amd.batched_env import BatchedEnv
    N, steps = 64, 30
    env = BatchedEnv(default_config("level5_dumb", n_envs=N, seed=5), DEV)
    P = int(env.cfg.n_pursuers)
    try:
        env.reset()
        rec = _Recorded(env)
        ds = dataset(N * P * steps, N * P)
        ds.collect(rec, steps)
        size = ds.size()
        assert 0 < size == ds.total() <= N * P * steps       # nothing wrapped
        got = ring_of(ds)
    finally:
        env.close()
    d = dump.ObservationDump(str(tmp_path), rows_per_file=10 ** 9, use_hdf5=False)
    inactive_with_mask = 0
    for stacked, mask, inertial, la, active in rec.steps:
        armed = active.reshape(-1) != 0         # the collector's env hands over its armed wingmen; ObservationDump.add drops the invalid
        inactive_with_mask += int((mask.reshape(N * P, -1)[~armed] != 0).any(axis=1).sum())
        d.add({"stacked_spheres": stacked.reshape(N * P, *stacked.shape[2:])[armed], "validity_mask": mask.reshape(N * P, -1)[armed],
               "inertial_data": inertial.reshape(N * P, -1)[armed], "last_action": la.reshape(N * P, -1)[armed]}, la.reshape(N * P, -1)[armed])
    d.close()
    print("kept", size, "of", N * P * steps, "; inactive rows with a mask:", inactive_with_mask)
    part = dump.load_part(d.files[0])
    assert len(part["teacher_actions"]) == size
    for k, name in KEYS.items():
        want = part[f"student/{name}"]
        assert np.array_equal(got[k][:size] != 0, want) if k == "mask" else np.array_equal(bits(got[k][:size]), bits(want)), k
    assert np.array_equal(bits(got["teacher"][:size]), bits(part["teacher_actions"]))
    assert not got["stacked"][size:size + 4].any()


def test_an_append_replays_from_a_graph(pool):
    need_gpu()
    import torch
    parts = []
    for a in range(3):
        keep = np.random.default_rng(10 + a).random(21) < 0.7
        parts.append(D.with_pattern({k: v[200 * a:200 * a + 21] for k, v in pool.items()}, keep))
    eager, ring = dataset(32, 21), D.Ring(32)
    for r, active in parts:
        eager.append(*to_dev(r, active))
        ring.append(r, active)
    want = ring_of(eager)
    assert_rings_equal(want, ring.a)

    ds = dataset(32, 21)
    obs, teacher, active = to_dev(*parts[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # a first call outside the capture, as torch.cuda.graph asks for
        ds.append(obs, teacher, active)
    torch.cuda.current_stream().wait_stream(side)
    ds.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ds.append(obs, teacher, active)
    torch.cuda.synchronize()
    assert ds.total() == 0                  # capturing runs nothing
    for r, act in parts:
        o2, t2, a2 = to_dev(r, act)
        for k in obs:
            obs[k].copy_(o2[k])
        teacher.copy_(t2)
        active.copy_(a2)
        graph.replay()
    assert ds.total() == eager.total() == ring.total
    assert_rings_equal(ring_of(ds), want)


def _state_bits(student):
    return {k: v.detach().cpu().numpy().copy() for k, v in student.state_dict().items()}


@pytest.fixture
def repeatable_convolutions():
    """PyTorch's own convolution backward does not repeat bit for bit on this device unless it is asked to: with the default setting
    the hand-written loop below differs from ITSELF in all 58 tensors when run twice (fused_encoder=False; measured), with
    torch.backends.cudnn.deterministic it repeats.  The fused encoder has no float atomics and repeats either way."""
    import torch
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("fused", [False, True])
def test_fit_is_the_hand_written_loop(filled, fused, repeatable_convolutions):
    import torch
    from dronechase_amd.student import FLIAStudent, StudentTrainer
    ds, ring = filled
    torch.manual_seed(1)
    a = FLIAStudent().to(DEV)
    b = copy.deepcopy(a)
    ta, tb = StudentTrainer(a, fused_encoder=fused), StudentTrainer(b, fused_encoder=fused)
    torch.manual_seed(99)
    losses = ta.fit(ds, epochs=2, batch_size=32, kill_high_correlation=False)
    assert tuple(losses.shape) == (6,) and losses.device.type == "cuda" and bool(torch.isfinite(losses).all())
    assert ta.last_modes == ["keep"] * 6

    torch.manual_seed(99)
    by_hand = []
    for _ in range(2):
        perm = torch.randperm(80, device=DEV)
        for at in range(0, 80, 32):
            idx = perm[at:at + 32]
            obs = {"stacked_spheres": ds.stacked.index_select(0, idx), "validity_mask": ds.mask.index_select(0, idx),
                   "inertial_data": ds.inertial.index_select(0, idx), "last_action": ds.last_action.index_select(0, idx)}
            by_hand.append(tb.step(obs, ds.teacher.index_select(0, idx)))
    sa, sb = _state_bits(a), _state_bits(b)
    assert len(sa) == 58
    for k in sa:
        assert np.array_equal(bits(sa[k]), bits(sb[k])), k
    assert np.array_equal(bits(losses.cpu().numpy()), bits(torch.stack(by_hand).cpu().numpy()))


def test_fit_draws_kill_high_correlations_branches(filled):
    import torch
    from dronechase_amd.imitation import last_action_mode
    from dronechase_amd.student import FLIAStudent, StudentTrainer
    ds, ring = filled
    torch.manual_seed(2)
    trainer = StudentTrainer(FLIAStudent().to(DEV), fused_encoder=True)
    losses = trainer.fit(ds, epochs=2, batch_size=32)
    want = [last_action_mode(p) for p in np.random.default_rng(42).random(6)]
    assert trainer.last_modes == want and len(set(want)) > 1
    assert tuple(losses.shape) == (6,) and bool(torch.isfinite(losses).all())
    rng = np.random.default_rng(7)
    trainer.fit(ds, epochs=1, batch_size=80, rng=rng)
    assert trainer.last_modes == [last_action_mode(np.random.default_rng(7).random())] and trainer.batches_fitted == 7
    with pytest.raises(ValueError, match="dataset is empty"):
        trainer.fit(dataset(8, 8))


def test_a_wrapped_ring_round_trips_through_the_dump(pool, tmp_path):
    need_gpu()
    from dronechase_amd.imitation import ImitationDataset
    ds = dataset(32, 21)
    for a in range(3):
        r = {k: v[300 * a:300 * a + 21].copy() for k, v in pool.items()}
        r["mask"] = (r["mask"] != 0).astype(np.uint8)         # the files hold the mask as bool
        ds.append(*to_dev(r))
    assert ds.total() == 63 and ds.size() == 32
    old = ring_of(ds)
    order = ds.logical_index().cpu().numpy()
    assert order.tolist() == [(31 + k) % 32 for k in range(32)]          # oldest first: slot 63 - 32 = 31, then 0, 1, ...
    written = ds.to_dump(str(tmp_path), rows_per_file=10, use_hdf5=False)
    assert written.rows_written == 32 and len(written.files) == 4
    new = ImitationDataset.from_dump(str(tmp_path), DEV, max_append_rows=7)
    assert new.total() == new.size() == new.capacity == 32
    got = ring_of(new)
    for k in D.FIELDS:
        assert np.array_equal(bits(got[k]), bits(old[k][order])), k
    assert np.array_equal(bits(old["stacked"][order[0]]), bits(pool["stacked"][310]))      # row 31 of the 63 appended: the second append's row 10


def test_the_front_end_names_what_is_wrong(filled, pool):
    import torch
    ds, _ = filled
    obs, teacher, _a = to_dev({k: v[:4] for k, v in pool.items()})
    for key, bad, msg in (("stacked_spheres", obs["stacked_spheres"].double(), "stacked_spheres must be a contiguous float32"),
                          ("validity_mask", obs["validity_mask"].float(), "validity_mask must be a contiguous uint8 or bool"),
                          ("inertial_data", obs["inertial_data"][:, :14], "inertial_data must be a contiguous float32"),
                          ("last_action", obs["last_action"].cpu(), "last_action must be a contiguous float32")):
        with pytest.raises(ValueError, match=msg):
            ds.append(dict(obs, **{key: bad}), teacher)
    with pytest.raises(ValueError, match="teacher must be a contiguous float32"):
        ds.append(obs, teacher[:, :3])
    with pytest.raises(ValueError, match="active must be a contiguous uint8 or bool"):
        ds.append(obs, teacher, torch.ones(4, device=DEV))
    big = {k: v[:81] for k, v in pool.items()}
    with pytest.raises(ValueError, match="max_append_rows"):
        ds.append(*to_dev(big))
    with pytest.raises(ValueError, match="last_action_mode must be one of"):
        ds.batch(4, last_action_mode="dropout")
    with pytest.raises(ValueError, match="index must be a contiguous 1-D int64"):
        ds.batch(4, index=torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="index has 3 entries"):
        ds.batch(4, index=torch.zeros(3, dtype=torch.int64, device=DEV))
    assert ds.size() == 80                  # nothing above touched the ring
