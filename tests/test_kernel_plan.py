"""te_kernel_plan: which kernels te_create picks per task, shard size and environment knob, pinned without a GPU.  Each row was derived
by hand from the selection te_create made before the choice became one plan (KernelPlan, te_env.hip), so a change of the selection
shows up here as a changed row."""
import pytest

F, T = "false", "true"


def sub(fam, fill, noise=T, ces=T, help=F):
    return f"substeps_kernel<{fam}, {noise}, {fill}, {ces}, {help}>"


def plan(fam, engage, noise=T, ces=T, help=F, push=None, view=None, wingman=None):
    out = {"substeps": sub(fam, T, noise, ces, help), "substeps_nofill": sub(fam, F, noise, ces, help), "engage": engage}
    if push:
        out["ring_push"] = push
    if view:
        out["stack_view"] = view
    if wingman:
        out["wingman_view"] = wingman
    return out


SLOTS = "engage_slots_kernel<16>"
S02_SLOTS = "engage_slots_stage02_kernel<16>"
MULTI = "engage_slots_multi_kernel<{}, {}, {}>"
V18, V37 = "stack_view_kernel<18>", "stack_view_kernel<37>"
P18_4, P18_1, P37_1 = "ring_push_kernel<18, 4>", "ring_push_kernel<18, 1>", "ring_push_kernel<37, 1>"
W1, W2 = "observe_ally_kernel", "ally_view_kernel+ally_patch_kernel"   # te_observe_wingman in one launch / in two

# (task, n_envs, config overrides, environment knobs) -> kernels
ROWS = [
    # every preset, a small (16 chunks) and a large (1 024 chunks) shard
    ("stage01", 1024, {}, {}, plan(1, "engage_stage01_kernel", help=T)),
    ("stage01", 65536, {}, {}, plan(1, "engage_stage01_kernel")),
    ("stage02", 1024, {}, {}, plan(2, S02_SLOTS, help=T)),
    ("stage02", 65536, {}, {}, plan(2, S02_SLOTS)),
    ("exp02", 1024, {}, {}, plan(0, SLOTS, help=T)),
    ("exp02", 65536, {}, {}, plan(0, SLOTS)),
    ("exp03", 1024, {}, {}, plan(0, SLOTS, help=T)),
    ("exp03", 65536, {}, {}, plan(0, SLOTS)),
    ("stage03", 1024, {}, {}, plan(0, SLOTS, help=T)),
    ("stage03", 65536, {}, {}, plan(0, SLOTS)),
    ("exp04", 1024, {}, {}, plan(0, SLOTS, help=T)),
    ("exp04", 65536, {}, {}, plan(0, SLOTS)),
    ("exp05", 1024, {}, {}, plan(0, SLOTS, help=T, wingman=W1)),
    ("exp05", 65536, {}, {}, plan(0, SLOTS, wingman=W2)),
    ("evaluation", 1024, {}, {}, plan(0, SLOTS, help=T)),
    ("evaluation", 65536, {}, {}, plan(0, SLOTS)),
    ("level5", 1024, {}, {}, plan(0, MULTI.format(2, F, F), push=P18_4, view=V18)),
    ("level5", 65536, {}, {}, plan(0, MULTI.format(3, F, F), push=P18_1, view=V18)),
    ("level5_c1", 1024, {}, {}, plan(0, MULTI.format(1, F, F), help=T, push=P18_4, view=V18)),
    ("level5_c1", 65536, {}, {}, plan(0, MULTI.format(2, F, F), push=P18_1, view=V18)),
    ("level5_2bt", 1024, {}, {}, plan(0, MULTI.format(2, T, F), help=T)),
    ("level5_2bt", 65536, {}, {}, plan(0, MULTI.format(2, T, F))),
    # 36 / 37 drones: 64-bit slot masks
    ("level5_fusion", 1024, {}, {}, plan(0, MULTI.format(3, F, T), push=P37_1, view=V37)),
    ("level5_fusion", 65536, {}, {}, plan(0, MULTI.format(3, F, T), push=P37_1, view=V37)),
    ("level5_dumb", 1024, {}, {}, plan(0, MULTI.format(3, F, T), push=P37_1, view=V37)),
    ("level5_dumb", 65536, {}, {}, plan(0, MULTI.format(3, F, T), push=P37_1, view=V37)),
    # drone contact: engage_kernel's own instantiation, no slot waves
    ("exp02", 1024, {"drone_contact": 1}, {}, plan(0, "engage_kernel<2, 9, true>", help=T)),
    ("exp03", 4096, {"drone_contact": 1, "n_pursuers": 4, "n_invaders": 12}, {}, plan(0, "engage_kernel<6, 12, true>", help=T)),
    # the noise helper: n_envs x D <= 98 304 pairs, or in the level4 family at most 1 280 chunk x min(D, P + 2) waves
    ("stage01", 32768, {}, {}, plan(1, "engage_stage01_kernel", help=T)),
    ("stage01", 32769, {}, {}, plan(1, "engage_stage01_kernel")),
    ("stage03", 20480, {}, {}, plan(0, SLOTS, help=T)),
    ("stage03", 20481, {}, {}, plan(0, SLOTS)),
    ("stage03", 1024, {"motor_noise": 0}, {}, plan(0, SLOTS, noise=F)),
    ("stage03", 1024, {"control_every_substep": 0}, {}, plan(0, SLOTS, ces=F, help=T)),
    ("stage03", 1024, {"substeps": 49}, {}, plan(0, SLOTS)),
    ("exp03", 1024, {"n_pursuers": 5, "n_invaders": 9}, {}, plan(0, "engage_kernel<6, 12, false>")),
    # level5: one more slot per wave once chunks x 9 waves exceed 256 CUs x 24 waves (682 / 683 chunks)
    ("level5", 43648, {}, {}, plan(0, MULTI.format(2, F, F), push=P18_1, view=V18)),
    ("level5", 43649, {}, {}, plan(0, MULTI.format(3, F, F), push=P18_1, view=V18)),
    # the ring push dealt over four waves up to 4 096 chunk x wingman x 4 waves
    ("level5", 10880, {}, {}, plan(0, MULTI.format(2, F, F), push=P18_4, view=V18)),
    ("level5", 10881, {}, {}, plan(0, MULTI.format(2, F, F), push=P18_1, view=V18)),
    # knobs
    ("stage03", 1024, {}, {"TE_ENGAGE": "slots"}, plan(0, SLOTS, help=T)),
    ("stage03", 1024, {}, {"TE_ENGAGE": "regs"}, plan(0, "engage_kernel<2, 9, false>", help=T)),
    ("stage03", 1024, {}, {"TE_ENGAGE": "lds"}, plan(0, "engage_observe_kernel<0, 256>", help=T)),
    ("exp03", 1024, {"n_pursuers": 4, "n_invaders": 12}, {"TE_ENGAGE": "regs"}, plan(0, "engage_kernel<6, 12, false>", help=T)),
    ("stage02", 1024, {}, {"TE_ENGAGE": "regs"}, plan(2, "engage_stage02_kernel<2, 8>", help=T)),
    ("stage02", 1024, {}, {"TE_ENGAGE": "lds"}, plan(2, "engage_observe_kernel<2, 256>", help=T)),
    ("stage01", 1024, {}, {"TE_ENGAGE": "lds"}, plan(1, "engage_observe_kernel<1, 256>", help=T)),
    ("level5", 1024, {}, {"TE_ENGAGE": "regs"}, plan(0, "engage_kernel<6, 12, false>", push=P18_4, view=V18)),
    ("level5", 1024, {}, {"TE_ENGAGE": "lds"}, plan(0, "engage_observe_kernel<0, 512>", push=P18_4, view=V18)),
    ("level5_dumb", 1024, {}, {"TE_ENGAGE": "regs"}, plan(0, "engage_kernel<7, 30, false>", push=P37_1, view=V37)),
    ("level5_2bt", 1024, {}, {"TE_ENGAGE": "regs"}, plan(0, "engage_kernel<7, 30, false>", help=T)),
    ("stage03", 1024, {}, {"TE_SLOT_SPW": "2"}, plan(0, MULTI.format(2, T, F), help=T)),
    ("stage03", 1024, {}, {"TE_SLOT_SPW": "1"}, plan(0, SLOTS, help=T)),
    ("level5", 1024, {}, {"TE_SLOT_SPW": "3"}, plan(0, MULTI.format(3, F, F), push=P18_4, view=V18)),
    ("level5_c1", 1024, {}, {"TE_SLOT_SPW": "2"}, plan(0, MULTI.format(2, F, F), help=T, push=P18_4, view=V18)),
    ("stage03", 1024, {}, {"TE_K1_HELP": "0"}, plan(0, SLOTS)),
    ("stage03", 65536, {}, {"TE_K1_HELP": "1"}, plan(0, SLOTS, help=T)),
    ("stage03", 1024, {"motor_noise": 0}, {"TE_K1_HELP": "1"}, plan(0, SLOTS, noise=F)),
    ("level5", 1024, {}, {"TE_K1_HELP": "1"}, plan(0, MULTI.format(2, F, F), push=P18_4, view=V18)),
    ("level5", 1024, {}, {"TE_PUSH_SPLIT": "0"}, plan(0, MULTI.format(2, F, F), push=P18_1, view=V18)),
    ("level5", 65536, {}, {"TE_PUSH_SPLIT": "1"}, plan(0, MULTI.format(3, F, F), push=P18_4, view=V18)),
    ("level5_dumb", 1024, {}, {"TE_PUSH_SPLIT": "1"}, plan(0, MULTI.format(3, F, T), push=P37_1, view=V37)),
    ("level5", 1024, {}, {"TE_STACKED": "lds"}, plan(0, MULTI.format(2, F, F), view="stacked_kernel")),
    ("level5_fusion", 1024, {}, {"TE_STACKED": "lds"}, plan(0, MULTI.format(3, F, T), view="stacked_kernel")),
    ("stage03", 1024, {}, {"TE_DENSE_MIN": "1"}, plan(0, SLOTS, help=T)),
    ("stage03", 1024, {}, {"TE_FILL_WAVES": "512"}, plan(0, SLOTS, help=T)),
    # a caller-driven pursuer's observation: two launches from 4 096 envs, when n_envs x lidar words is whole 16-byte quads
    # (3 channels: 1 014 words, so an odd n_envs is not; 2 channels: 676 words, always) fewer than 2^32
    ("exp05", 4095, {}, {}, plan(0, SLOTS, help=T, wingman=W1)),
    ("exp05", 4096, {}, {}, plan(0, SLOTS, help=T, wingman=W2)),
    ("exp05", 4097, {}, {}, plan(0, SLOTS, help=T, wingman=W1)),
    ("exp05", 4097, {"lidar_channels": 2}, {}, plan(0, SLOTS, help=T, wingman=W2)),
    # Evaluation_Task with both pursuers driven by the caller (9 rounds = te_calculate_rounds(2, 20)); the preset's own mask is 0: no line
    ("evaluation", 65536, {"evaluation": 1 | (0b11 << 8), "n_pursuers": 2, "n_rounds": 9, "n_invaders": 9}, {}, plan(0, SLOTS, wingman=W2)),
]
KNOBS = ("TE_ENGAGE", "TE_SLOT_SPW", "TE_K1_HELP", "TE_PUSH_SPLIT", "TE_STACKED", "TE_DENSE_MIN", "TE_FILL_WAVES")


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()  # hipcc cross-compiles gfx950 without a GPU
    return _lib


@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("task,n,over,env,want", ROWS, ids=[f"{r[0]}-{r[1]}-{i}" for i, r in enumerate(ROWS)])
def test_plan_table(lib, knobs, task, n, over, env, want):
    from dronechase_amd import default_config
    for k, v in env.items():
        knobs.setenv(k, v)
    assert lib.kernel_plan(default_config(task, n_envs=n, **over)) == want


def test_plan_fails_with_te_creates_message(lib, knobs):
    from dronechase_amd import default_config
    with pytest.raises(lib.TEError, match="te_create: n_envs < 1"):
        lib.kernel_plan(default_config("stage03", n_envs=0))
    with pytest.raises(lib.TEError, match="te_create: more than 32 drones per env are served for the stacked-observation tasks only"):
        lib.kernel_plan(default_config("exp03", n_envs=64, n_pursuers=2, n_invaders=31))
    with pytest.raises(lib.TEError, match="te_create: cfg.drone_contact is built into engage_kernel"):
        lib.kernel_plan(default_config("exp03", n_envs=64, drone_contact=1, n_pursuers=7, n_invaders=12))
    knobs.setenv("TE_ENGAGE", "lds")   # the LDS engage kernel has neither the contact pass nor the level5 rules
    with pytest.raises(lib.TEError, match="te_create: cfg.drone_contact is built into engage_kernel"):
        lib.kernel_plan(default_config("exp02", n_envs=64, drone_contact=1))
    with pytest.raises(lib.TEError, match="te_create: agent_scripted / reward_model"):
        lib.kernel_plan(default_config("level5_c1", n_envs=64))


def test_plan_output_buffer(lib):
    import ctypes as C
    from dronechase_amd import default_config
    cfg = default_config("level5", n_envs=64)
    small = C.create_string_buffer(16)
    assert lib.load().te_kernel_plan(C.byref(cfg), small, len(small)) != 0
    assert b"out_bytes too small" in lib.load().te_last_error()
    assert lib.load().te_kernel_plan(None, small, len(small)) != 0
