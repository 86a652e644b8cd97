"""The argument checks of the stateless entries that tests/test_policy_abi_messages.py does not cover (the sphere encoder, GAE and
the advantage statistics, the episode monitor, the imitation dataset, the optimiser step and the PPO epoch), message by message:
every entry is called with one bad argument, and the entries with six or more checked arguments with every pair of bad arguments
(which pins the order of the checks), and the return code and the full te_last_error text are compared with
tests/golden/abi_messages.json (the distinct texts, per entry the index of each case's text in the sweep's order, and a digest
of the case ids).

The recording was made from the library of commit 45ca185, the last one before these entries' host code moved out of te_env.hip
onto one pointer check and one launch: with that commit's dronechase_amd first on PYTHONPATH,
`python tests/test_abi_messages.py --record FILE` runs the sweep below and writes FILE.  Every call fails its argument check before
anything touches a device, so no GPU is needed (pointers are fakes, never dereferenced); no case is a valid call, and the recording
refuses a message that does not start with the entry's name."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_messages.json")
N_CASES = 5278          # a case cannot drop out silently
FAKE = 1 << 24          # aligned to everything the entries ask for; the fake buffers lie 2^24 bytes apart, none reaches the next
BO = (512, (128, 256, 512))
NAN, INF = float("nan"), float("inf")

# every distinct kind of text these entries can produce before a launch
FRAGMENTS = (
    ": channels must be 3 (the stacked observation's), not 4", ": n_spheres must be in 1 .. 8, not 9", ": n_rows must be positive, not 0",
    ": n_rows * n_spheres must be at most 2^31 - 1", ": null argument params", ": null argument out_words", ": null argument workspace",
    ": stacked must be 16-byte aligned", ": weights_bf16 must be 16-byte aligned", ": workspace must be 256-byte aligned",
    "te_sphere_encode_grad_workspace_bytes says ", ": null argument", ": n_steps must be positive", ": n_envs must be positive",
    ": n_steps * n_envs must be at most 2^31 - 1", ": gamma must be in [0, 1]", ": gae_lambda must be in [0, 1]",
    ": float arrays must be 4-byte aligned", ": adv and ret must not alias the inputs", ": adv and ret must not alias each other",
    ": n must be positive", ": n must be at most 2^40", ": index must be 8-byte aligned", ": workspace must be 8-byte aligned",
    "te_adv_stats_workspace_bytes says ", ": n_records must be >= 0", ": null monitor buffer", ": the monitor buffer must be 16-byte aligned",
    ": monitor buffer too small (", "te_monitor_bytes says ", ": reward must be 4-byte aligned", ": info must be 16-byte aligned",
    ": out must be 8-byte aligned", ": null argument geom", ": channels must be 3, not 2", ": capacity must be in 1 .. 2^31 - 1, not 0",
    ": max_append_rows must be in 1 .. capacity (1000), not 1001", ": null argument ds", ": ds must be 16-byte aligned", ": ds too small (bytes is ",
    ": n_rows must be in 1 .. max_append_rows (64), not 65", ": null argument mask", ": teacher must be 4-byte aligned",
    ": batch must be >= 1, not 0", ": last_action_mode must be 0 (keep), 1 (random) or 2 (noise), not 3", ": noise_std must be finite and >= 0",
    ": out_index must be 8-byte aligned", ": null argument out_teacher", ": out_stacked must be 16-byte aligned",
    ": words must be positive", ": words must be at most 2^40", ": state must be 16-byte aligned", ": state too small (",
    "te_policy_opt_state_bytes says ", ": lr must be finite and >= 0", ": beta1 must be in [0, 1)", ": beta2 must be in [0, 1)",
    ": eps must be finite and > 0", ": max_grad_norm must be > 0 (INFINITY: no clipping)", ": grad_scale must be finite",
    ": weights_bf16 is required", ": weights_bf16_t must be 16-byte aligned", ": args->struct_size is 0, sizeof(te_ppo_epoch_args) is ",
    ": batch must be >= 1", ": n_perm must be >= 1", ": n_perm must be at most 2^40", ": perm is required", ": perm must be 8-byte aligned",
    ": weights_bf16 and weights_bf16_t go together", ": adv_mean_std, stats and sums are required", ": sums must be 4-byte aligned",
    ": n must be at most 2^27", "te_policy_grad_bf16_workspace_bytes says ", ": clip_range must be finite and >= 0", ": null shape")


def _shape(c, features_dim, net_arch, n_hidden=None):
    from dronechase_amd import _lib
    h = list(net_arch)[:4] + [0] * (4 - min(4, len(net_arch)))
    return _lib.PolicyShape(c, features_dim, len(net_arch) if n_hidden is None else n_hidden, (C.c_int32 * 4)(*h))


def _bad_shapes():
    """(label, shape): the unserved shapes of tests/test_policy_abi_messages.py."""
    return [("shape=F300", _shape(3, 300, (64, 64))), ("shape=h128,256", _shape(3, 512, (128, 256))),
            ("shape=h128,256,100", _shape(3, 512, (128, 256, 100))), ("shape=C4", _shape(4, *BO)),
            ("shape=n_hidden0", _shape(3, 256, (64, 64), n_hidden=0))]


def _size(fn, *first):
    out = C.c_size_t()
    assert fn(*first, C.byref(out)) == 0
    return out.value


def _null(*names):
    return [(f"{k}=null", {k: None}) for k in names]


def _off(by, base, *names):
    """each pointer `by` bytes off: less than the alignment it must have"""
    return [(f"{k}+{by}", {k: base[k] + by}) for k in names]


def _values(name, *values):
    return [(f"{name}={v}", {name: v}) for v in values]


def _fakes(*names):
    return {k: FAKE * (i + 1) for i, k in enumerate(names)}


def _positional(lib, entry):
    return lambda a: getattr(lib, entry)(*a.values())


def _entries(lib):
    """(entry, call, base arguments by name, [(label, {argument: bad value})] swept alone and in pairs, the same swept alone only).
    call(arguments) makes the call.  The base arguments are valid and never passed as they are; each change on its own makes the
    call fail."""
    from dronechase_amd import _lib
    out, none = [], []
    size = C.c_size_t()
    ch_bad = _values("ch", 2, 4)

    def add(entry, base, bad, pairs, solo=(), call=None):
        out.append((entry, call or _positional(lib, entry), base, bad if pairs else none, list(solo) if pairs else list(bad) + list(solo)))

    # ---- the sphere encoder
    for entry in ("te_sphere_encode_param_words", "te_sphere_bf16_words"):
        add(entry, dict(ch=3, out=C.byref(size)), ch_bad + _null("out"), True)
    dom_bad = ch_bad + _values("n_spheres", 0, -1, 9) + _values("n_rows", 0, -3, (1 << 31) - 1)
    base = dict(_fakes("params"), ch=3, n_rows=5, n_spheres=6, **{k: v + FAKE for k, v in _fakes("stacked", "mask", "out").items()}, stream=None)
    add("te_sphere_encode", base, dom_bad + _null("params", "stacked", "out") + _off(8, base, "params", "stacked", "out"), True)
    base = dict(params=FAKE, ch=3, out=2 * FAKE, stream=None)
    add("te_sphere_pack_bf16", base, ch_bad + _null("params", "out") + _off(8, base, "params", "out"), False)
    base = dict(_fakes("params", "weights"), ch=3, n_rows=5, n_spheres=6,
                **{k: v + 2 * FAKE for k, v in _fakes("stacked", "mask", "out").items()}, stream=None)
    add("te_sphere_encode_bf16", base,
        dom_bad + _null("params", "weights", "stacked", "out") + _off(8, base, "params", "weights", "stacked", "out"), True)
    add("te_sphere_encode_grad_workspace_bytes", dict(ch=3, n_rows=5, n_spheres=6, out=C.byref(size)), dom_bad + _null("out"), False)
    need = _size(lib.te_sphere_encode_grad_workspace_bytes, 3, 5, 6)
    base = dict(params=FAKE, ch=3, n_rows=5, n_spheres=6, stacked=2 * FAKE, mask=3 * FAKE, out=4 * FAKE, d_out=5 * FAKE, grad=6 * FAKE,
                ws=7 * FAKE, ws_bytes=need, stream=None)
    add("te_sphere_encode_grad", base,
        dom_bad + _null("params", "stacked", "out", "d_out", "grad", "ws") + _off(8, base, "params", "stacked", "out", "d_out", "grad") +
        _off(128, base, "ws") + [("ws_bytes-1", dict(ws_bytes=need - 1))], True)

    # ---- GAE and the advantage statistics
    T, N = 3, 5
    base = dict(n_steps=T, n_envs=N, **{k: v + FAKE for k, v in _fakes("rewards", "values", "dones", "last_value").items()}, gamma=0.99, lam=0.95,
                adv=FAKE * 8, ret=FAKE * 9, stream=None)
    ins = ("rewards", "values", "dones", "last_value")
    alias = [(f"{o}={i}", {o: base[i]}) for o in ("adv", "ret") for i in ins] + \
        [(f"{o}=end of {i}", {o: base[i] + (N if i == "last_value" else T * N) * 4 - 4}) for o in ("adv", "ret") for i in ins] + \
        [(f"end of {o}={i}", {o: base[i] - T * N * 4 + 4}) for o in ("adv", "ret") for i in ins] + \
        [("adv=ret", dict(adv=base["ret"])), ("adv=end of ret", dict(adv=base["ret"] + T * N * 4 - 4)), ("end of adv=ret", dict(adv=base["ret"] - T * N * 4 + 4))]
    add("te_rollout_gae", base,
        _null(*ins, "adv", "ret") + _values("n_steps", 0, -1, (1 << 31) - 1) + _values("n_envs", 0, -1, (1 << 31) - 1) +
        _values("gamma", -0.1, 1.1, NAN) + _values("lam", -0.1, 1.1, NAN) + _off(2, base, *ins, "adv", "ret") + alias, True)
    n_bad = _values("n", 0, -1, (1 << 40) + 1)
    add("te_adv_stats_workspace_bytes", dict(n=4097, out=C.byref(size)), n_bad + _null("out"), True)
    need = _size(lib.te_adv_stats_workspace_bytes, 4097)
    base = dict(x=FAKE, index=2 * FAKE, n=4097, out=3 * FAKE, ws=4 * FAKE, ws_bytes=need, stream=None)
    add("te_adv_stats", base, _null("x", "out", "ws") + n_bad + _off(2, base, "x", "out") + _off(4, base, "index", "ws") +
        [("ws_bytes-1", dict(ws_bytes=need - 1))], False)

    # ---- the episode monitor
    offsets = _lib.MonitorOffsets()
    env_bad = _values("n_envs", 0, -1) + _values("n_records", -1)
    add("te_monitor_bytes", dict(n_envs=257, n_records=16, out=C.byref(size)), env_bad + _null("out"), True)
    add("te_monitor_layout", dict(n_envs=257, n_records=16, out=C.byref(offsets)), env_bad + _null("out"), True)
    need = _size(lib.te_monitor_bytes, 257, 16)
    mon = dict(mon=FAKE, bytes=need, n_envs=257, n_records=16)
    mon_bad = env_bad + _null("mon") + _off(8, mon, "mon") + [("bytes-1", dict(bytes=need - 1))]
    add("te_monitor_init", dict(mon, stream=None), mon_bad, False)
    base = dict(mon, reward=2 * FAKE, done=3 * FAKE, info=4 * FAKE, stream=None)
    add("te_monitor_step", base, mon_bad + _null("reward", "done", "info") + _off(2, base, "reward") + _off(8, base, "info"), False)
    base = dict(mon, out=2 * FAKE, reset_window=0, stream=None)
    add("te_monitor_stats", base, mon_bad + _null("out") + _off(4, base, "out"), False)

    # ---- the imitation dataset
    geom = lambda **kw: C.pointer(_lib.DatasetGeom(**{**dict(capacity=1000, max_append_rows=64, n_spheres=6, channels=3), **kw}))
    geom_bad = _null("geom") + [(f"geom.{k}={v}", dict(geom=geom(**{k: v}))) for k, v in (
        ("channels", 2), ("channels", 4), ("n_spheres", 0), ("n_spheres", 9), ("capacity", 0), ("capacity", -1), ("max_append_rows", 0),
        ("max_append_rows", 1001))]
    layout = _lib.DatasetOffsets()
    add("te_dataset_layout", dict(geom=geom(), out=C.byref(layout)), geom_bad + _null("out"), True)
    assert lib.te_dataset_layout(geom(), C.byref(layout)) == 0
    ds = dict(ds=FAKE, bytes=layout.bytes, geom=geom())
    ds_bad = geom_bad + _null("ds") + _off(8, ds, "ds") + [("bytes-1", dict(bytes=layout.bytes - 1))]
    add("te_dataset_init", dict(ds, stream=None), ds_bad, False)
    base = dict(ds, n_rows=64, **{k: v + FAKE for k, v in _fakes("stacked", "mask", "inertial", "last_action", "teacher", "active").items()},
                stream=None)
    add("te_dataset_append", base, ds_bad + _values("n_rows", 0, -1, 65) + _null("stacked", "mask", "inertial", "last_action", "teacher") +
        _off(8, base, "stacked") + _off(2, base, "inertial", "last_action", "teacher"), True)
    outs = ("out_stacked", "out_mask", "out_inertial", "out_last_action", "out_teacher")
    base = dict(ds, batch=33, index=2 * FAKE, seed=7, draw=1, last_action_mode=2, noise_std=0.1,
                **{k: v + 2 * FAKE for k, v in _fakes(*outs, "out_index").items()}, stream=None)
    add("te_dataset_gather", base, ds_bad + _values("batch", 0, -1) + _values("last_action_mode", -1, 3) + _values("noise_std", -0.1, NAN, INF) +
        _off(4, base, "index", "out_index") + _null(*outs) + _off(8, base, "out_stacked") +
        _off(2, base, "out_inertial", "out_last_action", "out_teacher"), True)

    # ---- the optimiser step
    add("te_policy_opt_state_bytes", dict(words=1000, out=C.byref(size)), _values("words", 0, (1 << 40) + 1) + _null("out"), True)
    hyper_bad = _values("lr", -1.0, NAN, INF) + _values("beta1", -0.1, 1.0, NAN) + _values("beta2", -0.1, 1.0, NAN) + \
        _values("eps", 0.0, -1.0, NAN, INF) + _values("max_grad_norm", 0.0, -1.0, NAN) + _values("grad_scale", NAN, INF)
    hyper = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, grad_scale=1.0)
    need = _size(lib.te_policy_opt_state_bytes, 1000)
    base = dict(params=FAKE, grad=2 * FAKE, state=3 * FAKE, state_bytes=need, words=1000, **hyper, stream=None)
    add("te_policy_adam_step", base, _null("params", "grad", "state") + _off(8, base, "params", "grad", "state") +
        _values("words", 0, (1 << 40) + 1) + [("state_bytes-1", dict(state_bytes=need - 1))] + hyper_bad, True)
    bo = _shape(3, *BO)
    shape_bad = [(label, dict(shape=C.pointer(s))) for label, s in _bad_shapes()]
    words = _size(lib.te_policy_param_words_shaped, C.byref(bo))
    state_bytes = _size(lib.te_policy_opt_state_bytes, words)
    base = dict(params=FAKE, grad=2 * FAKE, state=3 * FAKE, state_bytes=state_bytes, shape=C.pointer(bo), w=4 * FAKE, wt=5 * FAKE, **hyper, stream=None)
    add("te_policy_adam_step_bf16", base, _null("shape") + shape_bad + _null("params", "grad", "state", "w") +
        _off(8, base, "params", "grad", "state", "w", "wt") + [("state_bytes-1", dict(state_bytes=state_bytes - 1))] + hyper_bad, False)

    # ---- the PPO epoch: the bf16 form, 20 rows in minibatches of 8 (a tail of 4)
    ws_bytes = _size(lib.te_policy_grad_bf16_workspace_bytes, C.byref(bo), 8)
    adv_ws_bytes = _size(lib.te_adv_stats_workspace_bytes, 8)
    pointers = ("params", "weights_bf16", "weights_bf16_t", "lidar", "inertial", "last_action", "action", "old_logp", "adv", "ret", "perm", "grad",
                "state", "workspace", "adv_workspace", "adv_mean_std", "stats", "sums")
    base = dict(struct_size=C.sizeof(_lib.PpoEpochArgs), shape=bo, **_fakes(*pointers), n_perm=20, batch=8, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
                state_bytes=state_bytes, **hyper, workspace_bytes=ws_bytes, adv_workspace_bytes=adv_ws_bytes, stream=None)

    def epoch(a):
        a = dict(a)
        stream = a.pop("stream")
        if a.pop("args", 1) is None:
            return lib.te_policy_ppo_epoch(None, stream)
        return lib.te_policy_ppo_epoch(C.byref(_lib.PpoEpochArgs(**a)), stream)

    bad = _null("args") + _values("struct_size", 0, base["struct_size"] - 8) + [(label, dict(shape=s)) for label, s in _bad_shapes()] + \
        _values("batch", 0, -1) + _values("n_perm", 0, -1, (1 << 40) + 1) + \
        _null("perm", "weights_bf16", "adv_mean_std", "stats", "sums", "adv", "adv_workspace", "params", "lidar", "inertial", "last_action", "action",
              "old_logp", "ret", "grad", "workspace", "state") + \
        _off(4, base, "perm", "adv_workspace", "lidar") + _off(2, base, "sums", "adv", "adv_mean_std", "inertial", "last_action", "action", "old_logp",
                                                                "ret", "stats") + \
        _off(8, base, "params", "weights_bf16", "weights_bf16_t", "grad", "state") + _off(128, base, "workspace") + \
        [("adv_workspace_bytes-1", dict(adv_workspace_bytes=adv_ws_bytes - 1)), ("workspace_bytes-1", dict(workspace_bytes=ws_bytes - 1)),
         ("state_bytes-1", dict(state_bytes=state_bytes - 1)),
         ("batch=2^27+1", dict(batch=(1 << 27) + 1, n_perm=1 << 28, adv_workspace_bytes=_size(lib.te_adv_stats_workspace_bytes, 1 << 28)))] + \
        _values("clip_range", -0.1, NAN) + hyper_bad
    # weights_bf16_t=null is refused only while weights_bf16 is given: alone, never in a pair with weights_bf16=null (the fp32 form, a valid call)
    add("te_policy_ppo_epoch", base, bad, True, solo=_null("weights_bf16_t"), call=epoch)
    return out


def _sweep(lib):
    """[(case id, return code, te_last_error)] of every case, in a fixed order."""
    got = []
    for entry, call, base, bad, solo in _entries(lib):
        def case(label, *changes):
            rc = call({**base, **{k: v for kw in changes for k, v in kw.items()}})
            got.append((f"{entry}({label})", int(rc), lib.te_last_error().decode()))

        for label, kw in bad + solo:
            case(label, kw)
        for (la, a), (lb, b) in itertools.combinations(bad, 2):
            if not set(a) & set(b):      # two bad values of one argument are not a pair
                case(f"{la}, {lb}", a, b)
    return got


def _case_ids_digest(got):
    return hashlib.sha256("\n".join(k for k, _, _ in got).encode()).hexdigest()


def _record(lib, path):
    """The golden file: the distinct texts behind "entry: ", and per entry the index of each case's text in the order of the sweep (every
    return code is 1); the case ids themselves are pinned by their digest."""
    got = _sweep(lib)
    assert len({k for k, _, _ in got}) == len(got)
    for case, rc, msg in got:      # a call that got past its checks would say what HIP said
        assert rc == 1 and msg.startswith(case.split("(")[0] + ": "), (case, rc, msg)
    text = lambda case, msg: msg[len(case.split("(")[0]) + 2:]
    messages = sorted({text(k, m) for k, _, m in got})
    cases = {}
    for k, _, m in got:
        cases.setdefault(k.split("(")[0], []).append(messages.index(text(k, m)))
    with open(path, "w") as f:
        rows = lambda v: ",\n".join(", ".join(str(i) for i in v[at:at + 40]) for at in range(0, len(v), 40))
        f.write('{"case_ids_sha256": "' + _case_ids_digest(got) + '",\n"messages": [\n' + ",\n".join(json.dumps(m) for m in messages) +
                '],\n"cases": {\n' + ",\n".join(f"{json.dumps(e)}: [\n{rows(v)}]" for e, v in cases.items()) + "}}\n")
    print(f"{len(got)} cases, {len(messages)} distinct texts -> {path}")


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def test_every_message_is_the_recorded_one(lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sum(len(v) for v in golden["cases"].values()) == N_CASES
    for fragment in FRAGMENTS:
        assert any(fragment in ": " + m for m in golden["messages"]), fragment
    got = _sweep(lib)
    assert len(got) == N_CASES and _case_ids_digest(got) == golden["case_ids_sha256"]
    at = {entry: iter(v) for entry, v in golden["cases"].items()}
    want = [f"{k.split('(')[0]}: {golden['messages'][next(at[k.split('(')[0]])]}" for k, _, _ in got]
    wrong = [(k, rc, msg, w) for (k, rc, msg), w in zip(got, want) if (rc, msg) != (1, w)]
    assert not wrong, (len(wrong), wrong[:5])


if __name__ == "__main__":
    assert sys.argv[1] == "--record"
    from dronechase_amd import _lib as _abi
    _record(_abi.load(), sys.argv[2])
