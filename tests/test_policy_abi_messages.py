"""The policy entries' argument checks, message by message: every entry is called with one bad argument, and the act and gradient
entries with every pair of bad arguments (which pins the order of the checks), and the return code and the full te_last_error text
are compared with tests/golden/policy_abi_messages.json.

The recording was made from the library of commit 4a63be5, the last one before the entries' checks were merged into one function
per kind of call: with that commit's dronechase_amd first on PYTHONPATH, `python tests/test_policy_abi_messages.py --record FILE`
runs the sweep below and writes FILE.  Every call fails its argument check before anything touches a device, so no GPU is needed
(pointers are fakes, never dereferenced); no case is a valid call, and the recording refuses a message that is not an entry's own."""
import ctypes as C
import itertools
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_abi_messages.json")
N_CASES = 3160          # a case cannot drop out silently
FAKE = 1 << 20          # 2^20: aligned to everything the entries ask for
DEFAULT = (256, (64, 64))
BO = (512, (128, 256, 512))
NAN = float("nan")

# every distinct text the entries can produce before a launch (the shape messages go on with the list of served shapes)
FRAGMENTS = (
    "te_policy: lidar_channels must be 2 or 3", ": null shape", ": lidar_channels must be 2 or 3, not 4; the served shapes",
    ": n_hidden must be 1, 2 or 3, not 0", ": features_dim 300 is not served", ": hidden [128, 256] is not served with features_dim 512",
    ": hidden [128, 256, 100] is not served", ": null argument", ": n must be positive", ": n must be at most 2^27",
    ": eps given, so action, logp and action_env must be too", ": params must be 16-byte aligned", ": weights_bf16 must be 16-byte aligned",
    ": weights_bf16_t must be 16-byte aligned", ": out must be 16-byte aligned", ": grad must be 16-byte aligned",
    ": lidar must be 8-byte aligned", ": index must be 8-byte aligned", ": workspace must be 256-byte aligned",
    ": float arrays must be 4-byte aligned", ": workspace too small (", "te_policy_grad_workspace_bytes says ",
    "te_policy_grad_workspace_bytes_shaped says ", "te_policy_grad_bf16_workspace_bytes says ", ": clip_range must be finite and >= 0",
    "te_drive_wingman: null env", "te_drive_wingman_shaped: null env")


def _shape(c, features_dim, net_arch, n_hidden=None):
    from dronechase_amd import _lib
    h = list(net_arch)[:4] + [0] * (4 - min(4, len(net_arch)))
    return _lib.PolicyShape(c, features_dim, len(net_arch) if n_hidden is None else n_hidden, (C.c_int32 * 4)(*h))


def _bad_shapes():
    """(label, shape): null, and the unserved shapes of tests/test_policy_grad_shapes.py."""
    return [("shape=null", None), ("shape=F300", _shape(3, 300, (64, 64))), ("shape=h128,256", _shape(3, 512, (128, 256))),
            ("shape=h128,256,100", _shape(3, 512, (128, 256, 100))), ("shape=C4", _shape(4, *BO)),
            ("shape=n_hidden0", _shape(3, 256, (64, 64), n_hidden=0))]


def _size(fn, *first):
    out = C.c_size_t()
    assert fn(*first, C.byref(out)) == 0
    return out.value


def _entries(lib):
    """(entry, base arguments by name, in the entry's order, [(label, {argument: bad value})]) of the six entries swept in pairs.
    The base arguments are valid and never passed as they are; each change on its own makes the call fail."""
    bad_shapes = [(label, dict(shape=None if s is None else C.byref(s))) for label, s in _bad_shapes()]
    bad_channels = [("ch=1", dict(ch=1)), ("ch=4", dict(ch=4))]
    null = lambda *names: [(f"{k}=null", {k: None}) for k in names]
    off = lambda by, *names: [(f"{k}+{by}", {k: FAKE + by}) for k in names]
    bo = _shape(3, *BO)

    io = dict(lidar=FAKE, inertial=FAKE, last_action=FAKE, eps=FAKE, mu=FAKE, value=FAKE, action=FAKE, logp=FAKE, action_env=FAKE, stream=None)
    act_bad = [("n=0", dict(n=0)), ("n=-3", dict(n=-3))] + null("params", "lidar", "inertial", "last_action", "mu", "value", "action", "logp",
                                                                "action_env") + off(8, "params") + off(4, "lidar") + \
        off(2, "inertial", "last_action", "eps", "mu", "value", "action", "logp", "action_env")
    w_bad = null("weights") + off(8, "weights")
    out = [("te_policy_act", dict(params=FAKE, ch=3, n=8, **io), bad_channels + act_bad),
           ("te_policy_act_shaped", dict(params=FAKE, shape=C.byref(bo), n=8, **io), bad_shapes + act_bad),
           ("te_policy_act_bf16", dict(params=FAKE, weights=FAKE, shape=C.byref(bo), n=8, **io), bad_shapes + act_bad + w_bad)]

    rows = dict(index=None, lidar=FAKE, inertial=FAKE, last_action=FAKE, action=FAKE, old_logp=FAKE, adv=FAKE, ret=FAKE, ms=None, clip=0.2,
                vf=0.5, ent=0.0, grad=FAKE, stats=FAKE, ws=FAKE)
    grad_bad = [("n=0", dict(n=0)), ("n=-3", dict(n=-3)), ("n=2^27+1", dict(n=(1 << 27) + 1))] + \
        null("params", "lidar", "inertial", "last_action", "action", "old_logp", "adv", "ret", "grad", "stats", "ws") + \
        off(8, "params", "grad") + off(4, "lidar", "index") + off(128, "ws") + \
        off(2, "inertial", "last_action", "action", "old_logp", "adv", "ret", "ms", "stats") + \
        [("clip=-0.1", dict(clip=-0.1)), ("clip=nan", dict(clip=NAN))]
    wt_bad = w_bad + null("weights_t") + off(8, "weights_t")

    def sizes(need, other):      # one byte short, and the size of another shape's workspace, which must be a smaller one
        assert 0 < other < need
        return [("ws_bytes-1", dict(ws_bytes=need - 1)), ("ws_bytes=other", dict(ws_bytes=other))]

    need = _size(lib.te_policy_grad_workspace_bytes, 3, 8)
    out.append(("te_policy_ppo_grad", dict(params=FAKE, ch=3, n=8, **rows, ws_bytes=need, stream=None),
                bad_channels + grad_bad + sizes(need, _size(lib.te_policy_grad_workspace_bytes, 2, 8))))
    dflt = _shape(3, *DEFAULT)
    need = _size(lib.te_policy_grad_workspace_bytes_shaped, C.byref(bo), 8)
    out.append(("te_policy_ppo_grad_shaped", dict(params=FAKE, shape=C.byref(bo), n=8, **rows, ws_bytes=need, stream=None),
                bad_shapes + grad_bad + sizes(need, _size(lib.te_policy_grad_workspace_bytes_shaped, C.byref(dflt), 8))))
    need = _size(lib.te_policy_grad_bf16_workspace_bytes, C.byref(bo), 8)
    out.append(("te_policy_ppo_grad_bf16", dict(params=FAKE, weights=FAKE, weights_t=FAKE, shape=C.byref(bo), n=8, **rows, ws_bytes=need, stream=None),
                bad_shapes + grad_bad + wt_bad + sizes(need, _size(lib.te_policy_grad_bf16_workspace_bytes, C.byref(dflt), 8))))
    return out


def _sweep(lib):
    """[(case id, return code, te_last_error)] of every case, in a fixed order."""
    got = []

    def call(entry, label, *args):
        rc = getattr(lib, entry)(*args)
        got.append((f"{entry}({label})", int(rc), lib.te_last_error().decode()))

    for entry, base, bad in _entries(lib):
        for label, kw in bad:
            call(entry, label, *{**base, **kw}.values())
        for (la, a), (lb, b) in itertools.combinations(bad, 2):
            if not set(a) & set(b):      # two bad values of one argument are not a pair
                call(entry, f"{la}, {lb}", *{**base, **a, **b}.values())

    # the smaller entries, one bad argument at a time
    size, bo = C.c_size_t(), _shape(3, *BO)
    shapes = [(label, None if s is None else C.byref(s)) for label, s in _bad_shapes()]
    for entry in ("te_policy_pack_bf16", "te_policy_pack_bf16_grad"):
        for label, s in shapes:
            call(entry, label, FAKE, s, FAKE, None)
        for label, params, out in (("params=null", None, FAKE), ("out=null", FAKE, None), ("params+8", FAKE + 8, FAKE), ("out+8", FAKE, FAKE + 8)):
            call(entry, label, params, C.byref(bo), out, None)
    for entry in ("te_policy_param_words_shaped", "te_policy_bf16_words", "te_policy_bf16_grad_words"):
        for label, s in shapes:
            call(entry, label, s, C.byref(size))
        call(entry, "out=null", C.byref(bo), None)
        call(entry, "out=null, shape=null", None, None)
    for entry in ("te_policy_grad_workspace_bytes_shaped", "te_policy_grad_bf16_workspace_bytes"):
        for label, s in shapes:
            call(entry, label, s, 8, C.byref(size))
        for n in (0, -3, (1 << 27) + 1):
            call(entry, f"n={n}", C.byref(bo), n, C.byref(size))
        call(entry, "out=null", C.byref(bo), 8, None)
        call(entry, "out=null, shape=null, n=0", None, 0, None)
        call(entry, "shape=null, n=0", None, 0, C.byref(size))
    for c in (1, 4):
        call("te_policy_grad_workspace_bytes", f"ch={c}", c, 8, C.byref(size))
        call("te_policy_grad_workspace_bytes", f"ch={c}, n=0", c, 0, C.byref(size))
        call("te_policy_param_words", f"ch={c}", c, C.byref(size))
    for n in (0, -3, (1 << 27) + 1):
        call("te_policy_grad_workspace_bytes", f"n={n}", 3, n, C.byref(size))
    call("te_policy_grad_workspace_bytes", "out=null", 3, 8, None)
    call("te_policy_grad_workspace_bytes", "out=null, ch=4, n=0", 4, 0, None)
    call("te_policy_param_words", "out=null", 3, None)
    call("te_policy_param_words", "out=null, ch=4", 4, None)
    for label, s in shapes:
        call("te_policy_shape_check", label, s)
    # the wingman entries check their other arguments against a te_env, which needs a device
    call("te_drive_wingman", "env=null", None, 1, FAKE, 3, FAKE, FAKE, FAKE, FAKE, None)
    call("te_drive_wingman_shaped", "env=null", None, 1, FAKE, C.byref(bo), FAKE, FAKE, FAKE, FAKE, None)
    return got


def _record(lib, path):
    got = _sweep(lib)
    assert len({k for k, _, _ in got}) == len(got)
    for case, rc, msg in got:      # a call that got past its checks would say what HIP said
        assert rc == 1 and (msg.startswith(case.split("(")[0] + ": ") or msg == "te_policy: lidar_channels must be 2 or 3"), (case, rc, msg)
    messages = sorted({m for _, _, m in got})
    with open(path, "w") as f:
        lines = [f"{json.dumps(k)}: [{rc}, {messages.index(m)}]" for k, rc, m in sorted(got)]      # one case, one message per line
        f.write('{"messages": [\n' + ",\n".join(json.dumps(m) for m in messages) + '],\n"cases": {\n' + ",\n".join(lines) + "}}\n")
    print(f"{len(got)} cases, {len(messages)} distinct messages -> {path}")


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def test_every_message_is_the_recorded_one(lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    want = {k: (rc, golden["messages"][i]) for k, (rc, i) in golden["cases"].items()}
    assert len(want) == N_CASES
    for fragment in FRAGMENTS:
        assert any(fragment in m for m in golden["messages"]), fragment
    got = _sweep(lib)
    assert len(got) == N_CASES and {k for k, _, _ in got} == set(want)
    wrong = [(k, rc, msg, want[k]) for k, rc, msg in got if (rc, msg) != want[k]]
    assert not wrong, (len(wrong), wrong[:5])


if __name__ == "__main__":
    assert sys.argv[1] == "--record"
    from dronechase_amd import _lib as _abi
    _record(_abi.load(), sys.argv[2])
