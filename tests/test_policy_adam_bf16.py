"""te_policy_adam_step_bf16 (dronechase_amd/csrc/te_policy_opt.hpp, policy_adam_kernel<true>): the optimiser step that leaves the
bf16 copies of the weights current.  Everything is compared BITWISE with the calls it replaces: te_policy_adam_step on a clone of the
same buffers, then te_policy_pack_bf16 and te_policy_pack_bf16_grad on the stepped clone.  The step is one template of the plain
step's kernel, so there is no tolerance: params, the whole state buffer and both bf16 buffers are torch.equal after every step."""
import ctypes as C

import pytest

from tests._policy_cases import _gpu, _shape

pytestmark = pytest.mark.gpu

SHAPES = {"default": (256, (64, 64)), "BO": (512, (128, 256, 512)), "learn": (512, (512, 128, 256))}
INSTANCES = [(name, c) for name in SHAPES for c in (2, 3)]
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-5
MAX_NORMS = (0.5, float("inf"), 0.5)        # three consecutive steps: clipped, not clipped, clipped
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _sizes(lib, shape):
    words, half, half_t, state = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.te_policy_param_words_shaped(C.byref(shape), C.byref(words)) == 0, lib.te_last_error()
    assert lib.te_policy_bf16_words(C.byref(shape), C.byref(half)) == 0, lib.te_last_error()
    assert lib.te_policy_bf16_grad_words(C.byref(shape), C.byref(half_t)) == 0, lib.te_last_error()
    assert lib.te_policy_opt_state_bytes(words.value, C.byref(state)) == 0, lib.te_last_error()
    return words.value, half.value, half_t.value, state.value


def _pack(lib, torch, shape, params, w, wt):
    assert lib.te_policy_pack_bf16(params.data_ptr(), C.byref(shape), w.data_ptr(), _stream(torch)) == 0, lib.te_last_error()
    if wt is not None:
        assert lib.te_policy_pack_bf16_grad(params.data_ptr(), C.byref(shape), wt.data_ptr(), _stream(torch)) == 0, lib.te_last_error()


class Case:
    """Seeded params and three gradients of a shape, and fresh buffers on demand; the inputs are never written."""

    def __init__(self, lib, torch, name, c):
        self.shape = _shape(c, *SHAPES[name])
        self.words, self.half, self.half_t, self.state_bytes = _sizes(lib, self.shape)
        g = torch.Generator(device="cuda:0").manual_seed(7000 + 10 * list(SHAPES).index(name) + c)
        r = lambda scale: scale * torch.randn(self.words, generator=g, device="cuda:0")
        self.p0 = r(0.1)
        self.grads = [r(s) for s in (0.02, 1e-4, 0.3)]

    def fresh(self, lib, torch):
        """(params, state, weights_bf16, weights_bf16_t), the bf16 buffers packed once from the params as the contract asks."""
        i16 = dict(dtype=torch.int16, device="cuda:0")
        p, st = self.p0.clone(), torch.zeros(self.state_bytes // 4, device="cuda:0")
        w, wt = torch.empty(self.half, **i16), torch.empty(self.half_t, **i16)
        _pack(lib, torch, self.shape, p, w, wt)
        return p, st, w, wt


_CASES = {}


def _case(lib, torch, name, c):
    if (name, c) not in _CASES:
        _CASES[(name, c)] = Case(lib, torch, name, c)
    return _CASES[(name, c)]


def _step(lib, torch, case, p, g, st, w, wt, max_norm, plain=False, replace=()):
    a = dict(params=p.data_ptr(), grad=g.data_ptr(), state=st.data_ptr(), state_bytes=st.numel() * 4)
    tail = dict(lr=LR, b1=B1, b2=B2, eps=EPS, max_norm=max_norm, scale=1.0)
    if plain:
        a.update(words=case.words, **tail)
        fn = lib.te_policy_adam_step
    else:
        a.update(shape=C.byref(case.shape), w=None if w is None else w.data_ptr(), wt=None if wt is None else wt.data_ptr(), **tail)
        fn = lib.te_policy_adam_step_bf16
    a.update(replace)       # an argument replaced by name: the refusals
    return fn(*a.values(), _stream(torch))


def _pad_mask(torch, case):
    """True at every pad column of weights_bf16 ([n][Kp], columns K .. Kp - 1) for the case's shape, from the layer table's (N, K)."""
    c, (f, arch) = case.shape.lidar_channels, (case.shape.features_dim, [case.shape.hidden[i] for i in range(case.shape.n_hidden)])
    h = arch + [0] * (3 - len(arch))
    head = [(h[0], f), (h[1], h[0] if h[1] else 0), (h[2], h[1] if h[2] else 0)]
    layers = [(32, 16 * c), (64, 128), (128, 15), (128, 128), (128, 128), (128, 4), (128, 128), (128, 128), (f, 448)] + head + head
    parts = []
    for n, k in layers:
        kp = (k + 31) // 32 * 32
        parts.append((torch.arange(kp, device="cuda:0") >= k).repeat(n))
    return torch.cat(parts)


@pytest.mark.parametrize("name,c", INSTANCES)
def test_bitwise_the_plain_step_and_both_packs(lib, name, c):
    torch = _gpu()
    case = _case(lib, torch, name, c)
    p, st, w, wt = case.fresh(lib, torch)
    rp, rst, rw, rwt = case.fresh(lib, torch)
    pad = _pad_mask(torch, case)
    assert pad.numel() == case.half and bool((w[pad] == 0).all()) and bool(pad.any())
    for k, (g, max_norm) in enumerate(zip(case.grads, MAX_NORMS)):
        assert _step(lib, torch, case, p, g, st, w, wt, max_norm) == 0, lib.te_last_error()
        assert _step(lib, torch, case, rp, g, rst, None, None, max_norm, plain=True) == 0, lib.te_last_error()
        _pack(lib, torch, case.shape, rp, rw, rwt)
        torch.cuda.synchronize()
        assert int(st[0:1].view(torch.int32)) == k + 1
        assert torch.equal(p, rp), (name, c, k, "params")
        assert torch.equal(st.view(torch.int32), rst.view(torch.int32)), (name, c, k, "state")
        assert torch.equal(w, rw), (name, c, k, "weights_bf16", int((w != rw).sum()))
        assert torch.equal(wt, rwt), (name, c, k, "weights_bf16_t", int((wt != rwt).sum()))
        assert bool((w[pad] == 0).all()), (name, c, k, "pad columns")
    assert not torch.equal(p, case.p0) and bool(torch.isfinite(p).all())


def test_without_the_transposed_buffer_it_is_untouched(lib):
    torch = _gpu()
    case = _case(lib, torch, "BO", 3)
    p, st, w, wt = case.fresh(lib, torch)
    rp, rst, rw, _ = case.fresh(lib, torch)
    wt.fill_(SENTINEL)
    assert _step(lib, torch, case, p, case.grads[0], st, w, None, 0.5) == 0, lib.te_last_error()
    assert _step(lib, torch, case, rp, case.grads[0], rst, None, None, 0.5, plain=True) == 0, lib.te_last_error()
    _pack(lib, torch, case.shape, rp, rw, None)
    torch.cuda.synchronize()
    assert bool((wt == SENTINEL).all())
    assert torch.equal(p, rp) and torch.equal(st.view(torch.int32), rst.view(torch.int32)) and torch.equal(w, rw)


def test_pad_columns_are_never_written(lib):
    """The pad columns keep what the first pack left, whatever it was: a sentinel put there survives the step, while every other
    element is the stepped weight's rounding."""
    torch = _gpu()
    case = _case(lib, torch, "default", 2)
    p, st, w, wt = case.fresh(lib, torch)
    pad = _pad_mask(torch, case)
    w[pad] = SENTINEL
    assert _step(lib, torch, case, p, case.grads[0], st, w, wt, 0.5) == 0, lib.te_last_error()
    rw, rwt = torch.empty_like(w), torch.empty_like(wt)
    _pack(lib, torch, case.shape, p, rw, rwt)
    torch.cuda.synchronize()
    assert bool((w[pad] == SENTINEL).all()) and torch.equal(w[~pad], rw[~pad]) and torch.equal(wt, rwt)


def test_repeated_runs_are_equal(lib):
    torch = _gpu()
    case = _case(lib, torch, "learn", 3)
    runs = []
    for _ in range(2):
        p, st, w, wt = case.fresh(lib, torch)
        for g, max_norm in zip(case.grads, MAX_NORMS):
            assert _step(lib, torch, case, p, g, st, w, wt, max_norm) == 0, lib.te_last_error()
        torch.cuda.synchronize()
        runs.append((p, st.view(torch.int32), w, wt))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_refusals_leave_the_outputs_unchanged(lib):
    torch = _gpu()
    case = _case(lib, torch, "default", 3)
    p, st, w, wt = case.fresh(lib, torch)
    before = [t.clone() for t in (p, st, w, wt)]
    g = case.grads[0]
    short = torch.zeros(st.numel() - 1, device="cuda:0")
    unserved = _shape(3, 512, (128, 256))
    cases = [(dict(params=None), b"null"), (dict(grad=None), b"null"), (dict(state=None), b"null"), (dict(w=None), b"weights_bf16 is required"),
             (dict(params=p.data_ptr() + 4), b"params must be 16-byte"), (dict(grad=g.data_ptr() + 8), b"grad must be 16-byte"),
             (dict(state=st.data_ptr() + 4), b"state must be 16-byte"), (dict(w=w.data_ptr() + 2), b"weights_bf16 must be 16-byte"),
             (dict(wt=wt.data_ptr() + 8), b"weights_bf16_t must be 16-byte"), (dict(shape=C.byref(unserved)), b"the served shapes, for lidar_channels 2 and 3: features_dim 256, hidden 64, 64 | features_dim 512"),
             (dict(state=short.data_ptr(), state_bytes=short.numel() * 4), b"state too small"),
             (dict(state_bytes=st.numel() * 4 - 1), b"state too small"),
             (dict(max_norm=0.0), b"max_grad_norm must be > 0"), (dict(max_norm=-1.0), b"max_grad_norm must be > 0")]
    for kw, msg in cases:
        assert _step(lib, torch, case, p, g, st, w, wt, 0.5, replace=kw) != 0, kw
        err = lib.te_last_error()
        assert err.startswith(b"te_policy_adam_step_bf16: ") and msg in err, (kw, err)
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in zip((p, st, w, wt), before)), kw


def test_packed_adam_repack_keeps_the_fused_policy_current(lib):
    """The Python layer: PackedAdam.step(repack=True) on a bound bf16 FusedPolicy against step() + refresh() on a twin."""
    torch = _gpu()
    from dronechase_amd.ppo import FusedPolicy, PackedAdam
    from tests._policy_cases import _policy
    twins = []
    for _ in range(2):
        f = FusedPolicy(_policy(torch, 3, 11), grad_precision="bf16")
        f.bind_parameters()
        twins.append((f, PackedAdam(f, lr=LR)))
    (f, opt), (rf, ropt) = twins
    g = torch.Generator(device="cuda:0").manual_seed(5)
    grad = 0.05 * torch.randn(f.params.numel(), generator=g, device="cuda:0")
    opt.step(grad, 0.5, repack=True)
    ropt.step(grad, 0.5)
    rf.refresh()
    torch.cuda.synchronize()
    assert torch.equal(f.params, rf.params) and torch.equal(opt.state.view(torch.int32), ropt.state.view(torch.int32))
    assert torch.equal(f.weights_bf16, rf.weights_bf16) and torch.equal(f.weights_bf16_t, rf.weights_bf16_t)
    plain = FusedPolicy(_policy(torch, 3, 11))
    with pytest.raises(ValueError, match="repack=True.*owns none"):
        PackedAdam(plain, lr=LR).step(grad, 0.5, repack=True)
