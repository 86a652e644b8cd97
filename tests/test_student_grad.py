"""te_sphere_encode_grad without a GPU: the ABI's declarations, the host-side refusals (which return before anything is launched), the
conditions of the fixtures in tests/_student_grad_cases.py, and the Python front-end's refusals of a CPU student."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import _student_cases as S
from tests import _student_grad_cases as G

FAKE = 1 << 20          # never dereferenced: every call below fails a check first
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "threatengage.h")
WORDS = 32 * 75 + 32 + 64 * 288 + 64


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def test_header_declares_and_the_binding_exports_both_functions(lib):
    from dronechase_amd import _lib
    with open(HEADER) as f:
        body = f.read()
    for name in ("te_sphere_encode_grad_workspace_bytes", "te_sphere_encode_grad"):
        assert re.search(rf"\bint {name}\s*\(", body) and name in _lib.EXPORTS and getattr(lib, name) is not None, name
    assert "inference only, no backward" not in body
    assert lib.te_abi_version() == 5


def test_workspace_bytes_and_its_refusals(lib):
    need = C.c_size_t()
    for rows, spheres, groups in ((1, 1, 1), (3, 6, 18), (70, 6, 256), (1 << 20, 8, 256)):
        assert lib.te_sphere_encode_grad_workspace_bytes(3, rows, spheres, C.byref(need)) == 0
        assert need.value % 256 == 0 and 0 <= need.value - groups * WORDS * 4 < 256, (rows, spheres, need.value)
    who = b"te_sphere_encode_grad_workspace_bytes: "
    for args, msg in (((3, 4, 6, None), b"null argument out_bytes"), ((2, 4, 6, C.byref(need)), b"channels must be 3"),
                      ((3, 0, 6, C.byref(need)), b"n_rows must be positive, not 0"), ((3, 4, 9, C.byref(need)), b"n_spheres must be in 1 .. 8, not 9"),
                      ((3, 1 << 30, 8, C.byref(need)), b"n_rows * n_spheres must be at most")):
        assert lib.te_sphere_encode_grad_workspace_bytes(*args) != 0, args
        err = lib.te_last_error()
        assert err.startswith(who) and msg in err, (args, err)


def test_sphere_encode_grad_refusals_come_from_the_host(lib):
    need = C.c_size_t()
    assert lib.te_sphere_encode_grad_workspace_bytes(3, 4, 6, C.byref(need)) == 0
    base = dict(params=FAKE, channels=3, n_rows=4, n_spheres=6, stacked=FAKE, mask=FAKE, out=FAKE, d_out=FAKE, grad=FAKE, workspace=FAKE,
                workspace_bytes=need.value, stream=None)
    cases = [(dict(channels=2), b"channels must be 3"),
             (dict(n_spheres=0), b"n_spheres must be in 1 .. 8, not 0"), (dict(n_spheres=9), b"n_spheres must be in 1 .. 8, not 9"),
             (dict(n_rows=0), b"n_rows must be positive, not 0"), (dict(n_rows=-1), b"n_rows must be positive"),
             (dict(n_rows=1 << 30, n_spheres=8), b"n_rows * n_spheres must be at most"),
             (dict(workspace=None), b"null argument workspace"), (dict(workspace=FAKE + 128), b"workspace must be 256-byte aligned"),
             (dict(workspace_bytes=need.value - 1), b"workspace too small"), (dict(workspace_bytes=0), b"te_sphere_encode_grad_workspace_bytes says")]
    for name in ("params", "stacked", "out", "d_out", "grad"):
        cases.append(({name: None}, b"null argument " + name.encode()))
        cases.append(({name: FAKE + 4}, name.encode() + b" must be 16-byte aligned"))
    for kw, msg in cases:
        args = [kw.get(k, v) for k, v in base.items()]
        assert lib.te_sphere_encode_grad(*args) != 0, kw
        err = lib.te_last_error()
        assert err.startswith(b"te_sphere_encode_grad: ") and msg in err, (kw, err)


def test_the_kinkfree_fixture_keeps_its_margins():
    fx = G.kinkfree()
    m = fx["margins"]
    print(m)
    assert m["spheres"] == 19 <= 48
    assert m["min_abs_z1"] >= G.MARGIN and m["min_abs_z2"] >= G.MARGIN, m
    assert G.ACTIVE[0] <= m["active1"] <= G.ACTIVE[1] and G.ACTIVE[0] <= m["active2"] <= G.ACTIVE[1], m
    assert [tuple(g.shape) for g in fx["g64"]] == [(32, 3, 5, 5), (32,), (64, 32, 3, 3), (64,)]
    assert all(g.dtype == torch.float64 and torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in fx["g64"])
    # PyTorch's own fp32 gradient is inside the bound the kernel is held to: the bound asks nothing fp32 cannot give
    print("E", fx["E"], "scale", fx["scale"])
    assert all(e <= S.ATOL for e in fx["E"]), (fx["E"], fx["scale"])


@pytest.mark.parametrize("n_rows,n_spheres,mixed", G.EXACT_CASES)
def test_the_exact_fixture_is_exact_in_fp32(n_rows, n_spheres, mixed):
    fx = G.exact(n_rows, n_spheres, mixed)
    print(n_rows, n_spheres, int(fx["counts"].sum()), fx["units"], fx["min_abs_z1"], fx["z2_zeros"], fx["active1"], fx["active2"])
    assert all(u < 2 ** 24 for u in fx["units"].values()), fx["units"]
    assert fx["min_abs_z1"] >= 1 / 16
    assert 0.05 < fx["active1"] < 0.95 and 0.05 < fx["active2"] < 0.95
    assert all(float(g.abs().max()) > 0 for g in fx["g64"])
    assert (0 < fx["counts"].sum() < n_rows * n_spheres) if mixed else fx["counts"].all()


def test_a_cpu_student_cannot_use_the_fused_encoder():
    from dronechase_amd.student import FLIAStudent, StudentTrainer, fused_conv_stack
    student = FLIAStudent()
    with pytest.raises(ValueError, match="te_sphere_encode_grad"):
        StudentTrainer(student, fused_encoder=True)
    assert StudentTrainer(student).fused_encoder is False
    with pytest.raises(ValueError, match="te_sphere_encode_grad.*GPU"):
        fused_conv_stack(student, torch.zeros(2, 6, 3, 13, 26), torch.ones(2, 6, dtype=torch.uint8))
    with pytest.raises(TypeError, match="FLIAStudent"):
        fused_conv_stack(torch.nn.Linear(2, 2), torch.zeros(2, 6, 3, 13, 26), None)
    # the kernels read floats: a student of another dtype is refused before its buffer's address could reach them
    for other in (FLIAStudent().double(), FLIAStudent().half()):
        with pytest.raises(ValueError, match="conv tensors must be float32"):
            fused_conv_stack(other, torch.zeros(2, 6, 3, 13, 26), None)
