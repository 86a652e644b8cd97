"""te_sphere_encode_bf16 without a GPU: the CPU reference pair of its numerics contract (tests/_student_bf16_ref.py) held to the two
conditions the kernel is held to, the packed layout's size, every host-side refusal of the three calls (they return before anything is
launched), and StudentDriver's refusals of the switch.

Measured on the CPU, E32 against E64 on the fixture's 48 spheres with the recipe weights: see the printed figures (the share of
elements further than NEAR from E64, and the worst |d| / (NEAR + 2 B))."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _student_bf16_ref as R
from tests import _student_cases as S

FAKE = 1 << 20          # never dereferenced: every call below fails a check first


@pytest.fixture(scope="module")
def student():
    from dronechase_amd.student import load_flia_student
    w = S.recipe_weights(S.keys_and_shapes())
    return load_flia_student({k: torch.from_numpy(v).float() for k, v in w.items()})


@pytest.fixture(scope="module")
def lib():
    from dronechase_amd import _lib
    from dronechase_amd.build import build_library
    build_library()
    return _lib.load()


def test_the_reference_pair_meets_both_conditions_with_room(student):
    """E32 (fp32 sums) against E64 on the fixture's 48 spheres: the share at most a third of the cap, every element within its bound."""
    conv = R.conv_tensors(student)
    x = torch.from_numpy(S.fixture_inputs()["stacked_spheres"]).float().reshape(48, 3, 13, 26)
    e64, y1 = R.encode(conv, x, torch.float64)
    e32, _ = R.encode(conv, x, torch.float32)
    allowance = R.flip_allowance(conv, y1)
    gap, share, ratio = R.figures(e32.numpy(), e64.numpy(), allowance.numpy())
    print(f"E32 against E64: max |d| {gap:.3g}, share past NEAR {100 * share:.3g} %, worst ratio {ratio:.3g}")
    assert share <= R.SHARE_CAP / 3 and ratio <= 1.0, (gap, share, ratio)
    # the conditions see a geometry error: one output position or one channel of every sphere displaced
    wrong = e64.reshape(48, 64, 28).clone()
    wrong[:, :, 5] = wrong[:, :, 6]
    assert not R.holds(wrong.reshape(48, 1792).numpy(), e64.numpy(), allowance.numpy())
    wrong = e64.reshape(48, 64, 28).clone()
    wrong[:, 9] = wrong[:, 10]
    assert not R.holds(wrong.reshape(48, 1792).numpy(), e64.numpy(), allowance.numpy())
    # and the contract is not fp32: the module's own fp32 conv stack is outside them
    with torch.no_grad():
        fp32 = student.sphere_cnn.conv_stack(x)
    assert not R.holds(fp32.numpy(), e64.numpy(), allowance.numpy())


def test_the_packed_layouts_size(lib):
    from dronechase_amd import _lib
    assert {"te_sphere_bf16_words", "te_sphere_pack_bf16", "te_sphere_encode_bf16"} <= set(_lib.EXPORTS)
    words = C.c_size_t()
    assert lib.te_sphere_bf16_words(3, C.byref(words)) == 0
    assert words.value == R.WORDS == 32 * 128 + 64 * 288 and R.W2_AT % 8 == 0
    assert lib.te_sphere_bf16_words(2, C.byref(words)) != 0
    assert lib.te_last_error().startswith(b"te_sphere_bf16_words: ") and b"channels must be 3" in lib.te_last_error()
    assert lib.te_sphere_bf16_words(3, None) != 0
    assert lib.te_last_error().startswith(b"te_sphere_bf16_words: ") and b"out_halfwords" in lib.te_last_error()


def test_pack_refusals_come_from_the_host(lib):
    base = dict(params=FAKE, channels=3, out=FAKE, stream=None)
    cases = [(dict(params=None), b"null argument params"), (dict(out=None), b"null argument out"),
             (dict(params=FAKE + 4), b"params must be 16-byte aligned"), (dict(out=FAKE + 2), b"out must be 16-byte aligned"),
             (dict(channels=2), b"channels must be 3"), (dict(channels=4), b"channels must be 3")]
    for kw, msg in cases:
        assert lib.te_sphere_pack_bf16(*[kw.get(k, v) for k, v in base.items()]) != 0, kw
        err = lib.te_last_error()
        assert err.startswith(b"te_sphere_pack_bf16: ") and msg in err, (kw, err)


def test_encode_refusals_come_from_the_host(lib):
    base = dict(params=FAKE, weights_bf16=FAKE, channels=3, n_rows=4, n_spheres=6, stacked=FAKE, mask=FAKE, out=FAKE, stream=None)
    cases = [(dict(params=None), b"null argument params"), (dict(weights_bf16=None), b"null argument weights_bf16"),
             (dict(stacked=None), b"null argument stacked"), (dict(out=None), b"null argument out"),
             (dict(params=FAKE + 4), b"params must be 16-byte aligned"), (dict(weights_bf16=FAKE + 2), b"weights_bf16 must be 16-byte aligned"),
             (dict(stacked=FAKE + 8), b"stacked must be 16-byte aligned"), (dict(out=FAKE + 4), b"out must be 16-byte aligned"),
             (dict(channels=2), b"channels must be 3"),
             (dict(n_spheres=0), b"n_spheres must be in 1 .. 8, not 0"), (dict(n_spheres=9), b"n_spheres must be in 1 .. 8, not 9"),
             (dict(n_rows=0), b"n_rows must be positive, not 0"), (dict(n_rows=-1), b"n_rows must be positive"),
             (dict(n_rows=1 << 30, n_spheres=8), b"n_rows * n_spheres must be at most")]
    for kw, msg in cases:
        assert lib.te_sphere_encode_bf16(*[kw.get(k, v) for k, v in base.items()]) != 0, kw
        err = lib.te_last_error()
        assert err.startswith(b"te_sphere_encode_bf16: ") and msg in err, (kw, err)


def test_driver_refuses_bf16_without_the_fused_encoder_and_unknown_precisions(student):
    from dronechase_amd.student import StudentDriver
    with pytest.raises(ValueError, match="encoder_precision='bf16'.*needs fused_encoder=True"):
        StudentDriver(student, encoder_precision="bf16")
    with pytest.raises(ValueError, match="encoder_precision must be one of .*'fp32', 'bf16'.*not 'fp16'"):
        StudentDriver(student, fused_encoder=True, encoder_precision="fp16")
    with pytest.raises(ValueError, match="encoder_precision must be one of"):
        StudentDriver(student, encoder_precision="BF16")
    assert StudentDriver(student).encoder_precision == "fp32" and StudentDriver(student, encoder_precision="fp32").fused_encoder is False
