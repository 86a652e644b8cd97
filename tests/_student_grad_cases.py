"""Fixtures for te_sphere_encode_grad (tests/test_student_grad.py, tests/test_gpu_student_grad.py).  Everything here runs on the CPU,
is deterministic and sees no kernel output.

kinkfree()   the recipe's student (tests/_student_cases.py) with the two conv biases moved as tests/_kinkfree.py moves a policy's: per
             channel, into the midpoint of the widest gap of that channel's fp64 pre-activations inside the central half, over every
             position of every counting sphere of the 8 fixture rows (19 spheres); block1 first, block2 on the moved block1, every new
             bias rounded to fp32 at once.  The reference gradient is autograd through FLIAStudent.sphere_cnn.conv_stack in float64 (its
             forward is pinned to the reference module by tests/golden/student_flia.npz), the upstream gradient seeded N(0, 1).
exact(B, N)  inputs in {0, 1/2, 1}, weights in {-1, 0, 1}, both biases 1/16, upstream gradients in {-2 .. 2}: every term of every sum
             of the forward and the backward is a multiple of a power of two (the "grid" of that sum), and the sum of the terms'
             magnitudes stays below 2^24 grid units, so every partial sum in any order is exactly representable in fp32 and the fp32
             kernel must equal the fp64 reference bit for bit.  block1's pre-activations are k / 2 + 1 / 16, never 0; block2's are
             multiples of 1 / 16 and can be exactly 0, where the reference and the kernel both take ReLU's derivative as 0 (out > 0)."""
import functools

import numpy as np

from tests import _student_cases as S

MARGIN = 5e-4                      # every |pre-activation| of a counting sphere, about 100 x the forward's measured device error (5.7e-6)
ACTIVE = (0.25, 0.75)              # share of each block's units that are active
CONV_NAMES = ("block1.weight", "block1.bias", "block2.weight", "block2.bias")
EPS32 = 2.0 ** -23
# (n_rows, n_spheres, mixed masks) of the exact cases: one sphere; mixed masks; 420 spheres, more than the 256 compute units, so
# workgroups take one or two spheres and the sum over the workgroups' partial gradients has 256 terms
EXACT_CASES = ((1, 1, False), (3, 6, True), (70, 6, False))


def conv_tensors(student):
    cnn = student.sphere_cnn
    return [cnn.block1[0].conv.weight, cnn.block1[0].conv.bias, cnn.block2[0].conv.weight, cnn.block2[0].conv.bias]


def _preactivations(cnn, x):
    """(z1 [M, 32, 7, 13], z2 [M, 64, 4, 7]) of the module's two padded convolutions, in x's dtype."""
    import torch
    z1 = cnn.block1[0](x)
    return z1, cnn.block2[0](torch.relu(z1))


def _bias_shift(z):
    """Per channel of z [M, C, H, W]: the midpoint of the widest gap between consecutive sorted values inside the central half."""
    import torch
    v = z.permute(1, 0, 2, 3).reshape(z.shape[1], -1).t()              # [values, channels]
    s = v.sort(dim=0).values
    n = s.shape[0]
    lo, hi = n // 4, n - n // 4
    gaps = s[lo + 1:hi] - s[lo:hi - 1]
    i = gaps.argmax(dim=0) + lo
    col = torch.arange(s.shape[1])
    return 0.5 * (s[i, col] + s[i + 1, col])


def conv_grads(student, x, d_out, dtype):
    """Autograd through a copy of the student's conv_stack in `dtype`: x [M, 3, 13, 26], d_out [M, 1792] -> the four gradients, fp64."""
    import copy
    import torch
    net = copy.deepcopy(student).to(dtype)
    out = net.sphere_cnn.conv_stack(x.to(dtype))
    grads = torch.autograd.grad(out, conv_tensors(net), d_out.to(dtype))
    return [g.double() for g in grads]


@functools.lru_cache(maxsize=None)
def kinkfree():
    import copy
    import torch
    from dronechase_amd.student import load_flia_student
    w = S.recipe_weights(S.keys_and_shapes())
    student = load_flia_student({k: torch.from_numpy(v).float() for k, v in w.items()})
    inputs = S.fixture_inputs()
    mask = inputs["validity_mask"]
    counts = S.counting(mask.copy())
    stacked = torch.from_numpy(inputs["stacked_spheres"]).float()                   # [8, 6, 3, 13, 26], what the kernel reads
    x64 = stacked[torch.from_numpy(counts)].double()                                # the counting spheres, row-major
    with torch.no_grad():
        for block in (0, 1):
            cnn64 = copy.deepcopy(student).double().sphere_cnn
            z = _preactivations(cnn64, x64)[block]
            b = (student.sphere_cnn.block1, student.sphere_cnn.block2)[block][0].conv.bias
            b.copy_((b.double() - _bias_shift(z)).float())
        z1, z2 = _preactivations(copy.deepcopy(student).double().sphere_cnn, x64)
    margins = {"spheres": int(counts.sum()), "min_abs_z1": float(z1.abs().min()), "min_abs_z2": float(z2.abs().min()),
               "active1": float((z1 > 0).double().mean()), "active2": float((z2 > 0).double().mean())}
    g = torch.Generator().manual_seed(S.SEED + 4)
    d_out = torch.randn((8, 6, 1792), generator=g)                                   # fp32: the kernel and both references read these bits
    d_counting = d_out[torch.from_numpy(counts)]
    g64 = conv_grads(student, x64, d_counting, torch.float64)
    g32 = conv_grads(student, x64, d_counting, torch.float32)
    return {"student": student, "stacked": stacked, "mask": torch.from_numpy(mask), "counts": counts, "d_out": d_out, "margins": margins,
            "g64": g64, "E": [float((a - b).abs().max()) for a, b in zip(g32, g64)], "scale": [float(b.abs().max()) for b in g64]}


def kinkfree_figure(fx, grads):
    """{tensor: gap / max(E_t, 2^-23 ||g64||inf)} of four gradients against the fp64 reference: the figure of tests/_kinkfree.py,
    reported and not asserted (the bias sums run in the kernel's own order)."""
    out = {}
    for name, got, ref, e, scale in zip(CONV_NAMES, grads, fx["g64"], fx["E"], fx["scale"]):
        gap = float(np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref.numpy()).max())
        out[name] = {"gap": gap, "E": e, "norm": scale, "ratio": gap / max(e, EPS32 * scale)}
    return out


def split(flat):
    """A packed gradient (20 928 values) as the four arrays in the parameter buffer's order."""
    flat = np.asarray(flat)
    shapes, out, at = ((32, 3, 5, 5), (32,), (64, 32, 3, 3), (64,)), [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[at:at + n].reshape(s))
        at += n
    assert at == flat.size == 20928
    return out


def _hybrid_pad(x, p):
    import torch
    import torch.nn.functional as F
    return F.pad(F.pad(x, (p, p, 0, 0), mode="circular"), (0, 0, p, p), mode="constant", value=1.0)


@functools.lru_cache(maxsize=None)
def exact(n_rows, n_spheres, mixed, seed=0):
    """The exact-arithmetic case of n_rows x n_spheres; mixed: the rows' masks are S.MASKS' patterns, cycled (else every sphere is valid)."""
    import torch
    import torch.nn.functional as F
    from dronechase_amd.student import FLIAStudent
    rng = np.random.default_rng(S.SEED + 10 + seed + 1000 * n_rows + n_spheres)
    pick = lambda values, p, shape: rng.choice(np.asarray(values, np.float64), size=shape, p=p)
    w1 = pick([-1, 0, 1], [0.1, 0.8, 0.1], (32, 3, 5, 5))
    w2 = pick([-1, 0, 1], [0.05, 0.9, 0.05], (64, 32, 3, 3))
    stacked = pick([0, 0.5, 1], [0.4, 0.3, 0.3], (n_rows, n_spheres, 3, 13, 26))
    d_out = rng.integers(-2, 3, (n_rows, n_spheres, 1792)).astype(np.float64)
    if not mixed:
        mask = np.ones((n_rows, n_spheres), np.uint8)
    else:
        mask = np.array([[int(c) for c in S.MASKS[(r + 3) % len(S.MASKS)][:n_spheres]] for r in range(n_rows)], np.uint8)
    counts = S.counting(mask.copy())
    student = FLIAStudent()
    with torch.no_grad():
        for p, v in zip(conv_tensors(student), (w1, np.full(32, 1 / 16), w2, np.full(64, 1 / 16))):
            p.copy_(torch.from_numpy(v).float())
    x = torch.from_numpy(stacked)[torch.from_numpy(counts)]
    g = torch.from_numpy(d_out)[torch.from_numpy(counts)]
    g64 = conv_grads(student, x, g, torch.float64)

    # sum |terms| of every sum the kernel forms, in units of that sum's grid
    W1, W2 = torch.from_numpy(w1), torch.from_numpy(w2)
    b = 1 / 16
    xin = _hybrid_pad(x, 2)
    z1 = F.conv2d(xin, W1, torch.full((32,), b, dtype=torch.float64), stride=2)
    p1 = _hybrid_pad(torch.relu(z1), 1)
    z2 = F.conv2d(p1, W2, torch.full((64,), b, dtype=torch.float64), stride=2)
    dz2 = g.reshape(-1, 64, 4, 7) * (z2 > 0)
    dp1 = F.conv_transpose2d(dz2, W2, stride=2)                                       # [M, 32, 9, 15]
    dy1 = dp1[:, :, 1:8, 1:14].clone()
    dy1[..., 12] += dp1[:, :, 1:8, 0]
    dy1[..., 0] += dp1[:, :, 1:8, 14]
    dz1 = dy1 * (z1 > 0)
    cols = lambda t, k: F.unfold(t, k, stride=2)                                       # [M, C k k, positions]
    units = {
        "z1": (F.conv2d(xin.abs(), W1.abs(), stride=2) + b).max() * 16,               # terms: multiples of 1/2, and the bias 1/16
        "z2": (F.conv2d(p1.abs(), W2.abs(), stride=2) + b).max() * 16,                # Y1 and the bias: multiples of 1/16
        "dW2": torch.einsum("mcp,mkp->ck", dz2.abs().flatten(2), cols(p1.abs(), 3)).max() * 16,
        "db2": dz2.abs().sum(dim=(0, 2, 3)).max(),
        "dY1": (lambda a: a[:, :, 1:8, 1:14].max() + a[:, :, 1:8, 0].max() + a[:, :, 1:8, 14].max())(F.conv_transpose2d(dz2.abs(), W2.abs(), stride=2)),
        "dW1": torch.einsum("mcp,mkp->ck", dz1.abs().flatten(2), cols(xin.abs(), 5)).max() * 2,
        "db1": dz1.abs().sum(dim=(0, 2, 3)).max(),
    }
    units = {k: float(v) for k, v in units.items()}
    # the reference itself is exact: the fold above reproduces autograd's gradient
    assert torch.equal(torch.einsum("mcp,mkp->ck", dz1.flatten(2), cols(xin, 5)).reshape(32, 3, 5, 5), g64[0])
    assert torch.equal(dz2.sum(dim=(0, 2, 3)), g64[3])
    g32 = [t.float() for t in g64]
    assert all(torch.equal(a.double(), b64) for a, b64 in zip(g32, g64))
    return {"student": student, "stacked": torch.from_numpy(stacked).float(), "mask": torch.from_numpy(mask), "counts": counts,
            "d_out": torch.from_numpy(d_out).float(), "g64": g64, "units": units, "min_abs_z1": float(z1.abs().min()),
            "z2_zeros": int((z2 == 0).sum()), "active1": float((z1 > 0).double().mean()), "active2": float((z2 > 0).double().mean())}
