"""The CPU reference of te_sphere_encode_bf16's numerics contract (include/threatengage.h, csrc/te_sphere_bf16.hpp), and the bounds the
tests hold the kernel to.  Nothing here comes from the kernel.

The contract applied to a FLIAStudent's conv blocks: both conv weights, the sphere's cells and block1's post-ReLU output go through
`.float().bfloat16()` (round-to-nearest-even); the biases stay fp32; the padding is the module's hybrid padding (circular in W, 1.0 in
H); the sums run in a chosen dtype.  E64 accumulates in float64, E32 in float32: the pair brackets what any fp32 accumulation order can
do to the result, the MFMA's included.

Two things separate an fp32 accumulation from E64.  The sums differ by fp32 rounding: NEAR = 1e-5 (1 + |E64|) is generous for sums of
up to 288 products of magnitude below one.  And a block1 value that sits next to a bf16 rounding boundary can land on its other side:
that moves the value by one bf16 ulp and every block2 output that reads it by ulp * |weight|.  B[o], the flip allowance of output o,
is the largest such move over its 288 inputs: max_i ulp_bf16(y1[i]) * |q(w2)[o, i]| (the cells of the constant 1.0 padding excluded:
they are not computed; the columns the circular padding copies are block1 values and count).

  condition 1 (share):          at most SHARE_CAP = 1 % of the elements may be further than NEAR from E64.  One wrong output position is
                                3.6 % of the elements and one wrong channel 1.6 %, so the cap cannot hide a geometry error.
  condition 2 (every element):  |d| <= NEAR + 2 B[o].
"""
import numpy as np
import torch
import torch.nn.functional as F

NEAR_RTOL = 1e-5
SHARE_CAP = 0.01

W1_AT, W2_AT, WORDS = 0, 32 * 128, 32 * 128 + 64 * 288       # the packed bf16 buffer's documented layout (threatengage.h)


def q(t):
    """round-to-nearest-even to bf16, as a tensor of t's dtype"""
    return t.float().bfloat16().to(t.dtype)


def bf16_bits(t):
    """the bf16 bit patterns of a float tensor, as uint16 numpy"""
    return t.float().bfloat16().view(torch.int16).numpy().view(np.uint16)


def hybrid_pad(x, p, h_value=1.0):
    x = F.pad(x, (p, p, 0, 0), mode="circular")
    return F.pad(x, (0, 0, p, p), mode="constant", value=h_value)


def conv_tensors(student):
    cnn = student.sphere_cnn
    return [t.detach() for t in (cnn.block1[0].conv.weight, cnn.block1[0].conv.bias, cnn.block2[0].conv.weight, cnn.block2[0].conv.bias)]


def encode(conv, x, dtype):
    """The contract on spheres x [M, 3, 13, 26] (float32 tensor) with sums in `dtype` -> (out [M, 1792], q(y1) [M, 32, 7, 13])."""
    w1, b1, w2, b2 = conv
    with torch.no_grad():
        y1 = F.relu(F.conv2d(hybrid_pad(q(x.float()).to(dtype), 2), q(w1.float()).to(dtype), b1.float().to(dtype), stride=2))
        y1 = y1.float().bfloat16().to(dtype)
        y2 = F.relu(F.conv2d(hybrid_pad(y1, 1), q(w2.float()).to(dtype), b2.float().to(dtype), stride=2))
    return y2.flatten(1), y1


def ulp_bf16(y):
    """The spacing of bf16 at y >= 0 (0 at 0: a ReLU's zero has no boundary to cross that NEAR does not cover)."""
    _, e = torch.frexp(y.double())                     # y = m 2^e, m in [0.5, 1): the bf16 ulp is 2^(e - 8)
    return torch.where(y > 0, torch.ldexp(torch.ones_like(y, dtype=torch.float64), e - 8), torch.zeros((), dtype=torch.float64))


def flip_allowance(conv, y1q):
    """B [M, 1792] from E64's rounded block1 output y1q [M, 32, 7, 13]."""
    w2 = q(conv[2].float()).double().abs().reshape(64, 288)
    u = hybrid_pad(ulp_bf16(y1q), 1, h_value=0.0)                                   # the 1.0 rows are excluded: their ulp is 0
    cols = F.unfold(u, kernel_size=3, stride=2)                                   # [M, 288, 28], rows in (ci, kh, kw) order: w2's
    out = torch.empty((cols.shape[0], 64, 28), dtype=torch.float64)
    for m in range(cols.shape[0]):
        out[m] = (w2[:, :, None] * cols[m][None]).amax(dim=1)
    return out.reshape(-1, 1792)


def figures(got, e64, allowance):
    """(max |d|, the share of elements further than NEAR from E64, the worst |d| / (NEAR + 2 B)) of `got` against E64."""
    got, e64, allowance = (np.asarray(a, np.float64) for a in (got, e64, allowance))
    d = np.abs(got - e64)
    near = NEAR_RTOL * (1.0 + np.abs(e64))
    return float(d.max()), float((d > near).mean()), float((d / (near + 2.0 * allowance)).max())


def holds(got, e64, allowance, share_cap=SHARE_CAP):
    gap, share, ratio = figures(got, e64, allowance)
    return bool(np.isfinite(np.asarray(got)).all() and share <= share_cap and ratio <= 1.0)


def packed_weights(conv):
    """The documented packed buffer (uint16 numpy, WORDS elements) and the index sets of its pad columns."""
    w1, _, w2, _ = conv
    p1 = np.zeros((32, 16, 8), np.uint16)                                           # k = (ci * 5 + kh) * 8 + kw; row 15 and kw >= 5 zero
    p1[:, :15, :5] = bf16_bits(w1).reshape(32, 15, 5)
    p2 = bf16_bits(w2).reshape(64, 32, 9).transpose(0, 2, 1).reshape(64, 288)      # k = (kh * 3 + kw) * 32 + ci
    pad = np.ones((32, 16, 8), bool)
    pad[:, :15, :5] = False
    return np.concatenate([p1.ravel(), p2.ravel()]), np.flatnonzero(pad.ravel())
