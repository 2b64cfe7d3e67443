"""The fp32 edge convolution (csrc/conv_edge.hip, ops.conv_out_gn*): GroupNorm + SiLU + 3x3 conv with Cout <= 8 in one kernel, against an fp64
CPU computation of (x - mean) rstd gamma + beta -> SiLU -> conv2d from the SAME fp32 inputs and statistics.

Shapes: N = 2 (per-image statistics, zero padding at image boundaries); 9 x 35 and 17 x 33 maps (two 8 x 32 tiles in each direction, ragged
last tiles); Cin 64 / 128 with 32 groups (two / four 32-channel chunks); Cout 3 / 4 / 8 (a zero weight column, a full 4-column and the 8-column instantiation); one launch over two
tile-shape groups (9 x 35, two tiles, and 12 x 20) sharing the images' statistics. Every operand sits between NaN guard bands and every
output inside a fence (tests/guard_bands.py).

Tolerance, per output element, with S = sum |a_i w_i| + |bias| computed in fp64 next to the reference:
    |got - ref| <= ((9 Cin + 16) 2^-24 + SILU_REL) S
  (9 Cin + 16) 2^-24: a chain of 9 Cin fp32 FMAs in any order plus 16 roundings of slack for the affine, the cross-wave sum and the bias.
  SILU_REL: silu_f's (x * v_rcp_f32(1 + v_exp_f32(-x log2 e))) largest relative error against fp64. Measured once on an MI355X through this
  very kernel (identity statistics and affine, a weight that is 1 at the centre tap of channel 0: the output IS silu_f(x) in fp32) over
  2^21 points of [-SILU_RANGE, SILU_RANGE]: see profiles/edge_convs.md. The test asserts that its normalised values stay inside that range.
Second check: the kernel's largest error is no larger than that of the path it replaces (the apply pass writing a two-term fp16 split operand +
ops.conv2d on the split weight) on the same inputs."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as GB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 32
N = 2
SILU_RANGE = 12.0
SILU_REL = 9.5e-7       # measured 9.43e-7 (at x = -11.8; 5.3e-7 on [-6, -2), <= 2.4e-7 on [-2, 12]: profiles/edge_convs.md, "silu_f"), rounded up
MAPS = [(9, 35), (17, 33)]


def _ops():
    from omgsr_amd import ops
    return ops


@pytest.fixture
def accurate():
    ops = _ops()
    ops.set_compute_dtype(torch.float32)
    yield ops
    ops.set_compute_dtype(torch.bfloat16)


def _inputs(shapes, Cin, Cout, seed):
    """shapes: [(rows, H, W)]. fp32 inputs on the CPU (the reference's), statistics of N images."""
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randn((r, h, w, Cin), generator=gen) * 1.5 + 0.3 for r, h, w in shapes]
    mean = torch.randn((N, G), generator=gen) * 0.3 + 0.3
    rstd = torch.rand((N, G), generator=gen) * 0.4 + 0.5
    gamma, beta = torch.randn(Cin, generator=gen) * 0.3 + 1.0, torch.randn(Cin, generator=gen) * 0.3
    w = torch.randn((Cout, Cin, 3, 3), generator=gen) / (3.0 * Cin ** 0.5)
    b = torch.randn(Cout, generator=gen) * 0.1
    return xs, mean, rstd, gamma, beta, w, b


def _reference(x, mean, rstd, gamma, beta, w, b):
    """fp64: (result [rows, H, W, Cout], S = sum |a w| + |b|, largest |normalised value|)."""
    rows, C = x.shape[0], x.shape[-1]
    img = torch.arange(rows) % mean.shape[0]
    m = mean.double()[img].repeat_interleave(C // G, 1)[:, None, None, :]
    r = rstd.double()[img].repeat_interleave(C // G, 1)[:, None, None, :]
    v = (x.double() - m) * r * gamma.double() + beta.double()
    a = (v * torch.sigmoid(v)).permute(0, 3, 1, 2)
    ref = F.conv2d(a, w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(a.abs(), w.double().abs(), b.double().abs(), padding=1).permute(0, 2, 3, 1)
    return ref, mag, float(v.abs().max())


def _run(ops, xs, mean, rstd, gamma, beta, w, b, one_launch=True):
    """The kernel on guarded operands with fenced outputs; returns the outputs on the CPU."""
    dev = [GB.embed(t.to(DEV)) for t in (mean, rstd, gamma, beta)]
    ew = GB.embed(ops.pack_edge_out_weight(w.to(DEV), b.to(DEV)))
    gx = [GB.embed(x.to(DEV)) for x in xs]
    with GB.fenced_outputs():
        outs = ops.conv_out_gn_multi(gx, ew, *dev, G, one_launch=one_launch)
        torch.cuda.synchronize()
    return [o.cpu() for o in outs]


_CACHE = {}


def _case(h, w, Cin, Cout):
    key = (h, w, Cin, Cout)
    if key not in _CACHE:
        inp = _inputs([(N, h, w)], Cin, Cout, 1000 + h * 7 + Cin + Cout)
        _CACHE[key] = (inp, _reference(inp[0][0], *inp[1:]))
    return _CACHE[key]


def _check(got, ref, mag, vmax, Cin, Cout, what):
    assert vmax <= SILU_RANGE, f"{what}: normalised values reach {vmax}, beyond the range silu_f was measured on"
    assert got.shape == (*ref.shape[:-1], 8) and got.dtype == torch.float32
    assert torch.equal(got[..., Cout:].contiguous().view(torch.int32), torch.zeros_like(got[..., Cout:], dtype=torch.int32)), f"{what}: padding channels"
    err = (got[..., :Cout].double() - ref).abs()
    bound = ((9 * Cin + 16) * 2.0 ** -24 + SILU_REL) * mag
    worst = float((err / bound).max())
    print(f"{what}: max abs error {float(err.max()):.3e}, largest error / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements beyond the bound, worst ratio {worst}"
    return float(err.max())


@pytest.mark.parametrize("Cout", [3, 4, 8])
@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("hw", MAPS)
def test_conv_out_gn_against_fp64(accurate, hw, Cin, Cout):
    ops = accurate
    (xs, mean, rstd, gamma, beta, w, b), (ref, mag, vmax) = _case(*hw, Cin, Cout)
    got = _run(ops, xs, mean, rstd, gamma, beta, w, b)[0]
    again = _run(ops, xs, mean, rstd, gamma, beta, w, b)[0]
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two launches differ"
    new_err = _check(got, ref, mag, vmax, Cin, Cout, f"conv_out_gn {hw} {Cin}->{Cout}")
    # the path this kernel replaces: apply pass (two-term fp16 split operand) + the MFMA conv on the split weight
    d = [t.to(DEV) for t in (xs[0], mean, rstd, gamma, beta, w, b)]
    y = ops.group_norm_apply(d[0], d[1], d[2], d[3], d[4], G, ops.ACT_SILU, split=2)
    old = ops.conv2d(y, ops.pack_conv_weight(d[5], d[6], cout_multiple=8, split=2, w_split=2), stride=1, pad=1)
    old_err = float((old.cpu()[..., :Cout].double() - ref).abs().max())
    print(f"conv_out_gn {hw} {Cin}->{Cout}: max abs error new {new_err:.3e}, apply + conv2d {old_err:.3e}")
    assert new_err <= old_err


def test_conv_out_gn_tile_shape_groups(accurate):
    """Two shape groups (two tiles of 9 x 35, one of 12 x 20; rows tile-major, row r uses image r % N) in one launch: each against fp64,
    and the same bytes as one launch per group."""
    ops = accurate
    Cin, Cout = 64, 3
    xs, mean, rstd, gamma, beta, w, b = _inputs([(2 * N, 9, 35), (N, 12, 20)], Cin, Cout, 77)
    got = _run(ops, xs, mean, rstd, gamma, beta, w, b)
    each = _run(ops, xs, mean, rstd, gamma, beta, w, b, one_launch=False)
    for k, x in enumerate(xs):
        ref, mag, vmax = _reference(x, mean, rstd, gamma, beta, w, b)
        _check(got[k], ref, mag, vmax, Cin, Cout, f"group {k} {tuple(x.shape)}")
        assert torch.equal(got[k].view(torch.int32), each[k].view(torch.int32)), f"group {k}: one launch != a launch per group"


def test_conv_out_gn_graph_capture(accurate):
    ops = accurate
    (xs, mean, rstd, gamma, beta, w, b), _ = _case(9, 35, 64, 3)
    d = [t.to(DEV) for t in (xs[0], mean, rstd, gamma, beta)]
    ew = ops.pack_edge_out_weight(w.to(DEV), b.to(DEV))
    eager = ops.conv_out_gn(d[0], ew, d[1], d[2], d[3], d[4], G)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.conv_out_gn(d[0], ew, d[1], d[2], d[3], d[4], G)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))


def test_conv_out_gn_rejects_what_it_does_not_serve(accurate):
    ops = accurate
    from omgsr_amd._lib import OmgsrError
    st = torch.zeros((N, G), device=DEV)
    w = torch.zeros((3, 48, 3, 3))
    with pytest.raises(OmgsrError):          # Cin % 32 != 0
        ops.conv_out_gn(torch.zeros((N, 8, 8, 48), device=DEV), ops.pack_edge_out_weight(w.to(DEV), None), st, st, torch.ones(48, device=DEV), torch.zeros(48, device=DEV), 16)
    with pytest.raises(TypeError):           # a 16-bit stream tensor never comes here
        ops.conv_out_gn(torch.zeros((N, 8, 8, 64), device=DEV, dtype=torch.bfloat16), ops.pack_edge_out_weight(torch.zeros((3, 64, 3, 3), device=DEV), None),
                        st, st, torch.ones(64, device=DEV), torch.zeros(64, device=DEV), G)

