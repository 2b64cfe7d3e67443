"""The fused launch of norm1's GroupNorm apply and the block's 1x1 conv_shortcut (csrc/norm_shortcut.hip; accurate tier, fp16 operands):
y must be the apply pass's bytes, sc the fp32 shortcut of the un-normalised x to the three-fp16-segment accuracy, exact on dyadic inputs,
bit-repeatable and independent of the grouping into launches, and the kernel must stay inside its tensors (tests/guard_bands.py).

Shapes: maps of 9 x 35 and 17 x 33 pixels (315 and 561 pixels: no multiple of the 64 / 96 / 128-pixel tiles, so every case has a partly
filled last tile and more than one workgroup per image; tiles cross map rows), 2 images, every served direction of channel change."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guard_bands import embed, fenced_outputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(128, 256), (256, 128), (256, 512), (512, 256)]
MAPS = [(9, 35), (17, 33)]
G = 32


@pytest.fixture(autouse=True)
def precise_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.float32)
    assert ops.precise() and ops.act_dtype() == torch.float16 and ops.stream_dtype() == torch.float32
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.uint8)


_cache = {}


def _problem(C, Co, H, W):
    """Inputs of one case, built once: x, affine, weight, statistics, the float64 shortcut reference and the old path's result."""
    key = (C, Co, H, W)
    if key not in _cache:
        from omgsr_amd import ops
        x = torch.randn(2, H, W, C, generator=_g(C + H)) * 1.5 + 0.2
        gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=_g(91)), 0.05 * torch.randn(C, generator=_g(92))
        w = torch.randn(Co, C, 1, 1, generator=_g(93)) * C ** -0.5
        b = 0.1 * torch.randn(Co, generator=_g(94))
        ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double()).permute(0, 2, 3, 1).contiguous()
        xd = x.to(DEV)
        mean, rstd, _ = ops.group_norm_stats(xd, G, 1e-6)
        _, x3 = ops.group_norm_apply(xd, mean, rstd, gamma.to(DEV), beta.to(DEV), G, ops.ACT_SILU, split=1, also_cast=3)
        old = ops.conv2d(x3, ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=3), pad=0)
        _cache[key] = dict(x=xd, gamma=gamma.to(DEV), beta=beta.to(DEV), sw=ops.pack_gn_shortcut_weight(w, b, device=DEV), mean=mean, rstd=rstd,
                           ref=ref, old_err=_rel(old, ref))
    return _cache[key]


@pytest.mark.parametrize("act", [1, 0], ids=["silu", "none"])
@pytest.mark.parametrize("split", [1, 4], ids=["fp16", "mx6"])
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("C,Co", PAIRS)
def test_y_is_the_apply_pass_and_sc_is_accurate_inside_guard_bands(C, Co, H, W, split, act):
    """Every input between bands of NaN bytes, every output inside a patterned fence: y bit-identical to group_norm_apply without a twin,
    sc against F.conv2d in float64 below 2e-5 (the bound of test_precise_gpu.py::test_shortcut_conv_mx_from_groupnorm_second_output), no NaN."""
    import dataclasses
    from omgsr_amd import ops
    p = _problem(C, Co, H, W)
    sw = dataclasses.replace(p["sw"], w=embed(p["sw"].w), bias=embed(p["sw"].bias))
    with fenced_outputs():
        y, sc = ops.group_norm_shortcut(embed(p["x"]), sw, embed(p["mean"]), embed(p["rstd"]), embed(p["gamma"]), embed(p["beta"]), G, act, split)
        torch.cuda.synchronize()
    want = ops.group_norm_apply(p["x"], p["mean"], p["rstd"], p["gamma"], p["beta"], G, act, split=split)
    assert y.dtype == want.dtype and y.shape == want.shape and torch.equal(_bits(y), _bits(want))
    err = _rel(sc, p["ref"])
    print(f"gn_shortcut {C}->{Co} {H}x{W} split {split} act {act}: sc rel-L2 {err:.3e} (twin + MX GEMM path: {p['old_err']:.3e})")
    assert sc.dtype == torch.float32 and tuple(sc.shape) == (2, H, W, Co) and bool(torch.isfinite(sc).all())
    assert err < 2e-5


@pytest.mark.parametrize("C,Co", PAIRS)
def test_dyadic_inputs_are_exact(C, Co):
    """x = x_hi + x_lo and w = w_hi + w_lo with every part fp16-exact (|x_hi| in {1/4, 1/2}, x_lo in {0, +-2^-15}; |w_hi| in {1/8, 1/4}, w_lo in
    {0, +-2^-16}: below half an ulp of the hi part, so the split recovers them). The kernel computes x_hi w_hi + x_lo w_hi + x_hi w_lo: multiples
    of 2^-18 whose partial sums stay below C / 8 <= 64 = 2^(24 - 18), so every fp32 sum is exact in any order and sc must EQUAL the float64
    value: a wrong lane map, a swapped hi / lo fragment or a skipped chunk changes it."""
    from omgsr_amd import ops
    H, W = MAPS[0]
    g = _g(7 + C)

    def pick(shape, vals):
        return torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), shape, generator=g)]

    xh, xl = pick((2, H, W, C), [-0.5, -0.25, 0.25, 0.5]), pick((2, H, W, C), [-2.0 ** -15, 0.0, 2.0 ** -15])
    wh, wl = pick((Co, C), [-0.25, -0.125, 0.125, 0.25]), pick((Co, C), [-2.0 ** -16, 0.0, 2.0 ** -16])
    b = pick((Co,), [-1.0, 0.5, 2.0])
    x, w = (xh + xl).float(), (wh + wl).float()
    assert torch.equal(x.double(), xh + xl) and torch.equal(w.double(), wh + wl)
    assert torch.equal(x.to(torch.float16).double(), xh) and torch.equal(w.to(torch.float16).double(), wh)
    xf, xlf = xh.reshape(-1, C), xl.reshape(-1, C)
    ref = (xf @ wh.t() + xlf @ wh.t() + xf @ wl.t() + b).reshape(2, H, W, Co)
    assert ref.abs().max() < 32 and torch.equal(ref.float().double(), ref)
    xd = x.to(DEV)
    mean, rstd, _ = ops.group_norm_stats(xd, G, 1e-6)
    sw = ops.pack_gn_shortcut_weight(w.reshape(Co, C, 1, 1), b.float(), device=DEV)
    for split in (1, 4):
        _, sc = ops.group_norm_shortcut(xd, sw, mean, rstd, None, None, G, ops.ACT_NONE, split)
        assert torch.equal(sc.double().cpu(), ref), (split, (sc.double().cpu() - ref).abs().max().item())


@pytest.mark.parametrize("split", [1, 4], ids=["fp16", "mx6"])
def test_multi_launch_equals_a_launch_per_group_and_repeats(split):
    """Two tile-shape groups, (4, 9, 35) and (2, 12, 20): 2 and 1 tiles per image, sharing the statistics of 2 images (row r uses image r % 2).
    The one launch, one launch per group and the same launch again give the same bytes; y is group_norm_apply_multi's; inside guard bands."""
    from omgsr_amd import ops
    C, Co = 256, 128
    xs = [(torch.randn(4, 9, 35, C, generator=_g(21)) * 1.5 + 0.2).to(DEV), (torch.randn(2, 12, 20, C, generator=_g(22)) * 1.5 - 0.1).to(DEV)]
    gamma, beta = (1.0 + 0.1 * torch.randn(C, generator=_g(91))).to(DEV), (0.05 * torch.randn(C, generator=_g(92))).to(DEV)
    w = torch.randn(Co, C, 1, 1, generator=_g(93)) * C ** -0.5
    b = 0.1 * torch.randn(Co, generator=_g(94))
    sw = ops.pack_gn_shortcut_weight(w, b, device=DEV)
    mean, rstd, _ = ops.group_norm_stats_merged(xs, [2, 1], 2, G, 1e-6)
    assert tuple(mean.shape) == (2, G)
    with fenced_outputs():
        one = ops.group_norm_shortcut_multi([embed(x) for x in xs], sw, embed(mean), embed(rstd), embed(gamma), embed(beta), G, ops.ACT_SILU, split)
        torch.cuda.synchronize()
    again = ops.group_norm_shortcut_multi(xs, sw, mean, rstd, gamma, beta, G, ops.ACT_SILU, split)
    each = ops.group_norm_shortcut_multi(xs, sw, mean, rstd, gamma, beta, G, ops.ACT_SILU, split, one_launch=False)
    want = ops.group_norm_apply_multi(xs, mean, rstd, gamma, beta, G, ops.ACT_SILU, split=split)
    for k, x in enumerate(xs):
        for other in (again, each):
            assert torch.equal(_bits(one[k][0]), _bits(other[k][0])) and torch.equal(_bits(one[k][1]), _bits(other[k][1]))
        assert torch.equal(_bits(one[k][0]), _bits(want[k]))
        ref = F.conv2d(x.cpu().permute(0, 3, 1, 2).double(), w.double(), b.double()).permute(0, 2, 3, 1)
        assert bool(torch.isfinite(one[k][1]).all()) and _rel(one[k][1], ref) < 2e-5


def test_resnet_block_routes_through_the_fused_launch(monkeypatch):
    """ResnetBlock2D.nhwc takes the fused launch under fp16 operands and the old path with OMGSR_GN_SHORTCUT_FUSED=0; the two blocks agree
    to the accuracy of the shortcut forms (both carry the shortcut to ~2^-16 of its size; the rest of the block is the same launches)."""
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api.autoencoder_kl import ResnetBlock2D
    from omgsr_amd.precision import set_operand_split, set_weight_split
    from omgsr_amd.testing import seeded_init_
    C, Co = 256, 128
    xd = (torch.randn(2, 17, 33, C, generator=_g(90)) * 1.5 + 0.2).to(DEV)
    blk = ResnetBlock2D(C, Co, None, 32, 1e-6).to(DEV)
    seeded_init_(blk, 5, rounded=False)
    set_operand_split(blk, [r"."]); set_weight_split(blk, [r"."])
    blk.conv1.op_split = 1          # the decoder's form above 64 px: a plain fp16 operand from norm1
    calls = []
    real = ops.group_norm_shortcut_multi
    monkeypatch.setattr(ops, "group_norm_shortcut_multi", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    fused = blk.nhwc(xd)
    assert calls == [1]
    monkeypatch.setenv("OMGSR_GN_SHORTCUT_FUSED", "0")
    old = blk.nhwc(xd)
    assert calls == [1]
    assert _rel(fused, old.double()) < 2e-5
