"""OMGSR-S's opt-in MXFP8 UNet resnet convolutions on the MI355X: mxfp8_conv_deep_kernel (omgsr_conv_mxfp8_deep, timing variant 27) bit for bit
against the fp64 restatement of the bytes it reads (im2col + dyadic_probe.mxfp8_ref, as tests/test_fp8_vae_gpu.py builds it) on dyadic and
one-hot operands at Cin 320 / 960 / 1920, against the fp64 product of the dequantised operands on random ones, the GroupNorm apply pass at
C = 320 / 960 (10 / 30 channels per group), the fused GroupNorm statistics, refusals, determinism, guard bands, and the pipeline's routing on a
reduced UNet. Every map is ragged (45 rows x 86 columns: 6 x 3 spatial tiles, the last 22 pixels wide and 5 high) and large enough for the
dispatcher's 192-tile policy; every test asserts omgsr_conv_mxfp8_deep_ok == 1 for its problem."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyadic_probe as dp  # noqa: E402
import test_fp8_vae_gpu as V  # noqa: E402  (pack_planes / unpack_planes / conv_mxfp8_ref / _dequant_conv: the documented layouts, restated)

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARIANT = 27
H, W = 45, 86
CONV_REL_L2 = V.CONV_REL_L2                          # 3e-5: the project's bound for this instruction (measured 1.4e-5, K-independent)
GN_MEAN_TOL, GN_VAR_ATOL, GN_VAR_RTOL = V.GN_MEAN_TOL, V.GN_VAR_ATOL, V.GN_VAR_RTOL
# Small pipeline: the bf16 tier against the accurate tier on the same case (reduced UNet below, 3 x 768^2, seeded weights, draw 0), measured on
# MI355X: rel-L2 2.717e-2 (43.2 dB; draws 1 / 2: 2.87e-2 / 2.89e-2). The key's bound is that figure x 16: an e4m3 operand carries 3 mantissa bits
# where bf16 carries 7, so each served conv's operand rounding is 2^4 times the bf16 tier's; nothing else in the pipeline changes. Measured with the
# key: on against off 9.71e-2, on against the accurate tier 9.78e-2 (32.1 dB). DESIGN.md 3.5 records the figures.
S_BF16_VS_ACCURATE_REL_L2_MEASURED = 2.717e-2
FP8_MARGIN = 16.0


@pytest.fixture(autouse=True)
def _bf16_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.bfloat16)
    ops.set_batch_invariant(False)


def _launch(fn):
    """fn() must have made launches of variant 27 only."""
    out, v = V._launches(fn)
    print(f"variants ran: {sorted(set(v))}")
    assert v and set(v) == {VARIANT}, f"expected kernel variant {VARIANT}, the library ran {sorted(set(v))}"
    return out


def _deep_ok(xq, pw, residual=None, out_dtype=None) -> int:
    """omgsr_conv_mxfp8_deep_ok's answer for the problem ops.conv2d_mxfp8(xq, pw, ..., deep=True) launches (and the old predicate's)."""
    from omgsr_amd import _lib, ops
    a = _lib.IgemmArgs()
    keep = ops._conv_mxfp8_args(a, xq, pw, ops.ACT_NONE, residual, ops.OUT_STREAM if out_dtype is None else out_dtype, 0)
    ops._fill_conv_mxfp8(a, pw)
    ok = _lib.load().omgsr_conv_mxfp8_deep_ok(C.byref(a))
    del keep
    return ok


def _conv(xq, pw, **kw):
    from omgsr_amd import ops
    assert _deep_ok(xq, pw, kw.get("residual"), kw.get("out_dtype")) == 1
    return ops.conv2d_mxfp8(xq, pw, deep=True, **kw)


# ---- dyadic probes -----------------------------------------------------------------------------------------------------------------------------

def dyadic_case(seed, N, Cin, Cout, density, h=H, w=W):
    """tests/test_fp8_vae_gpu.py's dyadic_case with the per-block term c chosen so that EVERY pair of neighbouring blocks - the two blocks of a
    chunk and the two blocks on either side of every chunk (= scale window) boundary - is 2^52 ... 2^60 apart: c[b] = (-1)^b (30 - j[b]),
    j in 0 .. 4, on the operand side, -c on the weight side. Scale bytes 127 + r[pixel] + c[block] + d[pixel, block] (operand) and
    127 + t[cout] - c[block] + d'[cout, tap, block] (weight) differ per pixel, per block and per (cout, tap, block). Pixel (0, 0, 5) carries a
    saturated +448 code, pixel (0, 1, 2) an all-zero block."""
    g = torch.Generator().manual_seed(seed)
    nb = Cin // 32
    c = (30 - torch.randint(0, 5, (nb,), generator=g)) * (1 - 2 * (torch.arange(nb) % 2))
    assert int((c[1:] - c[:-1]).abs().min()) >= 52 and int((c[1:] - c[:-1]).abs().max()) <= 60
    f8 = lambda v: v.to(torch.float8_e4m3fn).view(torch.uint8)      # noqa: E731

    def codes(shape):
        return f8(dp.dyadic(g, torch.randint(0, 2, shape, generator=g).float()) * (torch.rand(shape, generator=g) < density))

    xc = codes((N, h, w, Cin))
    r = torch.randint(-2, 3, (N, h, w, 1), generator=g)
    xs = (127 + r + c + torch.randint(0, 2, (N, h, w, nb), generator=g)).to(torch.uint8)
    xc[0, 0, 5, 7] = f8(torch.tensor(448.0))
    xc[0, 1, 2, :32] = 0
    wc = codes((Cout, 9, Cin))
    t = torch.randint(-8, 9, (Cout, 1, 1), generator=g)
    wsc = (127 + t - c + torch.randint(0, 2, (Cout, 9, nb), generator=g)).to(torch.uint8)
    return g, xc, xs, wc, wsc, r.float(), t.float().reshape(1, 1, 1, Cout)


def _run_dyadic(seed, N, Cin, Cout, density, out_f32, res_f32):
    from omgsr_amd import ops
    g, xc, xs, wc, wsc, r, t = dyadic_case(seed, N, Cin, Cout, density)
    bias = V._terms(g, t.reshape(Cout))
    pw = V.pack_planes(wc, wsc, bias, DEV)
    xq = ops.Mxfp8(xc.to(DEV), xs.to(DEV))
    res = V._terms(g, (r + t).expand(N, H, W, Cout)).to(DEV, torch.float32 if res_f32 else torch.bfloat16)
    uc, us = V.unpack_planes(pw)
    want = dp.rounded(V.conv_mxfp8_ref(xq.codes, xq.scales, uc, us, Cout, bias=pw.bias, residual=res), torch.float32 if out_f32 else torch.bfloat16)
    y = _launch(lambda: _conv(xq, pw, residual=res, out_dtype=ops.OUT_F32 if out_f32 else ops.OUT_BF16))
    V._eq(y, want, f"mxfp8 deep conv {N}x{H}x{W}x{Cin} -> {Cout}")


def test_dyadic_cin320_bias_residual_bf16():
    """Cin 320: five chunks (odd), 10-byte scale rows (2-byte aligned), Cout 320 (Cout_pad 384, three column tiles, the last 64 wide), N = 4:
    216 tiles. Bias + bf16 residual, bf16 output."""
    _run_dyadic(2701, 4, 320, 320, 1 / 4, False, False)


def test_dyadic_cin960_crosses_windows():
    """Cin 960: 15 chunks, 30-byte scale rows, 14 window refills. Bias + bf16 residual, fp32 output."""
    _run_dyadic(2702, 4, 960, 320, 1 / 8, True, False)


def test_dyadic_cin1920_fp32_residual_fp32():
    """Cin 1920 -> 640: 30 chunks (K = 17280), 60-byte scale rows, 29 window refills, five column tiles, N = 3: 270 tiles. Bias + fp32
    residual, fp32 output. (The only 1920 case with an fp64 reference: the costliest.)"""
    _run_dyadic(2703, 3, 1920, 640, 1 / 16, True, True)


def test_one_hot_first_and_last_block_cin320():
    """Two live channels per pixel: channel 319 (the last byte of the 10-byte scale row's last block) and channel p % 32 of block 0; every other
    code is zero, so an output is 18 products, each through one lane position and one scale pair; every tap is live. Exact."""
    from omgsr_amd import ops
    N, Cin, Cout = 4, 320, 320
    g = torch.Generator().manual_seed(2704)
    nb = Cin // 32
    f8 = lambda v: v.to(torch.float8_e4m3fn).view(torch.uint8)      # noqa: E731
    pix = torch.arange(N * H * W)
    xv = torch.zeros(N * H * W, Cin)
    xv[pix, pix % 32] = dp.signed_ints(g, (N * H * W,), 1, 7)
    xv[pix, 319] = dp.signed_ints(g, (N * H * W,), 1, 7)
    xc = f8(xv).reshape(N, H, W, Cin)
    xs = (127 + ((pix[:, None] + 3 * torch.arange(nb)[None, :]) % 5) - 2).to(torch.uint8).reshape(N, H, W, nb)
    wc = f8(dp.dyadic(g, torch.randint(0, 2, (Cout, 9, Cin), generator=g).float()))
    co, tp, bl = torch.arange(Cout)[:, None, None], torch.arange(9)[None, :, None], torch.arange(nb)[None, None, :]
    wsc = (127 + ((co + 2 * tp + 3 * bl) % 7) - 3).to(torch.uint8)
    pw = V.pack_planes(wc, wsc, None, DEV)
    xq = ops.Mxfp8(xc.to(DEV), xs.to(DEV))
    uc, us = V.unpack_planes(pw)
    want = dp.rounded(V.conv_mxfp8_ref(xq.codes, xq.scales, uc, us, Cout), torch.float32)
    y = _launch(lambda: _conv(xq, pw, out_dtype=ops.OUT_F32))
    V._eq(y, want, "one-hot operand")


# ---- accuracy on random operands -----------------------------------------------------------------------------------------------------------------

def quantize_c64(x):
    """ops.quantize_mxfp8 of x [..., K], K % 64 == 0: K padded with zero channels to a multiple of 128 (blocks are independent), then cut back."""
    from omgsr_amd import ops
    K = x.shape[-1]
    Kp = (K + 127) // 128 * 128
    q = ops.quantize_mxfp8(torch.nn.functional.pad(x, (0, Kp - K)).contiguous())
    return ops.Mxfp8(q.codes[..., :K].contiguous(), q.scales[..., :K // 32].contiguous())


def _random_problem(seed, N, Cin, Cout, h=H, w=W):
    from omgsr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, h, w, Cin, generator=g, device=DEV) * torch.exp2(torch.randint(-3, 4, (N, h, w, Cin // 32, 1), generator=g, device=DEV).float()).expand(
        N, h, w, Cin // 32, 32).reshape(N, h, w, Cin)
    wt = (torch.randn(Cout, Cin, 3, 3, generator=g, device=DEV) / (3.0 * Cin ** 0.5)).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g, device=DEV)
    return quantize_c64(x), ops.pack_conv_weight_mxfp8(wt, b, cin_multiple=64)


def test_pack_c64_is_the_quantiser_in_the_documented_layout():
    from omgsr_amd import ops
    from omgsr_amd.testing import mxfp8_ref
    g = torch.Generator().manual_seed(2705)
    w = (torch.randn(200, 320, 3, 3, generator=g) * torch.exp2(torch.randint(-6, 6, (200, 1, 1, 1), generator=g).float())).to(torch.bfloat16)
    b = torch.randn(200, generator=g)
    pw = ops.pack_conv_weight_mxfp8(w.to(DEV), b.to(DEV), cin_multiple=64)
    wc, wsc = mxfp8_ref(w.permute(0, 2, 3, 1).reshape(200, 9, 320).float())
    want = V.pack_planes(wc, wsc, b, DEV)
    assert pw.cout == 200 and pw.cin == 320 and pw.w_cm.shape == (5, 9, 256, 64) and pw.w_scale.shape == (5, 256, 2, 16)
    assert torch.equal(pw.w_cm, want.w_cm) and torch.equal(pw.w_scale, want.w_scale) and torch.equal(pw.bias, want.bias)
    with pytest.raises(ValueError):
        ops.pack_conv_weight_mxfp8(w.to(DEV), b.to(DEV))                    # the % 128 form keeps refusing 320


@pytest.mark.parametrize("Cin", [320, 960])
def test_accuracy_random_operands(Cin):
    from omgsr_amd import ops
    N, Cout = 4, 320
    xq, pw = _random_problem(2800 + Cin, N, Cin, Cout)
    ref = V._dequant_conv(xq, pw, Cout)
    y = _launch(lambda: _conv(xq, pw, out_dtype=ops.OUT_F32))
    e = float((y.double() - ref).norm() / ref.norm())
    print(f"mxfp8 deep conv Cin {Cin} (K = {9 * Cin}) vs the fp64 product of the dequantised operands: rel-L2 {e:.3e} (bound {CONV_REL_L2:g})")
    assert torch.isfinite(y).all() and e <= CONV_REL_L2


# ---- the GroupNorm producer ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", [320, 960])
def test_group_norm_apply_mxfp8_c64_straddling_groups(Cc):
    """G = 32 over 320 / 960 channels: 10 / 30 channels per group, so a thread's octet and a 32-channel block straddle groups. bf16 input, SiLU.
    Judged as tests/test_fp8_vae_gpu.py judges the existing entry: against ops.quantize_mxfp8 of the fp32 statement - equal scales except where
    the block maximum sits on a power of two, codes at most one ordinal apart."""
    from omgsr_amd import _lib, ops
    N, h, w, G = 2, 40, 52, 32
    g = torch.Generator(device=DEV).manual_seed(2901)
    x = (torch.randn(N, h, w, Cc, generator=g, device=DEV) * 2 + 0.3).to(torch.bfloat16)
    # group means differ, so a channel normalised with its neighbour group's statistics would be off by whole units
    x = (x.float() + torch.arange(G, device=DEV).repeat_interleave(Cc // G).float() * 0.25).to(torch.bfloat16)
    gamma = torch.rand(Cc, generator=g, device=DEV) + 0.5
    beta = torch.randn(Cc, generator=g, device=DEV) * 0.2
    xf = x.float().reshape(N, h * w, G, Cc // G)
    mean = xf.mean((1, 3)).contiguous()
    rstd = torch.rsqrt(xf.var((1, 3), unbiased=False) + 1e-6).contiguous()
    x0 = x.clone()
    got = ops.group_norm_apply_mxfp8(x, mean, rstd, gamma, beta, G, ops.ACT_SILU, c64=True)
    assert isinstance(got, ops.Mxfp8) and torch.equal(x, x0)
    sc = rstd.repeat_interleave(Cc // G, 1) * gamma
    sh = beta - mean.repeat_interleave(Cc // G, 1) * sc
    v = x.float() * sc[:, None, None, :] + sh[:, None, None, :]
    ref32 = v * torch.sigmoid(v)
    want = quantize_c64(ref32.contiguous())
    blk = ref32.reshape(N, h, w, -1, 32).abs().amax(-1)
    near = (blk / torch.exp2(torch.round(torch.log2(blk))) - 1).abs() < 1e-5
    same = got.scales == want.scales
    print(f"C {Cc}: equal-scale share {float(same.float().mean()):.6f}")
    assert bool((same | near).all()) and float(same.float().mean()) > 0.999
    ordn = lambda c: torch.where(c >= 128, -(c.int() - 128), c.int())      # noqa: E731
    d = (ordn(got.codes) - ordn(want.codes)).abs().reshape(N, h, w, -1, 32)[same]
    assert int(d.max()) <= 1
    if Cc % 128:
        # the existing entry still refuses it
        rc = _lib.load().omgsr_groupnorm_apply_mxfp8(x.data_ptr(), got.codes.data_ptr(), got.scales.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                     beta.data_ptr(), N, h * w, Cc, G, ops.ACT_SILU, N, ops.EL_16, ops._stream())
        assert rc == -2
        with pytest.raises(ValueError):
            ops.group_norm_apply_mxfp8(x, mean, rstd, gamma, beta, G, ops.ACT_SILU)


def test_fused_groupnorm_statistics():
    """The partials the epilogue leaves (gn_groups = 32 over 320 output channels: per-channel entries) fold to the statistics
    ops.group_norm_stats computes from the kernel's own output."""
    from omgsr_amd import ops
    N, Cin, Cout, G = 4, 320, 320, 32
    xq, pw = _random_problem(3001, N, Cin, Cout)
    y = _launch(lambda: _conv(xq, pw, gn_groups=G))
    assert getattr(y, "_omgsr_gn", None) is not None, "the epilogue left no partials"
    m1, _, v1 = ops.group_norm_stats(y, G, 1e-6)
    y2 = y.clone()
    m2, _, v2 = ops.group_norm_stats(y2, G, 1e-6)
    print(f"fused GroupNorm statistics vs the read pass: mean abs {float((m1 - m2).abs().max()):.3e}, var rel {float(((v1 - v2).abs() / v2).max()):.3e}")
    assert torch.allclose(m1, m2, atol=GN_MEAN_TOL, rtol=GN_MEAN_TOL) and torch.allclose(v1, v2, atol=GN_VAR_ATOL, rtol=GN_VAR_RTOL)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from omgsr_amd import _lib, ops
    from omgsr_amd._lib import IgemmArgs
    lib = _lib.load()

    def args(Cin=320, h=256, w=256, stride=1, upsample=0):
        Ho, Wo = ((h << upsample) + 2 - 3) // stride + 1, ((w << upsample) + 2 - 3) // stride + 1
        a = IgemmArgs()
        keep = [torch.zeros(1 * h * w * Cin, dtype=torch.uint8, device=DEV), torch.zeros(1 * h * w * (Cin // 32 + 1), dtype=torch.uint8, device=DEV),
                torch.zeros(9 * 128 * (Cin + 64), dtype=torch.uint8, device=DEV), torch.zeros(128 * (Cin // 64 + 1) * 2 * 16, dtype=torch.uint8, device=DEV),
                torch.zeros(Ho * Wo * 128, dtype=torch.bfloat16, device=DEV)]
        a.in_, a.in_scale, a.weight_cm, a.w_scale, a.out = (t.data_ptr() for t in keep)
        a.weight = a.weight_cm
        a.N, a.H, a.W, a.Cin, a.Cout, a.Cout_pad, a.K_pad = 1, h, w, Cin, 128, 128, 9 * Cin
        a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample, a.Ho, a.Wo = 3, 3, stride, 1, 1, upsample, Ho, Wo
        a.batch, a.alpha = 1, 1.0
        return a, keep

    def refused(a, what):
        before = V._launches(lambda: lib.omgsr_conv_mxfp8_deep(C.byref(a), ops._stream()))
        assert lib.omgsr_conv_mxfp8_deep_ok(C.byref(a)) == 0, what
        assert before[0] == -2 and before[1] == [], what                    # OMGSR_E_SHAPE, and nothing was launched

    a, keep = args()
    rc, v = V._launches(lambda: lib.omgsr_conv_mxfp8_deep(C.byref(a), ops._stream()))
    assert lib.omgsr_conv_mxfp8_deep_ok(C.byref(a)) == 1 and rc == 0 and v == [VARIANT]      # the served twin of the cases below
    assert lib.omgsr_conv_mxfp8_ok(C.byref(a)) == 0 and lib.omgsr_conv_mxfp8(C.byref(a), ops._stream()) == -2      # the existing entry keeps its answer
    for kw in (dict(Cin=96), dict(Cin=2112), dict(stride=2), dict(upsample=1), dict(h=4096, w=16), dict(h=64, w=64)):       # (16-wide: 512 tiles, but the FLAT form's ground)
        a, keep = args(**kw)
        refused(a, kw)
    a, keep = args()
    a.mxf8 = 1
    refused(a, "mxf8")
    ops.set_compute_dtype(torch.float16)
    try:
        a, keep = args()
        refused(a, "fp16")
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    torch.cuda.synchronize()


# ---- determinism, guard bands ------------------------------------------------------------------------------------------------------------------

def test_same_launch_twice_same_bits():
    xq, pw = _random_problem(3101, 4, 960, 320)
    a = _conv(xq, pw)
    for _ in range(3):
        assert torch.equal(_conv(xq, pw), a)


def test_batch_invariant():
    """Batch B == B x batch 1 under ops.set_batch_invariant(True): one sample (256 x 256 pixels, 256 tiles) is served on its own."""
    from omgsr_amd import ops
    xq, pw = _random_problem(3102, 2, 320, 128, 256, 256)
    ops.set_batch_invariant(True)
    try:
        full = _launch(lambda: _conv(xq, pw))
        for b in range(2):
            one = ops.Mxfp8(xq.codes[b:b + 1].contiguous(), xq.scales[b:b + 1].contiguous())
            assert torch.equal(_launch(lambda: _conv(one, pw)), full[b:b + 1])
    finally:
        ops.set_batch_invariant(False)


def _guarded(t, guard, fill):
    """t inside a larger allocation whose `guard` bytes in front of and behind it hold `fill`; returns (view, whole buffer)."""
    big = torch.full((guard + t.numel() + guard,), fill, dtype=torch.uint8, device=DEV)
    view = big[guard:guard + t.numel()].view_as(t)
    view.copy_(t)
    return view, big


@pytest.mark.parametrize("Cin", [320, 960])
def test_nan_around_every_plane_never_reaches_the_result(Cin):
    """All four planes (operand codes / scales, weight codes / scales) sit inside larger allocations whose bytes in front of and behind them hold
    NaN codes (0x7f) and NaN scales (0xff). The operand's last scale row ends 10 (30) bytes after a 2-byte-aligned start: a wider read, or a
    window refill that runs past the last chunk, would pull a NaN scale in. The result equals the dense planes' bit for bit, and the guard
    bytes are unchanged."""
    from omgsr_amd import ops
    N, Cout = 4, 320
    xq, pw = _random_problem(3103 + Cin, N, Cin, Cout)
    want = _conv(xq, pw)
    gc = 4 * W * Cin
    gs = gc // 32                                                           # (even: the scale plane keeps its 2-byte alignment)
    c, big_c = _guarded(xq.codes, gc, 0x7F)
    s, big_s = _guarded(xq.scales, gs, 0xFF)
    wcm, big_w = _guarded(pw.w_cm, 4096, 0x7F)
    wsc, big_ws = _guarded(pw.w_scale, 4096, 0xFF)
    pwg = ops.PackedWeight(wcm.view(-1, 64), pw.bias, pw.cout, pw.cin, 3, 3, w_cm=wcm, w_scale=wsc)
    got = _launch(lambda: _conv(ops.Mxfp8(c, s), pwg))
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)
    for big, guard, fill in ((big_c, gc, 0x7F), (big_s, gs, 0xFF), (big_w, 4096, 0x7F), (big_ws, 4096, 0xFF)):
        assert bool((big[:guard] == fill).all()) and bool((big[-guard:] == fill).all())


# ---- the pipeline, small case --------------------------------------------------------------------------------------------------------------------

VAE_KW = dict(block_out_channels=[32, 64, 128, 128], layers_per_block=1)
UNET_KW = dict(block_out_channels=[320, 640], down_block_types=["CrossAttnDownBlock2D", "DownBlock2D"], up_block_types=["UpBlock2D", "CrossAttnUpBlock2D"],
               layers_per_block=1, attention_head_dim=[5, 10], cross_attention_dim=128)
# 3 x 768^2 pixels: latent 96 x 96 > 64 x 64, four 64 x 64 latent tiles per image ride in one UNet call of 12 samples. 64-wide level (Cout 320):
# 12 x 2 x 8 x 3 = 576 tiles; 32-wide level (Cout 640): 12 x 1 x 4 x 5 = 240 - both served. Resnets: down 0 (320 -> 320), down 1 (320 -> 640),
# mid x 2 (640), up 0 (1280 -> 640, 960 -> 640), up 1 (960 -> 320, 640 -> 320): 8 resnets x (conv1 + conv2) = 16 launches per forward.
SERVED = 16
ALL = {"unet": {"fp8": [r"\.resnets\."]}}


def _small_case():
    from omgsr_amd.diffusers_api import AutoencoderKL, UNet2DConditionModel
    from omgsr_amd.testing import seeded_init_, synthetic_lq
    vae = seeded_init_(AutoencoderKL(**VAE_KW), 1, rounded=False)
    unet = seeded_init_(UNet2DConditionModel(**UNET_KW), 2, rounded=False)
    g = torch.Generator().manual_seed(5)
    inp = dict(prompt=torch.randn(1, 77, 128, generator=g).to(DEV, torch.bfloat16), noise=torch.randn(3, 4, 96, 96, generator=g).to(DEV),
               xs=[synthetic_lq(3, 768, 768, seed=s).to(DEV, torch.bfloat16) for s in (1, 2, 3)],
               tiny=synthetic_lq(1, 256, 256, seed=4).to(DEV, torch.bfloat16), tiny_noise=torch.randn(1, 4, 32, 32, generator=g).to(DEV))
    return vae, unet, inp


def _pipe(vae, unet, policy=None, wd=torch.bfloat16):
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    return OMGSR_S_Infer(None, None, 273, DEV, wd, vae=vae, unet=unet, precision_policy=policy)


def _call(pipe, inp, x, noise=None):
    pipe.vae.posterior_noise = inp["noise"] if noise is None else noise
    return pipe(x, inp["prompt"], 64, 32)[0]


def test_pipeline_small_case():
    """Reduced UNet, both levels served (16 launches of variant 27 per forward). Measured on MI355X, draw 0: bf16 tier vs accurate tier rel-L2
    2.717e-2; key on vs key off 9.71e-2 (bound 16 x 2.717e-2 = 4.35e-1, see S_BF16_VS_ACCURATE_REL_L2_MEASURED above for the margin's reason)."""
    from omgsr_amd.precision import fp8_unet_conv_layers
    vae, unet, inp = _small_case()
    x = inp["xs"][0]
    with torch.no_grad():
        plain = _pipe(vae, unet)
        assert fp8_unet_conv_layers(unet) == []
        y_plain, v = V._launches(lambda: _call(plain, inp, x))
        assert VARIANT not in v
        marked = _pipe(vae, unet, ALL)
        assert len(fp8_unet_conv_layers(unet)) == 16
        y8, v = V._launches(lambda: _call(marked, inp, x))
        print(f"variant {VARIANT} launches: {v.count(VARIANT)} (expected {SERVED})")
        assert v.count(VARIANT) == SERVED
        assert torch.isfinite(y8.float()).all() and not torch.equal(y8, y_plain)
        e = float((y8.float() - y_plain.float()).norm() / y_plain.float().norm())
        print(f"small case, key on vs key off: rel-L2 {e:.3e} (bound {FP8_MARGIN:g} x {S_BF16_VS_ACCURATE_REL_L2_MEASURED:.3e})")
        assert e <= FP8_MARGIN * S_BF16_VS_ACCURATE_REL_L2_MEASURED
        # graph replay == eager (the MXFP8 packs are built by the eager warm-up in front of the capture)
        eager = [_call(marked, inp, xx) for xx in inp["xs"]]
        assert torch.equal(eager[0], y8)
        marked.enable_graphs(True)
        got = [_call(marked, inp, xx) for xx in inp["xs"]]
        assert marked.graphs.captures == 1 and marked.graphs.replays == 2
        for a, b in zip(eager, got):
            assert torch.equal(a, b)
        marked.enable_graphs(False)
        # a tiny input (latent 32 x 32, one untiled sample: 12 and 5 tiles): every problem is refused, the bf16 path runs bit for bit
        y_tiny8, v = V._launches(lambda: _call(marked, inp, inp["tiny"], inp["tiny_noise"]))
        assert VARIANT not in v
        # a later pipeline without the key unmarks, and computes what the first one did; an explicit False is the key off
        again = _pipe(vae, unet)
        assert fp8_unet_conv_layers(unet) == []
        assert torch.equal(_call(again, inp, x), y_plain)
        assert torch.equal(_call(again, inp, inp["tiny"], inp["tiny_noise"]), y_tiny8)
        off = _pipe(vae, unet, {"unet": {"fp8": False}})
        assert fp8_unet_conv_layers(unet) == [] and torch.equal(_call(off, inp, x), y_plain)
