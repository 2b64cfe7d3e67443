"""The fp8 tier's opt-in VAE convolutions on the MI355X: mxfp8_conv_kernel (omgsr_conv_mxfp8, timing variant 21) bit for bit against the fp64
restatement of the bytes it reads (im2col + dyadic_probe.mxfp8_ref) on dyadic and one-hot operands, against the fp64 product of the dequantised
operands on random ones, the GroupNorm apply pass that writes MXFP8, the fused GroupNorm statistics, determinism, refusals, the pipeline's
routing on a small case and one full-size quality case (the FLUX VAE's untiled 1024^2 decode against the accurate tier)."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyadic_probe as dp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARIANT = 21

# Random MXFP8 operands against the fp64 product of the dequantised operands: the bound tests/test_fp8_gpu.py asserts for the same instruction
# (GEMM_REL_L2; its error does not grow with K)
CONV_REL_L2 = 3e-5
# Fused GroupNorm statistics against ops.group_norm_stats' read pass over the kernel's own output: the tolerances tests/test_kernels_gpu.py uses
# for the bf16 halo kernel (mean atol = rtol = 2e-3; variance atol 2e-3, rtol 4e-3)
GN_MEAN_TOL, GN_VAR_ATOL, GN_VAR_RTOL = 2e-3, 2e-3, 4e-3
# Full-size quality case: untiled FLUX VAE decode of a seeded 128 x 128 latent (1024^2 pixels), batch 1, every eligible decoder conv in MXFP8,
# against the accurate-tier VAE on the same weights. Measured on draw 0 (MI355X): see DESIGN.md 3.4; the bound is that figure x 1.25.
# Draw 0: fp8 convs rel-L2 9.314e-2 / 30.78 dB (28 launches of variant 21), the bf16 VAE 1.372e-2 / 47.42 dB on the same latent.
VAE_FP8_VS_ACCURATE_REL_L2_MEASURED = 9.314e-2


@pytest.fixture(autouse=True)
def _bf16_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.bfloat16)
    ops.set_batch_invariant(False)


def _launches(fn):
    """Run fn() with the per-launch timing on; returns (result, sorted variants of the kind-1 launches, their count)."""
    from omgsr_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.omgsr_timing_enable(1)
    lib.omgsr_timing_reset()
    try:
        out = fn()
        buf = (_lib.TimingEntry * 4096)()
        n = lib.omgsr_timing_collect(buf, 4096)
    finally:
        lib.omgsr_timing_enable(0)
    v = [e.variant for e in buf[:n] if e.kind == 1]
    return out, v


def _launch(fn):
    """fn() must have made launches of variant 21 only."""
    out, v = _launches(fn)
    print(f"variants ran: {sorted(set(v))}")
    assert v and set(v) == {VARIANT}, f"expected kernel variant {VARIANT}, the library ran {sorted(set(v))}"
    return out


# ---- the documented layouts, restated ------------------------------------------------------------------------------------------------------------

def pack_planes(wc: torch.Tensor, wsc: torch.Tensor, bias, dev):
    """Weight planes codes uint8 [Cout, 9, Cin], scales uint8 [Cout, 9, Cin / 32] -> the PackedWeight omgsr_conv_mxfp8 reads (include/omgsr_hip.h):
    codes [Cin / 64][9][Cout_pad][64], scales [Cin / 64][Cout_pad][2][16] (byte t < 9 = tap t); zero rows up to a multiple of 128."""
    from omgsr_amd import ops
    cout, _, cin = wc.shape
    cp = (cout + 127) // 128 * 128
    c = torch.zeros(cp, 9, cin, dtype=torch.uint8)
    s = torch.zeros(cp, 9, cin // 32, dtype=torch.uint8)
    c[:cout], s[:cout] = wc, wsc
    codes = c.view(cp, 9, cin // 64, 64).permute(2, 1, 0, 3).contiguous().to(dev)
    sc = torch.zeros(cin // 64, cp, 2, 16, dtype=torch.uint8)
    sc[..., :9] = s.view(cp, 9, cin // 64, 2).permute(2, 0, 3, 1)
    return ops.PackedWeight(codes.view(-1, 64), None if bias is None else bias.to(dev), cout, cin, 3, 3, w_cm=codes, w_scale=sc.to(dev))


def unpack_planes(pw):
    """The inverse, from the packed bytes: codes [Cout_pad, 9, Cin], scales [Cout_pad, 9, Cin / 32]."""
    nch, _, cp, _ = pw.w_cm.shape
    codes = pw.w_cm.permute(2, 1, 0, 3).reshape(cp, 9, nch * 64)
    scales = pw.w_scale[..., :9].permute(1, 3, 0, 2).reshape(cp, 9, nch * 2)
    return codes, scales


def conv_mxfp8_ref(xc, xs, wc, wsc, cout, *, bias=None, residual=None, check=True, drop=None):
    """Exact 3x3 stride-1 pad-1 conv of the operand planes xc [N, H, W, C] / xs [N, H, W, C / 32] with the weight planes wc [Cout_pad, 9, C] /
    wsc [Cout_pad, 9, C / 32]: im2col (k = tap C + c; pixels outside the map are zero codes) + dyadic_probe.mxfp8_ref, float64 [N, H, W, cout].
    drop = (tap, side): that tap is NOT gathered at the border `side` ("top" | "left" | "bottom" | "right") - a deliberately wrong restatement."""
    N, H, W, Cc = xc.shape
    cp = F.pad(xc, (0, 0, 1, 1, 1, 1))
    sp = F.pad(xs, (0, 0, 1, 1, 1, 1), value=127)
    A, S = [], []
    for ky in range(3):
        for kx in range(3):
            a, s = cp[:, ky:ky + H, kx:kx + W].clone(), sp[:, ky:ky + H, kx:kx + W]
            if drop is not None and drop[0] == ky * 3 + kx:
                {"top": a[:, 0], "bottom": a[:, -1], "left": a[:, :, 0], "right": a[:, :, -1]}[drop[1]].zero_()
            A.append(a)
            S.append(s)
    A = torch.cat(A, -1).reshape(N * H * W, 9 * Cc)
    S = torch.cat(S, -1).reshape(N * H * W, 9 * Cc // 32)
    r = None if residual is None else residual.reshape(N * H * W, -1)
    y = dp.mxfp8_ref(A, S, wc.reshape(wc.shape[0], -1), wsc.reshape(wsc.shape[0], -1), cout, bias=bias, residual=r, check=check)
    return y.reshape(N, H, W, cout)


# ---- dyadic probes -----------------------------------------------------------------------------------------------------------------------------

def dyadic_case(seed, N, H, W, Cin, Cout, density, spread=30):
    """Operand codes m 2^j (|m| <= 7, j in {0, 1}) at `density`, scales 127 + r[pixel] + c[block] + d[pixel, block]; weight codes likewise, scales
    127 + t[cout] - c[block] + d'[cout, tap, block] (c in [-spread, spread]; d, d' in {0, 1}): the scale bytes differ per pixel, per block and per
    (cout, tap, block), neighbouring blocks by up to 2^(2 spread), and every output stays inside the bit budget and the 2^13 group window
    (dyadic_probe.mxfp8_ref asserts both). Pixel (0, 0, 5) carries a saturated +448 code, pixel (0, 1, 2) an all-zero block."""
    g = torch.Generator().manual_seed(seed)
    nb = Cin // 32
    c = torch.randint(-spread, spread + 1, (nb,), generator=g)
    f8 = lambda v: v.to(torch.float8_e4m3fn).view(torch.uint8)      # noqa: E731

    def codes(shape):
        return f8(dp.dyadic(g, torch.randint(0, 2, shape, generator=g).float()) * (torch.rand(shape, generator=g) < density))

    xc = codes((N, H, W, Cin))
    r = torch.randint(-2, 3, (N, H, W, 1), generator=g)
    xs = (127 + r + c + torch.randint(0, 2, (N, H, W, nb), generator=g)).to(torch.uint8)
    xc[0, 0, 5, 7] = f8(torch.tensor(448.0))
    xc[0, 1, 2, :32] = 0
    wc = codes((Cout, 9, Cin))
    t = torch.randint(-8, 9, (Cout, 1, 1), generator=g)
    wsc = (127 + t - c + torch.randint(0, 2, (Cout, 9, nb), generator=g)).to(torch.uint8)
    return g, xc, xs, wc, wsc, r.float(), t.float().reshape(1, 1, 1, Cout)


def _terms(g, e):
    """Epilogue terms +-{1..3} 2^(e + 0..4)."""
    return dp.dyadic(g, e + torch.randint(0, 5, tuple(e.shape), generator=g).float(), (1, 3))


def _eq(got, want, what):
    want = want.to(got.device)
    if not torch.equal(got, want):
        bad = got.double() != want.double()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from the exact restatement, first at {bad.nonzero()[:4].tolist()}")


def _run_dyadic(seed, N, H, W, Cin, Cout, density, out_f32, res_f32):
    from omgsr_amd import ops
    g, xc, xs, wc, wsc, r, t = dyadic_case(seed, N, H, W, Cin, Cout, density)
    bias = _terms(g, t.reshape(Cout))
    pw = pack_planes(wc, wsc, bias, DEV)
    xq = ops.Mxfp8(xc.to(DEV), xs.to(DEV))
    res = _terms(g, (r + t).expand(N, H, W, Cout)).to(DEV, torch.float32 if res_f32 else torch.bfloat16)
    uc, us = unpack_planes(pw)
    want = dp.rounded(conv_mxfp8_ref(xq.codes, xq.scales, uc, us, Cout, bias=pw.bias, residual=res), torch.float32 if out_f32 else torch.bfloat16)
    y = _launch(lambda: ops.conv2d_mxfp8(xq, pw, residual=res, out_dtype=ops.OUT_F32 if out_f32 else ops.OUT_BF16))
    _eq(y, want, f"mxfp8 conv {N}x{H}x{W}x{Cin} -> {Cout}")


def test_dyadic_ragged_map_cin128_bias_residual_bf16():
    """86 x 45 (ragged in W and H: 3 x 6 spatial tiles per image, the last of each row 22 pixels wide, the last row 5 pixels high), Cin 128 (two
    chunks), Cout 256 (two column tiles), bias + bf16 residual, bf16 output. Every image border carries data, so a lost border tap changes
    outputs (tests/test_fp8_vae_cpu.py shows the restatement itself depends on each of them)."""
    _run_dyadic(2101, 6, 45, 86, 128, 256, 1 / 4, False, False)


def test_dyadic_cin512_bias_residual_fp32():
    """Cin 512 (eight chunks, K = 4608: the weight-scale registers are reloaded seven times), 24 x 64 map, Cout 128, bias + fp32 residual, fp32 output."""
    _run_dyadic(2102, 32, 24, 64, 512, 128, 1 / 8, True, True)


def test_one_hot_lane_and_scale_map():
    """One nonzero code per (pixel, channel): pixel p carries a single code at channel (37 p) % Cin, so every output is nine products, each
    through one lane position and one scale pair; scales differ per block on both sides. Exact."""
    from omgsr_amd import ops
    N, H, W, Cin, Cout = 11, 48, 96, 256, 128
    g = torch.Generator().manual_seed(2103)
    nb = Cin // 32
    f8 = lambda v: v.to(torch.float8_e4m3fn).view(torch.uint8)      # noqa: E731
    pix = torch.arange(N * H * W)
    xv = torch.zeros(N * H * W, Cin)
    xv[pix, (37 * pix) % Cin] = dp.signed_ints(g, (N * H * W,), 1, 7)
    xc = f8(xv).reshape(N, H, W, Cin)
    xs = (127 + ((pix[:, None] + 3 * torch.arange(nb)[None, :]) % 5) - 2).to(torch.uint8).reshape(N, H, W, nb)
    wc = f8(dp.dyadic(g, torch.randint(0, 2, (Cout, 9, Cin), generator=g).float()))
    co, tp, bl = torch.arange(Cout)[:, None, None], torch.arange(9)[None, :, None], torch.arange(nb)[None, None, :]
    wsc = (127 + ((co + 2 * tp + 3 * bl) % 7) - 3).to(torch.uint8)
    pw = pack_planes(wc, wsc, None, DEV)
    xq = ops.Mxfp8(xc.to(DEV), xs.to(DEV))
    uc, us = unpack_planes(pw)
    want = dp.rounded(conv_mxfp8_ref(xq.codes, xq.scales, uc, us, Cout), torch.float32)
    y = _launch(lambda: ops.conv2d_mxfp8(xq, pw, out_dtype=ops.OUT_F32))
    _eq(y, want, "one-hot operand")


def test_pack_is_the_quantiser_in_the_documented_layout():
    """ops.pack_conv_weight_mxfp8 = the host reference quantiser applied to the bf16 weight per (cout, tap), in the layout pack_planes restates."""
    from omgsr_amd import ops
    from omgsr_amd.testing import mxfp8_ref
    g = torch.Generator().manual_seed(2104)
    w = (torch.randn(200, 256, 3, 3, generator=g) * torch.exp2(torch.randint(-6, 6, (200, 1, 1, 1), generator=g).float())).to(torch.bfloat16)
    b = torch.randn(200, generator=g)
    pw = ops.pack_conv_weight_mxfp8(w.to(DEV), b.to(DEV))
    wc, wsc = mxfp8_ref(w.permute(0, 2, 3, 1).reshape(200, 9, 256).float())
    want = pack_planes(wc, wsc, b, DEV)
    assert pw.cout == 200 and pw.cin == 256 and pw.w_cm.shape == (4, 9, 256, 64) and pw.w_scale.shape == (4, 256, 2, 16)
    assert torch.equal(pw.w_cm, want.w_cm) and torch.equal(pw.w_scale, want.w_scale) and torch.equal(pw.bias, want.bias)


# ---- accuracy on random operands -----------------------------------------------------------------------------------------------------------------

def _random_problem(seed, N, H, W, Cin, Cout):
    from omgsr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g, device=DEV) * torch.exp2(torch.randint(-3, 4, (N, H, W, Cin // 32, 1), generator=g, device=DEV).float()).expand(
        N, H, W, Cin // 32, 32).reshape(N, H, W, Cin)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g, device=DEV) / (3.0 * Cin ** 0.5)).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g, device=DEV)
    return ops.quantize_mxfp8(x), ops.pack_conv_weight_mxfp8(w, b)


def _dequant_conv(xq, pw, cout):
    """fp64 product of the dequantised operands (im2col matmul), [N, H, W, cout]."""
    uc, us = unpack_planes(pw)
    a = dp.mxfp8_values(xq.codes, xq.scales)
    wv = dp.mxfp8_values(uc.reshape(uc.shape[0], -1), us.reshape(us.shape[0], -1)).reshape(uc.shape[0], 9, -1)
    N, H, W, _ = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(N * H * W, cout, dtype=torch.float64, device=a.device)
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        acc += ap[:, ky:ky + H, kx:kx + W].reshape(N * H * W, -1) @ wv[:cout, tap].T
    return (acc + pw.bias.double()[:cout]).reshape(N, H, W, cout)


@pytest.mark.parametrize("Cin", [128, 256, 512])
def test_accuracy_random_operands(Cin):
    from omgsr_amd import ops
    N, H, W, Cout = 8, 48, 128, 128
    xq, pw = _random_problem(2200 + Cin, N, H, W, Cin, Cout)
    ref = _dequant_conv(xq, pw, Cout)
    y = _launch(lambda: ops.conv2d_mxfp8(xq, pw, out_dtype=ops.OUT_F32))
    e = float((y.double() - ref).norm() / ref.norm())
    print(f"mxfp8 conv Cin {Cin} (K = {9 * Cin}) vs the fp64 product of the dequantised operands: rel-L2 {e:.3e} (bound {CONV_REL_L2:g})")
    assert torch.isfinite(y).all() and e <= CONV_REL_L2


# ---- the GroupNorm producer ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_group_norm_apply_mxfp8_matches_quantised_fp32_statement(dtype):
    from omgsr_amd import ops
    N, H, W, Cc, G = 2, 40, 52, 256, 32
    g = torch.Generator(device=DEV).manual_seed(2301)
    x = (torch.randn(N, H, W, Cc, generator=g, device=DEV) * 2 + 0.3).to(dtype)
    gamma = torch.rand(Cc, generator=g, device=DEV) + 0.5
    beta = torch.randn(Cc, generator=g, device=DEV) * 0.2
    xf = x.float().reshape(N, H * W, G, Cc // G)
    mean = xf.mean((1, 3)).contiguous()
    rstd = torch.rsqrt(xf.var((1, 3), unbiased=False) + 1e-6).contiguous()
    x0 = x.clone()
    got = ops.group_norm_apply(x, mean, rstd, gamma, beta, G, ops.ACT_SILU, split=5)
    assert isinstance(got, ops.Mxfp8) and torch.equal(x, x0)                # the input tensor is read only
    sc = rstd.repeat_interleave(Cc // G, 1) * gamma                          # the apply kernels' arithmetic: x * (rstd gamma) + (beta - mean rstd gamma)
    sh = beta - mean.repeat_interleave(Cc // G, 1) * sc
    v = x.float() * sc[:, None, None, :] + sh[:, None, None, :]
    ref32 = v * torch.sigmoid(v)
    want = ops.quantize_mxfp8(ref32.contiguous())
    blk = ref32.reshape(N, H, W, -1, 32).abs().amax(-1)
    near = (blk / torch.exp2(torch.round(torch.log2(blk))) - 1).abs() < 1e-5
    same = got.scales == want.scales
    print(f"equal-scale share {float(same.float().mean()):.6f}")
    assert bool((same | near).all()) and float(same.float().mean()) > 0.999
    ordn = lambda c: torch.where(c >= 128, -(c.int() - 128), c.int())      # noqa: E731
    d = (ordn(got.codes) - ordn(want.codes)).abs().reshape(N, H, W, -1, 32)[same]
    assert int(d.max()) <= 1
    # GnSpec.apply is the same pass
    spec = ops.GnSpec(mean, rstd, gamma, beta, G, ops.ACT_SILU)
    again = spec.apply(x, 5)
    assert torch.equal(again.codes, got.codes) and torch.equal(again.scales, got.scales)


def test_fused_groupnorm_statistics():
    """The partials the epilogue leaves (gn_groups) fold to the statistics ops.group_norm_stats computes from the kernel's own output."""
    from omgsr_amd import ops
    N, H, W, Cin, Cout, G = 6, 45, 86, 128, 256, 32
    xq, pw = _random_problem(2401, N, H, W, Cin, Cout)
    y = _launch(lambda: ops.conv2d_mxfp8(xq, pw, gn_groups=G))
    assert getattr(y, "_omgsr_gn", None) is not None, "the epilogue left no partials"
    m1, _, v1 = ops.group_norm_stats(y, G, 1e-6)                             # folds the fused partials
    y2 = y.clone()                                                          # (a tensor without partials: the read pass)
    m2, _, v2 = ops.group_norm_stats(y2, G, 1e-6)
    print(f"fused GroupNorm statistics vs the read pass: mean abs {float((m1 - m2).abs().max()):.3e}, var rel {float(((v1 - v2).abs() / v2).max()):.3e}")
    assert torch.allclose(m1, m2, atol=GN_MEAN_TOL, rtol=GN_MEAN_TOL) and torch.allclose(v1, v2, atol=GN_VAR_ATOL, rtol=GN_VAR_RTOL)


# ---- determinism -------------------------------------------------------------------------------------------------------------------------------

def test_same_launch_twice_same_bits():
    from omgsr_amd import ops
    xq, pw = _random_problem(2501, 11, 45, 86, 256, 128)
    a = ops.conv2d_mxfp8(xq, pw)
    for _ in range(3):
        assert torch.equal(ops.conv2d_mxfp8(xq, pw), a)


def test_batch_invariant():
    """Batch B == B x batch 1 under ops.set_batch_invariant(True): one sample (256 x 256 pixels, 256 tiles) is served on its own."""
    from omgsr_amd import ops
    xq, pw = _random_problem(2502, 3, 256, 256, 128, 128)
    ops.set_batch_invariant(True)
    try:
        full = _launch(lambda: ops.conv2d_mxfp8(xq, pw))
        for b in range(3):
            one = ops.Mxfp8(xq.codes[b:b + 1].contiguous(), xq.scales[b:b + 1].contiguous())
            assert torch.equal(_launch(lambda: ops.conv2d_mxfp8(one, pw)), full[b:b + 1])
    finally:
        ops.set_batch_invariant(False)


def test_nan_around_the_planes_never_reaches_the_result():
    """The operand planes sit inside larger allocations whose bytes in front of and behind them (the rows a tap above the first image or below
    the last one would alias) hold NaN codes (0x7f) and NaN scales (0xff): a kernel that read a pixel outside the map, instead of the zero page
    and a zero scale byte, would return NaN. The result equals the dense planes' bit for bit."""
    from omgsr_amd import ops
    N, H, W, Cin, Cout = 10, 56, 96, 128, 128
    xq, pw = _random_problem(2503, N, H, W, Cin, Cout)
    want = ops.conv2d_mxfp8(xq, pw)
    # one allocation per plane, NaN bytes in front of and behind the dense [N, H, W, C] block (what the rows above / below the map would alias)
    guard = 4 * W * Cin
    big_c = torch.full((guard + xq.codes.numel() + guard,), 0x7F, dtype=torch.uint8, device=DEV)
    big_s = torch.full((guard // 32 + xq.scales.numel() + guard // 32,), 0xFF, dtype=torch.uint8, device=DEV)
    c = big_c[guard:guard + xq.codes.numel()].view_as(xq.codes)
    s = big_s[guard // 32:guard // 32 + xq.scales.numel()].view_as(xq.scales)
    c.copy_(xq.codes)
    s.copy_(xq.scales)
    got = _launch(lambda: ops.conv2d_mxfp8(ops.Mxfp8(c, s), pw))
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from omgsr_amd import _lib, ops
    from omgsr_amd._lib import IgemmArgs
    lib = _lib.load()

    def args(Cin=128, H=256, W=256, stride=1, upsample=0):
        Ho, Wo = ((H << upsample) + 2 - 3) // stride + 1, ((W << upsample) + 2 - 3) // stride + 1
        a = IgemmArgs()
        keep = [torch.zeros(1 * H * W * Cin, dtype=torch.uint8, device=DEV), torch.zeros(1 * H * W * (Cin // 32 + 1), dtype=torch.uint8, device=DEV),
                torch.zeros(9 * 128 * Cin, dtype=torch.uint8, device=DEV), torch.zeros(128 * 9 * Cin // 32 * 16, dtype=torch.uint8, device=DEV),
                torch.zeros(Ho * Wo * 128, dtype=torch.bfloat16, device=DEV)]
        a.in_, a.in_scale, a.weight_cm, a.w_scale, a.out = (t.data_ptr() for t in keep)
        a.weight = a.weight_cm
        a.N, a.H, a.W, a.Cin, a.Cout, a.Cout_pad, a.K_pad = 1, H, W, Cin, 128, 128, 9 * Cin
        a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample, a.Ho, a.Wo = 3, 3, stride, 1, 1, upsample, Ho, Wo
        a.batch, a.alpha = 1, 1.0
        return a, keep

    a, keep = args()
    assert lib.omgsr_conv_mxfp8_ok(C.byref(a)) == 1 and lib.omgsr_conv_mxfp8(C.byref(a), ops._stream()) == 0      # the served twin of the cases below
    for kw in (dict(Cin=320), dict(stride=2), dict(upsample=1)):
        a, keep = args(**kw)
        assert lib.omgsr_conv_mxfp8_ok(C.byref(a)) == 0, kw
        assert lib.omgsr_conv_mxfp8(C.byref(a), ops._stream()) == -2, kw
    a, keep = args(H=64, W=64)                                              # too few tiles for the halo form: the bf16 dispatcher would not pick it either
    assert lib.omgsr_conv_mxfp8_ok(C.byref(a)) == 0 and lib.omgsr_conv_mxfp8(C.byref(a), ops._stream()) == -2
    a, keep = args()
    a.mxf8 = 1                                                              # that field keeps its GEMM-only meaning
    assert lib.omgsr_conv_mxfp8(C.byref(a), ops._stream()) == -2
    ops.set_compute_dtype(torch.float16)
    try:
        a, keep = args()
        assert lib.omgsr_conv_mxfp8_ok(C.byref(a)) == 0 and lib.omgsr_conv_mxfp8(C.byref(a), ops._stream()) == -2
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    torch.cuda.synchronize()


# ---- the pipeline, small case --------------------------------------------------------------------------------------------------------------------

VAE_KW = dict(block_out_channels=[128, 128, 256, 256], layers_per_block=1, latent_channels=16, scaling_factor=0.3611, shift_factor=0.1159)
FLUX_KW = dict(num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64, pooled_projection_dim=32, in_channels=64)
# 256 x 256 pixels, batch 1: the 128-channel full-resolution resnets are 8 x 32 = 256 halo tiles (served), everything below full resolution has
# at most 64 (not the halo form: the bf16 path). Served: encoder.down_blocks.0.resnets.0 conv1 / conv2 and decoder.up_blocks.3.resnets.{0, 1} conv1 / conv2.
SERVED = 6
ALL = {"vae": {"fp8": [r"\.resnets\."]}}      # every eligible layer, encoder included (`True` marks precision.VAE_FP8: the decoder's)


def _small_case():
    from omgsr_amd.diffusers_api import AutoencoderKL, FluxTransformer2DModel
    from omgsr_amd.pipelines.omgsr_f import prepare_latent_image_ids
    from omgsr_amd.testing import seeded_init_, synthetic_lq
    vae = seeded_init_(AutoencoderKL(**VAE_KW), 3, rounded=False)
    flux = seeded_init_(FluxTransformer2DModel(**FLUX_KW), 4, rounded=False)
    g = torch.Generator().manual_seed(6)
    wd = torch.bfloat16
    inp = dict(pe=torch.randn(1, 32, 64, generator=g).to(DEV, wd), pooled=torch.randn(1, 32, generator=g).to(DEV, wd),
               tids=torch.zeros(32, 3, device=DEV, dtype=wd), iids=prepare_latent_image_ids(16, 16, DEV, wd),
               xs=[synthetic_lq(1, 256, 256, seed=s).to(DEV, wd) for s in (1, 2, 3)],
               n=torch.randn(1, 16, 32, 32, generator=g).to(DEV))
    return vae, flux, inp


def _pipe(vae, flux, policy=None):
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    return OMGSR_F_Infer(None, None, DEV, torch.float8_e4m3fn, 244, 1.0, vae=vae, flux_transformer=flux, precision_policy=policy)


def _call(pipe, inp, x):
    pipe.vae.posterior_noise = inp["n"]
    return pipe(x, inp["pe"], inp["pooled"], inp["tids"], inp["iids"], 32, 16)[0]


def test_pipeline_small_case():
    from omgsr_amd.diffusers_api import AutoencoderKL, FluxTransformer2DModel
    from omgsr_amd.precision import fp8_conv_layers
    vae, flux, inp = _small_case()
    x = inp["xs"][0]
    with torch.no_grad():
        plain = _pipe(vae, flux)
        assert fp8_conv_layers(vae) == []
        y_plain, v = _launches(lambda: _call(plain, inp, x))
        assert VARIANT not in v
        # an empty-policy pipeline and one built after a marked one are the same thing: bit-identical to the fp8 tier without the key
        marked = _pipe(vae, flux, ALL)
        assert len(fp8_conv_layers(vae)) == 2 * (4 + 2) + 2 * (4 * 2 + 2)    # every resnet conv1 / conv2 of encoder and decoder (mid blocks: 2 resnets each)
        y8, v = _launches(lambda: _call(marked, inp, x))
        print(f"variant {VARIANT} launches: {v.count(VARIANT)} (expected {SERVED})")
        assert v.count(VARIANT) == SERVED
        assert torch.isfinite(y8.float()).all() and not torch.equal(y8, y_plain)
        e = float((y8.float() - y_plain.float()).norm() / y_plain.float().norm())
        print(f"small case, fp8 VAE convs vs the fp8 tier without the key: rel-L2 {e:.3e}")
        assert e < 0.2
        # graph replay == eager
        eager = [_call(marked, inp, xx) for xx in inp["xs"]]
        assert torch.equal(eager[0], y8)
        marked.enable_graphs(True)
        got = [_call(marked, inp, xx) for xx in inp["xs"]]
        assert marked.graphs.captures == 1 and marked.graphs.replays == 2
        for a, b in zip(eager, got):
            assert torch.equal(a, b)
        marked.enable_graphs(False)
        # an in-place weight edit re-packs (both forms): equal to a fresh pipeline on the edited weights
        conv = vae.decoder.up_blocks[3].resnets[1].conv2
        assert conv.fp8
        w0 = conv.weight.detach().clone()
        conv.weight.mul_(1.5)
        y_edit = _call(marked, inp, x)
        assert not torch.equal(y_edit, y8)
        vae2 = AutoencoderKL(**VAE_KW).to(torch.bfloat16)                   # (the edited bf16 values themselves)
        vae2.load_state_dict(vae.state_dict())
        flux2 = FluxTransformer2DModel(**FLUX_KW).to(torch.bfloat16)
        flux2.load_state_dict(flux.state_dict())
        assert torch.equal(_call(_pipe(vae2, flux2, ALL), inp, x), y_edit)
        # `True` marks the default list (the decoder's layers: 4 of them served here)
        dflt = _pipe(vae, flux, {"vae": {"fp8": True}})
        assert all(n.startswith("decoder.") for n in fp8_conv_layers(vae)) and len(fp8_conv_layers(vae)) == 2 * (4 * 2 + 2)
        conv.weight.copy_(w0)
        _, v = _launches(lambda: _call(dflt, inp, x))
        assert v.count(VARIANT) == 4
        # a later pipeline without the key unmarks, and computes what the first one did
        conv.weight.copy_(w0)
        again = _pipe(vae, flux)
        assert fp8_conv_layers(vae) == []
        assert torch.equal(_call(again, inp, x), y_plain)


# ---- quality, one full-size case -----------------------------------------------------------------------------------------------------------------

def test_full_size_vae_decode_quality():
    """Untiled FLUX VAE decode of a seeded 128 x 128 latent (1024^2 pixels), batch 1, seeded full-mantissa weights: the fp8 VAE (every eligible
    decoder conv served) and, for the record, the bf16 VAE, against the accurate-tier VAE on the same weights and the same latent.
    The bound is the figure measured on draw 0 x 1.25 (the project's idiom; DESIGN.md 3.4 records it)."""
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
    from omgsr_amd.precision import apply_default_policy, fp8_conv_layers, set_fp8_conv
    from omgsr_amd.testing import psnr, rel_l2, seeded_init_
    sd = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303, rounded=False).state_dict()
    z = torch.randn(1, 16, 128, 128, generator=torch.Generator().manual_seed(77))

    def run(tier):
        wd = torch.float32 if tier == "fp32" else torch.bfloat16
        ops.set_compute_dtype(wd)
        p = AutoencoderKL(**FLUX_VAE_CONFIG)
        p.load_state_dict(sd)
        p = p.to(DEV, wd).eval()
        if tier == "fp32":
            apply_default_policy(vae=p)
        if tier == "fp8":
            set_fp8_conv(p, True)
        with torch.no_grad():
            y, v = _launches(lambda: p.decode(z.to(DEV, wd)).sample)
        return y.float().cpu(), v.count(VARIANT), len(fp8_conv_layers(p))

    try:
        ref, n0, _ = run("fp32")
        y16, n1, _ = run("bf16")
        y8, n8, marked = run("fp8")
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    e16, p16, e8, p8 = rel_l2(y16, ref), psnr(y16, ref), rel_l2(y8, ref), psnr(y8, ref)
    print(f"FLUX VAE decode 1024^2 vs the accurate tier: bf16 rel-L2 {e16:.3e} PSNR {p16:.2f} dB | fp8 convs ({n8} launches of {marked} marked layers) "
          f"rel-L2 {e8:.3e} PSNR {p8:.2f} dB")
    assert n0 == 0 and n1 == 0 and n8 == 2 * (2 + 3 * 4)                     # mid block + up_blocks 0-3: every decoder resnet conv is served
    assert torch.isfinite(y8).all()
    assert e8 <= 1.25 * VAE_FP8_VS_ACCURATE_REL_L2_MEASURED
