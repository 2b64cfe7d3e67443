"""The fp8 tier's opt-in MXFP8 up-sampling convolutions on the MI355X: mxfp8_conv_up_kernel / mxfp8_conv_up_multi_kernel (omgsr_conv_mxfp8_up(_multi),
timing variants 25 / 26) bit for bit against the fp64 F.conv2d of the nearest-up-sampled map on dyadic and one-hot operands, the pack against the
host quantiser in the documented layout, random operands against the fp64 product of the dequantised operands (bound: the nine-tap kernel's own
error in the same run), the fused GroupNorm statistics, determinism, launch groups, guard bands, refusals, the pipeline's routing on a small
case (untiled, graph replay, tiled) and one quality case against the accurate tier."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyadic_probe as dp  # noqa: E402
import guard_bands as gb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE, MULTI = 25, 26
E_SHAPE = -2

# Quality case: untiled FLUX VAE decode of a seeded 64 x 64 latent (512^2 pixels), batch 1, against the accurate-tier VAE on the same weights.
# First measurement (MI355X): {"fp8": True, "fp8_upsample": True} rel-L2 1.010e-1 / 30.07 dB (18 launches of variant 21, 3 of variant 25);
# {"fp8": True} alone 6.134e-2 / 34.40 dB; the bf16 VAE 1.376e-2 / 47.38 dB. The bound is the first figure x 1.25 (DESIGN.md 3.4 records all three:
# the up-samplers sit on the main path, with no residual around them, and cost more accuracy per layer than the resnet convs).
VAE_FP8_UP_VS_ACCURATE_REL_L2_MEASURED = 1.010e-1


@pytest.fixture(autouse=True)
def _bf16_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.bfloat16)
    ops.set_batch_invariant(False)


def _launches(fn):
    """Run fn() with the per-launch timing on; returns (result, variants of the kind-1 launches in order)."""
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
    return out, [e.variant for e in buf[:n] if e.kind == 1]


def _launch(fn, want=(ONE,)):
    out, v = _launches(fn)
    assert v and sorted(v) == sorted(want), f"expected kernel variants {sorted(want)}, the library ran {sorted(v)}"
    return out


def _eq(got, want, what):
    want = want.to(got.device)
    if not torch.equal(got, want):
        bad = got.double() != want.double()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from the exact reference, first at {bad.nonzero()[:4].tolist()}")


# ---- the problem as the C ABI sees it ----------------------------------------------------------------------------------------------------------

def raw_args(N, H, W, Cin, Cout, stride=1, upsample=1):
    """The geometry of conv3x3(up2(x)) (no pointers: the predicate does not look at them)."""
    from omgsr_amd._lib import IgemmArgs
    a = IgemmArgs()
    Ho, Wo = ((H << upsample) + 2 - 3) // stride + 1, ((W << upsample) + 2 - 3) // stride + 1
    a.N, a.H, a.W, a.Cin, a.Cout, a.Cout_pad, a.K_pad = N, H, W, Cin, Cout, (Cout + 127) // 128 * 128, 9 * Cin
    a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample, a.Ho, a.Wo = 3, 3, stride, 1, 1, upsample, Ho, Wo
    a.batch, a.alpha = 1, 1.0
    return a


def served_shape(Cin, Cout, N=2, H=44, W=72):
    """The smallest batch of 44 x 72 low-resolution maps (ragged in both directions: 44 % 8 = 4, 72 % 32 = 8) the predicate accepts: N grows
    only as the dispatcher's tile-count rule demands."""
    from omgsr_amd import _lib
    lib = _lib.load()
    assert H % 8 and W % 32
    while not lib.omgsr_conv_mxfp8_up_ok(C.byref(raw_args(N, H, W, Cin, Cout))):
        N += 1
        assert N <= 16, "the predicate accepts no batch of 44 x 72 maps"
    return N, H, W


# ---- the documented layout, restated --------------------------------------------------------------------------------------------------------------

def pack_up_planes(codes, scales, bias, cout, dev):
    """Planes codes uint8 [4 phases, cout, 4 taps, Cin], scales uint8 [4, cout, 4, Cin / 32] -> the PackedWeight omgsr_conv_mxfp8_up reads
    (include/omgsr_hip.h): codes [4][Cin / 64][4][Cout_pad][64], scales [4][Cin / 64][Cout_pad][2][4]; zero rows up to a multiple of 128."""
    from omgsr_amd import ops
    cin = codes.shape[-1]
    cout8 = (cout + 7) // 8 * 8
    cp = (cout8 + 127) // 128 * 128
    c = torch.zeros(4, cp, 4, cin, dtype=torch.uint8)
    s = torch.zeros(4, cp, 4, cin // 32, dtype=torch.uint8)
    c[:, :cout], s[:, :cout] = codes, scales
    w_ph = c.view(4, cp, 4, cin // 64, 64).permute(0, 3, 2, 1, 4).contiguous().to(dev)
    sc = s.view(4, cp, 4, cin // 64, 2).permute(0, 3, 1, 4, 2).contiguous().to(dev)
    b = None
    if bias is not None:
        b = torch.zeros(cout8)
        b[:cout] = bias
        b = b.to(dev)
    return ops.PackedWeight(w_ph.view(-1, 64), b, cout8, cin, 3, 3, w_ph=w_ph, w_scale=sc)


def unpack_up_planes(pw):
    """The inverse, from the packed bytes: codes [4, Cout_pad, 4, Cin], scales [4, Cout_pad, 4, Cin / 32]."""
    _, nch, _, cp, _ = pw.w_ph.shape
    codes = pw.w_ph.permute(0, 3, 2, 1, 4).reshape(4, cp, 4, nch * 64)
    scales = pw.w_scale.permute(0, 2, 4, 1, 3).reshape(4, cp, 4, nch * 2)
    return codes, scales


# ---- references --------------------------------------------------------------------------------------------------------------------------------

def conv_up_ref(x, w, bias=None):
    """fp64 F.conv2d (3x3, stride 1, pad 1) of the nearest-2x up-sampled map: x [N, H, W, Cin], w [Cout, Cin, 3, 3] -> float64 [N, 2H, 2W, Cout]."""
    xu = x.double().permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
    y = F.conv2d(xu, w.double(), None if bias is None else bias.double().to(x.device), padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def _phase_operands(t, pad_value=0):
    """t [N, H, W, K] -> {(phase, tap): [N H W, K]}: phase (a, b), tap (dy, dx) reads rows y - 1 + a + dy, columns x - 1 + b + dx."""
    N, H, W, K = t.shape
    tp = F.pad(t, (0, 0, 1, 1, 1, 1), value=pad_value)
    return {(2 * a + b, 2 * dy + dx): tp[:, a + dy:a + dy + H, b + dx:b + dx + W].reshape(N * H * W, K)
            for a in (0, 1) for b in (0, 1) for dy in (0, 1) for dx in (0, 1)}


def _interleave(phases, N, H, W, cout):
    """[4 phases] of [N H W, cout] -> [N, 2H, 2W, cout] (phase 2a + b is output pixel (2y + a, 2x + b))."""
    return torch.stack(phases, 0).reshape(2, 2, N, H, W, cout).permute(2, 3, 0, 4, 1, 5).reshape(N, 2 * H, 2 * W, cout)


def phase_ref(xv, wv, bias=None):
    """Four 2 x 2 convolutions of the low-resolution map: xv float64 [N, H, W, C], wv float64 [4 phases, cout, 4 taps, C] -> float64 [N, 2H, 2W, cout]."""
    N, H, W, _ = xv.shape
    ops_ = _phase_operands(xv)
    out = []
    for ph in range(4):
        acc = sum(ops_[(ph, tap)] @ wv[ph, :, tap].T for tap in range(4))
        out.append(acc if bias is None else acc + bias.double().to(acc.device)[:acc.shape[1]])
    return _interleave(out, N, H, W, wv.shape[1])


def mxfp8_phase_ref(xc, xs, uc, us, cout, bias=None):
    """Exact result from the bytes the kernel reads (operand planes, unpacked weight planes) through dyadic_probe.mxfp8_ref, which asserts the bit
    budget and the 2^13 window of every 8-wide K group on the way. float64 [N, 2H, 2W, cout]."""
    N, H, W, _ = xc.shape
    A, S = _phase_operands(xc), _phase_operands(xs, 127)
    out = []
    for ph in range(4):
        a = torch.cat([A[(ph, t)] for t in range(4)], -1)
        s = torch.cat([S[(ph, t)] for t in range(4)], -1)
        out.append(dp.mxfp8_ref(a, s, uc[ph].reshape(uc.shape[1], -1), us[ph].reshape(us.shape[1], -1), cout, bias=bias))
    return _interleave(out, N, H, W, cout)


# ---- dyadic probes -------------------------------------------------------------------------------------------------------------------------------

def dyadic_case(g, N, H, W, Cin, Cout, density=0.25, spread=12, bias=True):
    """x = m 2^(r[pixel] + c[block]) (|m| <= 7 at `density`, r in -2 .. 2), w = tap 2^(t[cout] - c[block] + d[cout, block]) with tap in -2 .. 2 and
    d in {0, 1} (c in [-spread, spread] per 32-channel block): every phase sum is an integer of magnitude <= 8 times the block's power of two and
    quantises exactly, the scale bytes differ between blocks on both sides (neighbouring blocks by up to 2^(2 spread)), and all products of a
    block - so of every 8-wide K group - lie within a factor 7 x 8. bf16 tensors; bias fp32 +-{1..3} 2^(t + 0..4)."""
    nb = Cin // 32
    c = torch.randint(-spread, spread + 1, (nb,), generator=g)
    r = torch.randint(-2, 3, (N, H, W, 1), generator=g)
    xe = (r + c).float().repeat_interleave(32, -1)
    x = dp.dyadic(g, xe) * (torch.rand((N, H, W, Cin), generator=g) < density)
    t = torch.randint(-6, 7, (Cout, 1), generator=g)
    we = (t - c + torch.randint(0, 2, (Cout, nb), generator=g)).float().repeat_interleave(32, -1)      # [Cout, Cin]
    taps = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=g).float()
    w = taps * torch.exp2(we)[:, :, None, None]
    b = dp.dyadic(g, t.reshape(Cout).float() + torch.randint(0, 5, (Cout,), generator=g).float(), (1, 3)) if bias else None
    assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.equal(w.to(torch.bfloat16).float(), w)
    return x.to(torch.bfloat16), w.to(torch.bfloat16), b


def _run_dyadic(seed, Cin, Cout, density, out_f32, bias):
    from omgsr_amd import ops
    N, H, W = served_shape(Cin, Cout)
    print(f"low-resolution maps {N} x {H} x {W}, {Cin} -> {Cout}")
    g = torch.Generator().manual_seed(seed)
    x, w, b = dyadic_case(g, N, H, W, Cin, Cout, density, bias=bias)
    x, w = x.to(DEV), w.to(DEV)
    pw = ops.pack_conv_weight_mxfp8_up(w, None if b is None else b.to(DEV))
    xq = ops.quantize_mxfp8(x)
    uc, us = unpack_up_planes(pw)
    # operand and phase sums quantise exactly, and the scale bytes differ between blocks
    assert torch.equal(dp.mxfp8_values(xq.codes, xq.scales), x.double())
    assert torch.equal(dp.mxfp8_values(uc[:, :Cout], us[:, :Cout]), ops._phase_kernels(w.float().permute(0, 2, 3, 1)).reshape(4, Cout, 4, Cin).double())
    assert int((xq.scales[..., 1:] != xq.scales[..., :-1]).sum()) > 0 and int((us[..., 1:] != us[..., :-1]).sum()) > 0
    ref = conv_up_ref(x, w, b)
    # the same value from the bytes the kernel reads, with dyadic_probe's budget and 2^13 group-window assertions
    assert torch.equal(mxfp8_phase_ref(xq.codes, xq.scales, uc, us, Cout, bias=pw.bias), ref)
    want = dp.rounded(ref, torch.float32 if out_f32 else torch.bfloat16)
    y = _launch(lambda: ops.conv2d_mxfp8_up(xq, pw, out_dtype=ops.OUT_F32 if out_f32 else ops.OUT_BF16))
    _eq(y, want, f"mxfp8 up-sampling conv {N}x{H}x{W}x{Cin} -> {Cout}")


def test_dyadic_ragged_map_cin256_cout256_bf16():
    """44 x 72 low-resolution maps (2 x 3 x 6 tiles, the last tile of each row 8 pixels wide, the last tile row 4 pixels high: ragged tiles in both
    directions, and every image border carries data for all four phases), Cin 256 (four chunks), Cout 256 (two column tiles), bf16 output."""
    _run_dyadic(3101, 256, 256, 1 / 4, False, False)


def test_dyadic_ragged_map_cin512_cout512_fp32_bias():
    """Cin 512 (eight chunks: the weight-scale registers are reloaded seven times), Cout 512 (four column tiles), fp32 output with bias."""
    _run_dyadic(3102, 512, 512, 1 / 8, True, True)


@pytest.mark.parametrize("tap", range(9))
def test_one_hot_lane_phase_tap_map(tap):
    """One nonzero code per pixel (pixel p at channel (37 p) % Cin) and ONE nonzero 3x3 tap (ky, kx): in every phase (a, b) that tap lands in
    exactly one 2 x 2 tap, so each output is a single product through one lane position and one scale pair. Equal to the fp64 conv."""
    from omgsr_amd import ops
    Cin, Cout = 128, 128
    N, H, W = served_shape(Cin, Cout)
    g = torch.Generator().manual_seed(3200 + tap)
    pix = torch.arange(N * H * W)
    x = torch.zeros(N * H * W, Cin)
    x[pix, (37 * pix) % Cin] = dp.signed_ints(g, (N * H * W,), 1, 7) * torch.exp2(((pix % 5) - 2).float())
    x = x.reshape(N, H, W, Cin).to(DEV, torch.bfloat16)
    co, ci = torch.arange(Cout)[:, None], torch.arange(Cin)[None, :]
    w = torch.zeros(Cout, Cin, 3, 3)
    w[:, :, tap // 3, tap % 3] = dp.signed_ints(g, (Cout, Cin), 1, 2) * torch.exp2((((co + 3 * (ci // 32)) % 7) - 3).float())
    w = w.to(DEV, torch.bfloat16)
    pw, xq = ops.pack_conv_weight_mxfp8_up(w, None), ops.quantize_mxfp8(x)
    y = _launch(lambda: ops.conv2d_mxfp8_up(xq, pw, out_dtype=ops.OUT_F32))
    _eq(y, dp.rounded(conv_up_ref(x, w), torch.float32), f"one-hot operand, tap ({tap // 3}, {tap % 3})")


def test_pack_is_the_quantiser_of_the_phase_kernels_in_the_documented_layout():
    from omgsr_amd import ops
    from omgsr_amd.testing import mxfp8_ref
    g = torch.Generator().manual_seed(3104)
    w = (torch.randn(200, 256, 3, 3, generator=g) * torch.exp2(torch.randint(-6, 6, (200, 1, 1, 1), generator=g).float())).to(torch.bfloat16)
    b = torch.randn(200, generator=g)
    pw = ops.pack_conv_weight_mxfp8_up(w.to(DEV), b.to(DEV))
    ph = ops._phase_kernels(w.float().permute(0, 2, 3, 1)).reshape(4, 200, 4, 256)          # fp64 sums, phase 2a + b, tap 2 dy + dx
    codes, scales = mxfp8_ref(ph)
    want = pack_up_planes(codes, scales, b, 200, DEV)
    assert pw.cout == 200 and pw.cin == 256 and pw.w_ph.shape == (4, 4, 4, 256, 64) and pw.w_scale.shape == (4, 4, 256, 2, 4)
    assert torch.equal(pw.w_ph, want.w_ph) and torch.equal(pw.w_scale, want.w_scale) and torch.equal(pw.bias, want.bias)


# ---- accuracy on random operands -----------------------------------------------------------------------------------------------------------------

def _random_problem(seed, N, H, W, Cin, Cout):
    from omgsr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g, device=DEV) * torch.exp2(torch.randint(-3, 4, (N, H, W, Cin // 32, 1), generator=g, device=DEV).float()).expand(
        N, H, W, Cin // 32, 32).reshape(N, H, W, Cin)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g, device=DEV) / (3.0 * Cin ** 0.5)).to(torch.bfloat16)
    b = torch.randn(Cout, generator=g, device=DEV)
    return x.to(torch.bfloat16), w, b


def _dequant_up(xq, pw, cout):
    uc, us = unpack_up_planes(pw)
    return phase_ref(dp.mxfp8_values(xq.codes, xq.scales), dp.mxfp8_values(uc, us)[:, :cout], pw.bias)


@pytest.mark.parametrize("Cin", [128, 256, 512])
def test_accuracy_random_operands_against_the_nine_tap_kernel(Cin):
    """rel-L2 against the fp64 convolution of the dequantised operands; the bound is not invented: it is twice the figure the nine-tap kernel
    (mxfp8_conv_kernel, the same instruction and epilogue, 9 / 4 of the K) reaches at the same Cin in the same run."""
    from omgsr_amd import ops
    import test_fp8_vae_gpu as T
    Cout = 128
    N, H, W = served_shape(Cin, Cout)
    x, w, b = _random_problem(3300 + Cin, N, H, W, Cin, Cout)
    xq, pw = ops.quantize_mxfp8(x), ops.pack_conv_weight_mxfp8_up(w, b)
    ref = _dequant_up(xq, pw, Cout)
    y = _launch(lambda: ops.conv2d_mxfp8_up(xq, pw, out_dtype=ops.OUT_F32))
    e_up = float((y.double() - ref).norm() / ref.norm())
    xq9, pw9 = T._random_problem(2200 + Cin, 8, 48, 128, Cin, Cout)
    ref9 = T._dequant_conv(xq9, pw9, Cout)
    y9 = ops.conv2d_mxfp8(xq9, pw9, out_dtype=ops.OUT_F32)
    e9 = float((y9.double() - ref9).norm() / ref9.norm())
    print(f"Cin {Cin}: up-sampling kernel rel-L2 {e_up:.3e}, nine-tap kernel {e9:.3e} (bound 2 x = {2 * e9:.3e})")
    assert torch.isfinite(y).all() and e_up <= 2 * e9


# ---- fused GroupNorm statistics ------------------------------------------------------------------------------------------------------------------

def test_fused_groupnorm_statistics_in_the_phase_forms_slots():
    """The partials have the 16-bit phase form's layout ([N][tile][upper / lower 4 tile rows][4 phases][G][2]: asked of omgsr_igemm for the same
    problem) and hold, slot by slot, the (sum, sum of squares) recomputed from the kernel's own fp32 output. Bound: fp32 accumulation of the
    n = 4 x 32 x 8 values of a slot entry, n eps relative to the sum of magnitudes (1024 x 6e-8 < 1e-4; 2e-4 asserted)."""
    from omgsr_amd import ops
    Cin, Cout, G = 128, 256, 32
    N, H, W = served_shape(Cin, Cout)
    x, w, b = _random_problem(3401, N, H, W, Cin, Cout)
    xq, pw = ops.quantize_mxfp8(x), ops.pack_conv_weight_mxfp8_up(w, b)
    y = _launch(lambda: ops.conv2d_mxfp8_up(xq, pw, out_dtype=ops.OUT_F32, gn_groups=G))
    h = getattr(y, "_omgsr_gn", None)
    assert h is not None, "the epilogue left no partials"
    y16 = ops.conv2d(x, ops.pack_conv_weight(w, b, cout_multiple=8, upsample_phases=True), upsample=True, gn_groups=G, out_dtype=ops.OUT_F32)
    ty, tx = (H + 7) // 8, (W + 31) // 32
    assert h.partial.shape == y16._omgsr_gn.partial.shape == (N, ty * tx * 2 * 4, G, 2)
    # recompute: low-resolution pixel (yy, xx) of phase (a, b) is output pixel (2 yy + a, 2 xx + b)
    yl = y.double().reshape(N, H, 2, W, 2, G, Cout // G).permute(0, 2, 4, 1, 3, 5, 6)              # [N, a, b, H, W, G, gsz]
    yp = F.pad(yl, (0, 0, 0, 0, 0, tx * 32 - W, 0, ty * 8 - H))                                      # zero rows / columns add nothing
    blk = yp.reshape(N, 2, 2, ty, 2, 4, tx, 32, G, Cout // G)                                         # [N, a, b, ty, wm, 4, tx, 32, G, gsz]
    def fold(v):
        return v.sum((5, 7, 9)).permute(0, 3, 5, 4, 1, 2, 6).reshape(N, ty * tx * 2 * 4, G)         # [N, ty, tx, wm, a, b, G]
    s1, s2, sa = fold(blk), fold(blk * blk), fold(blk.abs())
    got = h.partial.double()
    d1, d2 = (got[..., 0] - s1).abs(), (got[..., 1] - s2).abs()
    print(f"slot sums vs the output: worst {float((d1 / sa.clamp_min(1e-30)).max()):.3e} of the sum of magnitudes, squares {float((d2 / s2.clamp_min(1e-30)).max()):.3e}")
    assert bool((d1 <= 2e-4 * sa + 1e-30).all()) and bool((d2 <= 2e-4 * s2 + 1e-30).all())
    # ... and ops.group_norm_stats folds them to what its read pass over the tensor computes (the bf16 halo kernel's tolerances, tests/test_kernels_gpu.py)
    m1, _, v1 = ops.group_norm_stats(y, G, 1e-6)
    m2, _, v2 = ops.group_norm_stats(y.clone(), G, 1e-6)
    assert torch.allclose(m1, m2, atol=2e-3, rtol=2e-3) and torch.allclose(v1, v2, atol=2e-3, rtol=4e-3)


# ---- determinism and routing ---------------------------------------------------------------------------------------------------------------------

def test_same_launch_twice_same_bits():
    from omgsr_amd import ops
    N, H, W = served_shape(256, 128)
    x, w, b = _random_problem(3501, N, H, W, 256, 128)
    xq, pw = ops.quantize_mxfp8(x), ops.pack_conv_weight_mxfp8_up(w, b)
    a = ops.conv2d_mxfp8_up(xq, pw)
    for _ in range(3):
        assert torch.equal(ops.conv2d_mxfp8_up(xq, pw), a)


def test_batch_invariant():
    """Batch B == B x batch 1 under ops.set_batch_invariant(True): one sample (a 104 x 120 map: 13 x 4 tiles x 4 phases = 208) is served alone."""
    from omgsr_amd import ops
    x, w, b = _random_problem(3502, 3, 104, 120, 128, 128)
    xq, pw = ops.quantize_mxfp8(x), ops.pack_conv_weight_mxfp8_up(w, b)
    ops.set_batch_invariant(True)
    try:
        full = _launch(lambda: ops.conv2d_mxfp8_up(xq, pw))
        for i in range(3):
            one = ops.Mxfp8(xq.codes[i:i + 1].contiguous(), xq.scales[i:i + 1].contiguous())
            assert torch.equal(_launch(lambda: ops.conv2d_mxfp8_up(one, pw)), full[i:i + 1])
    finally:
        ops.set_batch_invariant(False)


GROUP_SHAPES = [(3, 44, 72), (4, 40, 80), (4, 54, 54), (6, 32, 54), (7, 54, 32), (12, 32, 32), (2, 100, 48), (4, 36, 96), (3, 64, 64)]


def test_launch_groups_equal_their_single_calls():
    """Nine problems of one layer (more than 8: two launches, 8 + 1 - variants 26 and 25), a group of one (variant 25): outputs and GroupNorm
    partials equal each problem's own call. Every shape is served alone too (checked), so the singles run the same kernel body."""
    from omgsr_amd import _lib, ops
    lib = _lib.load()
    Cin, Cout, G = 128, 128, 32
    _, w, b = _random_problem(3503, 1, 8, 32, Cin, Cout)
    pw = ops.pack_conv_weight_mxfp8_up(w, b)
    xqs = []
    for i, (N, H, W) in enumerate(GROUP_SHAPES):
        assert lib.omgsr_conv_mxfp8_up_ok(C.byref(raw_args(N, H, W, Cin, Cout))) == 1, (N, H, W)
        xqs.append(ops.quantize_mxfp8(_random_problem(3510 + i, N, H, W, Cin, Cout)[0]))
    singles = [_launch(lambda xq=xq: ops.conv2d_mxfp8_up(xq, pw, gn_groups=G)) for xq in xqs]
    ys = _launch(lambda: ops.conv2d_mxfp8_up_multi(xqs, pw, gn_groups=G), want=(MULTI, ONE))
    for y, s, shp in zip(ys, singles, GROUP_SHAPES):
        assert torch.equal(y, s), shp
        assert torch.equal(y._omgsr_gn.partial, s._omgsr_gn.partial), shp
    one = _launch(lambda: ops.conv2d_mxfp8_up_multi(xqs[:1], pw, gn_groups=G), want=(ONE,))
    assert torch.equal(one[0], singles[0])
    four = _launch(lambda: ops.conv2d_mxfp8_up_multi(xqs[2:6], pw), want=(MULTI,))
    for y, s in zip(four, singles[2:6]):
        assert torch.equal(y, s)


def test_nan_guard_bands_around_planes_weight_and_output():
    """Code, scale, weight, weight-scale and bias planes sit between bands of 0xFF bytes (NaN in e4m3 and E8M0) and every tensor the op allocates
    (output, GroupNorm partials) inside a fence: a pixel fetched from outside the map instead of the zero page would turn the result NaN, a
    stray store would change the fence. The result equals the dense call's bit for bit - one problem and a launch group."""
    from omgsr_amd import ops
    Cin, Cout = 128, 128
    N, H, W = served_shape(Cin, Cout)
    x, w, b = _random_problem(3504, N, H, W, Cin, Cout)
    xq, pw = ops.quantize_mxfp8(x), ops.pack_conv_weight_mxfp8_up(w, b)
    want = ops.conv2d_mxfp8_up(xq, pw, gn_groups=32)
    xe, pe = gb.embed(xq), gb.embed(pw)
    with gb.fenced_outputs():
        got = ops.conv2d_mxfp8_up(xe, pe, gn_groups=32)
    assert torch.isfinite(got.float()).all() and torch.equal(got, want) and torch.equal(got._omgsr_gn.partial, want._omgsr_gn.partial)
    xq2 = ops.quantize_mxfp8(_random_problem(3505, 2, 54, 54, Cin, Cout)[0])
    want2 = ops.conv2d_mxfp8_up_multi([xq, xq2], pw)
    with gb.fenced_outputs():
        got2 = ops.conv2d_mxfp8_up_multi([xe, gb.embed(xq2)], pe)
    for a, bb in zip(got2, want2):
        assert torch.isfinite(a.float()).all() and torch.equal(a, bb)
    torch.cuda.synchronize()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from omgsr_amd import _lib, ops
    lib = _lib.load()

    def full(N=1, H=128, W=128, Cin=128, Cout=128, **kw):
        a = raw_args(N, H, W, Cin, Cout, **kw)
        keep = [torch.zeros(N * H * W * Cin, dtype=torch.uint8, device=DEV), torch.zeros(N * H * W * (Cin // 32 + 1), dtype=torch.uint8, device=DEV),
                torch.zeros(16 * a.Cout_pad * Cin, dtype=torch.uint8, device=DEV), torch.zeros(a.Cout_pad * Cin, dtype=torch.uint8, device=DEV),
                torch.zeros(N * a.Ho * a.Wo * Cout, dtype=torch.bfloat16, device=DEV)]
        a.in_, a.in_scale, a.weight_ph, a.w_scale, a.out = (t.data_ptr() for t in keep)
        a.weight = a.weight_ph
        return a, keep

    def refused(a):
        ok = lib.omgsr_conv_mxfp8_up_ok(C.byref(a))
        rc, v = _launches(lambda: lib.omgsr_conv_mxfp8_up(C.byref(a), ops._stream()))
        rcm, vm = _launches(lambda: lib.omgsr_conv_mxfp8_up_multi(C.byref(a), 1, ops._stream()))
        return ok == 0 and lib.omgsr_conv_mxfp8_up_multi_ok(C.byref(a), 1) == 0 and rc == E_SHAPE and rcm == E_SHAPE and v == [] and vm == []

    a, keep = full()                                                          # the served twin of the cases below
    assert lib.omgsr_conv_mxfp8_up_ok(C.byref(a)) == 1
    rc, v = _launches(lambda: lib.omgsr_conv_mxfp8_up(C.byref(a), ops._stream()))
    assert rc == 0 and v == [ONE]
    for kw in (dict(stride=2), dict(Cin=320), dict(Cin=1024), dict(W=40, H=512), dict(W=8, H=2048), dict(upsample=0), dict(H=32, W=32)):
        a, keep = full(**kw)
        assert refused(a), kw
    for field, val in (("mxf8", 1), ("in_split", 1), ("w_split", 1), ("mx_chunks16", 2), ("out_mx", 1), ("out_lo_off", 128)):
        a, keep = full()
        setattr(a, field, val)
        assert lib.omgsr_conv_mxfp8_up_ok(C.byref(a)) == 0, field
        rc, v = _launches(lambda: lib.omgsr_conv_mxfp8_up(C.byref(a), ops._stream()))
        assert rc != 0 and v == [], field
    a, keep = full()
    table = torch.zeros(128 * 2, device=DEV)
    a.gn_scale_shift, a.gn_nimg, a.gn_act = table.data_ptr(), 1, ops.ACT_SILU  # the GroupNorm producer has no MXFP8 phase form
    assert lib.omgsr_conv_mxfp8_up_ok(C.byref(a)) == 0
    # the nine-tap entry point keeps refusing the up-sampling problem
    a, keep = full()
    assert lib.omgsr_conv_mxfp8_ok(C.byref(a)) == 0
    # fp16 compute type and the accurate tier: the predicate refuses, the pack raises, nothing is launched
    w = torch.zeros(128, 128, 3, 3, device=DEV, dtype=torch.bfloat16)
    for wd in (torch.float16, torch.float32):
        ops.set_compute_dtype(wd)
        try:
            a, keep = full()
            assert refused(a), wd
            with pytest.raises(ValueError):
                ops.pack_conv_weight_mxfp8_up(w, None)
        finally:
            ops.set_compute_dtype(torch.bfloat16)
    torch.cuda.synchronize()


def test_refused_layer_runs_exactly_as_without_the_mark():
    """ops.conv2d(upsample=True) with the layer's MXFP8 form on offer: a problem the predicate refuses (too few tiles) launches what it launched
    before and returns the same bits; a served one launches variant 25 and nothing else of kind 1."""
    from omgsr_amd import ops
    Cin, Cout = 128, 128
    x, w, b = _random_problem(3601, 1, 32, 32, Cin, Cout)
    pw16 = ops.pack_conv_weight(w, b, cout_multiple=8, upsample_phases=True)
    packs = []
    def pack8():
        packs.append(1)
        return ops.pack_conv_weight_mxfp8_up(w, b)
    y0, v0 = _launches(lambda: ops.conv2d(x, pw16, upsample=True))
    y1, v1 = _launches(lambda: ops.conv2d(x, pw16, upsample=True, fp8_up_pack=pack8))
    assert v0 == v1 and ONE not in v1 and torch.equal(y0, y1) and not packs       # (the pack is not even built for a refused problem)
    N, H, W = served_shape(Cin, Cout)
    x = _random_problem(3602, N, H, W, Cin, Cout)[0]
    y8, v8 = _launches(lambda: ops.conv2d(x, pw16, upsample=True, fp8_up_pack=pack8, gn_groups=32))
    assert v8 == [ONE] and packs == [1] and getattr(y8, "_omgsr_gn", None) is not None
    assert torch.equal(y8, ops.conv2d_mxfp8_up(ops.quantize_mxfp8(x), ops.pack_conv_weight_mxfp8_up(w, b)))
    ys, vs = _launches(lambda: ops.conv2d_multi([x, x[:1, :32, :32].contiguous()], pw16, upsample=True, fp8_up_pack=pack8))
    assert vs == [MULTI] and torch.equal(ys[0], y8)


# ---- the pipeline, small case --------------------------------------------------------------------------------------------------------------------
# tests/test_fp8_vae_gpu.py's reduced-width FLUX VAE ([128, 128, 256, 256]), 256 x 256 pixels, batch 1. The decoder's up-samplers see low-resolution
# maps 32^2 (256 ch: 1 x 4 x 2 x 4 = 32 phase tiles), 64^2 (256 ch: 2 x 8 x 2 x 4 = 128) and 128^2 (128 ch: 4 x 16 x 1 x 4 = 256): only the last
# reaches the dispatcher's 192 tiles, so ONE launch of variant 25 per decode.
UP = {"vae": {"fp8_upsample": True}}
FP8 = {"vae": {"fp8": True}}
BOTH = {"vae": {"fp8": True, "fp8_upsample": True}}


def test_pipeline_small_case():
    import test_fp8_vae_gpu as T
    from omgsr_amd.precision import fp8_conv_layers, fp8_upsample_layers
    vae, flux, inp = T._small_case()
    x = inp["xs"][0]
    with torch.no_grad():
        only8 = T._pipe(vae, flux, FP8)
        y_fp8, v = _launches(lambda: T._call(only8, inp, x))
        assert ONE not in v and MULTI not in v and fp8_upsample_layers(vae) == []
        plain = T._pipe(vae, flux)
        y_plain, v = _launches(lambda: T._call(plain, inp, x))
        assert ONE not in v
        on = T._pipe(vae, flux, UP)                                          # the key without "fp8"
        assert fp8_upsample_layers(vae) == [f"decoder.up_blocks.{i}.upsamplers.0.conv" for i in range(3)] and fp8_conv_layers(vae) == []
        y_up, v = _launches(lambda: T._call(on, inp, x))
        assert v.count(ONE) == 1 and T.VARIANT not in v
        assert torch.isfinite(y_up.float()).all() and not torch.equal(y_up, y_plain)
        e = float((y_up.float() - y_plain.float()).norm() / y_plain.float().norm())
        print(f"small case, fp8 up-samplers vs the fp8 tier without the key: rel-L2 {e:.3e}")
        assert e < 0.2
        both = T._pipe(vae, flux, BOTH)                                      # ... and with it
        y_both, v = _launches(lambda: T._call(both, inp, x))
        assert v.count(ONE) == 1 and v.count(T.VARIANT) == 4 and not torch.equal(y_both, y_fp8)
        # graph replay == eager (the pack was built by the eager / warm-up call in front of the capture)
        eager = [T._call(both, inp, xx) for xx in inp["xs"]]
        assert torch.equal(eager[0], y_both)
        both.enable_graphs(True)
        got = [T._call(both, inp, xx) for xx in inp["xs"]]
        assert both.graphs.captures == 1 and both.graphs.replays == 2
        for a, b in zip(eager, got):
            assert torch.equal(a, b)
        both.enable_graphs(False)
        # an in-place weight edit re-packs the MXFP8 form
        conv = vae.decoder.up_blocks[2].upsamplers[0].conv
        assert conv.fp8_up
        w0 = conv.weight.detach().clone()
        conv.weight.mul_(1.5)
        assert not torch.equal(T._call(both, inp, x), y_both)
        conv.weight.copy_(w0)
        assert torch.equal(T._call(both, inp, x), y_both)
        # the key off: a later {"fp8": ...}-only pipeline unmarks and computes, bit for bit, what the first one did; so does one without any key
        again8 = T._pipe(vae, flux, FP8)
        assert fp8_upsample_layers(vae) == []
        y, v = _launches(lambda: T._call(again8, inp, x))
        assert ONE not in v and torch.equal(y, y_fp8)
        assert torch.equal(T._call(T._pipe(vae, flux), inp, x), y_plain)


def test_tiled_pipeline_serves_each_upsampler_as_one_launch_group():
    """tests/test_fp8_vae_tiled_gpu.py's case (512 x 512 pixels, decoder tile 32: tile-shape groups 54 / 32 wide, one tile each). The three
    up-samplers see groups of 54 / 32, 108 / 64 and 216 / 128 low-resolution pixels: 264 phase tiles at the smallest level, so every layer is
    served as a group - three launches of variant 26 - and only under _init_tiled_vae(fp8_convs=True)."""
    import test_fp8_vae_gpu as T
    import test_fp8_vae_tiled_gpu as TT
    from omgsr_amd.pipelines.vaehook import VAEHook
    vae, flux, inp = TT._tiled_case()
    x = inp["xs"][0]
    kw = dict(encoder_tile_size=256, decoder_tile_size=32)
    with torch.no_grad():
        plain = T._pipe(vae, flux)
        plain._init_tiled_vae(**kw)
        y_plain, v = _launches(lambda: TT._call(plain, inp, x))
        assert ONE not in v and MULTI not in v
        on = T._pipe(vae, flux, UP)
        with pytest.raises(ValueError, match="tiled VAE"):
            on._init_tiled_vae(**kw)
        # hooks built without fp8_convs on the marked VAE: the 16-bit kernels, bit for bit
        vae.encoder._tile_hook = VAEHook(vae.encoder, 256, is_decoder=False, fast_decoder=False, fast_encoder=False, color_fix=False)
        vae.decoder._tile_hook = VAEHook(vae.decoder, 32, is_decoder=True, fast_decoder=False, fast_encoder=False, color_fix=False)
        y_off, v = _launches(lambda: TT._call(on, inp, x))
        assert ONE not in v and MULTI not in v and torch.equal(y_off, y_plain)
        on._init_tiled_vae(**kw, fp8_convs=True)
        y_up, v = _launches(lambda: TT._call(on, inp, x))
        print(f"variant {MULTI} launches: {v.count(MULTI)}, variant {ONE}: {v.count(ONE)}")
        assert v.count(MULTI) == 3 and v.count(ONE) == 0 and T.VARIANT not in v
        assert torch.isfinite(y_up.float()).all() and not torch.equal(y_up, y_plain)
        e = float((y_up.float() - y_plain.float()).norm() / y_plain.float().norm())
        print(f"small tiled case, fp8 up-samplers vs the tiled fp8 tier without the key: rel-L2 {e:.3e}")
        assert e < 0.2
        again = T._pipe(vae, flux)
        with pytest.raises(ValueError):
            again._init_tiled_vae(**kw, fp8_convs=True)
        again._init_tiled_vae(**kw)
        assert torch.equal(TT._call(again, inp, x), y_plain)
    vae.encoder._tile_hook = vae.decoder._tile_hook = None


# ---- quality, one case -------------------------------------------------------------------------------------------------------------------------

def test_vae_decode_quality_against_the_accurate_tier():
    """Untiled full-width FLUX VAE decode of a seeded 64 x 64 latent (512^2 pixels), batch 1, seeded full-mantissa weights: {"fp8", "fp8_upsample"}
    (all three up-samplers served: low-resolution maps 64^2 and 128^2 at 512 channels, 256^2 at 256), {"fp8"} alone and, for the record, the bf16
    VAE, each against the accurate-tier VAE on the same weights and latent. The bound is the first measured figure x 1.25 (the project's idiom)."""
    import test_fp8_vae_gpu as T
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
    from omgsr_amd.precision import apply_default_policy, set_fp8_conv, set_fp8_upsample
    from omgsr_amd.testing import psnr, rel_l2, seeded_init_
    sd = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303, rounded=False).state_dict()
    z = torch.randn(1, 16, 64, 64, generator=torch.Generator().manual_seed(77))

    def run(tier):
        wd = torch.float32 if tier == "fp32" else torch.bfloat16
        ops.set_compute_dtype(wd)
        p = AutoencoderKL(**FLUX_VAE_CONFIG)
        p.load_state_dict(sd)
        p = p.to(DEV, wd).eval()
        if tier == "fp32":
            apply_default_policy(vae=p)
        if tier in ("fp8", "fp8+up"):
            set_fp8_conv(p, True)
        if tier == "fp8+up":
            set_fp8_upsample(p, True)
        with torch.no_grad():
            y, v = _launches(lambda: p.decode(z.to(DEV, wd)).sample)
        return y.float().cpu(), v

    try:
        ref, v0 = run("fp32")
        y16, v16 = run("bf16")
        y8, v8 = run("fp8")
        yu, vu = run("fp8+up")
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    e16, e8, eu = rel_l2(y16, ref), rel_l2(y8, ref), rel_l2(yu, ref)
    print(f"FLUX VAE decode 512^2 vs the accurate tier: bf16 rel-L2 {e16:.3e} PSNR {psnr(y16, ref):.2f} dB | fp8 rel-L2 {e8:.3e} PSNR {psnr(y8, ref):.2f} dB | "
          f"fp8 + fp8_upsample ({vu.count(T.VARIANT)} + {vu.count(ONE)} launches) rel-L2 {eu:.3e} PSNR {psnr(yu, ref):.2f} dB")
    assert ONE not in v0 + v16 + v8 and vu.count(ONE) == 3 and vu.count(T.VARIANT) == v8.count(T.VARIANT) > 0
    assert torch.isfinite(yu).all()
    assert VAE_FP8_UP_VS_ACCURATE_REL_L2_MEASURED is not None and eu <= 1.25 * VAE_FP8_UP_VS_ACCURATE_REL_L2_MEASURED
