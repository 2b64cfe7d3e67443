"""Bit-exact dyadic probes: one or more per omgsr_igemm kernel variant (the id the dispatcher records, igemm.hip), each asserting the variant
that ran and torch.equal against the float64 restatement of the packed bytes after the one documented output rounding (tests/dyadic_probe.py).

A rel-L2 bound on random data cannot see a defect confined to a few outputs (a correction chunk read from the wrong K block, a border tap
lost, one ragged tile); with dyadic operands inside the bit budget every such defect changes the result. Routing comes from the shapes alone
(the OMGSR_* A/B knobs are read once per process). Nonlinear epilogues (SiLU, GELU, GEGLU) stay with the tolerance tests; the GroupNorm-fused
variants 10 / 11, whose producer always applies SiLU, are probed on data where that SiLU is the identity in fp32 (gn_fused_case).
tests/test_gn_stats_probes_gpu.py pins the GroupNorm statistics the same kernels' epilogues leave."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyadic_probe as dp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_TIER = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


class _DryRun(Exception):
    """Raised by the dry-run launcher once a probe has built its data and reference (the budget is asserted by then)."""


def _launch(variant, fn):
    """Run fn() with the per-launch timing on and assert that every omgsr_igemm launch it made was kernel variant `variant` (None: that it made
    no such launch - statistics kernels only; a tuple: ONE variant of these - a probe that pins what several GEMM-shaped kernels share)."""
    from omgsr_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.omgsr_timing_enable(1)
    lib.omgsr_timing_reset()
    try:
        out = fn()
        buf = (_lib.TimingEntry * 256)()
        n = lib.omgsr_timing_collect(buf, 256)
    finally:
        lib.omgsr_timing_enable(0)
    ran = sorted({e.variant for e in buf[:n] if e.kind == 1})
    print(f"variant ran: {ran}")
    if isinstance(variant, tuple):
        assert len(ran) == 1 and ran[0] in variant, f"expected one kernel variant of {variant}, the dispatcher ran {ran}"
    else:
        assert ran == ([] if variant is None else [variant]), f"expected kernel variant {variant}, the dispatcher ran {ran}"
    return out


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _eq(got, want, what):
    got = got.detach()
    want = want.to(got.device)
    if not torch.equal(got, want):
        bad = (got.double() != want.double()) & ~(got.double().isnan() & want.double().isnan())
        idx = bad.nonzero()[:4].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outputs differ from the exact restatement, first at {idx}")


def _act(g, shape, pix=(-2, 2), chan=(0, 1), block=1, split=False):
    """NHWC / token activations: one exponent per pixel (row) plus one per channel (or per `block` channels)."""
    C = shape[-1]
    rows = 1
    for d in shape[:-1]:
        rows *= d
    e = dp.exponents(g, rows, C, row=pix, col=chan, block=block).reshape(*shape)
    return dp.two_term(g, e) if split else dp.dyadic(g, e)


def _wt(g, cout, cin, R=3, S=3, nnz=12, row=(-2, 2), chan=(0, 1), block=1, split=False):
    """[Cout, Cin, R, S]: exponents per output channel plus per input channel (block), nnz nonzero (tap, channel) entries per output."""
    e = dp.exponents(g, cout, cin, row=row, col=chan, block=block)[:, :, None, None].expand(cout, cin, R, S).contiguous()
    v = dp.two_term(g, e) if split else dp.dyadic(g, e)
    return v * dp.sparse_mask(g, cout, cin * R * S, nnz).reshape(cout, cin, R, S)


def _small(g, shape, e=(-2, 1)):
    """bias / residual values: +-{1..3} 2^e."""
    return dp.dyadic(g, torch.randint(e[0], e[1] + 1, shape, generator=g).float(), (1, 3))


def _gate(g, n):
    return torch.exp2(torch.randint(-1, 2, (n,), generator=g).float()) * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)


def _ops():
    from omgsr_amd import ops
    return ops


# ---- variant 1: igemm_kernel (register staged) ------------------------------------------------------------------------------------

def v1_conv_in_128x128(dev, launch):
    """bf16; 3 input channels padded to 8 (no LDS-DMA K-step), 32768 rows: the 128 x 128 tile; bias + residual."""
    ops = _ops()
    g = _g(101)
    x = _act(g, (1, 128, 256, 8)).to(dev, ops.act_dtype())
    pw = ops.pack_conv_weight(_wt(g, 128, 3, nnz=12), _small(g, (128,)), device=dev)
    r = _small(g, (1, 128, 256, 128)).to(dev, ops.act_dtype())
    want = dp.rounded(dp.conv_ref(x, pw, bias=pw.bias, residual=r), ops.act_dtype())
    y = launch(1, lambda: ops.conv2d(x, pw, pad=1, residual=r))
    _eq(y, want, "conv_in")


def v1_stride2_asym_pad_cout4(dev, launch):
    """fp16; stride 2 with odd H / W and the VAE's asymmetric (0, 1, 0, 1) pad, Cout 4 widened to 8 (128 x 32 tile), fp32 output:
    the widened columns come out as exact zeros."""
    ops = _ops()
    g = _g(102)
    x = _act(g, (2, 33, 35, 64)).to(dev, ops.act_dtype())
    pw = ops.pack_conv_weight(_wt(g, 4, 64, nnz=24), _small(g, (4,)), device=dev, cout_multiple=8)
    assert pw.cout == 8
    want = dp.rounded(dp.conv_ref(x, pw, stride=2, pad=(0, 1, 0, 1), bias=pw.bias), torch.float32)
    y = launch(1, lambda: ops.conv2d(x, pw, stride=2, pad=(0, 1, 0, 1), out_dtype=ops.OUT_F32))
    assert tuple(y.shape) == (2, 16, 17, 8)
    _eq(y, want, "stride-2 conv")
    assert not bool(y[..., 4:].any()), "widened columns must be exact zeros"


def v1_cout3_widened(dev, launch):
    """bf16; a conv_out-like Cout 3 widened to 8 on a small map (128 x 32 tile), 16-bit output, zero padding columns."""
    ops = _ops()
    g = _g(103)
    x = _act(g, (1, 20, 24, 64)).to(dev, ops.act_dtype())
    pw = ops.pack_conv_weight(_wt(g, 3, 64, nnz=40), _small(g, (3,)), device=dev, cout_multiple=8)
    want = dp.rounded(dp.conv_ref(x, pw, bias=pw.bias), ops.act_dtype())
    y = launch(1, lambda: ops.conv2d(x, pw, pad=1))
    _eq(y, want, "Cout 3 conv")
    assert not bool(y[..., 3:].any())


def v1_bmm_grid_z(dev, launch):
    """fp16; batched bmm_nt on grid.z (3 images, ragged M = 100, 64 x 64 tile), alpha 2^-2, fp32 output."""
    ops = _ops()
    g = _g(104)
    a = _act(g, (3, 100, 64)).to(dev, ops.act_dtype())
    b = torch.stack([_wt(g, 128, 64, 1, 1, nnz=20)[:, :, 0, 0] for _ in range(3)]).to(dev, ops.act_dtype())
    want = torch.stack([dp.rounded(dp.gemm_ref(a[i], b[i], alpha=0.25), torch.float32) for i in range(3)])
    y = launch(1, lambda: ops.bmm_nt(a, b, alpha=0.25, out_dtype=ops.OUT_F32))
    _eq(y, want, "bmm_nt")


def v1_linear_rows_gate(dev, launch):
    """bf16; linear_rows over a row range of two images (grid.z), bias, gate and residual."""
    ops = _ops()
    g = _g(105)
    xb = _act(g, (2, 90, 128)).to(dev, ops.act_dtype())
    pw = ops.pack_linear_weight(_wt(g, 128, 128, 1, 1, nnz=16)[:, :, 0, 0], _small(g, (128,)), device=dev)
    gate = _gate(g, 128).to(dev)
    r = _small(g, (2, 50, 128)).to(dev, ops.act_dtype())
    want = dp.rounded(dp.conv_ref(xb[:, 17:67].reshape(1, 1, 100, 128), pw, pad=(0, 0, 0, 0), bias=pw.bias, gate=gate,
                                  residual=r.reshape(100, 128)), ops.act_dtype()).reshape(2, 50, 128)
    y = launch(1, lambda: ops.linear_rows(xb, 17, 50, pw, gate=gate, residual=r))
    _eq(y, want, "linear_rows")


def v1_linear_t_into_slice(dev, launch):
    """bf16; transposed output into a column slice of a V^T buffer: the slice is exact, nothing outside it moves."""
    ops = _ops()
    g = _g(106)
    x = _act(g, (70, 64)).to(dev, ops.act_dtype())
    pw = ops.pack_linear_weight(_wt(g, 128, 64, 1, 1, nnz=16)[:, :, 0, 0], _small(g, (128,)), device=dev)
    out = _small(g, (128, 200)).to(dev, ops.act_dtype())
    before = out.clone()
    want = dp.rounded(dp.conv_ref(x.reshape(1, 1, 70, 64), pw, pad=(0, 0, 0, 0), bias=pw.bias), ops.act_dtype()).reshape(70, 128)
    launch(1, lambda: ops.linear_t_into(x, pw, out, 40))
    _eq(out[:, 40:110], want.T, "linear_t_into slice")
    _eq(out[:, :40], before[:, :40], "left of the slice")
    _eq(out[:, 110:], before[:, 110:], "right of the slice")


# ---- variant 2: igemm_dma_kernel -----------------------------------------------------------------------------------------------------

def v2_linear_into_slice(dev, launch):
    """bf16; small-M GEMM (200 rows: not a multiple of 32) on the LDS-DMA kernel, written into a slice of a wider buffer."""
    ops = _ops()
    g = _g(201)
    x = _act(g, (200, 320), pix=(-3, 3)).to(dev, ops.act_dtype())
    pw = ops.pack_linear_weight(_wt(g, 128, 320, 1, 1, nnz=24)[:, :, 0, 0], _small(g, (128,)), device=dev)
    out = _small(g, (300, 512)).to(dev, ops.act_dtype())
    before = out.clone()
    want = dp.rounded(dp.conv_ref(x.reshape(1, 1, 200, 320), pw, pad=(0, 0, 0, 0), bias=pw.bias), ops.act_dtype()).reshape(200, 128)
    launch(2, lambda: ops.linear_into(x, pw, out, 37, 136))
    _eq(out[37:237, 136:264], want, "linear_into slice")
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[37:237, 136:264] = False
    _eq(out[mask], before[mask], "outside the slice")


def v2_stride2_conv(dev, launch):
    """fp16; a stride-2 conv with odd H / W and the asymmetric pad, large enough (193 tiles of 256 x 128) for the LDS-DMA kernel; residual."""
    ops = _ops()
    g = _g(202)
    x = _act(g, (1, 445, 445, 32)).to(dev, ops.act_dtype())
    pw = ops.pack_conv_weight(_wt(g, 128, 32, nnz=16), _small(g, (128,)), device=dev)
    r = _small(g, (1, 222, 222, 128)).to(dev, ops.act_dtype())
    want = dp.rounded(dp.conv_ref(x, pw, stride=2, pad=(0, 1, 0, 1), bias=pw.bias, residual=r), ops.act_dtype())
    y = launch(2, lambda: ops.conv2d(x, pw, stride=2, pad=(0, 1, 0, 1), residual=r))
    _eq(y, want, "stride-2 conv")


def v2_split_wsplit_out_split(dev, launch):
    """Accurate tier; two-term split operand x weight with its own low half ([w_hi | w_hi | w_lo], the third segment wrapping to a_hi),
    written as the two-term split output: hi == round(ref), lo == round(ref - hi)."""
    ops = _ops()
    g = _g(203)
    x = _act(g, (256, 256), pix=(-3, 3), chan=(0, 0), split=True)
    pw = ops.pack_linear_weight(_wt(g, 256, 256, 1, 1, nnz=4, chan=(0, 0), split=True)[:, :, 0, 0], _small(g, (256,)), device=dev,
                                split=2, w_split=2)
    assert pw.w_split == 2 and pw.cin == 3 * 256
    xo = dp.host_operand(x, "split").to(dev)
    ref = dp.conv_ref(xo.reshape(1, 1, 256, 512), pw, pad=(0, 0, 0, 0), bias=pw.bias).reshape(256, 256)
    hi, lo = dp.split_rounded(ref, torch.float16)
    y = launch(2, lambda: ops.linear(xo, pw, out_dtype=ops.OUT_BF16, out_split=2))
    _eq(y[:, :256], hi, "split output hi")
    _eq(y[:, 256:], lo, "split output lo")
    assert bool(lo.any())


# ---- variant 4: LDS-DMA split-K + splitk_reduce_kernel ----------------------------------------------------------------------------------

def v4_splitk_bias_gate_residual(dev, launch):
    """bf16; small M, long K: the contraction in K ranges, the reduce pass applies bias, gate and residual."""
    ops = _ops()
    g = _g(401)
    x = _act(g, (300, 2048), pix=(-3, 3)).to(dev, ops.act_dtype())
    pw = ops.pack_linear_weight(_wt(g, 256, 2048, 1, 1, nnz=32)[:, :, 0, 0], _small(g, (256,)), device=dev)
    gate = _gate(g, 256).to(dev)
    r = _small(g, (300, 256)).to(dev, ops.act_dtype())
    want = dp.rounded(dp.conv_ref(x.reshape(1, 1, 300, 2048), pw, pad=(0, 0, 0, 0), bias=pw.bias, gate=gate, residual=r), ops.act_dtype())
    y = launch(4, lambda: ops.linear(x, pw, gate=gate, residual=r))
    _eq(y, want.reshape(300, 256), "split-K")


def v4_splitk_split_operand_out_split(dev, launch):
    """Accurate tier; split operand, split-K, the reduce pass writing the two-term split output."""
    ops = _ops()
    g = _g(402)
    x = _act(g, (100, 1024), pix=(-3, 3), chan=(0, 0), split=True)
    pw = ops.pack_linear_weight(_wt(g, 256, 1024, 1, 1, nnz=6, chan=(0, 0))[:, :, 0, 0], _small(g, (256,)), device=dev, split=2)
    xo = dp.host_operand(x, "split").to(dev)
    ref = dp.conv_ref(xo.reshape(1, 1, 100, 2048), pw, pad=(0, 0, 0, 0), bias=pw.bias).reshape(100, 256)
    hi, lo = dp.split_rounded(ref, torch.float16)
    y = launch(4, lambda: ops.linear(xo, pw, out_dtype=ops.OUT_BF16, out_split=2))
    _eq(y[:, :256], hi, "split-K split output hi")
    _eq(y[:, 256:], lo, "split-K split output lo")


# ---- variant 5: igemm_p8_kernel ---------------------------------------------------------------------------------------------------------

def v5_p8_ragged_m(dev, launch):
    """bf16; 129 x 1 tiles of 256 x 256 with a ragged last tile (M = 32801), K = 640 (ten 64-wide K-tiles), bias, fp32 output."""
    ops = _ops()
    g = _g(501)
    x = _act(g, (32801, 640), pix=(-3, 3)).to(dev, ops.act_dtype())
    pw = ops.pack_linear_weight(_wt(g, 256, 640, 1, 1, nnz=16)[:, :, 0, 0], _small(g, (256,)), device=dev)
    want = dp.rounded(dp.conv_ref(x.reshape(1, 1, 32801, 640), pw, pad=(0, 0, 0, 0), bias=pw.bias), torch.float32).reshape(32801, 256)
    y = launch(5, lambda: ops.linear(x, pw, out_dtype=ops.OUT_F32))
    _eq(y, want, "p8")


def v5_p8_mx_operand(dev, launch):
    """Accurate tier; the mixed-precision (MX fp8) operand (320 channels = 640 16-bit slots) through the gmx route's ping-pong kernel;
    fp32 residual."""
    ops = _ops()
    g = _g(502)
    x = _act(g, (32801, 320), pix=(-3, 3), chan=(0, 0), split=True)
    pw = ops.pack_linear_weight(_wt(g, 256, 320, 1, 1, nnz=4, chan=(0, 0), split=True)[:, :, 0, 0], _small(g, (256,)), device=dev, split=3)
    xo = dp.host_operand(x, "mx").to(dev)
    r = _small(g, (32801, 256)).to(dev)
    want = dp.rounded(dp.conv_ref(xo.reshape(1, 1, 32801, 640), pw, pad=(0, 0, 0, 0), bias=pw.bias, residual=r), torch.float32)
    y = launch(5, lambda: ops.linear(xo, pw, residual=r))
    _eq(y, want.reshape(32801, 256), "p8 MX")


# ---- variant 9: igemm_gmx --------------------------------------------------------------------------------------------------------------

def v9_gmx_mx_operand(dev, launch):
    """Accurate tier; GEMM over an MX fp8 operand (300 rows), bias + fp32 residual; the operand is the cast kernel's bytes."""
    ops = _ops()
    g = _g(901)
    x = _act(g, (300, 256), pix=(-3, 3), chan=(0, 0), split=True)
    pw = ops.pack_linear_weight(_wt(g, 256, 256, 1, 1, nnz=4, chan=(0, 0), split=True)[:, :, 0, 0], _small(g, (256,)), device=dev, split=3)
    xo = dp.host_operand(x, "mx").to(dev)
    if not isinstance(launch, _DryLaunch):
        _eq(ops.to_operand(x.to(dev), 3), xo, "cast kernel's MX bytes")
    r = _small(g, (300, 256)).to(dev)
    want = dp.rounded(dp.conv_ref(xo.reshape(1, 1, 300, 512), pw, pad=(0, 0, 0, 0), bias=pw.bias, residual=r), torch.float32)
    y = launch(9, lambda: ops.linear(xo, pw, residual=r))
    _eq(y, want.reshape(300, 256), "gmx")


# ---- variant 3: igemm_halo_kernel --------------------------------------------------------------------------------------------------------

def v3_halo_bf16(dev, launch):
    """bf16; 192 halo tiles (spatial form), bias + residual."""
    ops = _ops()
    g = _g(301)
    x = _act(g, (4, 64, 96, 64)).to(dev, ops.act_dtype())
    pw = ops.pack_conv_weight(_wt(g, 256, 64, nnz=16), _small(g, (256,)), device=dev)
    r = _small(g, (4, 64, 96, 256)).to(dev, ops.act_dtype())
    want = dp.rounded(dp.conv_ref(x, pw, bias=pw.bias, residual=r), ops.act_dtype())
    y = launch(3, lambda: ops.conv2d(x, pw, pad=1, residual=r))
    _eq(y, want, "halo")


def v3_halo_flat_narrow_map(dev, launch):
    """fp16; 20 x 20 maps (narrower than one 32-pixel halo tile): the FLAT form; residual."""
    ops = _ops()
    g = _g(302)
    x = _act(g, (100, 20, 20, 64)).to(dev, ops.act_dtype())
    pw = ops.pack_conv_weight(_wt(g, 128, 64, nnz=16), _small(g, (128,)), device=dev)
    r = _small(g, (100, 20, 20, 128)).to(dev, ops.act_dtype())
    want = dp.rounded(dp.conv_ref(x, pw, bias=pw.bias, residual=r), ops.act_dtype())
    y = launch(3, lambda: ops.conv2d(x, pw, pad=1, residual=r))
    _eq(y, want, "halo FLAT")


def v3_halo_split(dev, launch):
    """Accurate tier; split operand x split weight (three K segments, the third wrapping), fp32 output."""
    ops = _ops()
    g = _g(303)
    x = _act(g, (4, 64, 96, 64), pix=(0, 1), chan=(0, 0), split=True)
    pw = ops.pack_conv_weight(_wt(g, 256, 64, nnz=4, chan=(0, 0), split=True), _small(g, (256,)), device=dev, split=2, w_split=2)
    assert pw.w_split == 2
    xo = dp.host_operand(x, "split").to(dev)
    want = dp.rounded(dp.conv_ref(xo, pw, bias=pw.bias), torch.float32)
    y = launch(3, lambda: ops.conv2d(xo, pw, pad=1))
    _eq(y, want, "halo split")


def v3_halo_mx(dev, launch):
    """Accurate tier; MX fp8 operand (128 tiles: no split-K), fp32 residual."""
    ops = _ops()
    g = _g(304)
    x = _act(g, (4, 64, 64, 128), pix=(0, 1), chan=(0, 0), split=True)
    pw = ops.pack_conv_weight(_wt(g, 256, 128, nnz=4, chan=(0, 0), split=True), _small(g, (256,)), device=dev, split=3)
    xo = dp.host_operand(x, "mx").to(dev)
    r = _small(g, (4, 64, 64, 256)).to(dev)
    want = dp.rounded(dp.conv_ref(xo, pw, bias=pw.bias, residual=r), torch.float32)
    y = launch(3, lambda: ops.conv2d(xo, pw, pad=1, residual=r))
    _eq(y, want, "halo MX")


# ---- variant 6: halo, phase-decomposed upsampling ---------------------------------------------------------------------------------------

def v6_phase_bf16(dev, launch):
    """bf16; nearest-2x upsampling conv as four 2 x 2 convs of phase-summed kernels (exact in bf16 here: the phase form then equals the
    nine-tap gather form too); bias."""
    ops = _ops()
    g = _g(601)
    x = _act(g, (2, 64, 96, 128)).to(dev, ops.act_dtype())
    pw = ops.pack_conv_weight(_wt(g, 128, 128, nnz=16), _small(g, (128,)), device=dev, upsample_phases=True)
    ref = dp.phase_conv_ref(x, pw, bias=pw.bias)
    assert torch.equal(ref, dp.conv_ref(x, pw, upsample=True, bias=pw.bias))
    want = dp.rounded(ref, ops.act_dtype())
    y = launch(6, lambda: ops.conv2d(x, pw, pad=1, upsample=True))
    _eq(y, want, "phase")


def v6_phase_split(dev, launch):
    """Accurate tier; phase form over a split operand and a split weight (the phase sums re-split: restated from w_ph's bytes)."""
    ops = _ops()
    g = _g(602)
    x = _act(g, (2, 64, 96, 64), pix=(0, 1), chan=(0, 0), split=True)
    pw = ops.pack_conv_weight(_wt(g, 128, 64, nnz=2, chan=(0, 0), split=True), _small(g, (128,)), device=dev, split=2, w_split=2,
                              upsample_phases=True)
    xo = dp.host_operand(x, "split").to(dev)
    want = dp.rounded(dp.phase_conv_ref(xo, pw, bias=pw.bias), torch.float32)
    y = launch(6, lambda: ops.conv2d(xo, pw, pad=1, upsample=True))
    _eq(y, want, "phase split")


def v6_phase_mx(dev, launch):
    """Accurate tier; phase form over an MX fp8 operand (fp16 + block-scaled fp8 chunks of the phase-summed kernels)."""
    ops = _ops()
    g = _g(603)
    x = _act(g, (2, 43, 86, 256), pix=(0, 1), chan=(0, 0), split=True)
    pw = ops.pack_conv_weight(_wt(g, 256, 256, nnz=4, chan=(0, 0), split=True), _small(g, (256,)), device=dev, split=3, upsample_phases=True)
    xo = dp.host_operand(x, "mx").to(dev)
    want = dp.rounded(dp.phase_conv_ref(xo, pw, bias=pw.bias), torch.float32)
    y = launch(6, lambda: ops.conv2d(xo, pw, pad=1, upsample=True))
    _eq(y, want, "phase MX")


# ---- variants 7 / 8: igemm_halo_multi_kernel ---------------------------------------------------------------------------------------------

def _multi(dev, launch, variant, groups, C, Cout, form, ups, seed, residual=False, nnz=None):
    ops = _ops()
    g = _g(seed)
    split = form in ("mx", "mx6")
    pw = ops.pack_conv_weight(_wt(g, Cout, C, nnz=nnz or (4 if split else 16), chan=(0, 0) if split else (0, 1), block=32, split=split),
                              _small(g, (Cout,)), device=dev, split={"16": 1, "mx": 3, "mx6": 4}[form], upsample_phases=ups)
    xs, rs, wants = [], [], []
    for n, h, w in groups:
        x = _act(g, (n, h, w, C), pix=(0, 1) if split else (-2, 2), chan=(0, 0) if split else (0, 1), block=32, split=split)
        xo = dp.host_operand(x, form, ops.act_dtype()).to(dev)
        hv, wv = (2 * h, 2 * w) if ups else (h, w)
        r = _small(g, (n, hv, wv, Cout)).to(dev, ops.stream_dtype()) if residual else None
        ref = dp.phase_conv_ref(xo, pw, bias=pw.bias) if ups else dp.conv_ref(xo, pw, bias=pw.bias, residual=r)
        xs.append(xo), rs.append(r), wants.append(dp.rounded(ref, ops.stream_dtype()))
    ys = launch(variant, lambda: ops.conv2d_multi(xs, pw, pad=1, upsample=ups, residuals=rs if residual else None))
    for y, want, shape in zip(ys, wants, groups):
        _eq(y, want, f"launch group member {shape}")


def v7_multi_bf16(dev, launch):
    """bf16; four tile-shape groups of one layer in one launch (unequal maps), residual."""
    _multi(dev, launch, 7, [(36, 40, 40), (12, 40, 32), (12, 32, 40), (4, 32, 32)], 128, 128, "16", False, 701, residual=True)


def v7_multi_mx(dev, launch):
    """Accurate tier; MX fp8 operands, four unequal groups in one launch (no split-K inside a launch group)."""
    _multi(dev, launch, 7, [(3, 40, 40), (1, 40, 32), (1, 32, 40), (1, 32, 32)], 128, 128, "mx", False, 702)


def v8_multi_phase_bf16(dev, launch):
    """bf16; the phase form of an upsampling conv over three unequal groups in one launch (low-res widths 32 / 48: no group falls back to
    the gather form)."""
    _multi(dev, launch, 8, [(4, 32, 48), (4, 48, 32), (4, 32, 32)], 256, 256, "16", True, 801)


def v8_multi_phase_mx(dev, launch):
    """Accurate tier; the phase form over MX fp8 operands, two unequal groups in one launch."""
    _multi(dev, launch, 8, [(2, 32, 40), (1, 32, 32)], 128, 128, "mx", True, 802)


# ---- variants 10 / 11: the GroupNorm-fused halo producer --------------------------------------------------------------------------------------

def gn_fused_case(dev, groups, nimg, seed, Cin=32, Cout=128, G=32):
    """Operands of a conv whose patch producer normalises: stream tensors x_k [n_k, h_k, w_k, Cin] = +-{1..3}, a dyadic (scale, shift) table
    [nimg, Cin, 2] (scale 2^(image % 2), shift 40 or 44 by channel parity; row n uses image n % nimg) and a weight of one +-2^e tap per output
    whose sign alternates with the output channel. SiLU is the one activation the producer has (omgsr_igemm refuses any other gn_act); every
    normalised value x scale + shift lies in 34 .. 50, where silu_f is the identity in fp32: exp(-v) < 2^-46, so 1.0f + exp(-v) is 1.0f, its
    v_rcp_f32 is 1.0f and v * 1.0f is v. The values are integers below 2^6: exact in the compute type the producer rounds to. The shift is
    nonzero, so a border tap that picked up `shift` instead of the zero padding of the NORMALISED map would change the result.
    Returns (xs, pw, make_spec, exact outputs float64 before the output rounding, G); make_spec() is a fresh GnSpec carrying the table."""
    ops = _ops()
    g = _g(seed)
    ce = dp.group_exponents(g, G, Cout)
    pw = ops.pack_conv_weight(dp.stats_wt(g, ce, Cin, 3, 3, 1, (1, 1), alt_sign=True), dp.stats_bias(g, ce), device=dev)
    table = torch.empty(nimg, Cin, 2)
    table[..., 0] = torch.exp2((torch.arange(nimg) % 2).float())[:, None]
    table[..., 1] = (40.0 + 4.0 * (torch.arange(Cin) % 2).float())[None, :]
    xs, exacts = [], []
    for n, h, w in groups:
        x = dp.stats_act(g, (n, h, w, Cin), img_e=(0, 0))
        t = table[torch.arange(n) % nimg][:, None, None]                     # [n, 1, 1, Cin, 2]
        a = x * t[..., 0] + t[..., 1]
        assert float(a.min()) >= 32.0 and torch.equal(a.to(ops.act_dtype()).float(), a)
        exacts.append(dp.conv_ref(a.to(dev, ops.act_dtype()), pw, bias=pw.bias))
        xs.append(x.to(dev, ops.stream_dtype()))
    table = table.to(dev)

    def make_spec():
        stat = torch.zeros(nimg, G, device=dev)
        spec = ops.GnSpec(stat, stat + 1.0, None, None, G, ops.ACT_SILU)
        spec._table = table
        return spec
    return xs, pw, make_spec, exacts, G


def v10_gn_fused_identity_silu(dev, launch):
    """bf16; GroupNorm apply as the halo kernel's patch producer: four rows sharing two images' (scale, shift), 96 x 160 maps, 32 -> 128 (240
    tiles), on data where its SiLU is the identity (gn_fused_case): x * scale + shift, the rounding to the compute type and the zero padding of the
    normalised map are exact."""
    ops = _ops()
    xs, pw, spec, exacts, _ = gn_fused_case(dev, [(4, 96, 160)], 2, 1001)
    y = launch(10, lambda: ops.conv2d(xs[0], pw, pad=1, gn=spec()))
    _eq(y, dp.rounded(exacts[0], ops.stream_dtype()), "GroupNorm-fused conv")


def v11_gn_fused_multi_identity_silu(dev, launch):
    """bf16; the same producer in a launch group: two tile shapes (120 + 96 tiles), rows of both sharing two images' table."""
    ops = _ops()
    xs, pw, spec, exacts, _ = gn_fused_case(dev, [(2, 96, 160), (2, 96, 128)], 2, 1101)
    ys = launch(11, lambda: ops.conv2d_multi(xs, pw, pad=1, gn=spec()))
    for y, want in zip(ys, exacts):
        _eq(y, dp.rounded(want, ops.stream_dtype()), "GroupNorm-fused launch group member")


# ---- variant 12: halo split-K (MX fp8) -------------------------------------------------------------------------------------------------

def v12_halo_splitk_mx(dev, launch):
    """Accurate tier; 36 halo tiles: the contraction in chunk ranges on both sides of the fp16 / fp8 boundary (6 + 6 chunks), ragged
    Cout 136, fp32 residual through the reduce pass."""
    ops = _ops()
    g = _g(1201)
    x = _act(g, (3, 24, 64, 192), pix=(0, 1), chan=(0, 0), split=True)
    pw = ops.pack_conv_weight(_wt(g, 136, 192, nnz=4, chan=(0, 0), split=True), _small(g, (136,)), device=dev, split=3, cout_multiple=8)
    xo = dp.host_operand(x, "mx").to(dev)
    r = _small(g, (3, 24, 64, 136)).to(dev)
    want = dp.rounded(dp.conv_ref(xo, pw, bias=pw.bias, residual=r), torch.float32)
    y = launch(12, lambda: ops.conv2d(xo, pw, pad=1, residual=r))
    _eq(y, want, "halo split-K MX")


# ---- variants 13 - 17: fp6 (MX6) correction chunks ---------------------------------------------------------------------------------------

def _mx6_single(dev, launch, variant, shape, Cout, seed, ups=False, residual=False, nnz=4):
    ops = _ops()
    g = _g(seed)
    N, H, W, C = shape
    x = _act(g, shape, pix=(0, 1), chan=(0, 1), block=32, split=True)
    pw = ops.pack_conv_weight(_wt(g, Cout, C, nnz=nnz, chan=(0, 1), block=32, split=True), _small(g, (Cout,)), device=dev, split=4,
                              upsample_phases=ups)
    assert pw.mx_fmt == 6
    xo = dp.host_operand(x, "mx6").to(dev)
    if not isinstance(launch, _DryLaunch):
        _eq(ops.to_operand(x.to(dev), 4).view(torch.int16), xo.view(torch.int16), "cast kernel's MX6 bytes")
    r = _small(g, (N, H, W, Cout)).to(dev) if residual else None
    ref = dp.phase_conv_ref(xo, pw, bias=pw.bias) if ups else dp.conv_ref(xo, pw, bias=pw.bias, residual=r)
    want = dp.rounded(ref, torch.float32)
    y = launch(variant, lambda: ops.conv2d(xo, pw, pad=1, upsample=ups, residual=r))
    _eq(y, want, f"MX6 variant {variant}")


def v13_mx6_single(dev, launch):
    """Accurate tier; fp6 correction chunks with per-32-channel-block exponents, 128 halo tiles, fp32 residual."""
    _mx6_single(dev, launch, 13, (4, 64, 64, 128), 256, 1301, residual=True)


def v14_mx6_multi(dev, launch):
    """Accurate tier; fp6 chunks, four unequal groups in one launch."""
    _multi(dev, launch, 14, [(3, 40, 40), (1, 40, 32), (1, 32, 40), (1, 32, 32)], 128, 128, "mx6", False, 1401)


def v15_mx6_splitk(dev, launch):
    """Accurate tier; fp6 chunks on a 2-tile problem: halo split-K (one-chunk halves), fp32 residual."""
    _mx6_single(dev, launch, 15, (1, 8, 64, 64), 128, 1501, residual=True)


def v16_mx6_phase(dev, launch):
    """Accurate tier; fp6 chunks of the phase-summed kernels."""
    _mx6_single(dev, launch, 16, (1, 32, 48, 128), 128, 1601, ups=True, nnz=2)


def v17_mx6_phase_multi(dev, launch):
    """Accurate tier; fp6 phase form, two unequal groups in one launch."""
    _multi(dev, launch, 17, [(2, 32, 40), (1, 32, 32)], 128, 128, "mx6", True, 1701, nnz=2)


# ---- variant 18: mxfp8_gemm_kernel ------------------------------------------------------------------------------------------------------

def _mxfp8_pair(g, M, N, K, density, spread=40):
    """Codes m 2^j (|m| <= 7, j in {0, 1}) at `density`; E8M0 scales 127 + r[row] + c[block] + d for the operand and 127 + t[col] - c[block] + d'
    for the weight (c in [-spread, spread], d, d' in {0, 1}): every output's sum stays in budget while neighbouring K blocks differ by up to
    2^(2 spread). Row 0 carries a saturated +448 code, row 2 a -448 one, row 1 an all-zero block. Returns the planes and the exponents
    r [M, 1], t [1, N] an epilogue term of output (m, n) is scaled by."""
    nb = K // 32
    c = torch.randint(-spread, spread + 1, (nb,), generator=g)

    def plane(rows, sign, lo, hi):
        v = dp.dyadic(g, torch.randint(0, 2, (rows, K), generator=g).float()) * (torch.rand(rows, K, generator=g) < density)
        e = torch.randint(lo, hi + 1, (rows, 1), generator=g)
        s = 127 + e + sign * c[None, :] + torch.randint(0, 2, (rows, nb), generator=g)
        return v.to(torch.float8_e4m3fn).view(torch.uint8), s.to(torch.uint8), e

    ac, asc, r = plane(M, 1, -3, 3)
    wc, wsc, t = plane(N, -1, -12, 12)
    ac[0, 5] = torch.tensor([448.0]).to(torch.float8_e4m3fn).view(torch.uint8)
    ac[min(2, M - 1), 40] = torch.tensor([-448.0]).to(torch.float8_e4m3fn).view(torch.uint8)
    ac[1, :32] = 0
    return ac, asc, wc, wsc, r.float(), t.float().T


def _scaled(g, e):
    """Epilogue terms +-{1..3} 2^(e + 0..4) for the MXFP8 probes."""
    return dp.dyadic(g, e + torch.randint(0, 5, tuple(e.shape), generator=g).float(), (1, 3))


def _mxfp8_weight(dev, wc, wsc, bias):
    ops = _ops()
    N, K = wc.shape
    Np = (N + 255) // 256 * 256
    codes = torch.zeros(Np, K, dtype=torch.uint8)
    scales = torch.zeros(Np, K // 32, dtype=torch.uint8)
    codes[:N], scales[:N] = wc, wsc
    return ops.PackedWeight(codes.to(dev), bias.to(dev), N, K, 1, 1, w_scale=scales.to(dev))


def v18_mxfp8_block_scales(dev, launch):
    """MXFP8; scales spread over 2^+-40 per row, column and K block (96 blocks), a saturated code, an all-zero block; bias, fp32 output."""
    ops = _ops()
    g = _g(1801)
    M, N, K = 300, 256, 3072
    ac, asc, wc, wsc, _, t = _mxfp8_pair(g, M, N, K, 1 / 8)
    pw = _mxfp8_weight(dev, wc, wsc, _scaled(g, t[0]))
    xq = ops.Mxfp8(ac.to(dev), asc.to(dev))
    want = dp.rounded(dp.mxfp8_ref(xq.codes, xq.scales, pw.w, pw.w_scale, N, bias=pw.bias), torch.float32)
    y = launch(18, lambda: ops.linear(xq, pw, out_dtype=ops.OUT_F32))
    _eq(y, want, "MXFP8 block scales")


def v18_mxfp8_single_ktile(dev, launch):
    """MXFP8; K = 128 (one K tile), ragged M = 37 and N = 200 (Cout_pad 256), bias + gate + bf16 residual, bf16 output."""
    ops = _ops()
    g = _g(1802)
    M, N, K = 37, 200, 128
    ac, asc, wc, wsc, r_e, t = _mxfp8_pair(g, M, N, K, 1.0)
    pw = _mxfp8_weight(dev, wc, wsc, _scaled(g, t[0]))
    xq = ops.Mxfp8(ac.to(dev), asc.to(dev))
    gate = _gate(g, N).to(dev)
    r = _scaled(g, r_e + t).to(dev, torch.bfloat16)
    want = dp.rounded(dp.mxfp8_ref(xq.codes, xq.scales, pw.w, pw.w_scale, N, bias=pw.bias, gate=gate, residual=r), torch.bfloat16)
    y = launch(18, lambda: ops.linear(xq, pw, gate=gate, residual=r))
    _eq(y, want, "MXFP8 K = 128")


def v18_mxfp8_linear_into_grid_z(dev, launch):
    """MXFP8; two images on grid.z written into row / column slices of [2, 100, 512]; nothing outside the slices moves."""
    ops = _ops()
    g = _g(1803)
    B, M, N, K = 2, 80, 256, 256
    ac, asc, wc, wsc, _, t = _mxfp8_pair(g, B * M, N, K, 1 / 2, spread=20)
    pw = _mxfp8_weight(dev, wc, wsc, _scaled(g, t[0]))
    xq = ops.Mxfp8(ac.reshape(B, M, K).to(dev), asc.reshape(B, M, K // 32).to(dev))
    out = _small(g, (B, 100, 512)).to(dev, torch.bfloat16)
    before = out.clone()
    want = dp.rounded(dp.mxfp8_ref(xq.codes, xq.scales, pw.w, pw.w_scale, N, bias=pw.bias), torch.bfloat16).reshape(B, M, N)
    launch(18, lambda: ops.linear_into(xq, pw, out, 5, 64))
    _eq(out[:, 5:85, 64:320], want, "MXFP8 linear_into slice")
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[:, 5:85, 64:320] = False
    _eq(out[mask], before[mask], "outside the slices")


# name -> (tier, probe). The name's "v<id>_" prefix is the variant the probe asserts (test_dyadic_probes_cpu.py checks every id the
# dispatcher can record has one).
PROBES = {
    "v1_conv_in_128x128": ("bf16", v1_conv_in_128x128),
    "v1_stride2_asym_pad_cout4": ("fp16", v1_stride2_asym_pad_cout4),
    "v1_cout3_widened": ("bf16", v1_cout3_widened),
    "v1_bmm_grid_z": ("fp16", v1_bmm_grid_z),
    "v1_linear_rows_gate": ("bf16", v1_linear_rows_gate),
    "v1_linear_t_into_slice": ("bf16", v1_linear_t_into_slice),
    "v2_linear_into_slice": ("bf16", v2_linear_into_slice),
    "v2_stride2_conv": ("fp16", v2_stride2_conv),
    "v2_split_wsplit_out_split": ("fp32", v2_split_wsplit_out_split),
    "v3_halo_bf16": ("bf16", v3_halo_bf16),
    "v3_halo_flat_narrow_map": ("fp16", v3_halo_flat_narrow_map),
    "v3_halo_split": ("fp32", v3_halo_split),
    "v3_halo_mx": ("fp32", v3_halo_mx),
    "v4_splitk_bias_gate_residual": ("bf16", v4_splitk_bias_gate_residual),
    "v4_splitk_split_operand_out_split": ("fp32", v4_splitk_split_operand_out_split),
    "v5_p8_ragged_m": ("bf16", v5_p8_ragged_m),
    "v5_p8_mx_operand": ("fp32", v5_p8_mx_operand),
    "v6_phase_bf16": ("bf16", v6_phase_bf16),
    "v6_phase_split": ("fp32", v6_phase_split),
    "v6_phase_mx": ("fp32", v6_phase_mx),
    "v7_multi_bf16": ("bf16", v7_multi_bf16),
    "v7_multi_mx": ("fp32", v7_multi_mx),
    "v8_multi_phase_bf16": ("bf16", v8_multi_phase_bf16),
    "v8_multi_phase_mx": ("fp32", v8_multi_phase_mx),
    "v9_gmx_mx_operand": ("fp32", v9_gmx_mx_operand),
    "v10_gn_fused_identity_silu": ("bf16", v10_gn_fused_identity_silu),
    "v11_gn_fused_multi_identity_silu": ("bf16", v11_gn_fused_multi_identity_silu),
    "v12_halo_splitk_mx": ("fp32", v12_halo_splitk_mx),
    "v13_mx6_single": ("fp32", v13_mx6_single),
    "v14_mx6_multi": ("fp32", v14_mx6_multi),
    "v15_mx6_splitk": ("fp32", v15_mx6_splitk),
    "v16_mx6_phase": ("fp32", v16_mx6_phase),
    "v17_mx6_phase_multi": ("fp32", v17_mx6_phase_multi),
    "v18_mxfp8_block_scales": ("bf16", v18_mxfp8_block_scales),
    "v18_mxfp8_single_ktile": ("bf16", v18_mxfp8_single_ktile),
    "v18_mxfp8_linear_into_grid_z": ("bf16", v18_mxfp8_linear_into_grid_z),
}


class _DryLaunch:
    """Host-only run of a probe up to its launch (test_dyadic_probes_cpu.py: every probe's data stay inside the bit budget)."""

    def __call__(self, variant, fn):
        raise _DryRun()


def dry_run(name: str) -> None:
    """Build probe `name` on the host with the tier's packing rules and check its reference and budget; stops before the launch."""
    from omgsr_amd import ops
    tier, fn = PROBES[name]
    dt = _TIER[tier]
    saved = ops._ACT, ops._PRECISE
    ops._ACT, ops._PRECISE = (torch.bfloat16 if dt == torch.bfloat16 else torch.float16), dt == torch.float32
    try:
        fn("cpu", _DryLaunch())
    except _DryRun:
        pass
    finally:
        ops._ACT, ops._PRECISE = saved


@pytest.fixture
def tier():
    from omgsr_amd import ops
    yield lambda t: ops.set_compute_dtype(_TIER[t])
    ops.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("name", list(PROBES))
def test_dyadic_probe(name, tier):
    t, fn = PROBES[name]
    tier(t)
    with torch.no_grad():
        fn(DEV, _launch)
