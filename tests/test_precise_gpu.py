"""The accurate tier (`--weight_dtype fp32`: fp32 stream tensors, fp16 MFMA operands, two-term split operands on the layers
the precision policy names) against fp32 references: kernel by kernel with a plain PyTorch fp32 op on the same inputs, then
module by module against the fp32 CPU oracle (reduced configs; the full SD2.1 / FLUX shapes are in
tests/test_fullsize_parity_gpu.py). Tolerances are the north-star's: rel-L2 <= 1e-3 for a whole model, and what one fp16
operand rounding (2^-11) or none (split operands: 2^-22) allows for a single kernel."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def test_to_operand_split_reconstructs_fp32():
    from omgsr_amd import ops
    x = torch.randn(37, 3, 64, generator=_g(1)) * torch.logspace(-3, 3, 64)
    y1 = ops.to_operand(x.to(DEV), 1)
    y2 = ops.to_operand(x.to(DEV), 2)
    assert y1.dtype == torch.float16 and tuple(y1.shape) == (37, 3, 64) and tuple(y2.shape) == (37, 3, 128)
    assert torch.equal(y1.cpu(), x.to(torch.float16))
    hi, lo = y2[..., :64].float().cpu(), y2[..., 64:].float().cpu()
    assert torch.equal(hi, x.to(torch.float16).float())
    assert torch.equal(lo, (x - hi).to(torch.float16).float())
    assert _rel(hi + lo, x) < 2.0 ** -20


@pytest.mark.parametrize("C,G,HW,act", [(128, 32, 4096, 1), (320, 32, 1024, 1), (512, 32, 300, 0)])
@pytest.mark.parametrize("split", [1, 2])
def test_group_norm_fp32_stream_to_operand(C, G, HW, act, split):
    from omgsr_amd import ops
    x = torch.randn(2, HW, 1, C, generator=_g(2)) * 3 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=_g(3)), 0.1 * torch.randn(C, generator=_g(4))
    y = ops.group_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), G, 1e-6, act, split=split)
    ref = F.group_norm(x.permute(0, 3, 1, 2).double(), G, gamma.double(), beta.double(), 1e-6).permute(0, 2, 3, 1)
    if act:
        ref = F.silu(ref)
    got = y.float()
    got = got[..., :C] + got[..., C:] if split == 2 else got
    assert y.dtype == torch.float16 and y.shape[-1] == split * C
    assert _rel(got, ref) < (3e-6 if split == 2 else 4e-4)


@pytest.mark.parametrize("C", [320, 1280, 3072])
@pytest.mark.parametrize("split", [1, 2])
def test_layer_norm_fp32_stream_to_operand(C, split):
    from omgsr_amd import ops
    x = torch.randn(3, 50, C, generator=_g(5)) * 2 - 0.3
    a, b = 1 + 0.1 * torch.randn(C, generator=_g(6)), 0.1 * torch.randn(C, generator=_g(7))
    y = ops.layer_norm(x.to(DEV), a.to(DEV), b.to(DEV), 1e-5, split=split).float()
    got = y[..., :C] + y[..., C:] if split == 2 else y
    ref = F.layer_norm(x.double(), (C,), a.double(), b.double(), 1e-5)
    assert _rel(got, ref) < (3e-6 if split == 2 else 4e-4)


@pytest.mark.parametrize("N,H,W,Cin,Cout,k", [(2, 64, 64, 128, 128, 3), (1, 32, 48, 320, 640, 3), (2, 16, 16, 1280, 1280, 3),
                                             (2, 40, 40, 256, 128, 1), (1, 64, 64, 8, 320, 3), (3, 24, 24, 512, 8, 3)])
@pytest.mark.parametrize("split", [1, 2])
def test_conv_fp32_stream_split_operand_residual(N, H, W, Cin, Cout, k, split):
    """Stream tensor in (cast / split inside conv2d), fp32 residual, fp32 stream out, fused GroupNorm statistics; weights are
    fp16-representable so a split operand leaves only the fp32 accumulation: ~1e-6 against an fp64 conv."""
    from omgsr_amd import ops
    x = torch.randn(N, H, W, Cin, generator=_g(8))
    w = (torch.randn(Cout, Cin, k, k, generator=_g(9)) * (k * k * Cin) ** -0.5).to(torch.float16).float()
    b = 0.1 * torch.randn(Cout, generator=_g(10))
    res = torch.randn(N, H, W, Cout, generator=_g(11))
    pw = ops.pack_conv_weight(w, b, device=DEV, split=split)
    y = ops.conv2d(x.to(DEV), pw, pad=k // 2, residual=res.to(DEV), gn_groups=8)
    assert y.dtype == torch.float32
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=k // 2).permute(0, 2, 3, 1) + res.double()
    assert _rel(y, ref) < (3e-6 if split == 2 else 3e-4)
    # the statistics the epilogue left agree with the stored tensor
    mean, rstd, var = ops.group_norm_stats(y, 8, 1e-6)
    r = y.double().cpu().reshape(N, H * W, 8, Cout // 8)
    assert torch.allclose(mean.double().cpu(), r.mean(dim=(1, 3)), atol=1e-5, rtol=1e-5)
    assert torch.allclose(var.double().cpu(), r.var(dim=(1, 3), unbiased=False), atol=1e-5, rtol=1e-4)


# (N, H, W, Cin, Cout, k): halo-tile conv, register-staged small conv, LDS-DMA GEMM (1x1, many rows), Cin % 32 != 0 (the
# wrap point falls inside a 32-channel step: register-staged kernel only), split-K (few rows, long K), strided conv
_WSPLIT_CASES = [(2, 64, 64, 128, 128, 3), (1, 64, 96, 320, 320, 3), (2, 16, 16, 1280, 640, 3), (4, 128, 128, 256, 128, 1),
                 (1, 64, 64, 8, 320, 3), (1, 24, 24, 48, 96, 3), (3, 24, 24, 512, 8, 3), (1, 8, 8, 1280, 1280, 3)]


@pytest.mark.parametrize("N,H,W,Cin,Cout,k", _WSPLIT_CASES)
@pytest.mark.parametrize("split,w_split", [(1, 2), (2, 2)])
def test_conv_weight_split(N, H, W, Cin, Cout, k, split, w_split):
    """Full-mantissa fp32 weights (what a checkpoint looks like after an fp32 LoRA merge): w_split 2 packs [w_hi | w_lo] (or
    [w_hi | w_hi | w_lo] against a split operand) and the contraction wraps over the operand row (omgsr_igemm_args.in_ld).
    With an operand that is exact (fp16-representable input, or the two-term split) only the fp32 accumulation is left: ~1e-6
    against an fp64 conv; the same weights rounded once to fp16 sit at ~2e-4."""
    from omgsr_amd import ops
    x = torch.randn(N, H, W, Cin, generator=_g(8))
    if split == 1:
        x = x.to(torch.float16).float()                     # no activation rounding left: isolates the weight side
    w = torch.randn(Cout, Cin, k, k, generator=_g(9)) * (k * k * Cin) ** -0.5
    b = 0.1 * torch.randn(Cout, generator=_g(10))
    res = torch.randn(N, H, W, Cout, generator=_g(11))
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=k // 2).permute(0, 2, 3, 1) + res.double()
    pw = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=split, w_split=w_split)
    assert pw.row_channels == split * Cin and pw.cin == (split + 1) * Cin
    y = ops.conv2d(x.to(DEV), pw, pad=k // 2, residual=res.to(DEV))
    assert _rel(y[..., :Cout], ref) < 3e-6
    pw1 = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=split, w_split=1)
    y1 = ops.conv2d(x.to(DEV), pw1, pad=k // 2, residual=res.to(DEV))
    assert 2e-5 < _rel(y1[..., :Cout], ref) < 4e-4          # one fp16 rounding of every weight


@pytest.mark.parametrize("split,w_split", [(1, 2), (2, 2)])
def test_conv_weight_split_upsample_stride(split, w_split):
    from omgsr_amd import ops
    x = torch.randn(2, 48, 48, 256, generator=_g(21))
    if split == 1:
        x = x.to(torch.float16).float()
    w = torch.randn(256, 256, 3, 3, generator=_g(22)) * (9 * 256) ** -0.5
    pw = ops.pack_conv_weight(w, None, device=DEV, split=split, w_split=w_split)
    up = ops.conv2d(x.to(DEV), pw, pad=1, upsample=True)
    ref = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2.0, mode="nearest"), w.double(), padding=1).permute(0, 2, 3, 1)
    assert _rel(up, ref) < 3e-6
    dn = ops.conv2d(x.to(DEV), pw, stride=2, pad=(0, 1, 0, 1))
    ref = F.conv2d(F.pad(x.permute(0, 3, 1, 2).double(), (0, 1, 0, 1)), w.double(), stride=2).permute(0, 2, 3, 1)
    assert _rel(dn, ref) < 3e-6


@pytest.mark.parametrize("split,w_split", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_upsample_conv_phase_form_accurate_tier(split, w_split):
    """The phase-decomposed upsampling conv with split operands / split (phase-summed) weights and fp32 output."""
    from omgsr_amd import ops
    x = torch.randn(2, 43, 86, 256, generator=_g(31))
    if split == 1:
        x = x.to(torch.float16).float()
    w = torch.randn(256, 256, 3, 3, generator=_g(32)) * (9 * 256) ** -0.5
    b = 0.1 * torch.randn(256, generator=_g(33))
    pw = ops.pack_conv_weight(w, b, device=DEV, split=split, w_split=w_split, upsample_phases=True)
    assert pw.w_ph is not None
    y = ops.conv2d(x.to(DEV), pw, pad=1, upsample=True)
    assert y.dtype == torch.float32
    ref = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    assert _rel(y, ref) < (3e-6 if w_split == 2 else 4e-4)


def _fp8(u8):
    return u8.contiguous().view(torch.float8_e4m3fn).float()


@pytest.mark.parametrize("C,G,HW", [(128, 32, 4096), (320, 32, 1024), (512, 32, 300)])
def test_group_norm_mx_operand(C, G, HW):
    """The mixed-precision operand form (OMGSR_EL_MX): [a_hi fp16 | a_lo' fp8 | a_hi' fp8] per pixel, a_lo' = (a - a_hi) 2^11."""
    from omgsr_amd import ops
    x = torch.randn(2, HW, 1, C, generator=_g(2)) * 3 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=_g(3)), 0.1 * torch.randn(C, generator=_g(4))
    y = ops.group_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), G, 1e-6, ops.ACT_SILU, split=3)
    y2 = ops.group_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), G, 1e-6, ops.ACT_SILU, split=2)
    assert y.dtype == torch.float16 and y.shape[-1] == 2 * C
    ref = F.silu(F.group_norm(x.permute(0, 3, 1, 2).double(), G, gamma.double(), beta.double(), 1e-6)).permute(0, 2, 3, 1)
    yb = y.cpu().view(torch.uint8).reshape(2, HW, 1, 4 * C)
    hi = yb[..., :2 * C].contiguous().view(torch.float16).float()
    lo, hi8 = _fp8(yb[..., 2 * C:3 * C]) * 2.0 ** -11, _fp8(yb[..., 3 * C:])
    assert torch.equal(hi, y2[..., :C].float().cpu())                       # the fp16 half is the two-term split's hi
    assert _rel(hi + lo, ref) < 2e-5                                         # lo' carries the residual to ~2^-4 of itself
    assert _rel(hi8, ref) < 5e-2 and torch.isfinite(hi8).all()               # the fp8 copy of a_hi (3 mantissa bits)


# N, H, W, C, Cout: halo-tile kernel with fp16 + block-scaled fp8 chunks; small and ragged maps included (MX problems always take it)
_MX_CASES = [(2, 64, 64, 128, 128), (1, 64, 96, 320, 320), (2, 16, 16, 1280, 640), (1, 40, 43, 512, 512), (1, 32, 32, 960, 640), (1, 9, 33, 64, 128), (4, 38, 38, 256, 256), (4, 75, 75, 256, 512)]


@pytest.mark.parametrize("N,H,W,C,Cout", _MX_CASES)
def test_conv_mx(N, H, W, C, Cout):
    """a w = a_hi w_hi (fp16 MFMAs) + a_lo w_hi + a_hi w_lo (block-scaled fp8 MFMAs, v_mfma_scale_f32_32x32x64_f8f6f4) with full-mantissa
    inputs and weights: the correction terms are carried to ~2^-4 of their own size, i.e. 2^-16 of the product - against one fp16
    rounding of each side at ~3e-4 and the three-segment fp16 form at ~1e-6."""
    from omgsr_amd import ops
    x = torch.randn(N, H, W, C, generator=_g(8))
    w = torch.randn(Cout, C, 3, 3, generator=_g(9)) * (9 * C) ** -0.5
    b = 0.1 * torch.randn(Cout, generator=_g(10))
    res = torch.randn(N, H, W, Cout, generator=_g(11))
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1) + res.double()
    pw = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=3)
    assert pw.mx is not None and pw.row_channels == 2 * C
    y = ops.conv2d(x.to(DEV), pw, pad=1, residual=res.to(DEV), gn_groups=32)
    e = _rel(y, ref)
    pw1 = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8)
    e1 = _rel(ops.conv2d(x.to(DEV), pw1, pad=1, residual=res.to(DEV)), ref)
    print(f"conv MX {N, H, W, C, Cout}: rel {e:.2e} (single fp16 rounding of both sides {e1:.2e})")
    assert e < 2e-5 and e1 > 10 * e
    mean, rstd, var = ops.group_norm_stats(y, 32, 1e-6)           # statistics left by the halo epilogue
    r = y.double().cpu().reshape(N, H * W, 32, Cout // 32)
    assert torch.allclose(mean.double().cpu(), r.mean(dim=(1, 3)), atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("N,H,W,C,Cout,act,res,osplit", [(1, 64, 64, 512, 512, 0, True, 1), (1, 32, 32, 640, 640, 1, False, 1), (1, 64, 64, 320, 320, 0, True, 2),
                                                        (1, 64, 64, 960, 320, 0, False, 1), (1, 8, 64, 64, 128, 1, True, 1), (3, 24, 64, 192, 136, 0, True, 1),
                                                        (1, 32, 32, 640, 640, 0, True, 3)])
def test_conv_mx_split_k_small_m(N, H, W, C, Cout, act, res, osplit):
    """Round 5: the reference's operating point is ONE image per call - its 3x3 convs are 16 ... 64 workgroup tiles on 512 slots. The halo-tile
    kernel then runs the contraction as up to 8 chunk ranges (one launch group: igemm_halo_multi_kernel, fp32 partial tiles) and
    splitk_reduce_kernel applies bias / activation / residual / output form once: same values as the one-pass epilogue up to fp32 summation
    order. Ragged chunk counts (C = 192: 6 + 6 chunks over 4 ranges), one-chunk halves (C = 64) and the two-term split output included."""
    import ctypes as C_
    from omgsr_amd import _lib, ops
    x = torch.randn(N, H, W, C, generator=_g(41))
    w = torch.randn(Cout, C, 3, 3, generator=_g(42)) * (9 * C) ** -0.5
    b = 0.1 * torch.randn(Cout, generator=_g(43))
    r = torch.randn(N, H, W, Cout, generator=_g(44)) if res else None
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    if act:
        ref = F.silu(ref)
    if r is not None:
        ref = ref + r.double()
    pw = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=3)
    xd = ops.to_operand(x.to(DEV), 3)
    a = _lib.IgemmArgs()
    ops._conv_args(a, xd, pw, 1, 1, False, ops.ACT_SILU if act else ops.ACT_NONE, None, None, ops.OUT_STREAM, 1.0, None, 1, 0)
    assert _lib.load().omgsr_igemm_workspace_bytes(C_.byref(a)) > 0, "this shape was meant to take the split-K form"
    if osplit == 2:
        y = ops.conv2d(xd, pw, pad=1, act=ops.ACT_SILU if act else ops.ACT_NONE, residual=None if r is None else r.to(DEV), out_dtype=ops.OUT_BF16, out_split=2)
        Cp = y.shape[-1] // 2
        y = y[..., :Cp].double() + y[..., Cp:].double()
        assert _rel(y[..., :Cout], ref) < 2e-5
        return
    if osplit == 3:            # the reduce pass writes the mixed-precision operand of the next GEMM (a ResnetBlock feeding an upsampler / proj_out)
        y = ops.conv2d(xd, pw, pad=1, residual=None if r is None else r.to(DEV), out_dtype=ops.OUT_BF16, out_split=3)
        hi, lo, hi8 = _mx_decode(y, Cout)
        assert _rel(hi.double() + lo.double(), ref) < 2e-4 and _rel(hi8, ref) < 5e-2      # hi + lo' 2^-11: ~2^-15; the fp8 copy: 3 mantissa bits
        return
    y = ops.conv2d(xd, pw, pad=1, act=ops.ACT_SILU if act else ops.ACT_NONE, residual=None if r is None else r.to(DEV), gn_groups=8)
    assert y.dtype == torch.float32 and _rel(y[..., :Cout], ref) < 2e-5
    mean, _, _ = ops.group_norm_stats(y, 8, 1e-6)                  # no fused statistics from a split-K launch: the stand-alone pass runs
    assert torch.allclose(mean.double().cpu(), y.double().cpu().reshape(N, H * W, 8, -1).mean(dim=(1, 3)), atol=1e-5, rtol=1e-5)
    again = ops.conv2d(xd, pw, pad=1, act=ops.ACT_SILU if act else ops.ACT_NONE, residual=None if r is None else r.to(DEV))
    assert torch.equal(again, y)                                   # fixed summation order: bit-repeatable


@pytest.mark.parametrize("M,K,Nn", [(256, 5120, 1280), (64, 11520, 1280), (1024, 2560, 640)])
def test_linear_split_k_writes_the_mx_operand(M, K, Nn):
    """Round 5: a small-M / long-K GEMM whose result is the mixed-precision operand of the next GEMM (the UNet's feed-forward output in front of
    proj_out at the 16 x 16 level, one image per call) takes the LDS-DMA kernel's split-K; its reduce pass writes [hi fp16 | lo' fp8 | hi' fp8]."""
    import ctypes as C_
    from omgsr_amd import _lib, ops
    x = torch.randn(1, M, K, generator=_g(51)).to(torch.float16).float()
    w = (torch.randn(Nn, K, generator=_g(52)) * K ** -0.5).to(torch.float16).float()
    b = 0.1 * torch.randn(Nn, generator=_g(53))
    r = torch.randn(1, M, Nn, generator=_g(54))
    ref = torch.addmm(b.double(), x[0].double(), w.double().t())[None] + r.double()
    pw = ops.pack_linear_weight(w, b, device=DEV)
    y = ops.linear(ops.to_operand(x.to(DEV)), pw, residual=r.to(DEV), out_dtype=ops.OUT_BF16, out_split=3)
    hi, lo, hi8 = _mx_decode(y, Nn)
    assert _rel(hi.double() + lo.double(), ref) < 2e-4 and _rel(hi8, ref) < 5e-2
    y32 = ops.linear(ops.to_operand(x.to(DEV)), pw, residual=r.to(DEV))
    assert _rel(y32, ref) < 3e-6


def test_conv_mx_upsample_phase_form_and_epilogue_output():
    """The producer / consumer pair of a decoder upsampler in the mixed-precision form: a GEMM epilogue writes the OMGSR_EL_MX operand
    (out_split 3) and the phase-decomposed upsampling conv consumes it (fp16 + block-scaled fp8 chunks of the phase-summed kernels)."""
    from omgsr_amd import ops
    C = 256
    x = torch.randn(2, 43, 86, C, generator=_g(31))
    w = torch.randn(C, C, 3, 3, generator=_g(32)) * (9 * C) ** -0.5
    b = 0.1 * torch.randn(C, generator=_g(33))
    ref = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    pw = ops.pack_conv_weight(w, b, device=DEV, split=3, upsample_phases=True)
    assert pw.w_ph is not None and pw.mx is not None
    y = ops.conv2d(x.to(DEV), pw, pad=1, upsample=True, gn_groups=32)
    assert _rel(y, ref) < 2e-5
    # an epilogue-written MX operand (identity GEMM of an fp16-representable x: the epilogue sees exactly x) equals the cast kernel's,
    # byte for byte, on every GEMM-shaped kernel that can produce it (few rows: register staged; many rows: LDS-DMA)
    eye = ops.pack_linear_weight(torch.eye(C), None, device=DEV)
    for rows in (2 * 43 * 86, 40 * 43 * 86):
        xr = (torch.randn(rows, C, generator=_g(34)) * 3).to(torch.float16).float().to(DEV)
        via_epilogue = ops.linear(xr.reshape(1, rows, C), eye, out_dtype=ops.OUT_BF16, out_split=3).reshape(rows, 2 * C)
        assert torch.equal(via_epilogue, ops.to_operand(xr, 3))
    xm = ops.linear(x.to(torch.float16).float().to(DEV).reshape(1, -1, C), eye, out_dtype=ops.OUT_BF16, out_split=3).reshape(2, 43, 86, 2 * C)
    y2 = ops.conv2d(xm, pw, pad=1, upsample=True)
    ref2 = F.conv2d(F.interpolate(x.to(torch.float16).permute(0, 3, 1, 2).double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    assert _rel(y2, ref2) < 2e-5


def test_conv_mx_multi_launch_and_saturation():
    """Several MX problems of one layer in one launch; operands far outside fp8's range degrade gracefully (the fp8 parts clamp at
    +-448: the correction is partly lost for those elements, nothing becomes NaN)."""
    from omgsr_amd import ops
    C, Cout = 128, 128
    w = torch.randn(Cout, C, 3, 3, generator=_g(9)) * (9 * C) ** -0.5
    pw = ops.pack_conv_weight(w, None, device=DEV, split=3)
    ops.overflow_seen(); ops.mx_saturation_seen()                 # clear both bits of the guard word
    # the tile-shape groups of a tiled-VAE level (FLAT plan for the whole group: 22-piece patch), a spatial group (one map too wide for the
    # FLAT form), and a group of maps 46-80 wide (FLAT plan, 27-piece patch): the three group kernels of the format
    for shapes in ([(3, 40, 40), (1, 40, 32), (1, 32, 40), (1, 32, 32)], [(2, 96, 96), (1, 96, 64), (1, 64, 96)], [(2, 48, 48), (1, 48, 40)]):
        xs = [torch.randn(n, h, wd, C, generator=_g(20 + i)) for i, (n, h, wd) in enumerate(shapes)]
        ys = ops.conv2d_multi([x.to(DEV) for x in xs], pw, pad=1)
        for x, y in zip(xs, ys):
            ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1)
            assert _rel(y, ref) < 2e-5
    torch.cuda.synchronize()
    assert not ops.mx_saturation_seen()
    big = torch.randn(3, 40, 40, C, generator=_g(20)) * 3000.0                                         # |a| up to ~1e4: a_hi' clamps at 448, a_lo' 2^11 clamps too
    y = ops.conv2d(big.to(DEV), pw, pad=1)
    ref = F.conv2d(big.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1)
    assert torch.isfinite(y).all() and _rel(y, ref) < 1e-3
    # the saturation of the fp8 correction fields is no longer silent - the MX producers raise the diagnostic bit of the guard
    # word (here: the fp32 -> MX cast in front of the conv), and it is NOT an fp16 overflow (no fallback is triggered)
    torch.cuda.synchronize()
    assert ops.mx_saturation_seen() and not ops.overflow_seen() and not ops.mx_saturation_seen()


@pytest.mark.parametrize("M,K,Nn", [(4608, 3072, 3072), (9216, 1536, 512), (300, 320, 1280), (147456, 320, 320)])
@pytest.mark.parametrize("split,w_split", [(1, 2), (2, 2)])
def test_linear_weight_split(M, K, Nn, split, w_split):
    """The GEMM-shaped kernels (ping-pong 256 x 256 for K >= 1536, LDS-DMA 256 x 128, register staged) with a wrapped contraction."""
    from omgsr_amd import ops
    x = torch.randn(1, M, K, generator=_g(23))
    if split == 1:
        x = x.to(torch.float16).float()
    w = torch.randn(Nn, K, generator=_g(24)) * K ** -0.5
    b = 0.1 * torch.randn(Nn, generator=_g(25))
    pw = ops.pack_linear_weight(w, b, device=DEV, split=split, w_split=w_split)
    y = ops.linear(x.to(DEV), pw)
    ref = torch.addmm(b.to(DEV).double(), x[0].to(DEV).double(), w.to(DEV).double().t())[None]
    assert _rel(y, ref) < 3e-6


def _mx_decode(y, C):
    """[..., 2C] fp16 view of an OMGSR_EL_MX tensor -> (hi fp32, lo fp32 = lo' 2^-11, hi' fp32) each [..., C]."""
    raw = y.contiguous().view(torch.uint8).reshape(*y.shape[:-1], 4 * C)
    hi = raw[..., :2 * C].contiguous().view(torch.float16).float()
    lo = raw[..., 2 * C:3 * C].contiguous().view(torch.float8_e4m3fn).float() * 2.0 ** -11
    hi8 = raw[..., 3 * C:].contiguous().view(torch.float8_e4m3fn).float()
    return hi, lo, hi8


@pytest.mark.parametrize("M,C,Nn", [(300, 320, 320), (147456, 320, 320), (36864, 640, 1280), (9216, 1280, 1280), (4100, 64, 192), (20000, 1280, 320),
                                    (147456, 320, 2560), (33000, 320, 1280), (40000, 448, 512)])
def test_linear_mx(M, C, Nn):
    """a Linear in the mixed-precision form - a_hi w_hi in fp16 MFMAs, a_lo w_hi + a_hi w_lo as block-scaled fp8 MFMAs,
    one fp32 accumulator - from a full-mantissa fp32 operand and weight: ~1e-5 of the fp64 product where one fp16 rounding of each side
    leaves ~3e-4; fp32 output with fp32 residual, ragged M. Narrow problems run on igemm_gmx_kernel (every K-step count mod 3: C / 32 = 10,
    20, 40, 2), wide ones (N >= 256-friendly, >= 128 tiles) on the ping-pong kernel's MX instantiation: an even number of fp16 K-tiles
    (C = 640, 1280), an odd one = the mixed fp16 / fp8 pair with the scale switch inside a K-tile (C = 320), and C = 448 (7 + 7 K-tiles,
    the a_lo' / a_hi' boundary in the middle of a K-tile pair)."""
    from omgsr_amd import ops
    x = torch.randn(1, M, C, generator=_g(60))
    w = torch.randn(Nn, C, generator=_g(61)) * C ** -0.5
    b = 0.1 * torch.randn(Nn, generator=_g(62))
    res = torch.randn(1, M, Nn, generator=_g(63))
    pw = ops.pack_linear_weight(w, b, device=DEV, split=3)
    assert pw.mx is not None and pw.row_channels == 2 * C and pw.w_cm is None
    xd = x.to(DEV)
    y = ops.linear(xd, pw, residual=res.to(DEV))
    ref = (torch.addmm(b.to(DEV).double(), xd[0].double(), w.to(DEV).double().t()) + res[0].to(DEV).double())[None]
    e = _rel(y, ref)
    e1 = _rel(ops.linear(xd, ops.pack_linear_weight(w, b, device=DEV), residual=res.to(DEV)), ref)
    print(f"linear MX {M, C, Nn}: rel {e:.2e} (single fp16 rounding of both sides {e1:.2e})")
    assert y.dtype == torch.float32 and e < 2e-5 and e1 > 8 * e
    # the operand the producers write (here: the cast kernel) and a 16-bit output
    xm = ops.to_operand(xd, 3)
    y16 = ops.linear(xm, pw, out_dtype=ops.OUT_BF16)
    assert y16.dtype == torch.float16 and _rel(y16, ref - res.to(DEV).double()) < 6e-4


def test_linear_mx_geglu_transposed_and_chained_outputs():
    """The producer / consumer chain of a transformer block's feed-forward and V projection in the mixed-precision form:
    LayerNorm writes the MX operand -> GEGLU projection (MX GEMM, epilogue a * gelu(gate)) writes the hidden tensor AS an MX operand
    -> output projection (MX GEMM) with the fp32 residual; and the V projection (LAYOUT_T output) over the same LayerNorm'd operand."""
    from omgsr_amd import ops
    B, L, C = 2, 1100, 320
    x = torch.randn(B, L, C, generator=_g(70)) * 2 + 0.3
    g, bb = 1.0 + 0.1 * torch.randn(C, generator=_g(71)), 0.05 * torch.randn(C, generator=_g(72))
    w1 = torch.randn(2 * 4 * C, C, generator=_g(73)) * C ** -0.5
    b1 = 0.1 * torch.randn(2 * 4 * C, generator=_g(74))
    w2 = torch.randn(C, 4 * C, generator=_g(75)) * (4 * C) ** -0.5
    b2 = 0.1 * torch.randn(C, generator=_g(76))
    wv = torch.randn(C, C, generator=_g(77)) * C ** -0.5
    xd = x.to(DEV)
    xn = ops.layer_norm(xd, g.to(DEV), bb.to(DEV), 1e-5, split=3)
    assert xn.dtype == torch.float16 and tuple(xn.shape) == (B, L, 2 * C)
    ln = F.layer_norm(x.double(), (C,), g.double(), bb.double(), 1e-5)
    hi, lo, hi8 = _mx_decode(xn.cpu(), C)
    assert _rel(hi + lo, ln) < 2e-5 and _rel(hi, ln) > 1e-4          # hi + lo' 2^-11 carries the operand to ~2^-15; hi alone is one fp16 rounding
    assert torch.equal(hi8, hi.clamp(-448, 448).to(torch.float8_e4m3fn).float())
    h = ops.linear(xn, ops.pack_geglu_weight(w1, b1, device=DEV, split=3), out_dtype=ops.OUT_BF16, out_split=3)
    assert tuple(h.shape) == (B, L, 2 * 4 * C)
    a, gate = (ln @ w1.double().t() + b1.double()).chunk(2, dim=-1)
    href = a * F.gelu(gate)
    hh, hl, _ = _mx_decode(h.cpu(), 4 * C)
    assert _rel(hh + hl, href) < 4e-5
    y = ops.linear(h, ops.pack_linear_weight(w2, b2, device=DEV, split=3), residual=xd)
    ref = href @ w2.double().t() + b2.double() + x.double()
    e = _rel(y, ref)
    print(f"LayerNorm -> GEGLU (MX) -> FF out (MX) + residual: rel {e:.2e}")
    assert y.dtype == torch.float32 and e < 3e-5
    # the same chain at a size whose GEGLU projection takes the ping-pong kernel's MX instantiation (36864 rows x 2 x 2560 packed columns)
    xb = torch.randn(1, 36864, C, generator=_g(78)).to(DEV)
    xnb = ops.layer_norm(xb, g.to(DEV), bb.to(DEV), 1e-5, split=3)
    hb = ops.linear(xnb, ops.pack_geglu_weight(w1, b1, device=DEV, split=3), out_dtype=ops.OUT_BF16, out_split=3)
    lnb = F.layer_norm(xb.double(), (C,), g.to(DEV).double(), bb.to(DEV).double(), 1e-5)
    ab, gb = (lnb @ w1.to(DEV).double().t() + b1.to(DEV).double()).chunk(2, dim=-1)
    hhb, hlb, _ = _mx_decode(hb.cpu(), 4 * C)
    assert _rel(hhb + hlb, (ab * F.gelu(gb)).cpu()) < 4e-5
    vt = ops.linear_t(xn, ops.pack_linear_weight(wv, None, device=DEV, split=3), L)          # [B, C, L8] fp16
    vref = (ln @ wv.double().t()).transpose(1, 2)
    # one fp16 rounding of the exact product; against the ROUNDED exact product only the values that sit on a rounding boundary differ
    assert _rel(vt[..., :L], vref) < 6e-4 and _rel(vt[..., :L].float(), vref.to(torch.float16).float()) < 1.5e-4


def test_shortcut_conv_mx_from_groupnorm_second_output():
    """A ResnetBlock's 1x1 shortcut in the mixed-precision form (round 4): norm1's apply pass writes conv1's operand AND x itself as an
    OMGSR_EL_MX operand (also_cast 3) in one pass; the 1x1 conv consumes it on igemm_gmx_kernel. Through the module and op by op."""
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api.autoencoder_kl import ResnetBlock2D
    from omgsr_amd.precision import set_mx, set_operand_split, set_weight_split
    N, H, W, C, Co = 2, 40, 56, 256, 128
    x = torch.randn(N, H, W, C, generator=_g(90)) * 1.5 + 0.2
    xd = x.to(DEV)
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=_g(91)), 0.05 * torch.randn(C, generator=_g(92))
    for ysplit in (1, 2, 3):
        y, x3 = ops.group_norm(xd, gamma.to(DEV), beta.to(DEV), 32, 1e-6, ops.ACT_SILU, split=ysplit, also_cast=3)
        assert torch.equal(x3, ops.to_operand(xd, 3))                      # the twin is exactly the cast kernel's MX operand
        assert torch.equal(y, ops.group_norm(xd, gamma.to(DEV), beta.to(DEV), 32, 1e-6, ops.ACT_SILU, split=ysplit))
    w = torch.randn(Co, C, 1, 1, generator=_g(93)) * C ** -0.5
    b = 0.1 * torch.randn(Co, generator=_g(94))
    pw = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=3)
    got = ops.conv2d(x3, pw, pad=0)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double()).permute(0, 2, 3, 1)
    assert got.dtype == torch.float32 and _rel(got, ref) < 2e-5
    blk = ResnetBlock2D(C, Co, None, 32, 1e-6).to(DEV)
    from omgsr_amd.testing import seeded_init_
    seeded_init_(blk, 5, rounded=False)
    set_operand_split(blk, [r"."]); set_weight_split(blk, [r"."])
    two = blk.nhwc(xd)
    assert set_mx(blk, [r"conv[12]$", r"conv_shortcut$"]) == 3 and blk.conv_shortcut.op_split == 3
    mx = blk.nhwc(xd)
    assert _rel(mx, two.double()) < 2e-5                                     # the MX block against the three-fp16-segment block


def test_attention_writes_mx_operand():
    """omgsr_attention with o_mx: the output projection's operand leaves the attention epilogue in the mixed-precision form; hi is
    bit-identical to the plain output, hi + lo' 2^-11 equals the two-term split's hi + lo to fp8 accuracy of the low part."""
    from omgsr_amd import ops
    B, L, H, D = 2, 1024, 5, 64
    q = torch.randn(B, L, H * D, generator=_g(80)).to(torch.float16).to(DEV)
    k = torch.randn(B, L, H * D, generator=_g(81)).to(torch.float16).to(DEV)
    vt = torch.randn(B, H * D, L, generator=_g(82)).to(torch.float16).to(DEV)
    o1 = ops.attention(q, k, vt, H, D, D ** -0.5)
    o2 = ops.attention(q, k, vt, H, D, D ** -0.5, out_split=2)
    o3 = ops.attention(q, k, vt, H, D, D ** -0.5, out_split=3)
    assert tuple(o3.shape) == (B, L, 2 * H * D)
    hi, lo, hi8 = _mx_decode(o3.cpu(), H * D)
    assert torch.equal(hi, o1.float().cpu()) and torch.equal(hi, o2[..., :H * D].float().cpu())
    lo2 = o2[..., H * D:].float().cpu()
    assert (lo - lo2).abs().max() <= 2.0 ** -4 * lo2.abs().max() and _rel(lo, lo2) < 0.05
    assert torch.equal(hi8, hi.to(torch.float8_e4m3fn).float())


def test_linear_epilogue_writes_split_operand():
    """A GEMM whose output is the next GEMM's operand (FF hidden, attention output): out_split 2 writes [hi | lo]."""
    from omgsr_amd import ops
    x = torch.randn(2, 300, 320, generator=_g(12))
    w = (torch.randn(1280, 320, generator=_g(13)) * 320 ** -0.5).to(torch.float16).float()
    pw = ops.pack_linear_weight(w, None, device=DEV, split=2)
    y = ops.linear(x.to(DEV), pw, out_dtype=ops.OUT_BF16, out_split=2)
    assert y.dtype == torch.float16 and tuple(y.shape) == (2, 300, 2560)
    got = y[..., :1280].float() + y[..., 1280:].float()
    ref = x.double() @ w.double().t()
    assert _rel(got, ref) < 3e-6
    assert torch.equal(y[..., 1280:].float().cpu(), (got.cpu() - y[..., :1280].float().cpu()).to(torch.float16).float())


def test_attention_split_output():
    from omgsr_amd import ops
    B, L, Hh, D = 2, 200, 5, 64
    q = (torch.randn(B, L, Hh * D, generator=_g(14))).to(torch.float16)
    k = (torch.randn(B, L, Hh * D, generator=_g(15))).to(torch.float16)
    v = (torch.randn(B, L, Hh * D, generator=_g(16))).to(torch.float16)
    vt = torch.zeros(B, Hh * D, 200, dtype=torch.float16)
    vt[:, :, :L] = v.transpose(1, 2)
    o1 = ops.attention(q.to(DEV), k.to(DEV), vt.to(DEV), Hh, D, D ** -0.5, Lk=L)
    o2 = ops.attention(q.to(DEV), k.to(DEV), vt.to(DEV), Hh, D, D ** -0.5, Lk=L, out_split=2)
    assert tuple(o2.shape) == (B, L, 2 * Hh * D)
    assert torch.equal(o1, o2[..., :Hh * D])
    qh, kh, vh = (t.double().reshape(B, L, Hh, D).transpose(1, 2) for t in (q, k, v))
    ref = (torch.softmax(qh @ kh.transpose(-1, -2) * D ** -0.5, -1) @ vh).transpose(1, 2).reshape(B, L, Hh * D)
    e1, e2 = _rel(o1.float(), ref), _rel(o2[..., :Hh * D].float() + o2[..., Hh * D:].float(), ref)
    assert e2 < e1 and e2 < 3e-4        # P is a 16-bit operand either way; the split removes the output rounding


@pytest.mark.parametrize("Lq,Lk,dt", [(1024, 1024, torch.bfloat16), (300, 77, torch.bfloat16), (1000, 1024, torch.float16), (128, 200, torch.bfloat16)],
                         ids=["self-bf16-dma", "cross-bf16-ragged", "self-fp16-dma", "ragged-keys-bf16"])
def test_attention_two_term_split_q_k_p(Lq, Lk, dt):
    """omgsr_attn_args.q_lo_off / k_lo_off / p_split (ABI v17): q, k and the probabilities as two-term splits inside the flash
    kernel - S^T = K_hi Q_hi^T + K_lo Q_hi^T + K_hi Q_lo^T, O^T += V^T (P_hi + P_lo)^T. Against the fp64 attention of the UNsplit q, k (V rounded
    once: it stays a single operand) the split form is limited by V and the fp32 accumulators only; the single form by the 8-bit (bf16) / 11-bit
    (fp16) mantissas of q, k and P. LDS-DMA path (Lk % 64 == 0) and the register-staged path (ragged Lk: cross-attention)."""
    from omgsr_amd import ops
    B, H, D = 2, 5, 64
    inner = H * D
    ops.set_compute_dtype(torch.float32, operand_dtype=dt)
    q = torch.randn(B, Lq, inner, generator=_g(90)) * 1.5
    k = torch.randn(B, Lk, inner, generator=_g(91)) * 1.5
    v = torch.randn(B, Lk, inner, generator=_g(92)).to(dt)
    L8 = -(-Lk // 8) * 8
    vt = torch.zeros(B, inner, L8, dtype=dt)
    vt[:, :, :Lk] = v.transpose(1, 2)
    sp = lambda t: torch.cat([t.to(dt), (t - t.to(dt).float()).to(dt)], -1)        # noqa: E731  [hi | lo]
    qq, kk = sp(q).to(DEV), sp(k).to(DEV)
    qh, kh, vh = (t.double().reshape(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    ref = (torch.softmax(qh @ kh.transpose(-1, -2) * D ** -0.5, -1) @ vh).transpose(1, 2).reshape(B, Lq, inner)
    both = lambda o: o[..., :inner].float() + o[..., inner:].float()                # noqa: E731
    single = ops.attention(qq[..., :inner].contiguous(), kk[..., :inner].contiguous(), vt.to(DEV), H, D, D ** -0.5, Lk=Lk, out_split=2)
    split = ops.attention(qq, kk, vt.to(DEV), H, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=inner, k_lo_col=inner)
    qk_only = ops.attention(qq, kk, vt.to(DEV), H, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=inner, k_lo_col=inner, p_split=False)
    e1, e2, e3 = _rel(both(single), ref), _rel(both(split), ref), _rel(both(qk_only), ref)
    # V as a two-term split too (omgsr_transpose_split from the fp32 values): against the fp64 attention of the UNROUNDED v
    v32 = torch.randn(B, Lk, inner, generator=_g(92))
    vts = ops.transpose_split(v32.to(DEV), L8)
    assert tuple(vts.shape) == (B, 2 * inner, L8)
    assert torch.equal(vts[:, :inner, :Lk].cpu(), v32.to(dt).transpose(1, 2)) and torch.equal(
        vts[:, inner:, :Lk].cpu(), (v32 - v32.to(dt).float()).to(dt).transpose(1, 2)) and bool((vts[..., Lk:] == 0).all())
    ref_v = (torch.softmax(qh @ kh.transpose(-1, -2) * D ** -0.5, -1) @ v32.double().reshape(B, -1, H, D).transpose(1, 2)).transpose(1, 2).reshape(B, Lq, inner)
    allsp = ops.attention(qq, kk, vts, H, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=inner, k_lo_col=inner)
    e4, e5 = _rel(both(allsp), ref_v), _rel(both(split), ref_v)
    print(f"attention {Lq} x {Lk} {dt}: single {e1:.2e}  q/k split {e3:.2e}  q/k/P split {e2:.2e}; vs unrounded V: q/k/P split {e5:.2e}, q/k/P/V split {e4:.2e}")
    bound = 3e-5 if dt == torch.bfloat16 else 3e-6
    assert e2 < bound and e2 < e3 < e1 and e1 > 20 * e2
    assert e4 < bound and e5 > 20 * e4
    assert torch.equal(ops.attention(qq, kk, vts, H, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=inner, k_lo_col=inner), allsp)
    assert torch.equal(ops.attention(qq, kk, vt.to(DEV), H, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=inner, k_lo_col=inner), split)
    # a fused [q | k] projection buffer: [q_hi | k_hi | q_lo | k_lo] (the UNet's self-attention in the range-fallback tier)
    if Lq == Lk:
        fused = torch.cat([qq[..., :inner], kk[..., :inner], qq[..., inner:], kk[..., inner:]], -1).contiguous()
        got = ops.attention(fused, fused, vt.to(DEV), H, D, D ** -0.5, q_col=0, k_col=inner, Lk=Lk, out_split=2, q_lo_col=2 * inner, k_lo_col=3 * inner)
        assert torch.equal(got, split)
    with pytest.raises(Exception):
        ops.attention(qq, kk, vt.to(DEV), H, D, D ** -0.5, Lk=Lk, q_lo_col=inner)            # one low half without the other


@pytest.mark.parametrize("L,valid,dt", [(4096, 4096, torch.bfloat16), (1152, 1089, torch.bfloat16), (16384, 16384, torch.float16), (128, 100, torch.bfloat16)])
def test_softmax_rows_split_and_vae_attention_pv_split(L, valid, dt):
    """omgsr_softmax_rows_split: p = [p_hi | p_lo] per row, hi bit-equal to the single form, hi + lo = the fp32 softmax to 2^-16; padded keys are
    exact zeros in both halves. Then the range-fallback tier's PV product p_hi v_hi + p_lo v_hi + p_hi v_lo through bmm_nt(both_split) with V^T
    from omgsr_transpose_split, against fp64."""
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.float32, operand_dtype=dt)
    rows, Cc = 256, 128
    s = (torch.randn(1, rows, L, generator=_g(95)) * 3).to(DEV)
    p1 = ops.softmax_rows(s, valid=valid)
    p2 = ops.softmax_rows(s, valid=valid, split=True)
    assert tuple(p2.shape) == (1, rows, 2 * L) and torch.equal(p2[..., :L], p1)
    ref = torch.softmax(s[..., :valid].double().cpu(), -1)
    got = p2[..., :L].double().cpu() + p2[..., L:].double().cpu()
    # (fp16 at 16384 keys: probabilities ~6e-5 sit at fp16's smallest normal, their low halves are subnormal - the tier that uses the split is bf16)
    assert bool((got[..., valid:] == 0).all()) and _rel(got[..., :valid], ref) < (2e-5 if (dt == torch.bfloat16 or L > 8192) else 2e-6)
    assert _rel(p1[..., :valid], ref) > 20 * _rel(got[..., :valid], ref)
    v = torch.randn(1, valid, Cc, generator=_g(96))
    vts = ops.transpose_split(v.to(DEV), L)
    vt3 = torch.cat([vts[:, :Cc], vts[:, :Cc], vts[:, Cc:]], -1)
    o = ops.bmm_nt(p2, vt3, out_split=2, both_split=True)
    o1 = ops.bmm_nt(p1, vts[:, :Cc].contiguous(), out_split=2)
    oref = ref @ v.double()
    e2, e1 = _rel(o[..., :Cc].float() + o[..., Cc:].float(), oref), _rel(o1[..., :Cc].float() + o1[..., Cc:].float(), oref)
    print(f"PV {L} keys {dt}: single {e1:.2e}  split {e2:.2e}")
    assert e2 < (3e-5 if (dt == torch.bfloat16 or L > 8192) else 3e-6) and e1 > 10 * e2


def test_stream_plumbing_fp32():
    from omgsr_amd import ops
    x = torch.randn(2, 5, 20, 24, generator=_g(17))
    n = ops.nchw_to_nhwc(x.to(DEV), 8)
    assert n.dtype == torch.float32 and tuple(n.shape) == (2, 20, 24, 8)
    assert torch.equal(n[..., :5].cpu(), x.permute(0, 2, 3, 1)) and bool((n[..., 5:] == 0).all())
    back = ops.nhwc_to_nchw(n, channels=5, clamp=(-1.0, 1.0))
    assert back.dtype == torch.float32 and torch.equal(back.cpu(), x.clamp(-1, 1))
    a, b = torch.randn(2, 6, 6, 16, generator=_g(18)), torch.randn(2, 6, 6, 8, generator=_g(19))
    assert torch.equal(ops.concat_channels(a.to(DEV), b.to(DEV)).cpu(), torch.cat([a, b], -1))
    c = ops.crop_nhwc(a.to(DEV), 1, 2, 3, 4)
    assert torch.equal(c.cpu(), a[:, 1:4, 2:6])
    dst = torch.zeros(2, 8, 8, 16, device=DEV)
    ops.paste_nhwc(a.to(DEV), dst, 1, 1, 2, 3, 4, 5)
    ref = torch.zeros(2, 8, 8, 16); ref[:, 2:6, 3:8] = a[:, 1:5, 1:6]
    assert torch.equal(dst.cpu(), ref)
    z = torch.randn(2, 8, 8, 16, generator=_g(20))
    tok = ops.flux_pack(z.to(DEV), 16)
    ref_tok = F.pixel_unshuffle(z.permute(0, 3, 1, 2), 2).flatten(2).transpose(1, 2)
    assert torch.equal(tok.cpu(), ref_tok) and torch.equal(ops.flux_unpack(tok, 8, 8).cpu(), z)
    mom, eps = torch.randn(2, 4, 4, 8, generator=_g(21)), torch.randn(2, 4, 4, 4, generator=_g(22))
    zz = ops.vae_sample(mom.to(DEV), eps.to(DEV), 4, 0.1, 0.5)
    ref_z = ((mom[..., :4] + torch.exp(0.5 * mom[..., 4:].clamp(-30, 20)) * eps) - 0.1) * 0.5
    assert zz.dtype == torch.float32 and torch.allclose(zz[..., :4].cpu(), ref_z, rtol=1e-5, atol=1e-6)
    out = ops.axpby(a.to(DEV), a.to(DEV) * 2, 1.0, -0.5, 0.25, 2.0)
    assert torch.allclose(out.cpu(), (a - a + 0.25) * 2.0, atol=1e-6)


SMALL_VAE = dict(block_out_channels=[32, 64, 128, 128], layers_per_block=1, norm_num_groups=32)
SMALL_UNET = dict(block_out_channels=[64, 128, 256, 256], attention_head_dim=[1, 2, 4, 4], cross_attention_dim=128, layers_per_block=2)


def _pair(product_cls, oracle_cls, cfg, seed):
    from omgsr_amd.testing import seeded_init_
    o = seeded_init_(oracle_cls(**cfg), seed).eval()
    p = product_cls(**cfg)
    p.load_state_dict(o.state_dict())
    return p.to(DEV, torch.float32).eval(), o


def _report(name, got, ref, tol=1e-3):
    from omgsr_amd.testing import psnr, rel_l2
    e = rel_l2(got, ref)
    print(f"{name}: rel-L2 {e:.3e}  PSNR {psnr(got, ref):.1f} dB")
    assert torch.isfinite(got.float()).all()
    assert e < tol, f"{name}: rel-L2 {e:.3e} >= {tol}"


@pytest.mark.parametrize("policy", ["none", "default", "all"])
def test_models_accurate_tier(policy):
    """Small VAE + UNet through the reference-shaped pipeline in the accurate tier. With no split operand what is left is one
    fp16 rounding per GEMM input (1.7e-3 on these narrow random-weight nets, which amplify more than the SD2.1 shapes:
    tests/test_fullsize_parity_gpu.py); the default policy brings it under the north-star 1e-3, splitting everything to 2e-4 (what is left: softmax probabilities and q, k, v are single fp16 operands)."""
    from omgsr_amd import precision
    from omgsr_amd.diffusers_api import AutoencoderKL, UNet2DConditionModel
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    from omgsr_amd.testing import rel_l2, synthetic_lq
    from oracle import diffusers_ref as R
    from oracle.pipeline_ref import OmgsrSRef
    pv, ov = _pair(AutoencoderKL, R.AutoencoderKL, SMALL_VAE, 11)
    pu, ou = _pair(UNet2DConditionModel, R.UNet2DConditionModel, SMALL_UNET, 12)
    g = _g(13)
    x = synthetic_lq(2, 24 * 8, 32 * 8)
    ehs = torch.randn(1, 77, 128, generator=g)
    eps = torch.randn(2, 4, 24, 32, generator=g)
    ov.posterior_noise = eps
    pv.posterior_noise = eps
    pipe = OMGSR_S_Infer(None, None, 273, DEV, torch.float32, vae=pv, unet=pu)
    pats = {"none": [], "all": [r"."]}.get(policy)
    if pats is not None:
        precision.set_operand_split(pipe.vae, pats)
        precision.set_operand_split(pipe.unet, pats)
    with torch.no_grad():
        ref = OmgsrSRef(ov, ou, R.DDPMScheduler().alphas_cumprod[273], 273)(x, ehs, 16, 8)
        got, _ = pipe(x.to(DEV), ehs.to(DEV), 16, 8)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    _report(f"OMGSR-S small, accurate tier, policy {policy}", got, ref, {"none": 3e-3, "default": 1e-3, "all": 4e-4}[policy])


def test_flux_accurate_tier():
    from omgsr_amd import precision
    from omgsr_amd.diffusers_api import FluxTransformer2DModel
    from oracle import diffusers_ref as R
    from oracle.pipeline_ref import prepare_latent_image_ids
    cfg = dict(num_layers=2, num_single_layers=3, num_attention_heads=2, attention_head_dim=128, joint_attention_dim=64,
               pooled_projection_dim=32, in_channels=64)
    p, o = _pair(FluxTransformer2DModel, R.FluxTransformer2DModel, cfg, 21)
    B, h, w, Lc = 2, 16, 24, 40
    g = _g(22)
    pe, pooled = torch.randn(1, Lc, 64, generator=g), torch.randn(1, 32, generator=g)
    tids, iids = torch.zeros(Lc, 3), prepare_latent_image_ids(h // 2, w // 2)
    x = torch.randn(B, (h // 2) * (w // 2), 64, generator=g)
    t, gd = torch.tensor([0.5051124691963196]), torch.full((B,), 1.0)
    with torch.no_grad():
        ref = o(hidden_states=x, timestep=t, guidance=gd, pooled_projections=pooled, encoder_hidden_states=pe, txt_ids=tids,
                img_ids=iids, return_dict=False)[0]
        for pats, tol in (([], 1e-3), ([r"."], 4e-4)):
            precision.set_operand_split(p, pats)
            got = p(hidden_states=x.to(DEV), timestep=t.to(DEV), guidance=gd.to(DEV), pooled_projections=pooled.to(DEV),
                    encoder_hidden_states=pe.to(DEV), txt_ids=tids.to(DEV), img_ids=iids.to(DEV), return_dict=False)[0]
            assert got.dtype == torch.float32
            _report(f"flux velocity, accurate tier, split {'all' if pats else 'none'}", got, ref, tol)


@pytest.mark.parametrize("fast", [False, True])
def test_tiled_vae_accurate_tier(fast):
    from omgsr_amd.diffusers_api import AutoencoderKL
    from omgsr_amd.pipelines.vaehook import VAEHook
    from oracle import diffusers_ref as R
    from oracle import vaehook_ref as V
    cfg = dict(block_out_channels=[32, 32, 64, 64], layers_per_block=2, norm_num_groups=32)
    p, o = _pair(AutoencoderKL, R.AutoencoderKL, cfg, 9)
    from omgsr_amd.precision import apply_default_policy
    apply_default_policy(vae=p)                  # what OMGSR_{S,F}_Infer(weight_dtype=float32) installs
    g = _g(41)
    img = torch.randn(2, 3, 160, 224, generator=g).clamp(-2, 2)
    z = torch.randn(2, 4, 28, 36, generator=g)
    with torch.no_grad():
        ref_e = V.tiled_forward(o.encoder, img, 64, is_decoder=False, fast=fast)
        ref_d = V.tiled_forward(o.decoder, z, 12, is_decoder=True, fast=fast)
        p.encoder._tile_hook = VAEHook(p.encoder, 64, is_decoder=False, fast_decoder=fast, fast_encoder=fast, color_fix=False)
        p.decoder._tile_hook = VAEHook(p.decoder, 12, is_decoder=True, fast_decoder=fast, fast_encoder=fast, color_fix=False)
        got_e, got_d = p.encoder(img.to(DEV)), p.decoder(z.to(DEV))
    _report(f"tiled encoder accurate ({'fast' if fast else 'exact'})", got_e, ref_e, 1e-3)
    _report(f"tiled decoder accurate ({'fast' if fast else 'exact'})", got_d, ref_d, 1e-3)


# ---- fp16 range guard ------------------------------------------------------------------------------------------------------------
def test_range_guard_flags_clipped_operands():
    """A 16-bit operand written past +-65504 (GEMM epilogue, stream -> operand cast, the GroupNorm pass's raw cast) raises the
    overflow word; values inside the range, fp32 outputs and the guard switched off do not."""
    from omgsr_amd import ops
    ops.overflow_seen()
    x = torch.randn(1, 300, 320, generator=_g(40)).to(DEV)
    w = torch.randn(640, 320, generator=_g(41)) * 320 ** -0.5
    pw = ops.pack_linear_weight(w, None, device=DEV)
    big = ops.pack_linear_weight(w * 3e4, None, device=DEV)           # outputs ~ 3e4 x N(0,1): some beyond 65504
    ops.linear(x, pw, out_dtype=ops.OUT_BF16)
    assert not ops.overflow_seen()
    ops.linear(x, big, out_dtype=ops.OUT_F32)                         # an fp32 output cannot clip
    assert not ops.overflow_seen()
    y = ops.linear(x, big, out_dtype=ops.OUT_BF16)
    assert ops.overflow_seen() and not ops.overflow_seen()            # read resets
    assert y.float().abs().max().item() == 65504.0                    # the stores saturate, they do not make inf
    ops.linear(x, big, out_dtype=ops.OUT_BF16, out_split=2)
    assert ops.overflow_seen()
    ops.linear(x * 1e5, pw, out_dtype=ops.OUT_F32)                    # the INPUT cast (fp32 stream -> fp16 operand) clips
    assert ops.overflow_seen()
    huge = torch.full((2, 16, 64), 7e4, device=DEV)
    ops.to_operand(huge, 2)
    assert ops.overflow_seen()
    ops.group_norm(torch.randn(1, 64, 1, 64, generator=_g(42)).to(DEV) * 1e5, None, None, 8, 1e-6, also_cast=1)
    assert ops.overflow_seen()
    ops.set_range_guard(False)
    try:
        ops.to_operand(huge, 1)
        assert not ops.overflow_seen()
    finally:
        ops.set_range_guard(True)


def test_range_guard_covers_split_k_and_residual_paths(monkeypatch):
    """the split-K reduce pass clamps 16-bit outputs like the fused epilogues, so it must raise the overflow word like
    them (few rows, long K: the shape class of the UNet's 16 x 16 / 8 x 8 projections), GEGLU reduce branch included; and the
    generic (non-16-byte-row) epilogue path notes the value it STORES, i.e. after the residual add."""
    import ctypes as C
    from omgsr_amd import _lib, ops
    ws_bytes = []
    orig = ops._igemm
    def spy(a, device, what):
        ws_bytes.append(int(_lib.load().omgsr_igemm_workspace_bytes(C.byref(a))))
        return orig(a, device, what)
    monkeypatch.setattr(ops, "_igemm", spy)
    ops.overflow_seen()
    g = _g(50)
    x = torch.randn(1, 256, 2560, generator=g).to(DEV)
    w = torch.randn(1280, 2560, generator=g) * 2560 ** -0.5
    pw, big = ops.pack_linear_weight(w, None, device=DEV), ops.pack_linear_weight(w * 4e4, None, device=DEV)
    ops.linear(x, pw, out_dtype=ops.OUT_BF16)
    assert ws_bytes[-1] > 0, "shape no longer takes split-K: pick another"
    assert not ops.overflow_seen()
    y = ops.linear(x, big, out_dtype=ops.OUT_BF16)
    assert ws_bytes[-1] > 0 and ops.overflow_seen() and y.float().abs().max().item() == 65504.0
    ops.linear(x, big, out_dtype=ops.OUT_F32)
    assert ws_bytes[-1] > 0 and not ops.overflow_seen()
    ops.linear(x, big, out_dtype=ops.OUT_BF16, out_split=2)
    assert ws_bytes[-1] > 0 and ops.overflow_seen()
    wg = torch.randn(2 * 1280, 2560, generator=g) * 2560 ** -0.5
    pg = ops.pack_geglu_weight(wg * 300.0, None, device=DEV)                       # a * gelu(gate) ~ 9e4 x N(0,1) x ...
    ops.linear(x, pg, out_dtype=ops.OUT_BF16, act=ops.ACT_GEGLU)
    assert ws_bytes[-1] > 0 and ops.overflow_seen()
    # generic epilogue path (Cout % 8 != 0) with a residual: only the SUM leaves the range
    xs = torch.randn(1, 300, 320, generator=g).to(DEV)
    w2 = torch.randn(324, 320, generator=g) * 320 ** -0.5
    p2 = ops.pack_linear_weight(w2, None, device=DEV)
    res = torch.full((1, 300, 324), 6.0e4, device=DEV, dtype=ops.stream_dtype())
    ops.linear(xs * 2000.0, p2, out_dtype=ops.OUT_BF16, residual=res)             # |x W| ~ 2e3 x N(0,1): + 6e4 crosses 65504 in places
    assert ops.overflow_seen()
    ops.linear(xs, p2, out_dtype=ops.OUT_BF16, residual=res * 0.5)
    assert not ops.overflow_seen()


def test_pipeline_falls_back_to_bf16_operands_on_fp16_overflow():
    """Activations past 65504 inside the model: every attention V projection of the UNet is scaled by 2e5 and its output projection
    by 1 / 2e5 - the same function (attention is linear in V) whose V operand no longer fits fp16. The accurate tier notices (one
    flag read at forward()'s sync), recomputes the call with bf16 operands and warns; the result stays close to the fp32 oracle
    where the clipped fp16 result is far off."""
    import warnings
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api import AutoencoderKL, UNet2DConditionModel
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    from omgsr_amd.testing import rel_l2, seeded_init_, synthetic_lq
    from oracle import diffusers_ref as R
    from oracle.pipeline_ref import OmgsrSRef
    vcfg = dict(block_out_channels=[32, 64, 128, 128], layers_per_block=1)
    ucfg = dict(block_out_channels=[64, 128, 256, 256], attention_head_dim=[1, 2, 4, 4], cross_attention_dim=128)
    ov, ou = seeded_init_(R.AutoencoderKL(**vcfg), 1).eval(), seeded_init_(R.UNet2DConditionModel(**ucfg), 2).eval()
    with torch.no_grad():
        for n, m in ou.named_modules():
            if n.endswith("attn1") or n.endswith("attn2"):
                m.to_v.weight.mul_(2.0 ** 18)
                m.to_out[0].weight.mul_(2.0 ** -18)
    pv, pu = AutoencoderKL(**vcfg), UNet2DConditionModel(**ucfg)
    pv.load_state_dict(ov.state_dict()); pu.load_state_dict(ou.state_dict())
    g = _g(3)
    x = synthetic_lq(1, 128, 128)
    ehs = torch.randn(1, 77, 128, generator=g)
    eps = torch.randn(1, 4, 16, 16, generator=g)
    ov.posterior_noise = eps; pv.posterior_noise = eps
    with torch.no_grad():
        ref = OmgsrSRef(ov, ou, R.DDPMScheduler().alphas_cumprod[273], 273)(x, ehs, 16, 8)
    pipe = OMGSR_S_Infer(None, None, 273, DEV, torch.float32, vae=pv, unet=pu)
    snap = [(m.op_split, m.w_split) for m in pipe.unet.modules() if hasattr(m, "op_split")]
    with torch.no_grad():
        ops.set_range_guard(False)
        try:
            clipped, _ = pipe(x.to(DEV), ehs.to(DEV), 16, 8)
        finally:
            ops.set_range_guard(True)
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            got, _ = pipe(x.to(DEV), ehs.to(DEV), 16, 8)
        assert any("65504" in str(w.message) for w in wlist)
        # the fallback is STICKY: the pipeline stays range-safe, so the next call is ONE bf16-operand pass with no
        # warning, no fp16 pass in front of it and no re-pack (same bits as the recomputed call)
        assert pipe.range_fallback.count == 1 and pipe.range_fallback.sticky
        assert ops.precise() and ops.act_dtype() == torch.bfloat16
        with warnings.catch_warnings(record=True) as wlist2:
            warnings.simplefilter("always")
            again, _ = pipe(x.to(DEV), ehs.to(DEV), 16, 8)
        assert not any("65504" in str(w.message) for w in wlist2) and pipe.range_fallback.count == 1
        assert torch.equal(again, got)
        ops.set_compute_dtype(torch.bfloat16)                                        # (another pipeline switches the process-wide tier ...)
        third, _ = pipe(x.to(DEV), ehs.to(DEV), 16, 8)                               # ... and the sticky one re-asserts its own)
        assert torch.equal(third, got)
        pipe.range_fallback.reset()
    assert ops.precise() and ops.act_dtype() == torch.float16                     # reset(): tier and policy are back
    assert snap == [(m.op_split, m.w_split) for m in pipe.unet.modules() if hasattr(m, "op_split")]
    e_clip, e = rel_l2(clipped, ref), rel_l2(got, ref)
    print(f"fp16 operands clipped: rel-L2 {e_clip:.3e}; bf16-operand fallback: rel-L2 {e:.3e}")
    assert torch.isfinite(got).all() and e <= 1e-2 and e_clip > 3 * e


@pytest.mark.parametrize("B,M,Nk,C", [(2, 200, 256, 512), (1, 1024, 1000, 512), (3, 96, 130, 128)])
def test_bmm_nt_both_factors_split(B, M, Nk, C):
    """Score GEMM of the VAE's one-head attention with q AND k as two-term splits (ops.bmm_nt both_split: q_hi k_hi + q_lo k_hi + q_hi k_lo,
    the third segment wrapping back to q_hi): 2^-20-ish against fp64, where the single-term form sits at 2^-11; ragged key counts are padded
    with zero rows by split_rows_hhl."""
    from omgsr_amd import ops
    q, k = torch.randn(B, M, C, generator=_g(70)) * 2, torch.randn(B, Nk, C, generator=_g(71)) * 2
    ref = torch.einsum("bmc,bnc->bmn", q.double(), k.double()) * C ** -0.5
    q2, k2 = ops.to_operand(q.to(DEV), 2), ops.to_operand(k.to(DEV), 2)
    Np = ops._round_up(Nk, 128)
    kh = ops.split_rows_hhl(k2, Np)
    assert tuple(kh.shape) == (B, Np, 3 * C) and torch.equal(kh[:, :Nk, :C], kh[:, :Nk, C:2 * C]) and torch.equal(kh[:, :Nk, 2 * C:], k2[..., C:])
    assert Np == Nk or (kh[:, Nk:] == 0).all()
    s = ops.bmm_nt(q2, kh, alpha=C ** -0.5, out_dtype=ops.OUT_F32, both_split=True)
    assert tuple(s.shape) == (B, M, Np) and s.dtype == torch.float32
    e2 = _rel(s[..., :Nk], ref)
    s1 = ops.bmm_nt(ops.to_operand(q.to(DEV), 1), ops.split_rows_hhl(k2, Np)[..., :C].contiguous(), alpha=C ** -0.5, out_dtype=ops.OUT_F32)
    e1 = _rel(s1[..., :Nk], ref)
    assert e2 < 3e-6 and e1 > 20 * e2, (e1, e2)
    assert Np == Nk or (s[..., Nk:] == 0).all()


def test_vae_attention_qk_split_path():
    """VaeAttention with the policy's qk_split mark (omgsr_amd/precision.py VAE_QK_SPLIT) against the fp64 block. The logits of the marked
    block are exact to ~2^-20 (single-term q / k: 2^-11 x the logit spread); on the block's OUTPUT that shows only when a row has several
    comparable keys (a dominant key's own perturbation cancels in the normalisation), so the block-level bound is 'no worse, and a different
    result', the logit-level one is the strict one."""
    from omgsr_amd import ops, precision as P
    from omgsr_amd.diffusers_api.autoencoder_kl import VaeAttention
    torch.manual_seed(5)
    C, H, W = 128, 24, 20
    L, Lp = H * W, 512
    a = VaeAttention(C, 32)
    with torch.no_grad():
        for n, p_ in a.named_parameters():
            p_.copy_(torch.randn(p_.shape, generator=_g(80 + len(n))) * (1.7 * C ** -0.5 if ("to_q.weight" in n or "to_k.weight" in n) else C ** -0.5 if p_.dim() == 2 else 0.1))
        a.group_norm.weight.add_(1.0)
    x = torch.randn(1, C, H, W, generator=_g(81)) * 2
    xd = x.double()
    g64 = F.group_norm(xd, 32, a.group_norm.weight.double(), a.group_norm.bias.double(), 1e-6).reshape(1, C, L).transpose(1, 2)
    q64, k64, v64 = (F.linear(g64, m.weight.double(), m.bias.double()) for m in (a.to_q, a.to_k, a.to_v))
    s64 = q64 @ k64.transpose(1, 2) * C ** -0.5
    want = F.linear(s64.softmax(-1) @ v64, a.to_out[0].weight.double(), a.to_out[0].bias.double()).transpose(1, 2).reshape(1, C, H, W) + xd
    a = a.to(DEV)
    P.apply_policy(a, [r"."], [r"."], qk=[])
    with torch.no_grad():
        plain = a(x.to(DEV)).float().cpu()
        assert not a.qk_split
        P.set_qk_split(a, [r"^$"])                     # the root module's own name is ""
        assert a.qk_split
        sharp = a(x.to(DEV)).float().cpu()
        # the logits themselves, through the module's own projections
        g = a.group_norm.nhwc(x.to(DEV).permute(0, 2, 3, 1).contiguous(), split=2).reshape(1, L, 2 * C)
        q2, k2 = a.to_q.nhwc(g, out_dtype=ops.OUT_BF16, out_split=2), a.to_k.nhwc(g, out_dtype=ops.OUT_BF16, out_split=2)
        s2 = ops.bmm_nt(q2, ops.split_rows_hhl(k2, Lp), alpha=a.scale, out_dtype=ops.OUT_F32, both_split=True)[..., :L]
        q1, k1 = a.to_q.nhwc(g, out_dtype=ops.OUT_BF16), a.to_k.nhwc(g, out_dtype=ops.OUT_BF16)
        kp = torch.zeros((1, Lp, C), device=DEV, dtype=k1.dtype); kp[:, :L] = k1
        s1 = ops.bmm_nt(q1, kp, alpha=a.scale, out_dtype=ops.OUT_F32)[..., :L]
    e1, e2 = _rel(s1, s64), _rel(s2, s64)
    e_plain, e_sharp = _rel(plain - x, want - xd), _rel(sharp - x, want - xd)
    print(f"VAE attention: logits q / k single {e1:.2e} -> split {e2:.2e}; branch output {e_plain:.2e} -> {e_sharp:.2e}")
    assert e2 < 3e-6 and e1 > 30 * e2, (e1, e2)
    assert not torch.equal(plain, sharp) and e_sharp <= 1.05 * e_plain and e_sharp < 4e-4, (e_plain, e_sharp)


# ---- round 5: fp6 (e2m3) correction segments with per-block scales (OMGSR_EL_MX6, split 4) -----------------------------------

_E2M3 = torch.tensor([0, .125, .25, .375, .5, .625, .75, .875, 1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
                      2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5], dtype=torch.float64)


def _mx6_third(raw):
    """[..., C] uint8 (one correction third of an OMGSR_EL_MX6 row) -> [..., C] float64, decoded straight from the format's definition
    (include/omgsr_hip.h): per 64-byte group two blocks; block h = bytes [16h, 16h + 16) + [32 + 16h, 40 + 16h), scale byte 40 + 16h."""
    lead, C = raw.shape[:-1], raw.shape[-1]
    g = raw.reshape(-1, C // 64, 64).to(torch.int64)
    out = torch.zeros(g.shape[0], C // 64, 2, 32, dtype=torch.float64)
    for h in (0, 1):
        st = torch.cat([g[..., 16 * h:16 * h + 16], g[..., 32 + 16 * h:40 + 16 * h]], -1)
        sc = 2.0 ** (g[..., 40 + 16 * h].double() - 127)
        for i in range(32):
            by, sh = (6 * i) // 8, (6 * i) % 8
            code = ((st[..., by] | (st[..., min(by + 1, 23)] << 8)) >> sh) & 63
            out[..., h, i] = torch.where((code & 32) != 0, -1.0, 1.0) * _E2M3[code & 31] * sc
    return out.reshape(*lead, C)


def test_to_operand_mx6_is_the_documented_byte_format():
    """The cast kernel's OMGSR_EL_MX6 row against the host packer (ops._e2m3_blocks: the same integer arithmetic, so BYTES are compared) and
    against the format's definition (decode: a_hi + a_lo' reproduces a to 2^-4 of the block's largest residual)."""
    from omgsr_amd import ops
    x = torch.randn(3, 50, 2, 256, generator=_g(70)) * torch.exp(torch.randn(256, generator=_g(71)))
    x[0, 0, 0, :32] = 0.0                                      # an all-zero block: scale byte 0, codes 0
    x[1, 3, 1, 64:96] *= 1e-30                                 # a block below the E8M0 range of interest
    y = ops.to_operand(x.to(DEV), 4)
    assert y.dtype == torch.float16 and y.shape[-1] == 2 * 256
    raw = y.cpu().view(torch.uint8).reshape(3, 50, 2, 4 * 256)
    hi = x.to(torch.float16)
    want = torch.cat([hi.contiguous().view(torch.uint8).reshape(3, 50, 2, 512), ops._e2m3_blocks(x - hi.float()), ops._e2m3_blocks(hi.float())], -1)
    assert torch.equal(raw, want)
    lo = _mx6_third(raw[..., 512:768])
    resid = (x - hi.float()).double()
    bmax = resid.reshape(3, 50, 2, 8, 32).abs().amax(-1, keepdim=True).expand(3, 50, 2, 8, 32).reshape(resid.shape)
    assert ((lo - resid).abs() <= bmax * (0.25 / 3.75) + 1e-300).all()
    assert _rel(hi.double() + lo, x) < 3e-5


@pytest.mark.parametrize("C,G,HW,twin", [(128, 32, 4096, 0), (320, 32, 1000, 3), (512, 32, 300, 2), (256, 32, 77, 1)])
def test_group_norm_mx6_operand(C, G, HW, twin):
    """GroupNorm apply (+ SiLU) writing the fp6 form: the fp16 third is bit-equal to the other forms', the fp6 thirds decode to the residual and to
    a_hi within the format's step; the shortcut twin (plain / split / MX) is untouched by the first output's form. Ragged pixel counts: the lane
    quads that share a block stay together in the kernel's tail loop."""
    from omgsr_amd import ops
    if C % 64:
        pytest.skip("whole 64-channel chunks")
    x = torch.randn(2, HW, 1, C, generator=_g(2)) * 3 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=_g(3)), 0.1 * torch.randn(C, generator=_g(4))
    xd = x.to(DEV)
    mean, rstd, _ = ops.group_norm_stats(xd, G, 1e-6)
    out = ops.group_norm_apply(xd, mean, rstd, gamma.to(DEV), beta.to(DEV), G, ops.ACT_SILU, split=4, also_cast=twin)
    y, y2 = out if twin else (out, None)
    ref2 = ops.group_norm_apply(xd, mean, rstd, gamma.to(DEV), beta.to(DEV), G, ops.ACT_SILU, split=2, also_cast=twin)
    s2, t2 = ref2 if twin else (ref2, None)
    if twin:
        assert torch.equal(y2, t2)
    raw = y.cpu().view(torch.uint8).reshape(2, HW, 1, 4 * C)
    hi = raw[..., :2 * C].contiguous().view(torch.float16)
    assert torch.equal(hi, s2[..., :C].cpu())
    lo_ref = s2[..., C:].double().cpu()                         # the two-term split's low half: the residual to 2^-11 of itself
    lo, hi6 = _mx6_third(raw[..., 2 * C:3 * C]), _mx6_third(raw[..., 3 * C:])
    nb = C // 32
    bm = lambda t: t.reshape(2, HW, 1, nb, 32).abs().amax(-1, keepdim=True).expand(2, HW, 1, nb, 32).reshape(t.shape)     # noqa: E731
    assert ((lo - lo_ref).abs() <= bm(lo_ref) * 0.07).all()
    assert ((hi6 - hi.double()).abs() <= bm(hi.double()) * 0.07).all()
    ref = F.silu(F.group_norm(x.permute(0, 3, 1, 2).double(), G, gamma.double(), beta.double(), 1e-6)).permute(0, 2, 3, 1)
    assert _rel(hi.double() + lo, ref) < 3e-5


_MX6_CASES = [(2, 64, 64, 128, 128), (1, 64, 96, 320, 320), (2, 16, 16, 1280, 640), (1, 40, 43, 512, 512), (1, 9, 33, 64, 128), (4, 38, 38, 256, 256), (4, 75, 75, 256, 512),
              (1, 128, 128, 128, 136)]


@pytest.mark.parametrize("N,H,W,C,Cout", _MX6_CASES)
def test_conv_mx6(N, H, W, C, Cout):
    """a w = a_hi w_hi (fp16 MFMAs) + a_lo w_hi + a_hi w_lo with the correction terms as fp6 (e2m3) codes and per-32-channel E8M0 scales from the
    data, in the f8f6f4 MFMA's 8-pass form (igemm_halo_mx6.hip: spatial and FLAT forms, ragged maps). Same 3 mantissa bits as the fp8 form: the
    corrections are carried to ~2^-4 of their block's largest, i.e. the result to ~1e-5, against ~3e-4 for one fp16 rounding of both sides."""
    from omgsr_amd import ops
    x = torch.randn(N, H, W, C, generator=_g(8)) * torch.exp(0.7 * torch.randn(C, generator=_g(12)))      # channel gains: blocks with a dominant channel
    w = torch.randn(Cout, C, 3, 3, generator=_g(9)) * (9 * C) ** -0.5
    b = 0.1 * torch.randn(Cout, generator=_g(10))
    res = torch.randn(N, H, W, Cout, generator=_g(11))
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1) + res.double()
    pw = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=4)
    assert pw.mx_fmt == 6 and pw.split == 4 and pw.row_channels == 2 * C
    y = ops.conv2d(x.to(DEV), pw, pad=1, residual=res.to(DEV), gn_groups=8)
    e = _rel(y[..., :Cout], ref)
    pw8 = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8, split=3)
    e8 = _rel(ops.conv2d(x.to(DEV), pw8, pad=1, residual=res.to(DEV))[..., :Cout], ref)
    pw1 = ops.pack_conv_weight(w, b, device=DEV, cout_multiple=8)
    e1 = _rel(ops.conv2d(x.to(DEV), pw1, pad=1, residual=res.to(DEV))[..., :Cout], ref)
    print(f"conv MX6 {N, H, W, C, Cout}: rel {e:.2e} (fp8 form {e8:.2e}, single fp16 rounding of both sides {e1:.2e})")
    assert e < 3e-5 and e1 > 8 * e and e < 3 * e8 + 1e-5
    mean, _, _ = ops.group_norm_stats(y, 8, 1e-6)                  # statistics left by the halo epilogue
    assert torch.allclose(mean.double().cpu(), y.double().cpu().reshape(N, H * W, 8, -1).mean(dim=(1, 3)), atol=1e-5, rtol=1e-5)
    assert torch.equal(ops.conv2d(x.to(DEV), pw, pad=1, residual=res.to(DEV)), y)


def test_conv_mx6_multi_launch_split_k_and_refusals():
    from omgsr_amd import ops
    C, Cout = 128, 128
    w = torch.randn(Cout, C, 3, 3, generator=_g(9)) * (9 * C) ** -0.5
    pw = ops.pack_conv_weight(w, None, device=DEV, split=4)
    # the tile-shape groups of a tiled-VAE level in one launch (FLAT plan for the whole group), then a spatial group, then a group of maps
    # 46-80 wide (FLAT plan with the 27-piece patch)
    for shapes in ([(3, 40, 40), (1, 40, 32), (1, 32, 40), (1, 32, 32)], [(2, 96, 96), (1, 96, 64), (1, 64, 96)], [(2, 48, 48), (1, 48, 40)]):
        xs = [torch.randn(n, h, wd, C, generator=_g(20 + i)) for i, (n, h, wd) in enumerate(shapes)]
        ys = ops.conv2d_multi([ops.to_operand(x.to(DEV), 4) for x in xs], pw, pad=1)
        for x, y in zip(xs, ys):
            ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1)
            assert _rel(y, ref) < 3e-5
    # one image per call: the chunk ranges of the contraction as one launch group (halo split-K), fp6 chunks included
    for (N, H, W, Ci, Co) in [(1, 64, 64, 512, 512), (1, 32, 32, 640, 640), (1, 8, 64, 64, 128)]:
        x = torch.randn(N, H, W, Ci, generator=_g(41))
        wk = torch.randn(Co, Ci, 3, 3, generator=_g(42)) * (9 * Ci) ** -0.5
        r = torch.randn(N, H, W, Co, generator=_g(44))
        ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wk.double(), padding=1).permute(0, 2, 3, 1) + r.double()
        y = ops.conv2d(ops.to_operand(x.to(DEV), 4), ops.pack_conv_weight(wk, None, device=DEV, split=4), pad=1, residual=r.to(DEV))
        assert _rel(y, ref) < 3e-5
    # no 1x1 weight is packed in the form (the GEMM-shaped MX kernels read fp8 corrections)
    with pytest.raises(ValueError):
        ops.pack_conv_weight(torch.randn(128, 128, 1, 1), None, device=DEV, split=4)


@pytest.mark.parametrize("H,W", [(48, 48), (40, 40), (72, 72), (64, 64)])
def test_conv_mx6_split_k_with_fp6_output_on_narrow_maps(H, W):
    """ONE image per call through a ResnetBlock conv2 that feeds an up-sampler in the accurate tier - fp6 operand in, fp6 operand
    out (out_split = 4), 512 -> 512 on a latent that is not 64 wide. The real arguments plan a spatial split-K (an out_mx = 6 problem is never FLAT);
    the stripped chunk-range parts used to re-plan themselves onto the FLAT form (W <= 80) and the launch refused with OMGSR_E_SHAPE. The result
    is the same operand the cast kernel makes of the one-pass conv's stream output: fp16 third equal up to summation order, corrections decoding to it."""
    import ctypes as C_
    from omgsr_amd import _lib, ops
    Ci = Co = 512
    x = torch.randn(1, H, W, Ci, generator=_g(61))
    wk = torch.randn(Co, Ci, 3, 3, generator=_g(62)) * (9 * Ci) ** -0.5
    r = torch.randn(1, H, W, Co, generator=_g(63))
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), wk.double(), padding=1).permute(0, 2, 3, 1) + r.double()
    pw = ops.pack_conv_weight(wk, None, device=DEV, split=4)
    xo = ops.to_operand(x.to(DEV), 4)
    a = _lib.IgemmArgs()
    ops._conv_args(a, xo, pw, 1, 1, False, ops.ACT_NONE, r.to(DEV), None, ops.OUT_BF16, 1.0, None, 4, 0)
    cols = -(-Co // 128) * 128
    splits = _lib.load().omgsr_igemm_workspace_bytes(C_.byref(a)) // (4 * H * W * cols)
    assert a.out_mx == 6 and splits >= 2, "this shape was meant to plan a halo split-K with an fp6 output"
    got = ops.conv2d(xo, pw, pad=1, residual=r.to(DEV), out_dtype=ops.OUT_BF16, out_split=4)
    raw = got.cpu().view(torch.uint8).reshape(1, H, W, 4 * Co)
    hi = raw[..., :2 * Co].contiguous().view(torch.float16).double()
    lo = _mx6_third(raw[..., 2 * Co:3 * Co])
    hi6 = _mx6_third(raw[..., 3 * Co:])
    assert _rel(hi + lo, ref) < 3e-5 and _rel(hi6, ref) < 5e-2
    again = ops.conv2d(xo, pw, pad=1, residual=r.to(DEV), out_dtype=ops.OUT_BF16, out_split=4)
    assert torch.equal(again.view(torch.int16), got.view(torch.int16))       # raw bytes (fp6 codes read as fp16 may be NaN patterns)


def test_conv_mx6_upsample_phase_form_and_out6_producers():
    """The producer / consumer pair of a VAE up-sampler in the fp6 form: the previous 3x3 conv writes the OMGSR_EL_MX6 operand from the halo-tile kernel's
    OUT6 instantiations (plain fp16 and fp6 operands, single launches and launch groups) byte for byte as the cast kernel would; problems those
    instantiations cannot run (small maps, GEMM-shaped ones) take a stream tensor + the cast kernel, with the same bytes; the phase-decomposed
    up-sampling conv consumes the operand (fp16 chunks + fp6 chunks of the phase-summed kernels)."""
    import ctypes as C_
    from omgsr_amd import _lib, ops
    bits = lambda t: t.contiguous().view(torch.int16)              # noqa: E731  (raw bytes behind a 16-bit dtype: compare patterns, not values)
    C = 128
    wi = torch.zeros(C, C, 3, 3); wi[:, :, 1, 1] = torch.eye(C)      # identity centre tap: the epilogue sees exactly its input
    res = torch.randn(4, 96, 128, C, generator=_g(50))
    xh = (torch.randn(4, 96, 128, C, generator=_g(35)) * 3).to(torch.float16).float()
    want = ops.to_operand((xh + res).to(DEV), 4)
    for split in (1, 4):                                            # the decoder's single (plain fp16) layers / the fp6 layers in front of an up-sampler
        pw = ops.pack_conv_weight(wi, None, device=DEV, split=split)
        a = _lib.IgemmArgs()
        xo = ops.to_operand(xh.to(DEV), split)
        ops._conv_args(a, xo, pw, 1, 1, False, ops.ACT_NONE, res.to(DEV), None, ops.OUT_BF16, 1.0, None, 4, 0)
        assert _lib.load().omgsr_igemm_out_mx6_ok(C_.byref(a)) == 1, "this shape was meant to take an OUT6 instantiation"
        got = ops.conv2d(xo, pw, pad=1, residual=res.to(DEV), out_dtype=ops.OUT_BF16, out_split=4)
        assert torch.equal(bits(got), bits(want))
        # a launch group (the tile-shape groups of a tiled-VAE level)
        parts = [(xh[:2], res[:2]), (xh[2:, :64], res[2:, :64]), (xh[2:, 64:, :96], res[2:, 64:, :96])]
        outs = ops.conv2d_multi([ops.to_operand(p[0].contiguous().to(DEV), split) for p in parts], pw, pad=1, residuals=[p[1].contiguous().to(DEV) for p in parts],
                                out_dtype=ops.OUT_BF16, out_split=4)
        for o, p_ in zip(outs, parts):
            assert torch.equal(bits(o), bits(ops.to_operand((p_[0] + p_[1]).contiguous().to(DEV), 4)))
    # fall-backs: a small map (not a halo-kernel problem) and a Linear - stream tensor + cast kernel, same bytes
    xs = (torch.randn(1, 16, 16, C, generator=_g(51)) * 3).to(torch.float16).float().to(DEV)
    got = ops.conv2d(ops.to_operand(xs, 1), ops.pack_conv_weight(wi, None, device=DEV), pad=1, out_dtype=ops.OUT_BF16, out_split=4)
    assert torch.equal(bits(got), bits(ops.to_operand(xs, 4)))
    eye = ops.pack_linear_weight(torch.eye(C), None, device=DEV)
    xr = (torch.randn(1, 5000, C, generator=_g(52)) * 3).to(torch.float16).float().to(DEV)
    assert torch.equal(bits(ops.linear(xr, eye, out_dtype=ops.OUT_BF16, out_split=4)), bits(ops.to_operand(xr, 4)))
    # the consumer: nearest-2x + 3x3 conv in the phase form over the fp6 operand
    C2 = 256
    x = torch.randn(2, 43, 86, C2, generator=_g(31))
    w = torch.randn(C2, C2, 3, 3, generator=_g(32)) * (9 * C2) ** -0.5
    b = 0.1 * torch.randn(C2, generator=_g(33))
    ref = F.conv2d(F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    pw = ops.pack_conv_weight(w, b, device=DEV, split=4, upsample_phases=True)
    assert pw.w_ph is not None and pw.mx_fmt == 6
    y = ops.conv2d(x.to(DEV), pw, pad=1, upsample=True, gn_groups=32)
    e = _rel(y, ref)
    y8 = ops.conv2d(x.to(DEV), ops.pack_conv_weight(w, b, device=DEV, split=3, upsample_phases=True), pad=1, upsample=True)
    print(f"phase-form fp6 conv: rel {e:.2e} (fp8 form {_rel(y8, ref):.2e})")
    assert e < 3e-5 and torch.equal(ops.conv2d(x.to(DEV), pw, pad=1, upsample=True), y)
    ys = ops.conv2d_multi([ops.to_operand(x.to(DEV), 4), ops.to_operand(x[:1, :, :64].contiguous().to(DEV), 4)], pw, pad=1, upsample=True)
    ref1 = F.conv2d(F.interpolate(x[:1, :, :64].permute(0, 3, 1, 2).double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    assert _rel(ys[0], ref) < 3e-5 and _rel(ys[1], ref1) < 3e-5
