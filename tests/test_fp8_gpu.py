"""The fp8 tier on the MI355X: the MXFP8 quantiser bit for bit against the host reference, the MXFP8 x MXFP8 GEMM (mxfp8_gemm_kernel)
against the dequantised operands multiplied in fp64 in every output form the DiT issues, the full-depth OMGSR-F 256 -> 1024 pipeline
against the accurate tier, and the tier's invariants (batch invariance, graph replay, in-place weight edits)."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# fp8 tier vs the accurate tier, full-depth OMGSR-F 256 -> 1024, seeded weights (DESIGN.md §4 records draws 0-2): measured draw 0
# (rel-L2 6.61e-2, PSNR 33.45 dB on MI355X) x 1.25; the tier's target is >= 30 dB
FP8_VS_ACCURATE_REL_L2 = 8.3e-2
FP8_VS_ACCURATE_PSNR = 30.0
# MXFP8 GEMM vs the dequantised operands multiplied in fp64. Measured 1.40-1.49e-5 at every K from 384 to 15360 (bias, GELU, gate and
# residual alike). The kernel's wiring is exact: the dyadic probes of tests/test_dyadic_probes_gpu.py (scale bytes 2^+-40 apart per row, column
# and K block, saturated and all-zero blocks, K = 128, grid.z slices) match the fp64 restatement bit for bit. The residual is the instruction's:
# v_mfma_scale_f32_32x32x64_f8f6f4 drops a product 2^14 or more below the largest of its 8-wide K group, and random e4m3
# blocks span up to 2^17.6 per operand
GEMM_REL_L2 = 3e-5


@pytest.fixture(autouse=True)
def _bf16_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _edge_rows(K: int) -> torch.Tensor:
    x = torch.zeros(6, K)
    x[1, :32] = torch.tensor([2.0 ** e for e in range(-16, 16)])
    x[2, :32] = 448.0 * 2.0 ** 3
    x[2, 32:64] = -448.0 * 2.0 ** -20
    x[3, :32] = torch.tensor([(-1) ** i * 1.5 * 2.0 ** (i % 15) for i in range(32)])
    x[4, 64:96] = 2.0 ** -60
    x[5] = torch.linspace(-3.0, 5.0, K)
    return x


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantiser_bit_exact(dtype):
    from omgsr_amd import _lib, ops
    from omgsr_amd.testing import mxfp8_ref
    K, ld = 384, 448
    g = torch.Generator().manual_seed(3)
    x = torch.randn(203, ld, generator=g) * torch.exp2(torch.randint(-30, 30, (203, 1), generator=g).float())
    x[:6, :K] = _edge_rows(K)
    x = x.to(dtype)
    xd = x.to(DEV)
    codes = torch.full((203, K), 0xAB, dtype=torch.uint8, device=DEV)
    scales = torch.full((203, K // 32), 0xAB, dtype=torch.uint8, device=DEV)
    el = ops.EL_F32 if dtype == torch.float32 else ops.EL_16
    _lib.check(_lib.load().omgsr_quantize_mxfp8(xd.data_ptr(), el, 203, K, ld, codes.data_ptr(), scales.data_ptr(), ops._stream()), "quantize")
    want_c, want_s = mxfp8_ref(x[:, :K])
    assert torch.equal(scales.cpu(), want_s)
    assert torch.equal(codes.cpu(), want_c)
    # the wrapper (dense rows) agrees
    q = ops.quantize_mxfp8(xd[:, :K].contiguous())
    assert torch.equal(q.codes, codes) and torch.equal(q.scales, scales)


def _ref(xq, pw, bias=True):
    """fp64 product of the dequantised operands (+ bias): [M, Cout]."""
    from omgsr_amd.testing import mxfp8_dequant
    a = mxfp8_dequant(xq.codes.reshape(-1, pw.cin), xq.scales.reshape(-1, pw.cin // 32))
    w = mxfp8_dequant(pw.w[:pw.cout], pw.w_scale[:pw.cout])
    y = a @ w.T
    return y + pw.bias.double() if (bias and pw.bias is not None) else y


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def _problem(M, K, N, seed, batch=None):
    from omgsr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    shape = (M, K) if batch is None else (batch, M, K)
    x = torch.randn(shape, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g, device=DEV) * 0.1
    return ops.quantize_mxfp8(x), ops.pack_linear_weight_mxfp8(w, b)


@pytest.mark.parametrize("M,K,N", [(1000, 3072, 3072), (4608, 3072, 6144), (600, 12288, 3072), (512, 15360, 3072), (300, 384, 512)])
def test_gemm_bias_fp32_out(M, K, N):
    from omgsr_amd import ops
    xq, pw = _problem(M, K, N, M + K + N)
    y = ops.linear(xq, pw, out_dtype=ops.OUT_F32)
    assert y.shape == (M, N) and y.dtype == torch.float32
    assert _rel(y, _ref(xq, pw)) <= GEMM_REL_L2


def test_gemm_gelu_and_gate_residual():
    import math
    from omgsr_amd import ops
    xq, pw = _problem(777, 3072, 3072, 11)
    y = ops.linear(xq, pw, act=ops.ACT_GELU_TANH, out_dtype=ops.OUT_F32)
    r = _ref(xq, pw)
    gelu = 0.5 * r * (1 + torch.tanh(math.sqrt(2 / math.pi) * (r + 0.044715 * r ** 3)))
    assert _rel(y, gelu) <= GEMM_REL_L2
    gate = torch.randn(3072, device=DEV)
    res = torch.randn(777, 3072, device=DEV)
    y = ops.linear(xq, pw, gate=gate, residual=res, out_dtype=ops.OUT_F32)
    assert _rel(y, r * gate.double() + res.double()) <= GEMM_REL_L2
    # bf16 stream output: the same values rounded once
    y16 = ops.linear(xq, pw, gate=gate, residual=res.to(torch.bfloat16))
    assert y16.dtype == torch.bfloat16 and _rel(y16, r * gate.double() + res.to(torch.bfloat16).double()) <= 4e-3


def test_gemm_rows_do_not_depend_on_the_batch():
    from omgsr_amd import ops
    xq, pw = _problem(1000, 3072, 3072, 5)
    full = ops.linear(xq, pw)
    part = ops.linear(ops.Mxfp8(xq.codes[:300].contiguous(), xq.scales[:300].contiguous()), pw)
    assert torch.equal(full[:300], part)


def test_linear_into_slice_on_grid_z():
    from omgsr_amd import ops
    B, M, K, N, rows, ld, row0, col0 = 2, 600, 3072, 3072, 700, 2 * 3072 + 64, 50, 3072 + 64
    xq, pw = _problem(M, K, N, 21, batch=B)
    out = torch.full((B, rows, ld), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.linear_into(xq, pw, out, row0, col0)
    for b in range(B):
        ref = _ref(ops.Mxfp8(xq.codes[b], xq.scales[b]), pw)
        assert _rel(out[b, row0:row0 + M, col0:col0 + N], ref) <= 4e-3
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[:, row0:row0 + M, col0:col0 + N] = False
    assert bool((out[mask] == 7.0).all())                                     # nothing outside the slice moved


def test_linear_rows_range_on_grid_z():
    from omgsr_amd import ops
    B, L, K, N, row0, rows = 2, 700, 3072, 3072, 100, 500
    xq, pw = _problem(L, K, N, 22, batch=B)
    gate = torch.randn(N, device=DEV)
    res = torch.randn(B, rows, N, device=DEV).to(torch.bfloat16)
    y = ops.linear_rows(xq, row0, rows, pw, residual=res, gate=gate)
    for b in range(B):
        ref = _ref(ops.Mxfp8(xq.codes[b, row0:row0 + rows], xq.scales[b, row0:row0 + rows]), pw) * gate.double() + res[b].double()
        assert _rel(y[b], ref) <= 4e-3


def test_linear_t_into_transposed_on_grid_z():
    from omgsr_amd import ops
    B, L, K, N, ld, key0 = 2, 600, 3072, 3072, 712, 100
    xq, pw = _problem(L, K, N, 23, batch=B)
    out = torch.full((B, N, ld), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.linear_t_into(xq, pw, out, key0)
    for b in range(B):
        ref = _ref(ops.Mxfp8(xq.codes[b], xq.scales[b]), pw)
        assert _rel(out[b, :, key0:key0 + L], ref.T) <= 4e-3
    assert bool((out[:, :, :key0] == 7.0).all()) and bool((out[:, :, key0 + L:] == 7.0).all())


def test_unsupported_problem_is_refused():
    from omgsr_amd import _lib, ops
    from omgsr_amd._lib import IgemmArgs
    xq, pw = _problem(256, 384, 256, 1)
    a = IgemmArgs()
    ops._fill_mxfp8(a, xq.codes.data_ptr(), xq.scales.data_ptr(), pw)
    y = torch.empty(256, 256, device=DEV, dtype=torch.bfloat16)
    a.out, a.N, a.H, a.W, a.Ho, a.Wo, a.batch, a.alpha = y.data_ptr(), 1, 1, 256, 1, 256, 1, 1.0
    a.Cin = a.K_pad = 320                                                   # K % 128 != 0
    assert _lib.load().omgsr_igemm(C.byref(a), ops._stream()) == -2
    a.Cin = a.K_pad = 384
    a.Cout_pad = 384                                                        # Cout_pad % 256 != 0
    assert _lib.load().omgsr_igemm(C.byref(a), ops._stream()) == -2


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------

def _small_case():
    from omgsr_amd.diffusers_api import AutoencoderKL, FluxTransformer2DModel
    from omgsr_amd.pipelines.omgsr_f import prepare_latent_image_ids
    from omgsr_amd.testing import seeded_init_, synthetic_lq
    vae = seeded_init_(AutoencoderKL(block_out_channels=[32, 64, 128, 128], layers_per_block=1, latent_channels=16, scaling_factor=0.3611, shift_factor=0.1159), 3, rounded=False)
    flux = seeded_init_(FluxTransformer2DModel(num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64,
                                               pooled_projection_dim=32, in_channels=64), 4, rounded=False)
    g = torch.Generator().manual_seed(6)
    wd = torch.bfloat16
    inp = dict(pe=torch.randn(1, 32, 64, generator=g).to(DEV, wd), pooled=torch.randn(1, 32, generator=g).to(DEV, wd),
               tids=torch.zeros(32, 3, device=DEV, dtype=wd), iids=prepare_latent_image_ids(8, 8, DEV, wd),
               xs=[synthetic_lq(1, 128, 128, seed=s).to(DEV, wd) for s in (1, 2, 3)],
               ns=[torch.randn(1, 16, 16, 16, generator=g).to(DEV) for _ in range(3)])
    return vae, flux, inp


def _fp8_pipe(vae, flux):
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    return OMGSR_F_Infer(None, None, DEV, torch.float8_e4m3fn, 244, 1.0, vae=vae, flux_transformer=flux)


def _call(pipe, inp, x, n):
    pipe.vae.posterior_noise = n
    return pipe(x, inp["pe"], inp["pooled"], inp["tids"], inp["iids"], 16, 8)[0]


def test_fp8_tier_runs_the_fp8_kernel_and_differs_from_bf16():
    from omgsr_amd import _lib, ops
    from omgsr_amd.precision import fp8_layers
    vae, flux, inp = _small_case()
    pipe = _fp8_pipe(vae, flux)
    assert len(fp8_layers(flux)) == 2 * 12 + 2 * 5
    lib = _lib.load()
    with torch.no_grad():
        lib.omgsr_timing_enable(1); lib.omgsr_timing_reset()
        y8 = _call(pipe, inp, inp["xs"][0], inp["ns"][0])
        buf = (_lib.TimingEntry * 4096)()
        n = lib.omgsr_timing_collect(buf, 4096)
        lib.omgsr_timing_enable(0)
        assert sum(1 for e in buf[:n] if e.kind == 1 and e.variant == 18) >= 2 * 8 + 2 * 4      # every fp8 GEMM launch
        from omgsr_amd.precision import set_fp8_linear
        set_fp8_linear(flux, [])
        y16 = _call(pipe, inp, inp["xs"][0], inp["ns"][0])
    assert torch.isfinite(y8.float()).all() and not torch.equal(y8, y16)
    assert float((y8.float() - y16.float()).norm() / y16.float().norm()) < 0.1
    assert ops.compute_dtype_name() == "bf16"


def test_fp8_tier_batch_invariant():
    from omgsr_amd import ops
    vae, flux, inp = _small_case()
    pipe = _fp8_pipe(vae, flux)
    ops.set_batch_invariant(True)
    try:
        with torch.no_grad():
            a = _call(pipe, inp, inp["xs"][0], inp["ns"][0])
            b = _call(pipe, inp, inp["xs"][1], inp["ns"][1])
            ab = _call(pipe, inp, torch.cat(inp["xs"][:2]), torch.cat(inp["ns"][:2]))
    finally:
        ops.set_batch_invariant(False)
    assert torch.equal(ab[0:1], a) and torch.equal(ab[1:2], b)


def test_fp8_tier_graph_replay_equals_eager():
    vae, flux, inp = _small_case()
    pipe = _fp8_pipe(vae, flux)
    with torch.no_grad():
        eager = [_call(pipe, inp, x, inp["ns"][0]) for x in inp["xs"]]
        pipe.enable_graphs(True)
        got = [_call(pipe, inp, x, inp["ns"][0]) for x in inp["xs"]]
    assert pipe.graphs.captures == 1 and pipe.graphs.replays == 2
    for a, b in zip(eager, got):
        assert torch.equal(a, b)


def test_fp8_tier_in_place_weight_edit_repacks():
    from omgsr_amd.diffusers_api import AutoencoderKL, FluxTransformer2DModel
    vae, flux, inp = _small_case()
    vae_sd = {k: v.clone() for k, v in vae.state_dict().items()}
    pipe = _fp8_pipe(vae, flux)
    x, n = inp["xs"][0], inp["ns"][0]
    with torch.no_grad():
        y0 = _call(pipe, inp, x, n)
        lin = flux.single_transformer_blocks[0].proj_out
        assert lin.fp8
        lin.weight.mul_(1.5)
        y1 = _call(pipe, inp, x, n)
        assert not torch.equal(y0, y1)
        vae2 = AutoencoderKL(block_out_channels=[32, 64, 128, 128], layers_per_block=1, latent_channels=16, scaling_factor=0.3611, shift_factor=0.1159)
        vae2.load_state_dict(vae_sd)
        flux2 = FluxTransformer2DModel(num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64,
                                       pooled_projection_dim=32, in_channels=64).to(torch.bfloat16)
        flux2.load_state_dict(flux.state_dict())
        fresh = _fp8_pipe(vae2, flux2)
        assert torch.equal(_call(fresh, inp, x, n), y1)


def test_fp8_tier_full_depth_f1024_vs_accurate_tier():
    """Full depth (19 + 38 blocks, FLUX.1-dev width), OMGSR-F 256 -> 1024, batch 1, seeded weights generated on the device (as
    test_flux_fullsize_gpu.py does): the fp8 tier against the accurate tier (itself pinned <= 1e-3 from the fp32 oracle there)."""
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG, FluxTransformer2DModel
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer, prepare_latent_image_ids
    from omgsr_amd.testing import psnr, rel_l2, seeded_init_, seeded_init_device_, synthetic_lq
    draw = int(os.environ.get("OMGSR_FLUX_DRAW", "0"))
    ops.set_compute_dtype(torch.float32)
    with torch.device("meta"):
        pf = FluxTransformer2DModel()
    pf = pf.to_empty(device=DEV)
    seeded_init_device_(pf, 404 + 31 * draw)
    vae_sd = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303 + 31 * draw, rounded=False).state_dict()
    g = torch.Generator().manual_seed(4321 + draw)
    x = synthetic_lq(1, 1024, 1024, seed=1234 + draw).to(DEV)
    eps = torch.randn(1, 16, 128, 128, generator=torch.Generator().manual_seed(99 + draw)).to(DEV)
    pe, pooled = torch.randn(1, 512, 4096, generator=g).to(DEV), torch.randn(1, 768, generator=g).to(DEV)
    tids, iids = torch.zeros(512, 3, device=DEV), prepare_latent_image_ids(64, 64, DEV, torch.float32)
    pf.round_timestep_to_weight_dtype = False

    def run(wd):
        pv = AutoencoderKL(**FLUX_VAE_CONFIG)
        pv.load_state_dict(vae_sd)
        pipe = OMGSR_F_Infer(None, None, DEV, wd, 244, 1.0, vae=pv, flux_transformer=pf)
        pipe.vae.posterior_noise = eps
        cd = torch.float32 if wd == torch.float32 else torch.bfloat16
        with torch.no_grad():
            return pipe(x.to(cd), pe.to(cd), pooled.to(cd), tids.to(cd), iids.to(cd), 128, 64)[0].float()

    ref = run(torch.float32)
    y16 = run(torch.bfloat16)       # (the bf16 tier for the record: the module is cast to bf16 in place from here on)
    y8 = run(torch.float8_e4m3fn)
    e8, p8 = rel_l2(y8, ref), psnr(y8, ref)
    e16, p16 = rel_l2(y16, ref), psnr(y16, ref)
    print(f"draw {draw}: fp8 tier vs accurate tier rel-L2 {e8:.4e} PSNR {p8:.2f} dB; bf16 tier {e16:.4e} / {p16:.2f} dB")
    assert torch.isfinite(y8).all()
    assert e8 <= FP8_VS_ACCURATE_REL_L2 and p8 >= FP8_VS_ACCURATE_PSNR, (e8, p8)
