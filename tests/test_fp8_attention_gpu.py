"""The fp8 tier's MXFP8 attention on the MI355X: mxfp8_attn_kernel against the torch restatement of its arithmetic
(omgsr_amd.testing.mxfp8_attention_ref) and against exact attention, its invariants (constant V, masked keys, repeatability, batch
invariance), rmsnorm_rope_mxfp8 against quantize_mxfp8 of the fp32 RMSNorm + RoPE, the refusals, and the pipeline with
precision_policy={"flux": {"fp8_attention": ...}} (small case and full depth)."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128

# kernel vs its torch restatement (same operands, same P rule). The issue's guess was 1e-3; measured on MI355X 1.92e-3 / 1.82e-3 / 1.90e-3
# (self_4608 / ragged_1000 / broadcast), 1.27e-3 / 1.10e-3 / 1.24e-3 against the restatement rounded to bf16: the bf16 output's rounding plus
# P codes that round the other way where the instruction's fp32 scores differ from the fp64 ones (asserted: the largest x 1.5)
KERNEL_VS_EMULATOR_REL_L2 = 3e-3
# kernel vs exact fp64 attention on the original bf16 q / k / v: e4m3 q / k move these (large: std 2.25) logits by a few percent, which
# dominates. Measured 1.005e-1 / 9.09e-2 / 9.00e-2 (asserted: the largest x 1.5)
KERNEL_VS_EXACT_REL_L2 = 1.5e-1
# fp8 tier + fp8_attention vs the accurate tier, full depth OMGSR-F 256 -> 1024, draw 0: measured rel-L2 6.65e-2, PSNR 33.40 dB on MI355X
# (the fp8 tier alone: 6.61e-2 / 33.45 dB) x 1.25; the target is >= 30 dB
FP8_ATTN_VS_ACCURATE_REL_L2 = 8.3e-2
FP8_ATTN_VS_ACCURATE_PSNR = 30.0


@pytest.fixture(autouse=True)
def _bf16_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _rup(x, m):
    return (x + m - 1) // m * m


def _operands(B, Bk, H, Lq, Lk, seed, ld=None):
    """bf16 q [B, Lq, H D], k [Bk, Lk, H D], V^T [Bk, H D, ld] (zero columns >= Lk) with per-32-key magnitudes of V spread over 2^+-3, and
    their MXFP8 forms."""
    from omgsr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(seed)
    ld = ld or _rup(Lk, 128)
    q = (torch.randn(B, Lq, H * D, generator=g, device=DEV) * 1.5).to(torch.bfloat16)
    k = (torch.randn(Bk, Lk, H * D, generator=g, device=DEV) * 1.5).to(torch.bfloat16)
    v = torch.randn(Bk, H * D, Lk, generator=g, device=DEV)
    nb = (Lk + 31) // 32
    spread = torch.exp2(torch.randint(-3, 4, (Bk, H * D, nb), generator=g, device=DEV).float()).repeat_interleave(32, -1)[..., :Lk]
    vt = torch.zeros(Bk, H * D, ld, device=DEV, dtype=torch.bfloat16)
    vt[..., :Lk] = (v * spread).to(torch.bfloat16)
    return (q, k, vt), (ops.quantize_mxfp8(q), ops.quantize_mxfp8(k), ops.quantize_mxfp8(vt))


def _heads(x, H):          # [B, L, H D] -> [B, H, L, D]
    return x.reshape(x.shape[0], x.shape[1], H, D).permute(0, 2, 1, 3)


def _emulate(mq, mk, mvt, H, Lk, B):
    from omgsr_amd.testing import mxfp8_attention_ref, mxfp8_dequant
    q = _heads(mxfp8_dequant(mq.codes, mq.scales), H)
    k = _heads(mxfp8_dequant(mk.codes, mk.scales), H)
    vt = mxfp8_dequant(mvt.codes, mvt.scales).reshape(mvt.codes.shape[0], H, D, -1)
    k, vt = k.expand(B, -1, -1, -1), vt.expand(B, -1, -1, -1)
    return mxfp8_attention_ref(q, k, vt, D ** -0.5, Lk=Lk)                 # [B, H, Lq, D]


def _exact(q, k, vt, H, Lk, B):
    """fp64 softmax attention of the original bf16 operands, head by head: [B, H, Lq, D]."""
    qh, kh = _heads(q.double(), H), _heads(k.double(), H).expand(B, -1, -1, -1)
    vh = vt.double().reshape(vt.shape[0], H, D, -1)[..., :Lk].transpose(-1, -2).expand(B, -1, -1, -1)
    out = torch.empty(*qh.shape, dtype=torch.float64, device=DEV)
    for h in range(H):
        s = (qh[:, h] @ kh[:, h, :Lk].transpose(-1, -2)) * D ** -0.5
        out[:, h] = torch.softmax(s, -1) @ vh[:, h]
    return out


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.mark.parametrize("name,B,Bk,H,Lq,Lk", [("self_4608", 2, 2, 24, 4608, 4608), ("ragged_1000", 2, 2, 4, 1000, 1000),
                                               ("broadcast", 3, 1, 2, 333, 777)])
def test_kernel_vs_emulator_and_exact(name, B, Bk, H, Lq, Lk):
    from omgsr_amd import ops
    (q, k, vt), (mq, mk, mvt) = _operands(B, Bk, H, Lq, Lk, Lq + Lk + H)
    o = ops.attention(mq, mk, mvt, H, D, D ** -0.5, Lk=Lk)
    assert o.dtype == torch.bfloat16 and o.shape == (B, Lq, H * D)
    got = _heads(o, H)
    emu = _emulate(mq, mk, mvt, H, Lk, B)
    e_emu, e_emu16 = _rel(got, emu), _rel(got, emu.to(torch.bfloat16).double())
    e_exact = _rel(got, _exact(q, k, vt, H, Lk, B))
    print(f"{name}: rel-L2 vs emulator {e_emu:.3e} (vs the emulator rounded to bf16 {e_emu16:.3e}), vs exact fp64 attention {e_exact:.3e}")
    assert torch.isfinite(o.float()).all()
    assert e_emu <= KERNEL_VS_EMULATOR_REL_L2, (e_emu, e_emu16)
    assert e_exact <= KERNEL_VS_EXACT_REL_L2, e_exact


def _mx(codes, scales):
    from omgsr_amd import ops
    return ops.Mxfp8(codes.to(DEV).contiguous(), scales.to(DEV).contiguous())


def test_lane_map_one_hot_pv():
    """Direct probe of the PV product's operand / scale lane map: q = 0 makes every probability 1 (code 2^8), and channel d of V^T holds ONE
    nonzero code, at key 37 d mod 128 (every key slot of both tiles once), under a scale that differs from block to block and from channel to
    channel. O[., d] must be exactly that value / 128: a slot, lane half or scale block taken from the wrong place changes it."""
    from omgsr_amd import ops
    Lq, Lk, ld = 64, 128, 128
    mq = _mx(torch.zeros(1, Lq, D, dtype=torch.uint8), torch.zeros(1, Lq, D // 32, dtype=torch.uint8))
    mk = _mx(torch.zeros(1, Lk, D, dtype=torch.uint8), torch.zeros(1, Lk, D // 32, dtype=torch.uint8))
    codes = torch.zeros(1, D, ld, dtype=torch.uint8)
    scales = torch.tensor([[124 + (d + 3 * blk) % 7 for blk in range(ld // 32)] for d in range(D)], dtype=torch.uint8)[None]
    want = torch.empty(D, dtype=torch.float64)
    for d in range(D):
        key, code = (37 * d) % Lk, 0x38 + d % 8                             # 1.0 ... 1.875
        codes[0, d, key] = code
        want[d] = (1.0 + (d % 8) / 8) * 2.0 ** (int(scales[0, d, key // 32]) - 127) / Lk
    o = ops.attention(mq, mk, _mx(codes, scales), 1, D, D ** -0.5)
    assert torch.equal(o[0].float().cpu(), want.float().expand(Lq, D))


def test_lane_map_one_hot_qk():
    """Direct probe of the QK product's map: V^T = identity (O[., j] = P_j), k row j one-hot at head-dim position 53 j mod 128 under a scale
    that varies per row and block, q all ones under per-block scales - so key j's score is 2^(its two scale exponents). The kernel must match
    its restatement; a K / Q slot or scale taken from the wrong lane moves a score by a power of two."""
    from omgsr_amd import ops
    from omgsr_amd.testing import mxfp8_attention_ref, mxfp8_dequant
    Lq, Lk = 64, 128
    qc = torch.full((1, Lq, D), 0x38, dtype=torch.uint8)
    qs = torch.tensor([127, 126, 125, 124], dtype=torch.uint8).expand(1, Lq, 4)
    kc = torch.zeros(1, Lk, D, dtype=torch.uint8)
    ks = torch.tensor([[125 + (j + blk) % 3 for blk in range(4)] for j in range(Lk)], dtype=torch.uint8)[None]
    for j in range(Lk):
        kc[0, j, (53 * j) % D] = 0x38
    vc = torch.zeros(1, D, Lk, dtype=torch.uint8)
    vc[0, torch.arange(D), torch.arange(D)] = 0x38
    vs = torch.full((1, D, Lk // 32), 127, dtype=torch.uint8)
    mq, mk, mvt = _mx(qc, qs), _mx(kc, ks), _mx(vc, vs)
    o = ops.attention(mq, mk, mvt, 1, D, 4.0)[0].double().cpu()
    ref = mxfp8_attention_ref(mxfp8_dequant(qc, qs)[0], mxfp8_dequant(kc, ks)[0], mxfp8_dequant(vc, vs)[0], 4.0)
    assert float(ref.max() / ref.min()) > 30                                # scores spread over > 3 binades of probability
    assert float((o - ref).abs().max() / ref.abs().max()) <= 2 ** -8        # bf16 rounding of the output, nothing more


def test_constant_v_comes_out_unchanged():
    from omgsr_amd import ops
    B, H, L = 2, 3, 700
    (q, k, _), (mq, mk, _) = _operands(B, B, H, L, L, 41)
    c = torch.tensor([(-1) ** d * (1.0 + (d % 7) / 8) * 2.0 ** (d % 5 - 2) for d in range(H * D)], device=DEV)   # exact in e4m3 under its scale
    vt = torch.zeros(B, H * D, _rup(L, 128), device=DEV, dtype=torch.bfloat16)
    vt[..., :L] = c[None, :, None].to(torch.bfloat16)
    o = ops.attention(mq, mk, ops.quantize_mxfp8(vt), H, D, D ** -0.5)
    assert torch.equal(o, c.to(torch.bfloat16).expand(B, L, -1))


def test_masked_keys_never_reach_the_result():
    from omgsr_amd import ops
    B, H, Lq, Lk, rows = 2, 2, 300, 1000, 1100
    (_, k, vt), (mq, mk, mvt) = _operands(B, B, H, Lq, Lk, 43)
    clean = ops.attention(mq, mk, mvt, H, D, D ** -0.5, Lk=Lk)
    codes = torch.full((B, rows, H * D), 0x7F, device=DEV, dtype=torch.uint8)          # NaN codes in every k row >= Lk ...
    scales = torch.full((B, rows, H * D // 32), 0xFF, device=DEV, dtype=torch.uint8)  # ... and NaN scales
    codes[:, :Lk], scales[:, :Lk] = mk.codes, mk.scales
    codes[:, Lk + 1::3] = torch.randint(0, 256, codes[:, Lk + 1::3].shape, device=DEV, dtype=torch.uint8)
    mk2 = ops.Mxfp8(codes, scales)
    vc, vs = mvt.codes.clone(), mvt.scales.clone()
    vc[..., Lk:] = 0x7F                                                                # NaN V^T codes past Lk
    vc[..., Lk + 5::7] = 0xFE
    vs[..., _rup(Lk, 32) // 32:] = 0xFF                                               # blocks wholly past Lk: NaN scales
    got = ops.attention(mq, mk2, ops.Mxfp8(vc, vs), H, D, D ** -0.5, Lk=Lk)
    assert torch.equal(got, clean)


def test_repeatable_and_batch_invariant():
    from omgsr_amd import ops
    B, H, L = 2, 4, 1111
    _, (mq, mk, mvt) = _operands(B, B, H, L, L, 47)
    first = ops.attention(mq, mk, mvt, H, D, D ** -0.5)
    for _ in range(19):
        assert torch.equal(ops.attention(mq, mk, mvt, H, D, D ** -0.5), first)
    ops.set_batch_invariant(True)
    try:
        ab = ops.attention(mq, mk, mvt, H, D, D ** -0.5)
        one = lambda m, b: ops.Mxfp8(m.codes[b:b + 1].contiguous(), m.scales[b:b + 1].contiguous())      # noqa: E731
        for b in range(B):
            assert torch.equal(ops.attention(one(mq, b), one(mk, b), one(mvt, b), H, D, D ** -0.5)[0], ab[b])
    finally:
        ops.set_batch_invariant(False)


def _rms_rope_ref(x, w, w2, split_at, cos, sin, eps=1e-6):
    """fp32 torch statement of omgsr_rmsnorm_rope over every head of x [B, L, nh D]."""
    B, L, C_ = x.shape
    f = x.float().reshape(B, L, C_ // D, D)
    r = torch.rsqrt((f * f).mean(-1, keepdim=True) + eps)
    wt = torch.where((torch.arange(L, device=DEV) >= split_at)[None, :, None, None], w2[None, None], w[None, None])
    f = f * r * wt
    a, b = f[..., 0::2], f[..., 1::2]
    c, s = cos[:L, None, :], sin[:L, None, :]
    out = torch.empty_like(f)
    out[..., 0::2] = a * c[..., 0::2] - b * s[..., 0::2]
    out[..., 1::2] = b * c[..., 1::2] + a * s[..., 1::2]
    return out.reshape(B, L, C_)


def test_rmsnorm_rope_mxfp8_matches_quantised_fp32_statement():
    from omgsr_amd import ops
    B, L, H, Lc = 2, 333, 3, 40
    g = torch.Generator(device=DEV).manual_seed(53)
    x = (torch.randn(B, L, 2 * H * D, generator=g, device=DEV) * 3).to(torch.bfloat16)
    w = torch.rand(2 * H, D, generator=g, device=DEV) + 0.5
    w2 = torch.rand(2 * H, D, generator=g, device=DEV) + 0.5
    ang = torch.rand(L, D // 2, generator=g, device=DEV) * 6.3
    cos, sin = torch.cos(ang).repeat_interleave(2, -1).contiguous(), torch.sin(ang).repeat_interleave(2, -1).contiguous()
    x0 = x.clone()
    got = ops.rmsnorm_rope_mxfp8(x, w, cos, sin, 2 * H, D, w_after=w2, split_at=Lc)
    assert torch.equal(x, x0)                                                # the bf16 input is read only
    ref32 = _rms_rope_ref(x, w, w2, Lc, cos, sin)
    want = ops.quantize_mxfp8(ref32)
    # scales: equal except where a block's maximum sits within fp32 rounding of a power of two
    blk = ref32.reshape(B, L, -1, 32).abs().amax(-1)
    near = (blk / torch.exp2(torch.round(torch.log2(blk))) - 1).abs() < 1e-5
    same = got.scales == want.scales
    assert bool((same | near).all()) and float(same.float().mean()) > 0.999
    # codes: at most one unit in the last place apart (signed ordinals of e4m3 are consecutive), on blocks of equal scale
    ordn = lambda c: torch.where(c >= 128, -(c.int() - 128), c.int())      # noqa: E731
    d = (ordn(got.codes) - ordn(want.codes)).abs().reshape(B, L, -1, 32)[same]
    assert int(d.max()) <= 1
    # the bf16 in-place path stays what it was: fp32 math, one rounding
    y = ops.rmsnorm_rope_(x.clone(), w, cos, sin, 2 * H, D, w_after=w2, split_at=Lc)
    assert _rel(y, ref32.double()) < 4e-3


def test_refusals():
    from omgsr_amd import _lib, ops
    from omgsr_amd._lib import AttnArgs
    _, (mq, mk, mvt) = _operands(1, 1, 2, 128, 256, 59)
    with pytest.raises(ValueError):
        ops.attention(mq, mk, mvt, 4, 64, 0.125)                            # head_dim 64
    bad = ops.quantize_mxfp8(torch.zeros(1, 2 * D, 384, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.attention(mq, mk, ops.Mxfp8(bad.codes[..., :320].contiguous(), bad.scales[..., :10].contiguous()), 2, D, 0.1, Lk=256)   # ld % 128 != 0
    with pytest.raises(ValueError):
        ops.attention(mq, mk, torch.zeros(1, 2 * D, 256, device=DEV, dtype=torch.bfloat16), 2, D, 0.1)  # mixed forms
    ops.set_compute_dtype(torch.float16)
    with pytest.raises(ValueError):
        ops.attention(mq, mk, mvt, 2, D, 0.1)
    ops.set_compute_dtype(torch.bfloat16)
    # the C entry point itself
    o = torch.empty(1, 128, 2 * D, device=DEV, dtype=torch.bfloat16)
    a = AttnArgs()
    a.qkv_el = ops.EL_MXFP8
    a.q, a.k, a.vt, a.o = mq.codes.data_ptr(), mk.codes.data_ptr(), mvt.codes.data_ptr(), o.data_ptr()
    a.q_scale, a.k_scale, a.vt_scale = mq.scales.data_ptr(), mk.scales.data_ptr(), mvt.scales.data_ptr()
    a.B, a.H, a.D, a.Lq, a.Lk = 1, 2, D, 128, 256
    a.q_ld = a.k_ld = 2 * D
    a.vt_ld, a.o_ld = 256, 2 * D
    a.q_sld = a.k_sld = 2 * D // 32
    a.vt_sld = 8
    a.scale = 0.1
    lib = _lib.load()
    assert lib.omgsr_attention(C.byref(a), ops._stream()) == 0
    a.D, a.H = 64, 4
    assert lib.omgsr_attention(C.byref(a), ops._stream()) == -2            # OMGSR_E_SHAPE
    a.D, a.H = D, 2
    a.vt_ld = 320
    assert lib.omgsr_attention(C.byref(a), ops._stream()) == -2
    a.vt_ld = 256
    a.o_mx = 1
    assert lib.omgsr_attention(C.byref(a), ops._stream()) == -2
    a.o_mx = 0
    ops.set_compute_dtype(torch.float16)
    try:
        assert lib.omgsr_attention(C.byref(a), ops._stream()) == -2
    finally:
        ops.set_compute_dtype(torch.bfloat16)


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


def _pipe(vae, flux, policy=None):
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    return OMGSR_F_Infer(None, None, DEV, torch.float8_e4m3fn, 244, 1.0, vae=vae, flux_transformer=flux, precision_policy=policy)


def _call(pipe, inp, x, n):
    pipe.vae.posterior_noise = n
    return pipe(x, inp["pe"], inp["pooled"], inp["tids"], inp["iids"], 16, 8)[0]


ATTN = {"flux": {"fp8_attention": True}}


def test_pipeline_small_case():
    from omgsr_amd import _lib, ops
    from omgsr_amd.precision import FLUX_FP8, fp8_attention_blocks
    vae, flux, inp = _small_case()
    x, n = inp["xs"][0], inp["ns"][0]
    with torch.no_grad():
        y0 = _call(_pipe(vae, flux), inp, x, n)                              # the fp8 tier as it was
        pipe = _pipe(vae, flux, ATTN)
        assert len(fp8_attention_blocks(flux)) == 4
        lib = _lib.load()
        lib.omgsr_timing_enable(1); lib.omgsr_timing_reset()
        y8 = _call(pipe, inp, x, n)
        buf = (_lib.TimingEntry * 4096)()
        cnt = lib.omgsr_timing_collect(buf, 4096)
        lib.omgsr_timing_enable(0)
        attn = [e for e in buf[:cnt] if e.kind == 2]
        assert len(attn) == 4 and all(e.variant == 19 for e in attn)       # one mxfp8_attn_kernel launch per block, no bf16 attention
        assert torch.isfinite(y8.float()).all() and not torch.equal(y8, y0)
        assert float((y8.float() - y0.float()).norm() / y0.float().norm()) < 0.1
        # batch invariance
        ops.set_batch_invariant(True)
        try:
            a = _call(pipe, inp, inp["xs"][1], inp["ns"][1])
            b = _call(pipe, inp, inp["xs"][2], inp["ns"][2])
            ab = _call(pipe, inp, torch.cat(inp["xs"][1:]), torch.cat(inp["ns"][1:]))
        finally:
            ops.set_batch_invariant(False)
        assert torch.equal(ab[0:1], a) and torch.equal(ab[1:2], b)
        # graph replay == eager
        eager = [_call(pipe, inp, xx, n) for xx in inp["xs"]]
        pipe.enable_graphs(True)
        got = [_call(pipe, inp, xx, n) for xx in inp["xs"]]
        assert pipe.graphs.captures == 1 and pipe.graphs.replays == 2
        for e, g in zip(eager, got):
            assert torch.equal(e, g)
        # without the key the fp8 tier is bit-identical to what it was (the key's marks are cleared on the shared modules)
        assert torch.equal(_call(_pipe(vae, flux), inp, x, n), y0)
        assert fp8_attention_blocks(flux) == []
        assert torch.equal(_call(_pipe(vae, flux, {"flux": {"fp8": FLUX_FP8}}), inp, x, n), y0)
        # per-block patterns: the named blocks only
        p1 = _pipe(vae, flux, {"flux": {"fp8_attention": [r"^single_transformer_blocks\.1$"]}})
        lib.omgsr_timing_enable(1); lib.omgsr_timing_reset()
        y1 = _call(p1, inp, x, n)
        cnt = lib.omgsr_timing_collect(buf, 4096)
        lib.omgsr_timing_enable(0)
        assert [e.variant for e in buf[:cnt] if e.kind == 2] == [0, 0, 0, 19]
        assert not torch.equal(y1, y0) and not torch.equal(y1, y8)


def test_fp8_attention_full_depth_f1024_vs_accurate_tier():
    """Full depth (19 + 38 blocks, FLUX.1-dev width), OMGSR-F 256 -> 1024, batch 1, seeded weights generated on the device (as
    test_fp8_gpu.py's full-depth test): the fp8 tier with fp8_attention against the accurate tier. Further draws: OMGSR_FLUX_DRAW=1, 2."""
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

    def run(wd, policy=None):
        pv = AutoencoderKL(**FLUX_VAE_CONFIG)
        pv.load_state_dict(vae_sd)
        pipe = OMGSR_F_Infer(None, None, DEV, wd, 244, 1.0, vae=pv, flux_transformer=pf, precision_policy=policy)
        pipe.vae.posterior_noise = eps
        cd = torch.float32 if wd == torch.float32 else torch.bfloat16
        with torch.no_grad():
            return pipe(x.to(cd), pe.to(cd), pooled.to(cd), tids.to(cd), iids.to(cd), 128, 64)[0].float()

    ref = run(torch.float32)
    y8 = run(torch.float8_e4m3fn)
    ya = run(torch.float8_e4m3fn, ATTN)
    e8, p8 = rel_l2(y8, ref), psnr(y8, ref)
    ea, pa = rel_l2(ya, ref), psnr(ya, ref)
    print(f"draw {draw}: fp8 tier + fp8_attention vs accurate tier rel-L2 {ea:.4e} PSNR {pa:.2f} dB; fp8 tier {e8:.4e} / {p8:.2f} dB")
    assert torch.isfinite(ya).all()
    assert ea <= FP8_ATTN_VS_ACCURATE_REL_L2 and pa >= FP8_ATTN_VS_ACCURATE_PSNR, (ea, pa)
