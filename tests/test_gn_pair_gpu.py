"""GroupNorm of a channel concatenation without the concatenation (the UNet's up path in the accurate tier): statistics folded from the
per-channel partials of the two producers (omgsr_groupnorm_finalize2) and an apply pass that reads the two tensors
(omgsr_groupnorm_apply2), at the UNet's real channel pairs; the old path where a handle is missing or per group."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 32
PAIRS = [(640, 320), (320, 320), (640, 640), (1280, 640), (1280, 1280)]       # (decoder tensor | skip tensor) of the SD2.1 UNet's up resnets


def _ops():
    from omgsr_amd import ops
    return ops


@pytest.fixture
def accurate():
    ops = _ops()
    ops.set_compute_dtype(torch.float32)
    ops.overflow_seen(); ops.mx_saturation_seen()
    yield ops
    ops.overflow_seen(); ops.mx_saturation_seen()
    ops.set_compute_dtype(torch.bfloat16)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def _halo_producer(ops, N, Cin, Cout, H, W, seed):
    """A 3x3 conv on the halo-tile path: (stream tensor with its statistics handle, fp32 reference NCHW)."""
    x = rnd(N, Cin, H, W, seed=seed)
    w = rnd(Cout, Cin, 3, 3, seed=seed + 1, scale=(9 * Cin) ** -0.5); b = rnd(Cout, seed=seed + 2)
    y = ops.conv2d(nhwc(x), ops.pack_conv_weight(w, b, device=DEV), pad=1, gn_groups=G)
    return y, F.conv2d(x, w, b, padding=1)


def _gemm_producer(ops, N, Cin, Cout, H, W, seed):
    """A linear layer with a residual (the attention block's proj_out) on the GEMM-shaped path, viewed as [N, H, W, C]."""
    x = rnd(N, H * W, Cin, seed=seed)
    w = rnd(Cout, Cin, seed=seed + 1, scale=Cin ** -0.5); b = rnd(Cout, seed=seed + 2)
    r = rnd(N, H * W, Cout, seed=seed + 3)
    y = ops.linear(x.to(DEV), ops.pack_linear_weight(w, b, device=DEV), residual=r.to(DEV), gn_groups=G)
    y4 = ops.carry_gn(y, y.reshape(N, H, W, Cout))
    ref = (F.linear(x, w, b) + r).transpose(1, 2).reshape(N, Cout, H, W)
    return y4, ref


@pytest.mark.parametrize("Ca,Cb", PAIRS)
@pytest.mark.parametrize("kinds", ["halo|gemm", "gemm|halo", "halo|halo"])
def test_two_source_statistics(accurate, Ca, Cb, kinds):
    ops = accurate
    N, H, W = 2, 32, 32
    ka, kb = kinds.split("|")
    make = {"halo": _halo_producer, "gemm": _gemm_producer}
    a, ref_a = make[ka](ops, N, 128, Ca, H, W, 700)
    b, ref_b = make[kb](ops, N, 64, Cb, H, W, 710)
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    for t, c in ((a, Ca), (b, Cb)):
        h = getattr(t, "_omgsr_gn", None)
        assert h is not None and h[0].shape[2] == c, "the producer should have left per-channel statistics"
    st = ops.group_norm_pair_stats(a, b, G, 1e-5)
    assert st is not None, "the two-source path must be taken"
    mean, rstd, var = st
    g = torch.cat([ref_a, ref_b], 1).reshape(N, G, -1)
    em = (mean.cpu() - g.mean(-1)).abs().max().item(); ev = (var.cpu() - g.var(-1, unbiased=False)).abs().max().item()
    cat = ops.concat_channels(a, b)
    assert getattr(cat, "_omgsr_gn", None) is None
    m2, r2, v2 = ops.group_norm_stats(cat, G, 1e-5)
    print(f"{Ca}|{Cb} {kinds}: max |mean - torch| {em:.3e}, max |var - torch| {ev:.3e}; against the read pass: mean {(mean - m2).abs().max().item():.3e}, "
          f"var {(var - v2).abs().max().item():.3e}")
    assert torch.allclose(mean.cpu(), g.mean(-1), atol=3e-3, rtol=3e-3)
    assert torch.allclose(var.cpu(), g.var(-1, unbiased=False), atol=3e-3, rtol=6e-3)
    assert torch.allclose(mean, m2, atol=2e-3, rtol=2e-3) and torch.allclose(var, v2, atol=2e-3, rtol=4e-3)
    assert torch.allclose(rstd, torch.rsqrt(var + 1e-5), rtol=1e-5)
    # the skip's handle is still the down path's: the one-source fold of b alone keeps working
    mb, _, vb = ops.group_norm_stats(b, G, 1e-5)
    gb = ref_b.reshape(N, G, -1)
    assert torch.allclose(mb.cpu(), gb.mean(-1), atol=3e-3, rtol=3e-3) and torch.allclose(vb.cpu(), gb.var(-1, unbiased=False), atol=3e-3, rtol=6e-3)
    assert torch.equal(torch.stack(st), torch.stack(ops.group_norm_pair_stats(a, b, G, 1e-5))), "repeated folds differ"


# (operand form of the normalised tensor, form of the shortcut twin): what the up resnets ask for under the shipped policies
FORMS_F16 = [(1, 1), (2, 2), (3, 3), (4, 3), (2, 1), (1, 2), (3, 2), (4, 2), (3, 1), (4, 1), (1, 0), (2, 0), (3, 0), (4, 0)]
FORMS_BF16 = [(1, 1), (2, 2), (2, 1), (1, 2), (1, 0), (2, 0)]


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("mode", ["accurate", "range-fallback", "mx-saturation"])
def test_two_source_apply_writes_the_bytes_of_the_concatenated_pass(mode):
    """accurate: fp16 operands; range-fallback: bf16 operands (plain / split forms); mx-saturation: fp16 operands with values beyond the
    fp8 correction range (and, last, beyond the fp16 range: the guard word must be raised by both passes alike)."""
    ops = _ops()
    ops.set_compute_dtype(torch.float32, operand_dtype=torch.bfloat16 if mode == "range-fallback" else None)
    try:
        ops.overflow_seen(); ops.mx_saturation_seen()
        gen = torch.Generator(device=DEV).manual_seed(21)
        N = 2
        for (Ca, Cb), hw in zip(PAIRS, (64, 64, 32, 16, 8)):
            amp = 300.0 if mode == "mx-saturation" else 2.0
            a = torch.randn((N, hw, hw, Ca), device=DEV, generator=gen) * amp + 0.3
            b = torch.randn((N, hw, hw, Cb), device=DEV, generator=gen) * amp * 0.5 - 0.2
            mean = torch.randn((N, G), device=DEV, generator=gen) * 0.3
            rstd = (torch.rand((N, G), device=DEV, generator=gen) + 0.2) / amp
            gamma, beta = torch.randn(Ca + Cb, device=DEV, generator=gen) + 1.0, torch.randn(Ca + Cb, device=DEV, generator=gen)
            cat = ops.concat_channels(a, b)
            for split, twin in (FORMS_BF16 if mode == "range-fallback" else FORMS_F16):
                ref = ops.group_norm_apply(cat, mean, rstd, gamma, beta, G, ops.ACT_SILU, split=split, also_cast=twin)
                sat_ref = ops.mx_saturation_seen()
                got = ops.group_norm_apply_pair(a, b, mean, rstd, gamma, beta, G, ops.ACT_SILU, split=split, also_cast=twin)
                sat_got = ops.mx_saturation_seen()
                for name, r, g2 in zip(("y", "y2"), ref if twin else (ref,), got if twin else (got,)):
                    assert _same_bytes(r, g2), f"{mode} {Ca}|{Cb} split {split} twin {twin}: {name} differs"
                assert sat_ref == sat_got == (mode == "mx-saturation" and twin == 3), (mode, split, twin, sat_ref, sat_got)
            assert not ops.overflow_seen()
        if mode == "mx-saturation":            # a value beyond the fp16 range in each half in turn: both passes raise the guard word
            for which in (0, 1):
                a2, b2 = a.clone(), b.clone()
                (a2, b2)[which][1, 3, 2, 5] = 7.0e4
                cat = ops.concat_channels(a2, b2)
                ref = ops.group_norm_apply(cat, mean, rstd, gamma, beta, G, ops.ACT_NONE, split=2, also_cast=2)
                assert ops.overflow_seen()
                got = ops.group_norm_apply_pair(a2, b2, mean, rstd, gamma, beta, G, ops.ACT_NONE, split=2, also_cast=2)
                assert ops.overflow_seen()
                assert _same_bytes(ref[0], got[0]) and _same_bytes(ref[1], got[1])
    finally:
        ops.overflow_seen(); ops.mx_saturation_seen()
        ops.set_compute_dtype(torch.bfloat16)


def test_old_path_when_a_handle_is_missing_or_per_group(accurate):
    ops = accurate
    N, H, W = 2, 32, 32
    gamma, beta = (rnd(960, seed=730) + 1.0).to(DEV), rnd(960, seed=731).to(DEV)
    a, ref_a = _halo_producer(ops, N, 128, 640, H, W, 700)
    b, ref_b = _halo_producer(ops, N, 64, 320, H, W, 710)
    ref = F.silu(F.group_norm(torch.cat([ref_a, ref_b], 1), G, gamma.cpu(), beta.cpu(), eps=1e-5))

    def close(y, name):
        e = ((y.float().cpu().permute(0, 3, 1, 2) - ref).norm() / ref.norm()).item()
        print(f"{name}: rel-L2 {e:.3e}")
        assert e < 6e-3, name         # the bound test_fused_groupnorm_statistics_all_paths sets for a GroupNorm on producer-side statistics

    close(ops.group_norm_pair(a, b, gamma, beta, G, 1e-5, ops.ACT_SILU), "two-source")
    # no handle on one side (a copy: what a split-K producer leaves)
    a_plain = a.clone()
    assert ops.group_norm_pair_stats(a_plain, b, G, 1e-5) is None and ops.group_norm_pair_stats(b, a_plain, G, 1e-5) is None
    y_old = ops.group_norm_pair(a_plain, b, gamma, beta, G, 1e-5, ops.ACT_SILU)
    close(y_old, "old path (missing handle)")
    assert _same_bytes(y_old, ops.group_norm(ops.concat_channels(a_plain, b), gamma, beta, G, 1e-5, ops.ACT_SILU))
    # per-group partials (group size 8: 256 channels in 32 groups) cannot be regrouped: old path
    c, ref_c = _halo_producer(ops, N, 64, 256, H, W, 720)
    d, ref_d = _halo_producer(ops, N, 64, 256, H, W, 724)
    assert c._omgsr_gn is not None and c._omgsr_gn[0].shape[2] == G, "group size 8 leaves per-group partials"
    assert ops.group_norm_pair_stats(c, d, G, 1e-5) is None
    g2, b2 = (rnd(512, seed=732) + 1.0).to(DEV), rnd(512, seed=733).to(DEV)
    y = ops.group_norm_pair(c, d, g2, b2, G, 1e-5, ops.ACT_NONE)
    assert _same_bytes(y, ops.group_norm(ops.concat_channels(c, d), g2, b2, G, 1e-5, ops.ACT_NONE))
    ref2 = F.group_norm(torch.cat([ref_c, ref_d], 1), G, g2.cpu(), b2.cpu(), eps=1e-5)
    assert ((y.float().cpu().permute(0, 3, 1, 2) - ref2).norm() / ref2.norm()).item() < 6e-3
    # a 16-bit tier: the concatenated tensor is the shortcut's operand, nothing changes
    ops.set_compute_dtype(torch.float16)
    x16, y16 = torch.randn((1, 8, 8, 64), device=DEV).half(), torch.randn((1, 8, 8, 64), device=DEV).half()
    assert ops.group_norm_pair_stats(x16, y16, G, 1e-5) is None
    assert _same_bytes(ops.group_norm_pair(x16, y16, None, None, G, 1e-5), ops.group_norm(ops.concat_channels(x16, y16), None, None, G, 1e-5))
