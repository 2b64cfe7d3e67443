"""The fp8 tier's MXFP8 attention without a GPU: the `fp8_attention` policy (parsed, validated, resolved to blocks on the full-size FLUX.1-dev
module tree built on the meta device), the invariants of the kernel's torch restatement (omgsr_amd.testing.mxfp8_attention_ref) and the
compiler's resource figures of the new kernels."""
import os
import shutil

import pytest
import torch

from omgsr_amd.testing import mxfp8_attention_ref, mxfp8_dequant, mxfp8_ref


def _meta_flux():
    from omgsr_amd.diffusers_api import FluxTransformer2DModel
    with torch.device("meta"):
        return FluxTransformer2DModel()


def test_fp8_attention_patterns_resolve_to_blocks():
    from omgsr_amd.precision import clear_fp8_attention, fp8_attention_blocks, set_fp8_attention
    m = _meta_flux()
    assert fp8_attention_blocks(m) == []                                    # nothing is marked by default
    assert set_fp8_attention(m, True) == 19 + 38
    assert set(fp8_attention_blocks(m)) == {f"transformer_blocks.{i}" for i in range(19)} | {f"single_transformer_blocks.{i}" for i in range(38)}
    n = set_fp8_attention(m, [r"^transformer_blocks\.(0|18)$", r"^single_transformer_blocks\.3\d$"])
    assert set(fp8_attention_blocks(m)) == {"transformer_blocks.0", "transformer_blocks.18"} | {f"single_transformer_blocks.{i}" for i in range(30, 38)}
    assert n == 10
    assert m.transformer_blocks[0].attn.fp8 and not m.transformer_blocks[1].attn.fp8 and m.single_transformer_blocks[37].attn.fp8
    clear_fp8_attention(m)
    assert fp8_attention_blocks(m) == []
    with pytest.raises(ValueError):
        set_fp8_attention(m, r"^transformer_blocks\.0$")                    # a bare string is not a list of patterns
    for bad in (1, None, [1], [r"^transformer_block\.3$"], [r"^transformer_blocks\.0$", r"^single_transformer_blocks\.38$"]):
        with pytest.raises(ValueError):                                     # not a list of strings / a pattern that names no block
            set_fp8_attention(m, bad)
    assert fp8_attention_blocks(m) == []                                    # a refused call marks nothing


def test_fp8_attention_policy_is_fp8_tier_only(monkeypatch):
    from omgsr_amd import ops
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    from omgsr_amd.precision import set_fp8_attention
    pol = {"flux": {"fp8_attention": True}}
    for wd in (torch.bfloat16, torch.float16, torch.float32):
        with pytest.raises(ValueError):
            OMGSR_F_Infer(None, None, "cpu", wd, precision_policy=pol)
    with pytest.raises(ValueError):
        OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy={"unet": {"fp8_attention": True}})
    with pytest.raises(ValueError):                                         # an unknown key of the fp8 tier's policy
        OMGSR_F_Infer(None, None, "cpu", torch.float8_e4m3fn, precision_policy={"flux": {"fp8_attn": True}})
    m = _meta_flux()
    monkeypatch.setattr(ops, "_PRECISE", True)
    with pytest.raises(ValueError):
        set_fp8_attention(m, True)
    monkeypatch.setattr(ops, "_PRECISE", False)
    monkeypatch.setattr(ops, "_ACT", torch.float16)
    with pytest.raises(ValueError):
        set_fp8_attention(m, True)


def test_fp8_tier_policy_marks_attention_only_with_the_key(monkeypatch):
    """The pipeline's policy handling on meta modules (vae / transformer injected; nothing runs): the key marks the named blocks, its absence
    marks none and a pipeline of another tier unmarks what an earlier fp8-tier pipeline marked."""
    from omgsr_amd import ops
    from omgsr_amd.pipelines import omgsr_f
    from omgsr_amd.precision import fp8_attention_blocks

    class _Vae(torch.nn.Module):
        config = type("cfg", (), {"block_out_channels": [1, 2, 3, 4]})()

    flux = _meta_flux()
    monkeypatch.setattr(ops, "set_compute_dtype", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_PRECISE", False)
    monkeypatch.setattr(ops, "_ACT", torch.bfloat16)
    mk = lambda wd, pol=None: omgsr_f.OMGSR_F_Infer(None, None, "meta", wd, vae=_Vae(), flux_transformer=flux, precision_policy=pol)  # noqa: E731
    mk(torch.float8_e4m3fn, {"flux": {"fp8_attention": [r"^single_transformer_blocks\.(0|1)$"]}})
    assert fp8_attention_blocks(flux) == ["single_transformer_blocks.0", "single_transformer_blocks.1"]
    mk(torch.float8_e4m3fn, {"flux": {"fp8": [r"ff\.net"]}})
    assert fp8_attention_blocks(flux) == []
    mk(torch.float8_e4m3fn, {"flux": {"fp8_attention": True}})
    assert len(fp8_attention_blocks(flux)) == 57
    mk(torch.bfloat16)
    assert fp8_attention_blocks(flux) == []


def _quantised(shape, seed, spread=0):
    """An MXFP8 operand's dequantised values: randn (per-32-block magnitudes spread over 2^+-spread)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if spread:
        x = x * torch.exp2(torch.randint(-spread, spread + 1, (*shape[:-1], shape[-1] // 32, 1), generator=g).float()).repeat_interleave(32, -1).reshape(shape)
    return mxfp8_dequant(*mxfp8_ref(x))


def test_emulator_constant_v_returns_the_constant():
    Lq, Lk, D = 70, 200, 128
    q = _quantised((Lq, D), 1) * 2.0
    k = _quantised((Lk, D), 2) * 2.0
    c = torch.tensor([2.0 ** (i % 7 - 3) * (1.0 + (i % 8) / 8) * (-1) ** i for i in range(D)], dtype=torch.float64)   # exact in e4m3
    vt = c[:, None].expand(D, 256).contiguous()
    o = mxfp8_attention_ref(q, k, vt, D ** -0.5, Lk=Lk)
    assert torch.allclose(o, c.expand(Lq, D), rtol=1e-12, atol=0)


def test_emulator_masked_keys_have_no_effect_and_codes_stay_in_range():
    Lq, Lk, D = 64, 150, 128
    q, k, vt = _quantised((Lq, D), 3, 3) * 4.0, _quantised((256, D), 4, 3) * 4.0, _quantised((D, 256), 5, 4)
    stats = {}
    o = mxfp8_attention_ref(q, k, vt, D ** -0.5, Lk=Lk, stats=stats)
    k2, vt2 = k.clone(), vt.clone()
    k2[Lk:] = 1e6
    vt2[:, Lk:] = -3e5
    assert torch.equal(mxfp8_attention_ref(q, k2, vt2, D ** -0.5, Lk=Lk), o)
    assert torch.equal(mxfp8_attention_ref(q, k[:Lk], vt[:, :Lk], D ** -0.5), o)
    assert 0 < stats["max_code"] <= 448
    # close to exact softmax attention on the same (dequantised) operands: only P's 3-bit mantissa separates them
    s = (q @ k[:Lk].T) * D ** -0.5
    exact = torch.softmax(s, -1) @ vt[:, :Lk].T
    assert float((o - exact).norm() / exact.norm()) < 2e-2


def _kernel_resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import kernel_resources
    return kernel_resources()


def test_mxfp8_attention_kernel_resources():
    res = _kernel_resources()
    k = [v for name, v in res.items() if "mxfp8_attn_kernel" in name]
    assert len(k) == 1, sorted(res)
    k = k[0]
    # designed for two workgroups of 4 waves per CU (2 waves / SIMD, 32 KB of LDS each): 214 VGPRs at the time of writing
    assert k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["scratch"] == 0 and k["occupancy"] >= 2, k
    r = [v for name, v in res.items() if "rmsnorm_rope_mxfp8_kernel" in name]
    assert len(r) == 1 and r[0]["spill_vgpr"] == 0 and r[0]["scratch"] == 0, r
