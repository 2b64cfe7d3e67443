"""The fp8 tier's opt-in VAE convolutions without a GPU: the layer policy (precision.set_fp8_conv / VAE_FP8 on the full-size FLUX VAE, built on
the meta device), the pipeline's handling of the "vae" policy key, the compiler's resource figures of mxfp8_conv_kernel, the timing-variant
constraint on igemm.hip, and the restatement the GPU probes compare against (its data stay in budget; every border tap matters)."""
import os
import re
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = 21


def _meta_vae():
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
    with torch.device("meta"):
        return AutoencoderKL(**FLUX_VAE_CONFIG)


def _meta_flux():
    from omgsr_amd.diffusers_api import FluxTransformer2DModel
    with torch.device("meta"):
        return FluxTransformer2DModel(num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=2, joint_attention_dim=64,
                                      pooled_projection_dim=32, in_channels=64)


@pytest.fixture
def bf16(monkeypatch):
    from omgsr_amd import ops
    monkeypatch.setattr(ops, "set_compute_dtype", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_PRECISE", False)
    monkeypatch.setattr(ops, "_ACT", torch.bfloat16)
    return monkeypatch


def test_policy_marks_exactly_the_resnet_convs(bf16):
    from omgsr_amd.nn import Conv2d
    from omgsr_amd.precision import VAE_FP8, VAE_FP8_ELIGIBLE, clear_fp8_conv, fp8_conv_layers, set_fp8_conv
    vae = _meta_vae()
    assert VAE_FP8, "VAE_FP8 is empty: `True` would be refused (DESIGN.md 3.4 would have to say so)"
    assert all(any(re.search(p, n) for p in VAE_FP8_ELIGIBLE) for n, m in vae.named_modules() if any(re.search(q, n) for q in VAE_FP8))
    n = set_fp8_conv(vae, True)
    names = set(fp8_conv_layers(vae))
    want = {f"encoder.down_blocks.{b}.resnets.{r}.conv{c}" for b in range(4) for r in range(2) for c in (1, 2)}
    want |= {f"decoder.up_blocks.{b}.resnets.{r}.conv{c}" for b in range(4) for r in range(3) for c in (1, 2)}
    want |= {f"{s}.mid_block.resnets.{r}.conv{c}" for s in ("encoder", "decoder") for r in range(2) for c in (1, 2)}
    want = {w for w in want if any(re.search(p, w) for p in VAE_FP8)}
    assert names == want and n == len(want) > 0
    others = [name for name, m in vae.named_modules() if isinstance(m, Conv2d) and name not in want]
    for must_stay in ("encoder.conv_in", "encoder.conv_out", "decoder.conv_in", "decoder.conv_out", "encoder.down_blocks.0.downsamplers.0.conv",
                      "decoder.up_blocks.0.upsamplers.0.conv", "encoder.down_blocks.1.resnets.0.conv_shortcut", "decoder.up_blocks.2.resnets.0.conv_shortcut"):
        assert must_stay in others, must_stay
    # a pattern list narrows; a pattern may also name ineligible layers (they never move) as long as it names an eligible one
    n2 = set_fp8_conv(vae, [r"^decoder\.mid_block\.", r"conv_shortcut$|up_blocks\.3\.resnets\.0\.conv1$"])
    assert set(fp8_conv_layers(vae)) == {f"decoder.mid_block.resnets.{r}.conv{c}" for r in range(2) for c in (1, 2)} | {"decoder.up_blocks.3.resnets.0.conv1"}
    assert n2 == 5
    clear_fp8_conv(vae)
    assert fp8_conv_layers(vae) == []


def test_policy_refusals(bf16):
    from omgsr_amd import ops
    from omgsr_amd.precision import fp8_conv_layers, set_fp8_conv
    vae = _meta_vae()
    for bad in ("all", 1, [], [1], {"x": 1}, False, None):
        with pytest.raises(ValueError):
            set_fp8_conv(vae, bad)
    with pytest.raises(ValueError):                                         # a dead pattern (a typo would otherwise run the plain tier without a word)
        set_fp8_conv(vae, [r"^decoder\.mid_block\.", r"resnet\.9"])
    with pytest.raises(ValueError):                                         # names only layers that are not eligible
        set_fp8_conv(vae, [r"conv_shortcut$"])
    assert fp8_conv_layers(vae) == []                                       # a refused call marks nothing
    bf16.setattr(ops, "_PRECISE", True)
    with pytest.raises(ValueError):
        set_fp8_conv(vae, True)
    bf16.setattr(ops, "_PRECISE", False)
    bf16.setattr(ops, "_ACT", torch.float16)
    with pytest.raises(ValueError):
        set_fp8_conv(vae, True)
    conv = vae.decoder.mid_block.resnets[0].conv1
    with pytest.raises(ValueError):                                         # fp16: the MXFP8 form cannot be packed
        conv.packed_mxfp8()


def test_key_is_fp8_tier_only():
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    pol = {"vae": {"fp8": True}}
    for wd in (torch.bfloat16, torch.float16, torch.float32):
        with pytest.raises(ValueError):
            OMGSR_F_Infer(None, None, "cpu", wd, precision_policy=pol)
    with pytest.raises(ValueError):
        OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy=pol)
    with pytest.raises(ValueError):
        OMGSR_S_Infer(None, None, 273, "cpu", torch.float8_e4m3fn, precision_policy=pol)
    for bad in ({"vae": {"fp8_conv": True}}, {"vae": {"fp8": True, "tiled": True}}, {"vae": True}, {"unet": {"fp8": True}}):
        with pytest.raises(ValueError):                                     # an unknown key of the fp8 tier's policy
            OMGSR_F_Infer(None, None, "cpu", torch.float8_e4m3fn, precision_policy=bad)


def test_pipeline_marks_only_with_the_key_and_refuses_the_tiled_vae(bf16):
    """The pipeline's policy handling on meta modules (nothing runs): the key marks, its absence unmarks what an earlier pipeline marked, another
    tier unmarks too, a dead pattern and a non-list value are refused, and the tiled VAE is refused with the key."""
    from omgsr_amd.pipelines import omgsr_f
    from omgsr_amd.precision import VAE_FP8, fp8_conv_layers
    vae, flux = _meta_vae(), _meta_flux()
    mk = lambda wd, pol=None: omgsr_f.OMGSR_F_Infer(None, None, "meta", wd, vae=vae, flux_transformer=flux, precision_policy=pol)  # noqa: E731
    p = mk(torch.float8_e4m3fn, {"vae": {"fp8": True}})
    marked = fp8_conv_layers(vae)
    assert marked and all(any(re.search(q, n) for q in VAE_FP8) for n in marked)
    with pytest.raises(ValueError, match="tiled VAE"):
        p._init_tiled_vae()
    mk(torch.float8_e4m3fn, {"flux": {"fp8": [r"ff\.net"]}})
    assert fp8_conv_layers(vae) == []
    mk(torch.float8_e4m3fn, {"flux": {"fp8_attention": True}, "vae": {"fp8": [r"^decoder\.up_blocks\.0\."]}})
    assert fp8_conv_layers(vae) == [f"decoder.up_blocks.0.resnets.{r}.conv{c}" for r in range(3) for c in (1, 2)]
    for bad in ([r"no_such_layer"], "all", []):
        with pytest.raises(ValueError):
            mk(torch.float8_e4m3fn, {"vae": {"fp8": bad}})
    mk(torch.float8_e4m3fn, {"vae": {"fp8": True}})
    assert fp8_conv_layers(vae) == marked
    mk(torch.bfloat16)
    assert fp8_conv_layers(vae) == []
    q = mk(torch.float8_e4m3fn)
    assert fp8_conv_layers(vae) == [] and not q.fp8_vae


def test_mxfp8_conv_kernel_resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import SOURCES, kernel_resources
    assert "conv_mxfp8.hip" in SOURCES
    res = kernel_resources()
    k = [(name, v) for name, v in res.items() if "mxfp8_conv_kernel" in name]
    assert len(k) == 1, sorted(res)
    name, k = k[0]
    assert not name.startswith("igemm_") and k["source"] == "conv_mxfp8.hip"
    assert k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["scratch"] == 0 and k["occupancy"] >= 2, k
    g = [v for name, v in res.items() if "gn_apply_mxfp8_kernel" in name]
    assert len(g) == 2 and all(v["spill_vgpr"] == 0 and v["scratch"] == 0 for v in g)


def test_variant_is_not_assigned_in_the_igemm_dispatcher():
    import dyadic_probe as dp
    src = open(os.path.join(ROOT, "omgsr_amd", "csrc", "igemm.hip")).read()
    assert VARIANT not in dp.variant_ids(src)
    assert not re.search(rf"ts\.rec\.variant\s*=[^;]*\b{VARIANT}\b", src)
    own = open(os.path.join(ROOT, "omgsr_amd", "csrc", "conv_mxfp8.hip")).read()
    assert re.search(rf"ts\.rec\.variant = {VARIANT};", own) and "OMGSR_TK_IGEMM" in own          # kind 1, the next free id after 18-20


def test_abi_v22_symbols():
    from omgsr_amd import _lib
    assert _lib.ABI_VERSION == 22
    hdr = open(os.path.join(ROOT, "include", "omgsr_hip.h")).read()
    for sym in ("omgsr_conv_mxfp8_ok", "omgsr_conv_mxfp8", "omgsr_groupnorm_apply_mxfp8"):
        assert sym in _lib.SIGNATURES and re.search(rf"\b{sym}\(", hdr), sym


@pytest.mark.parametrize("Cin,density", [(128, 1 / 4), (512, 1 / 8)])
def test_probe_data_stay_in_budget_and_every_border_tap_matters(Cin, density):
    """The GPU probes' generator and restatement on the host, one image: the bit budget and the 2^13 group window hold (dyadic_probe.mxfp8_ref asserts
    them), and a restatement that does not gather one tap on one border row / column differs from the exact one for every (border, tap) pair
    that reads inside the map there (the three taps that read the padding contribute zeros either way) - so a kernel that lost such a tap
    could not match the probes."""
    import dyadic_probe as dp
    import test_fp8_vae_gpu as T
    N, H, W, Cout = 1, 13, 40, 16
    g, xc, xs, wc, wsc, r, t = T.dyadic_case(2101, N, H, W, Cin, Cout, density)
    bias = T._terms(g, t.reshape(Cout))
    res = T._terms(g, (r + t).expand(N, H, W, Cout)).to(torch.bfloat16)
    pw = T.pack_planes(wc, wsc, bias, "cpu")
    uc, us = T.unpack_planes(pw)
    assert torch.equal(uc[:Cout], wc) and torch.equal(us[:Cout], wsc) and int(uc[Cout:].max()) == 0      # the layout round-trips
    want = T.conv_mxfp8_ref(xc, xs, uc, us, Cout, bias=bias, residual=res)
    dp.rounded(want, torch.float32)
    outside = {"top": (0, 1, 2), "bottom": (6, 7, 8), "left": (0, 3, 6), "right": (2, 5, 8)}    # taps that read the padding at that border
    for side, pad_taps in outside.items():
        for tap in range(9):
            got = T.conv_mxfp8_ref(xc, xs, uc, us, Cout, bias=bias, residual=res, check=False, drop=(tap, side))
            assert torch.equal(got, want) == (tap in pad_taps), (side, tap)
