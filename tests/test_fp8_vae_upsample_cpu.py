"""The fp8 tier's opt-in MXFP8 up-sampling convolutions without a GPU: the layer policy (precision.set_fp8_upsample / VAE_FP8_UP_ELIGIBLE on the
full-size FLUX VAE, built on the meta device), the pipeline's handling of the "fp8_upsample" key next to "fp8", the C ABI's new symbols under
the unchanged v22, the documented timing variants, the compiler's resource figures of the two kernels, and the host-side halves of the GPU
probes (the phase restatement equals the fp64 conv of the up-sampled map; the dyadic generator stays in budget and quantises exactly)."""
import os
import re
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPSAMPLERS = [f"decoder.up_blocks.{b}.upsamplers.0.conv" for b in range(3)]
SYMBOLS = ("omgsr_conv_mxfp8_up_ok", "omgsr_conv_mxfp8_up", "omgsr_conv_mxfp8_up_multi_ok", "omgsr_conv_mxfp8_up_multi")


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


def test_policy_marks_exactly_the_decoder_upsamplers(bf16):
    from omgsr_amd.nn import Conv2d
    from omgsr_amd.precision import (VAE_FP8_UP_ELIGIBLE, clear_fp8_conv, clear_fp8_upsample, fp8_conv_layers, fp8_upsample_layers, set_fp8_conv,
                                     set_fp8_upsample)
    vae = _meta_vae()
    assert [n for n, m in vae.named_modules() if isinstance(m, Conv2d) and any(re.search(p, n) for p in VAE_FP8_UP_ELIGIBLE)] == UPSAMPLERS
    assert set_fp8_upsample(vae, True) == 3 and fp8_upsample_layers(vae) == UPSAMPLERS
    assert fp8_conv_layers(vae) == []                                       # the new key marks nothing the old one marks
    # a list narrows; a pattern may also name ineligible layers as long as it names an eligible one
    assert set_fp8_upsample(vae, [r"up_blocks\.1\.upsamplers", r"downsamplers|up_blocks\.2\.upsamplers"]) == 2 and fp8_upsample_layers(vae) == UPSAMPLERS[1:]
    # {"fp8": True} still marks none of the up-samplers, and leaves the other key's marks alone (the keys are independent)
    n = set_fp8_conv(vae, True)
    assert n == 28 and not set(fp8_conv_layers(vae)) & set(UPSAMPLERS) and fp8_upsample_layers(vae) == UPSAMPLERS[1:]
    clear_fp8_upsample(vae)
    assert fp8_upsample_layers(vae) == [] and len(fp8_conv_layers(vae)) == 28
    set_fp8_upsample(vae, True)
    clear_fp8_conv(vae)
    assert fp8_upsample_layers(vae) == UPSAMPLERS and fp8_conv_layers(vae) == []
    clear_fp8_upsample(vae)


def test_policy_refusals(bf16):
    from omgsr_amd import ops
    from omgsr_amd.precision import fp8_upsample_layers, set_fp8_upsample
    vae = _meta_vae()
    for bad in ("all", 1, [], [1], {"x": 1}, False, None):
        with pytest.raises(ValueError):
            set_fp8_upsample(vae, bad)
    with pytest.raises(ValueError):                                         # a dead pattern next to a live one
        set_fp8_upsample(vae, [r"up_blocks\.0\.upsamplers", r"up_blocks\.9"])
    with pytest.raises(ValueError):                                         # names only layers that are not eligible (encoder samplers, resnets)
        set_fp8_upsample(vae, [r"downsamplers\.0\.conv$"])
    with pytest.raises(ValueError):
        set_fp8_upsample(vae, [r"resnets\.0\.conv1$"])
    assert fp8_upsample_layers(vae) == []                                   # a refused call marks nothing
    bf16.setattr(ops, "_PRECISE", True)
    with pytest.raises(ValueError):
        set_fp8_upsample(vae, True)
    bf16.setattr(ops, "_PRECISE", False)
    bf16.setattr(ops, "_ACT", torch.float16)
    with pytest.raises(ValueError):
        set_fp8_upsample(vae, True)
    with pytest.raises(ValueError):                                         # fp16: the MXFP8 form cannot be packed
        vae.decoder.up_blocks[0].upsamplers[0].conv.packed_mxfp8_up()


def test_key_is_fp8_tier_only():
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    for pol in ({"vae": {"fp8_upsample": True}}, {"vae": {"fp8": True, "fp8_upsample": [r"up_blocks\.0"]}}):
        for wd in (torch.bfloat16, torch.float16, torch.float32):
            with pytest.raises(ValueError):
                OMGSR_F_Infer(None, None, "cpu", wd, precision_policy=pol)
        with pytest.raises(ValueError):
            OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy=pol)
        with pytest.raises(ValueError):
            OMGSR_S_Infer(None, None, 273, "cpu", torch.float8_e4m3fn, precision_policy=pol)
    for bad in ({"vae": {"fp8_up": True}}, {"flux": {"fp8_upsample": True}}):
        with pytest.raises(ValueError):                                     # an unknown key of the fp8 tier's policy
            OMGSR_F_Infer(None, None, "cpu", torch.float8_e4m3fn, precision_policy=bad)


def test_pipeline_marks_with_or_without_fp8_and_refuses_the_tiled_vae_unless_asked(bf16):
    from omgsr_amd.pipelines import omgsr_f
    from omgsr_amd.precision import fp8_conv_layers, fp8_upsample_layers
    vae, flux = _meta_vae(), _meta_flux()
    mk = lambda wd, pol=None: omgsr_f.OMGSR_F_Infer(None, None, "meta", wd, vae=vae, flux_transformer=flux, precision_policy=pol)  # noqa: E731
    p = mk(torch.float8_e4m3fn, {"vae": {"fp8_upsample": True}})
    assert fp8_upsample_layers(vae) == UPSAMPLERS and fp8_conv_layers(vae) == [] and p.fp8_vae_upsample and not p.fp8_vae
    with pytest.raises(ValueError, match="tiled VAE"):                      # the same rule and error as the resnet convs
        p._init_tiled_vae()
    p._init_tiled_vae(fp8_convs=True)
    assert vae.decoder._tile_hook.fp8_convs
    p = mk(torch.float8_e4m3fn, {"vae": {"fp8": True, "fp8_upsample": [r"up_blocks\.2\."]}})
    assert fp8_upsample_layers(vae) == UPSAMPLERS[2:] and len(fp8_conv_layers(vae)) == 28 and p.fp8_vae and p.fp8_vae_upsample
    p = mk(torch.float8_e4m3fn, {"vae": {"fp8": True}})                     # what {"fp8": True} marks does not change; the other key's marks go
    assert fp8_upsample_layers(vae) == [] and len(fp8_conv_layers(vae)) == 28 and not p.fp8_vae_upsample
    for bad in ([r"no_such_layer"], "all", []):
        with pytest.raises(ValueError):
            mk(torch.float8_e4m3fn, {"vae": {"fp8_upsample": bad}})
    mk(torch.float8_e4m3fn, {"vae": {"fp8_upsample": True}})
    mk(torch.bfloat16)                                                      # another tier unmarks
    assert fp8_upsample_layers(vae) == []
    q = mk(torch.float8_e4m3fn)
    assert fp8_upsample_layers(vae) == [] and not q.fp8_vae_upsample
    with pytest.raises(ValueError):
        q._init_tiled_vae(fp8_convs=True)
    vae.encoder._tile_hook = vae.decoder._tile_hook = None


def test_symbols_under_abi_v22_and_documented_variants():
    from omgsr_amd import _lib
    assert _lib.ABI_VERSION == 22
    hdr = open(os.path.join(ROOT, "include", "omgsr_hip.h")).read()
    lib_src = open(os.path.join(ROOT, "omgsr_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"omgsr_abi_version\(void\)\s*\{\s*return 22;", lib_src)        # additive: no struct changed, the version stays
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and re.search(rf"\b{sym}\(", hdr), sym
    assert re.search(r"\b25 mxfp8_conv_up_kernel\b", hdr) and re.search(r"\b26 mxfp8_conv_up_multi_kernel\b", hdr)
    own = open(os.path.join(ROOT, "omgsr_amd", "csrc", "conv_mxfp8_up.hip")).read()
    assert re.search(r"ts\.rec\.variant = 25;", own) and re.search(r"ts\.rec\.variant = 26;", own) and "OMGSR_TK_IGEMM" in own
    assert "launch_lds<mxfp8_conv_up_kernel>" in own and "launch_lds<mxfp8_conv_up_multi_kernel>" in own
    import dyadic_probe as dp
    disp = open(os.path.join(ROOT, "omgsr_amd", "csrc", "igemm.hip")).read()
    assert not {25, 26} & dp.variant_ids(disp)                              # the dispatcher's own ids stay what they were


def test_kernel_resources():
    """At most 80 KB LDS (asserted at compile time in the source), at most 256 registers, no spills, no scratch, two workgroups per CU."""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import SOURCES, kernel_resources
    assert "conv_mxfp8_up.hip" in SOURCES
    res = kernel_resources()
    ks = {name: v for name, v in res.items() if "mxfp8_conv_up" in name}
    assert sorted(ks) == ["mxfp8_conv_up_kernel", "mxfp8_conv_up_multi_kernel"], sorted(ks)
    for name, k in ks.items():
        print(name, k)
        assert k["source"] == "conv_mxfp8_up.hip"
        assert k["vgpr"] + k.get("agpr", 0) <= 256 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["scratch"] == 0 and k["occupancy"] >= 2, k
    src = open(os.path.join(ROOT, "omgsr_amd", "csrc", "conv_mxfp8_up.hip")).read()
    assert 'static_assert(MXU_LDS_BYTES <= 81920' in src


def test_phase_restatement_is_the_conv_of_the_upsampled_map():
    """The restatement the GPU probes trust, on the host: four 2 x 2 convolutions of the low-resolution map with ops._phase_kernels' sums equal
    the fp64 F.conv2d of the nearest-up-sampled map, for a dyadic case made by the GPU probes' generator (whose taps lie in -2 .. 2)."""
    import test_fp8_vae_upsample_gpu as T
    g = torch.Generator().manual_seed(11)
    x, w, bias = T.dyadic_case(g, 1, 5, 7, 128, 8)
    ref = T.conv_up_ref(x, w, bias)
    from omgsr_amd import ops
    ph = ops._phase_kernels(w.float().permute(0, 2, 3, 1))                  # [4, Cout, 2, 2, Cin]
    assert float(ph.abs().max() / w.float().abs().max()) <= 4.0 and int(w.float().abs().max() / w.float().abs()[w != 0].min()) >= 4
    got = T.phase_ref(x.double(), ph.reshape(4, 8, 4, 128).double(), bias)
    assert got.shape == ref.shape == (1, 10, 14, 8) and torch.equal(got, ref)
    # the phase sums of the generator's weights quantise exactly: integers of magnitude <= 8 times one power of two per 32-channel block
    from omgsr_amd.testing import mxfp8_ref
    import dyadic_probe as dp
    codes, scales = mxfp8_ref(ph.reshape(-1, 128))
    assert torch.equal(dp.mxfp8_values(codes, scales), ph.reshape(-1, 128).double())
    assert len(set(scales.flatten().tolist())) > 4                          # ... and the scale bytes differ between blocks
