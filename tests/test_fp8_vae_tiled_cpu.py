"""The tiled VAE on the fp8 tier's MXFP8 convolutions without a GPU: the compiler's resource figures of mxfp8_conv_multi_kernel and
gn_apply_mxfp8_multi_kernel, the kernel census the one-tensor tests pin, the timing-variant constraint on igemm.hip, the three symbols that are
additive under ABI v22, and - on meta modules - OMGSR_F_Infer._init_tiled_vae's fp8_convs keyword and the VAEHook default."""
import os
import re
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_fp8_vae_cpu as T  # noqa: E402
from test_fp8_vae_cpu import bf16  # noqa: E402,F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = 22
SYMBOLS = ("omgsr_conv_mxfp8_multi_ok", "omgsr_conv_mxfp8_multi", "omgsr_groupnorm_apply_mxfp8_multi")


def _resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import kernel_resources
    return kernel_resources()


def test_multi_kernel_resources():
    res = _resources()
    k = [(name, v) for name, v in res.items() if "mxfp8_conv_multi_kernel" in name]
    assert len(k) == 1, sorted(res)
    name, k = k[0]
    assert "mxfp8_conv_kernel" not in name and not name.startswith(("igemm_", "attn_kernel", "splitk_reduce")) and k["source"] == "conv_mxfp8.hip"
    assert k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["scratch"] == 0 and k["occupancy"] >= 2, k
    g = [(name, v) for name, v in res.items() if "gn_apply_mxfp8_multi_kernel" in name]
    assert len(g) == 2 and all(v["source"] == "norm.hip" and v["spill_vgpr"] == 0 and v["spill_sgpr"] == 0 and v["scratch"] == 0 for _, v in g), g
    assert all("gn_apply_mxfp8_kernel" not in name for name, _ in g)


def test_kernel_census_of_the_one_tensor_forms_is_unchanged():
    res = _resources()
    assert len([n for n in res if "mxfp8_conv_kernel" in n]) == 1
    assert len([n for n in res if "gn_apply_mxfp8_kernel" in n]) == 2
    # the shared tile body is inlined into both kernels: the same register budget after the lookup
    one = next(v for n, v in res.items() if "mxfp8_conv_kernel" in n)
    multi = next(v for n, v in res.items() if "mxfp8_conv_multi_kernel" in n)
    assert one["vgpr"] == multi["vgpr"] and one["agpr"] == multi["agpr"], (one, multi)


def test_variant_22_is_assigned_in_conv_mxfp8_only():
    import dyadic_probe as dp
    src = open(os.path.join(ROOT, "omgsr_amd", "csrc", "igemm.hip")).read()
    assert VARIANT not in dp.variant_ids(src)
    assert not re.search(rf"ts\.rec\.variant\s*=[^;]*\b{VARIANT}\b", src)
    own = open(os.path.join(ROOT, "omgsr_amd", "csrc", "conv_mxfp8.hip")).read()
    assert re.search(rf"ts\.rec\.variant = {VARIANT};", own) and re.search(r"ts\.rec\.variant = 21;", own) and "OMGSR_TK_IGEMM" in own
    assert len(re.findall(r"__global__[^\n]*\bmxfp8_conv_kernel\(", own)) == 1 and len(re.findall(r"__global__[^\n]*\bmxfp8_conv_multi_kernel\(", own)) == 1
    # both kernels are the shared body after the lookup: each __global__ calls the <9, false> instantiation of the one tile body, and nothing else does
    assert re.findall(r"\bmxfp8_conv_tile<([^>]*)>\(", own) == ["9, false", "9, false"] and "mxfp8_conv_body" not in own
    for kernel in ("mxfp8_conv_kernel", "mxfp8_conv_multi_kernel"):
        body = own[own.index(f"void {kernel}("):].split("\n}\n")[0]
        assert len(re.findall(r"\bmxfp8_conv_tile<9, false>\(", body)) == 1, kernel


def test_the_three_units_share_one_tile_body():
    """Where the one body lives: conv_mxfp8_body.hip.h holds the scaled-MFMA statement, the three units include it and hold none of their own."""
    csrc = os.path.join(ROOT, "omgsr_amd", "csrc")
    mfma = "v_mfma_scale_f32_32x32x64_f8f6f4"
    body = open(os.path.join(csrc, "conv_mxfp8_body.hip.h")).read()
    assert len(re.findall(rf'asm volatile\("[^"]*{mfma}', body)) == 1
    assert re.search(r"static_assert\(!\(WINDOWED && TAPS == 4\)", body)
    for unit, inst in (("conv_mxfp8.hip", "9, false"), ("conv_mxfp8_up.hip", "4, false"), ("conv_mxfp8_deep.hip", "9, true")):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "conv_mxfp8_body.hip.h"' in src and mfma not in src, unit
        assert set(re.findall(r"\bmxfp8_conv_tile<([^>]*)>\(", src)) == {inst}, unit


def test_symbols_are_additive_under_abi_v22():
    from omgsr_amd import _lib
    assert _lib.ABI_VERSION == 22
    hdr = open(os.path.join(ROOT, "include", "omgsr_hip.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and re.search(rf"\b{sym}\(", hdr), sym
    assert len(re.findall(r"[Aa]dditive under ABI v22", hdr)) >= 2
    src = open(os.path.join(ROOT, "omgsr_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"omgsr_abi_version\(void\)\s*\{\s*return 22;", src)


def test_host_signatures():
    import inspect
    from omgsr_amd import ops
    from omgsr_amd.nn import Conv2d
    assert inspect.signature(ops.conv2d_multi).parameters["fp8_pack"].default is None
    assert inspect.signature(ops.conv2d_mxfp8_multi).parameters["residuals"].default is None
    assert callable(ops.group_norm_apply_mxfp8_multi)
    assert inspect.signature(Conv2d.nhwc_multi).parameters["fp8"].default is False


def test_init_tiled_vae_fp8_convs_keyword_and_hook_default(bf16):  # noqa: F811
    """Nothing runs (meta modules). The key without the keyword raises as before; the keyword with the key installs hooks with fp8_convs set; the
    keyword without the key is refused; a hook built today has fp8_convs False."""
    from omgsr_amd.pipelines import omgsr_f
    from omgsr_amd.pipelines.vaehook import VAEHook
    from omgsr_amd.precision import fp8_conv_layers
    vae, flux = T._meta_vae(), T._meta_flux()
    mk = lambda wd, pol=None: omgsr_f.OMGSR_F_Infer(None, None, "meta", wd, vae=vae, flux_transformer=flux, precision_policy=pol)  # noqa: E731
    assert VAEHook.fp8_convs is False
    assert VAEHook(vae.decoder, 64, is_decoder=True, fast_decoder=False, fast_encoder=False, color_fix=False).fp8_convs is False
    p = mk(torch.float8_e4m3fn, {"vae": {"fp8": True}})
    assert fp8_conv_layers(vae)
    with pytest.raises(ValueError, match="tiled VAE"):                     # case 1: exactly as before
        p._init_tiled_vae()
    with pytest.raises(ValueError, match="tiled VAE"):
        p._init_tiled_vae(fp8_convs=False)
    assert getattr(vae.decoder, "_tile_hook", None) is None                # a refused call installs nothing
    p._init_tiled_vae(encoder_tile_size=256, decoder_tile_size=64, fp8_convs=True)      # case 2
    enc, dec = vae.encoder._tile_hook, vae.decoder._tile_hook
    assert isinstance(enc, VAEHook) and isinstance(dec, VAEHook) and enc.fp8_convs is True and dec.fp8_convs is True
    assert (enc.tile_size, dec.tile_size, enc.is_decoder, dec.is_decoder) == (256, 64, False, True)
    vae.encoder._tile_hook = vae.decoder._tile_hook = None
    q = mk(torch.float8_e4m3fn)                                             # case 3: the keyword without the key
    assert fp8_conv_layers(vae) == [] and not q.fp8_vae
    with pytest.raises(ValueError):
        q._init_tiled_vae(fp8_convs=True)
    assert getattr(vae.decoder, "_tile_hook", None) is None
    q._init_tiled_vae()                                                     # ... and tiling without it is what it was
    assert vae.decoder._tile_hook.fp8_convs is False and vae.encoder._tile_hook.fp8_convs is False
    r = mk(torch.bfloat16)                                                  # another tier: no key possible, the keyword refused
    with pytest.raises(ValueError):
        r._init_tiled_vae(fp8_convs=True)
    # the precision_policy grammar did not change: no new key
    for bad in ({"vae": {"fp8": True, "tiled": True}}, {"vae": {"fp8_convs": True}}):
        with pytest.raises(ValueError):
            mk(torch.float8_e4m3fn, bad)
