"""OMGSR-S's opt-in MXFP8 UNet resnet convolutions without a GPU: the policy contract of the "unet" / "fp8" key (bf16 tier only), the layer
policy on the full-size SD 2.1 UNet built on the meta device, the new symbols under the unchanged ABI v22, the host restatement the GPU probes
trust (it depends on every block's scale at Cin 320 and on the scale window a block belongs to), and the compiler's resource figures."""
import os
import re
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("omgsr_conv_mxfp8_deep_ok", "omgsr_conv_mxfp8_deep", "omgsr_groupnorm_apply_mxfp8_c64")
DEEP_SRC = os.path.join(ROOT, "omgsr_amd", "csrc", "conv_mxfp8_deep.hip")
# the SD 2.1 UNet: 2 resnets per down block (4), 2 in the mid block, 3 per up block (4); conv1 + conv2 each
ELIGIBLE = ([f"down_blocks.{b}.resnets.{r}.conv{c}" for b in range(4) for r in range(2) for c in (1, 2)] +
            [f"mid_block.resnets.{r}.conv{c}" for r in range(2) for c in (1, 2)] +
            [f"up_blocks.{b}.resnets.{r}.conv{c}" for b in range(4) for r in range(3) for c in (1, 2)])


def _meta_unet():
    from omgsr_amd.diffusers_api import UNet2DConditionModel
    with torch.device("meta"):
        return UNet2DConditionModel()


def _meta_vae():
    from omgsr_amd.diffusers_api import AutoencoderKL
    with torch.device("meta"):
        return AutoencoderKL()


@pytest.fixture
def bf16(monkeypatch):
    from omgsr_amd import ops
    monkeypatch.setattr(ops, "set_compute_dtype", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_PRECISE", False)
    monkeypatch.setattr(ops, "_ACT", torch.bfloat16)
    return monkeypatch


def _window_chunks() -> int:
    m = re.search(r"constexpr int MXD_WINDOW_CHUNKS = (\d+);", open(DEEP_SRC).read())
    assert m, "conv_mxfp8_deep.hip no longer names its scale window"
    return int(m.group(1))


# ---- policy contract -----------------------------------------------------------------------------------------------------------------------------

def test_key_is_bf16_tier_only_and_checked_before_anything_loads():
    from omgsr_amd import precision
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    for val in (True, [r"down_blocks\.0"]):
        for wd in (torch.float16, torch.float32, torch.float8_e4m3fn):
            with pytest.raises(ValueError):
                OMGSR_S_Infer(None, None, 273, "cpu", wd, precision_policy={"unet": {"fp8": val}})
    with pytest.raises(ValueError, match="no fp8 tier"):                     # float8_e4m3fn keeps raising first, with its own message
        OMGSR_S_Infer(None, None, 273, "cpu", torch.float8_e4m3fn, precision_policy={"unet": {"fp8": True}})
    for bad in ({"unet": {"fp8_conv": True}}, {"unet": {"fp8": True, "tiled": True}}, {"unet": True}, {"unet": {"fp8": "all"}}, {"unet": {"fp8": []}},
                {"unet": {"fp8": [1]}}, {"unet": {"fp8": 1}}):
        with pytest.raises(ValueError):                                     # an unknown sub-key, a malformed value
            OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy=bad)
    if not precision.UNET_FP8:
        with pytest.raises(ValueError, match="name the layers"):            # `True` with an empty default
            OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy={"unet": {"fp8": True}})
    # the other keys OMGSR-S refuses are refused as before, next to the new one
    with pytest.raises(ValueError):
        OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy={"unet": {"fp8": [r"resnets"]}, "vae": {"fp8": True}})
    # OMGSR-F has no UNet: every tier refuses the key
    for wd in (torch.float8_e4m3fn, torch.bfloat16, torch.float16, torch.float32):
        with pytest.raises(ValueError):
            OMGSR_F_Infer(None, None, "cpu", wd, precision_policy={"unet": {"fp8": True}})
        with pytest.raises(ValueError):
            OMGSR_F_Infer(None, None, "cpu", wd, precision_policy={"unet": {"fp8": [r"resnets"]}})


def test_policy_marks_exactly_the_eligible_resnet_convs(bf16):
    from omgsr_amd import precision as P
    from omgsr_amd.nn import Conv2d
    unet = _meta_unet()
    assert [n for n, m in unet.named_modules() if isinstance(m, Conv2d) and any(re.search(p, n) for p in P.UNET_FP8_ELIGIBLE)] == ELIGIBLE
    everything = [r"."]                                                     # names every module: only the eligible ones are marked
    assert P.set_fp8_unet_conv(unet, everything) == len(ELIGIBLE) == 44 and P.fp8_unet_conv_layers(unet) == ELIGIBLE
    for name in ("conv_in", "conv_out", "down_blocks.0.downsamplers.0.conv", "up_blocks.0.upsamplers.0.conv", "up_blocks.0.resnets.0.conv_shortcut"):
        assert not unet.get_submodule(name).fp8_deep
    # a list narrows; a pattern may also name ineligible layers as long as it names an eligible one
    want = [n for n in ELIGIBLE if n.startswith("up_blocks.3.") or n.startswith("down_blocks.0.")]
    assert P.set_fp8_unet_conv(unet, [r"^up_blocks\.3\.", r"^down_blocks\.0\.|conv_in"]) == 10 and P.fp8_unet_conv_layers(unet) == want
    P.clear_fp8_unet_conv(unet)
    assert P.fp8_unet_conv_layers(unet) == []
    if P.UNET_FP8:
        n = P.set_fp8_unet_conv(unet, True)
        assert n == len([x for x in ELIGIBLE if any(re.search(p, x) for p in P.UNET_FP8)]) > 0
        P.clear_fp8_unet_conv(unet)
    else:
        with pytest.raises(ValueError, match="name the layers"):
            P.set_fp8_unet_conv(unet, True)


def test_policy_refusals(bf16):
    from omgsr_amd import ops
    from omgsr_amd import precision as P
    unet = _meta_unet()
    for bad in ("all", 1, [], [1], {"x": 1}, False, None):
        with pytest.raises(ValueError):
            P.set_fp8_unet_conv(unet, bad)
    with pytest.raises(ValueError):                                         # a dead pattern next to a live one
        P.set_fp8_unet_conv(unet, [r"^down_blocks\.0\.resnets", r"down_blocks\.9"])
    for dead in (r"conv_shortcut$", r"downsamplers\.0\.conv$", r"^conv_in$", r"attentions"):
        with pytest.raises(ValueError):                                     # names only layers that are not eligible
            P.set_fp8_unet_conv(unet, [dead])
    assert P.fp8_unet_conv_layers(unet) == []                               # a refused call marks nothing
    bf16.setattr(ops, "_PRECISE", True)
    with pytest.raises(ValueError):
        P.set_fp8_unet_conv(unet, [r"resnets"])
    bf16.setattr(ops, "_PRECISE", False)
    bf16.setattr(ops, "_ACT", torch.float16)
    with pytest.raises(ValueError):
        P.set_fp8_unet_conv(unet, [r"resnets"])
    with pytest.raises(ValueError):                                         # fp16: the MXFP8 form cannot be packed
        unet.down_blocks[0].resnets[0].conv1.packed_mxfp8_deep()


def test_pipeline_marks_and_unmarks_and_leaves_the_vae_marks_alone(bf16):
    from omgsr_amd import precision as P
    from omgsr_amd.pipelines import omgsr_s
    vae, unet = _meta_vae(), _meta_unet()
    mk = lambda wd, pol=None: omgsr_s.OMGSR_S_Infer(None, None, 273, "meta", wd, vae=vae, unet=unet, precision_policy=pol)  # noqa: E731
    p = mk(torch.bfloat16, {"unet": {"fp8": [r"\.resnets\."]}})
    assert P.fp8_unet_conv_layers(unet) == ELIGIBLE and p.fp8_unet
    assert P.fp8_conv_layers(vae) == [] and P.fp8_upsample_layers(vae) == [] and P.fp8_unet_conv_layers(vae) == []
    p = mk(torch.bfloat16, {"unet": {"fp8": [r"^mid_block"]}})
    assert P.fp8_unet_conv_layers(unet) == [n for n in ELIGIBLE if n.startswith("mid_block")]
    for bad in ([r"no_such_layer"], [r"conv_shortcut"]):                    # a dead pattern, through the pipeline
        with pytest.raises(ValueError):
            mk(torch.bfloat16, {"unet": {"fp8": bad}})
    mk(torch.bfloat16, {"unet": {"fp8": [r"\.resnets\."]}})
    q = mk(torch.bfloat16)                                                  # a pipeline built without the key unmarks
    assert P.fp8_unet_conv_layers(unet) == [] and not q.fp8_unet
    mk(torch.bfloat16, {"unet": {"fp8": [r"\.resnets\."]}})
    q = mk(torch.bfloat16, {"unet": {"fp8": False}})
    assert P.fp8_unet_conv_layers(unet) == [] and not q.fp8_unet
    # VAE marks and UNet marks do not touch each other (set_fp8_conv on a VAE, set_fp8_unet_conv on a UNet, and each on the other's model)
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
    with torch.device("meta"):
        fvae = AutoencoderKL(**FLUX_VAE_CONFIG)
    P.set_fp8_conv(fvae, True)
    P.set_fp8_unet_conv(unet, [r"\.resnets\."])
    assert len(P.fp8_conv_layers(fvae)) == 28 and P.fp8_unet_conv_layers(fvae) == [] and P.fp8_conv_layers(unet) == []
    P.clear_fp8_unet_conv(fvae)
    P.clear_fp8_conv(unet)
    assert len(P.fp8_conv_layers(fvae)) == 28 and P.fp8_unet_conv_layers(unet) == ELIGIBLE
    with pytest.raises(ValueError):                                         # a UNet has resnets the VAE key's patterns do not name, and vice versa
        P.set_fp8_unet_conv(fvae, [r"^decoder\."])
    P.clear_fp8_unet_conv(unet)
    P.clear_fp8_conv(fvae)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------

def test_symbols_under_abi_v22_and_documented_variant():
    from omgsr_amd import _lib
    assert _lib.ABI_VERSION == 22
    hdr = open(os.path.join(ROOT, "include", "omgsr_hip.h")).read()
    lib_src = open(os.path.join(ROOT, "omgsr_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"omgsr_abi_version\(void\)\s*\{\s*return 22;", lib_src)        # additive: no struct changed, the version stays
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES and re.search(rf"\b{sym}\(", hdr), sym
    assert re.search(r"\b27 mxfp8_conv_deep_kernel\b", hdr)
    own = open(DEEP_SRC).read()
    assert re.search(r"ts\.rec\.variant = 27;", own) and "OMGSR_TK_IGEMM" in own and "launch_lds<mxfp8_conv_deep_kernel>" in own
    import dyadic_probe as dp
    assert 27 not in dp.variant_ids(open(os.path.join(ROOT, "omgsr_amd", "csrc", "igemm.hip")).read())      # the dispatcher's own ids stay what they were
    for other in ("conv_mxfp8.hip", "conv_mxfp8_up.hip"):                   # ... and so do the two existing kernels' (21 / 22, 25 / 26)
        assert 27 not in dp.variant_ids(open(os.path.join(ROOT, "omgsr_amd", "csrc", other)).read())
    # the existing predicate's limits are still in its source
    old = open(os.path.join(ROOT, "omgsr_amd", "csrc", "conv_mxfp8.hip")).read()
    assert "(a.Cin % 128) == 0 && a.Cin <= MXC_MAX_CIN" in old and "constexpr int MXC_MAX_CIN = 512;" in old
    assert "(a.Cin % 64) == 0" in own and "constexpr int MXD_MAX_CIN = 2048;" in own


def test_kernel_resources():
    """mxfp8_conv_deep_kernel: at most 256 registers, no spills, no scratch, at most 80 KB of LDS (two workgroups per CU); mxfp8_conv_kernel /
    _multi keep today's figures (242 VGPRs, 77 184 bytes of LDS)."""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import SOURCES, kernel_resources
    assert "conv_mxfp8_deep.hip" in SOURCES
    res = kernel_resources()
    ks = {name: v for name, v in res.items() if "mxfp8_conv_deep" in name}
    assert sorted(ks) == ["mxfp8_conv_deep_kernel"], sorted(ks)
    k = ks["mxfp8_conv_deep_kernel"]
    print("mxfp8_conv_deep_kernel", k)
    assert k["source"] == "conv_mxfp8_deep.hip"
    assert k["vgpr"] + k.get("agpr", 0) <= 256 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["scratch"] == 0 and k["occupancy"] >= 2, k
    # the dynamic LDS size, from the source's constants: the halo stage (HaloGeo<9>::LDS_BYTES, 71 680) + two windows of W chunks x 2 blocks x 344
    src = open(DEEP_SRC).read()
    assert "static_assert(MXD_LDS_BYTES <= 81920" in src and "MXD_SA_LD = 344" in src
    assert "constexpr int MXD_WIN_BYTES = MXD_WINDOW_CHUNKS * 2 * MXD_SA_LD;" in src and "constexpr int MXD_LDS_BYTES = MXD_SA_OFF + 2 * MXD_WIN_BYTES;" in src
    lds = 71680 + 2 * _window_chunks() * 2 * 344
    print("LDS bytes", lds)
    assert lds <= 81920
    halo = open(os.path.join(ROOT, "omgsr_amd", "csrc", "igemm_halo_body.hip.h")).read()
    assert "LDS_BYTES" in halo
    for name in ("mxfp8_conv_kernel", "mxfp8_conv_multi_kernel"):
        o = res[name]
        assert o["vgpr"] == 242 and o.get("agpr", 0) == 0 and o["spill_vgpr"] == 0 and o["scratch"] == 0 and o["source"] == "conv_mxfp8.hip", (name, o)
    old = open(os.path.join(ROOT, "omgsr_amd", "csrc", "conv_mxfp8.hip")).read()
    assert "MXC_SA_LD = 344" in old and "MXC_LDS_BYTES = MXC_SA_OFF + MXC_SA_LD * (MXC_MAX_CIN / 32);" in old and 71680 + 344 * (512 // 32) == 77184


# ---- the restatement the GPU probes trust ---------------------------------------------------------------------------------------------------------

def _small_dyadic(Cin, seed):
    """The GPU probes' generator on a 3 x 5 map, one image, 8 output channels: planes + the exact reference."""
    import test_fp8_unet_gpu as T
    import test_fp8_vae_gpu as V
    g, xc, xs, wc, wsc, r, t = T.dyadic_case(seed, 1, Cin, 8, 1 / 4, h=3, w=7)
    ref = V.conv_mxfp8_ref(xc, xs, wc, wsc, 8)
    return xc, xs, wc, wsc, ref


def test_windows_are_crossed_by_the_probed_channel_counts():
    W = _window_chunks()
    assert W >= 1
    for Cin in (960, 1920):
        assert Cin // 64 > W, f"Cin {Cin} fits one scale window of {W} chunks: the GPU probes would never see a refill"
    assert 320 // 64 == 5 and (320 // 32) % 4 == 2                            # odd chunk count, a scale row that is no whole number of dwords


def test_restatement_depends_on_every_block_scale_at_cin320():
    """Dropping any one of the 10 blocks' operand scales (byte -> 127), or shifting the scale row by one block, changes the reference: a kernel
    that lost the last blocks of a 10-byte row, or read rows at a 12-byte pitch, cannot pass the bit-exact probes."""
    import test_fp8_vae_gpu as V
    xc, xs, wc, wsc, ref = _small_dyadic(320, 41)
    assert xs.shape[-1] == 10
    for b in range(10):
        s2 = xs.clone()
        s2[..., b] = 127
        assert not torch.equal(V.conv_mxfp8_ref(xc, s2, wc, wsc, 8, check=False), ref), f"block {b}'s scale does not reach the reference"
    for shift in (1, -1):
        assert not torch.equal(V.conv_mxfp8_ref(xc, torch.roll(xs, shift, -1), wc, wsc, 8, check=False), ref)
    # ... and on the weight side
    for b in range(10):
        w2 = wsc.clone()
        w2[..., b] = 127
        assert not torch.equal(V.conv_mxfp8_ref(xc, xs, wc, w2, 8, check=False), ref)


@pytest.mark.parametrize("Cin", [960])
def test_restatement_depends_on_the_window_a_block_belongs_to(Cin):
    """Past the window constant: a block of the second window given the first window's scale (what a refill that never landed would leave in
    LDS) changes the reference, for each block of the window and for the last window too."""
    import test_fp8_vae_gpu as V
    W = _window_chunks()
    xc, xs, wc, wsc, ref = _small_dyadic(Cin, 42)
    nwin = (Cin // 64 + W - 1) // W
    assert nwin >= 2
    for win in (1, nwin - 1):
        for j in range(2 * W):
            b = 2 * W * win + j
            if b >= Cin // 32:
                continue
            s2 = xs.clone()
            s2[..., b] = xs[..., b - 2 * W * win]                           # the same slot of window 0
            assert not torch.equal(V.conv_mxfp8_ref(xc, s2, wc, wsc, 8, check=False), ref), f"block {b} (window {win})"
            s2 = xs.clone()
            s2[..., b] = xs[..., b - 2 * W]                                 # the same slot of the window before (the other half's neighbour)
            assert not torch.equal(V.conv_mxfp8_ref(xc, s2, wc, wsc, 8, check=False), ref), f"block {b} (window {win}, stale by one)"


def test_dyadic_generator_stays_in_budget_at_every_probed_depth():
    """dyadic_probe.mxfp8_ref asserts the bit budget and the 2^13 group window per output, so a small map at the full K is representative of the
    GPU probes' (same densities)."""
    import test_fp8_unet_gpu as T
    import test_fp8_vae_gpu as V
    import dyadic_probe as dp
    for Cin, density, seed in ((320, 1 / 4, 2701), (960, 1 / 8, 2702), (1920, 1 / 16, 2703)):
        g, xc, xs, wc, wsc, r, t = T.dyadic_case(seed, 1, Cin, 8, density, h=3, w=7)
        bias = V._terms(g, t.reshape(8))
        res = V._terms(g, (r + t).expand(1, 3, 7, 8)).float()
        y = V.conv_mxfp8_ref(xc, xs, wc, wsc, 8, bias=bias, residual=res)
        dp.rounded(y, torch.float32)
        assert float(y.abs().max()) > 0
