"""OMGSR-S's opt-in MXFP8 UNet feed-forwards without a GPU: the policy contract of the "unet" / "fp8_ff" key (bf16 tier only, beside "fp8"), the block
policy on the full-size SD 2.1 UNet built on the meta device, the routing rule, the new symbols under the unchanged ABI v22, the compiler's
resource figures (the new kernel's, and the parent commit's for the kernels this change must not move), the fp32 GELU restatement the GPU
probe's saturated gate trusts, and the packer's layout."""
import os
import re
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("omgsr_igemm_geglu_mxfp8_ok", "omgsr_igemm_geglu_mxfp8", "omgsr_layernorm_mxfp8_pad")
GEGLU_SRC = os.path.join(ROOT, "omgsr_amd", "csrc", "gemm_mxfp8_geglu.hip")
# the SD 2.1 UNet: two transformers per attention down block (3), one in the mid block, three per attention up block (3); one block each
BLOCKS = ([f"down_blocks.{b}.attentions.{j}.transformer_blocks.0" for b in range(3) for j in range(2)] +
          ["mid_block.attentions.0.transformer_blocks.0"] +
          [f"up_blocks.{b}.attentions.{j}.transformer_blocks.0" for b in (1, 2, 3) for j in range(3)])


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


# ---- policy contract -----------------------------------------------------------------------------------------------------------------------------

def test_key_is_bf16_tier_only_and_checked_before_anything_loads():
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    for val in (True, [r"down_blocks\.0"]):
        for wd in (torch.float16, torch.float32, torch.float8_e4m3fn):
            with pytest.raises(ValueError):
                OMGSR_S_Infer(None, None, 273, "cpu", wd, precision_policy={"unet": {"fp8_ff": val}})
            with pytest.raises(ValueError):
                OMGSR_S_Infer(None, None, 273, "cpu", wd, precision_policy={"unet": {"fp8": True, "fp8_ff": val}})
    with pytest.raises(ValueError, match="fp8_ff"):                         # the 16-bit / accurate tiers name the key they refuse
        OMGSR_S_Infer(None, None, 273, "cpu", torch.float32, precision_policy={"unet": {"fp8_ff": True}})
    for bad in ({"unet": {"fp8_ffn": True}}, {"unet": {"fp8_ff": True, "tiled": True}}, {"unet": {"fp8_ff": "all"}}, {"unet": {"fp8_ff": []}},
                {"unet": {"fp8_ff": [1]}}, {"unet": {"fp8_ff": 1}}, {"unet": {"fp8": True, "fp8_ff": "all"}}):
        with pytest.raises(ValueError):                                     # an unknown sub-key, a malformed value
            OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy=bad)
    with pytest.raises(ValueError):                                         # the other keys OMGSR-S refuses are refused as before
        OMGSR_S_Infer(None, None, 273, "cpu", torch.bfloat16, precision_policy={"unet": {"fp8_ff": True}, "vae": {"fp8": True}})
    for wd in (torch.float8_e4m3fn, torch.bfloat16, torch.float16, torch.float32):      # OMGSR-F has no UNet: every tier refuses the key
        for val in (True, [r"transformer_blocks"]):
            with pytest.raises(ValueError):
                OMGSR_F_Infer(None, None, "cpu", wd, precision_policy={"unet": {"fp8_ff": val}})


def test_policy_marks_exactly_the_transformer_blocks(bf16):
    from omgsr_amd import precision as P
    from omgsr_amd.diffusers_api.unet_2d_condition import BasicTransformerBlock
    unet = _meta_unet()
    assert [n for n, m in unet.named_modules() if isinstance(m, BasicTransformerBlock)] == BLOCKS and len(BLOCKS) == 16
    assert P.fp8_unet_ff_layers(unet) == []
    assert P.set_fp8_unet_ff(unet, [r"."]) == 16 and P.fp8_unet_ff_layers(unet) == BLOCKS       # names every module: only the blocks are marked
    for n in BLOCKS:
        blk = unet.get_submodule(n)
        assert blk.ff.net[0].fp8 and blk.ff.net[2].fp8
        for other in (blk.attn1.to_q, blk.attn1.to_out[0], blk.attn2.to_q, blk.attn2.to_k, blk.ff.net[0].proj):
            assert not other.fp8                                            # no other linear of the block moves
    assert not unet.get_submodule("down_blocks.0.attentions.0.proj_in").fp8 and not unet.get_submodule("down_blocks.0.attentions.0.proj_out").fp8
    want = [n for n in BLOCKS if n.startswith("up_blocks.3.") or n.startswith("down_blocks.0.")]
    assert P.set_fp8_unet_ff(unet, [r"^up_blocks\.3\.", r"^down_blocks\.0\.|conv_in"]) == 5 and P.fp8_unet_ff_layers(unet) == want
    assert not unet.get_submodule("mid_block.attentions.0.transformer_blocks.0").ff.net[2].fp8     # a narrower list unmarks the rest
    P.clear_fp8_unet_ff(unet)
    assert P.fp8_unet_ff_layers(unet) == [] and not any(unet.get_submodule(n).ff.net[2].fp8 for n in BLOCKS)
    assert P.UNET_FP8_FF, "True marks the default list"
    n = P.set_fp8_unet_ff(unet, True)
    assert n == len([x for x in BLOCKS if any(re.search(p, x) for p in P.UNET_FP8_FF)]) > 0
    assert P.check_fp8_unet_ff(True) == list(P.UNET_FP8_FF) and P.check_fp8_unet_ff(["a", "b"]) == ["a", "b"]
    P.clear_fp8_unet_ff(unet)
    # the conv key and the feed-forward key do not touch each other
    P.set_fp8_unet_conv(unet, [r"\.resnets\."])
    P.set_fp8_unet_ff(unet, [r"^mid_block"])
    assert len(P.fp8_unet_conv_layers(unet)) == 44 and P.fp8_unet_ff_layers(unet) == ["mid_block.attentions.0.transformer_blocks.0"]
    P.clear_fp8_unet_conv(unet)
    assert P.fp8_unet_ff_layers(unet) == ["mid_block.attentions.0.transformer_blocks.0"]
    P.clear_fp8_unet_ff(unet)


def test_policy_refusals(bf16):
    from omgsr_amd import ops
    from omgsr_amd import precision as P
    unet = _meta_unet()
    for bad in ("all", 1, [], [1], {"x": 1}, False, None):
        with pytest.raises(ValueError):
            P.set_fp8_unet_ff(unet, bad)
        with pytest.raises(ValueError):
            P.check_fp8_unet_ff(bad)
    with pytest.raises(ValueError):                                         # a dead pattern next to a live one
        P.set_fp8_unet_ff(unet, [r"^down_blocks\.0\.", r"down_blocks\.9"])
    for dead in (r"conv_shortcut$", r"resnets\.0\.conv1$", r"^conv_in$", r"^down_blocks\.3\."):
        with pytest.raises(ValueError):                                     # names no transformer block (down_blocks.3 has no attention)
            P.set_fp8_unet_ff(unet, [dead])
    assert P.fp8_unet_ff_layers(unet) == []                                 # a refused call marks nothing
    bf16.setattr(ops, "_PRECISE", True)
    with pytest.raises(ValueError):
        P.set_fp8_unet_ff(unet, True)
    bf16.setattr(ops, "_PRECISE", False)
    bf16.setattr(ops, "_ACT", torch.float16)
    with pytest.raises(ValueError):
        P.set_fp8_unet_ff(unet, True)
    with pytest.raises(ValueError):                                         # fp16: the MXFP8 form cannot be packed
        unet.down_blocks[0].attentions[0].transformer_blocks[0].ff.net[0].packed_mxfp8()
    for pol, where in (({"unet": {"fp8_ff": True}}, "x"), ({"unet": {"fp8": True, "fp8_ff": False}}, "x")):
        with pytest.raises(ValueError, match="fp8_ff"):
            P.refuse_fp8_unet_ff(pol, where)
    for pol in (None, "default", {"unet": {"fp8": True}}, {"vae": {"fp8": True}}):
        P.refuse_fp8_unet_ff(pol, "x")


def test_pipeline_marks_and_unmarks(bf16):
    from omgsr_amd import precision as P
    from omgsr_amd.pipelines import omgsr_s
    vae, unet = _meta_vae(), _meta_unet()
    mk = lambda wd, pol=None: omgsr_s.OMGSR_S_Infer(None, None, 273, "meta", wd, vae=vae, unet=unet, precision_policy=pol)  # noqa: E731
    p = mk(torch.bfloat16, {"unet": {"fp8_ff": True}})
    assert P.fp8_unet_ff_layers(unet) == [n for n in BLOCKS if any(re.search(q, n) for q in P.UNET_FP8_FF)] and p.fp8_unet_ff and not p.fp8_unet
    assert P.fp8_unet_conv_layers(unet) == []
    p = mk(torch.bfloat16, {"unet": {"fp8_ff": [r"^mid_block"], "fp8": [r"^mid_block"]}})
    assert P.fp8_unet_ff_layers(unet) == ["mid_block.attentions.0.transformer_blocks.0"] and len(P.fp8_unet_conv_layers(unet)) == 4
    assert p.fp8_unet_ff and p.fp8_unet
    for bad in ([r"no_such_block"], [r"conv_shortcut"]):                    # a dead pattern, through the pipeline
        with pytest.raises(ValueError):
            mk(torch.bfloat16, {"unet": {"fp8_ff": bad}})
    mk(torch.bfloat16, {"unet": {"fp8_ff": True}})
    q = mk(torch.bfloat16)                                                  # a pipeline built without the key unmarks
    assert P.fp8_unet_ff_layers(unet) == [] and not q.fp8_unet_ff
    mk(torch.bfloat16, {"unet": {"fp8_ff": True}})
    q = mk(torch.bfloat16, {"unet": {"fp8_ff": False}})
    assert P.fp8_unet_ff_layers(unet) == [] and not q.fp8_unet_ff
    mk(torch.bfloat16, {"unet": {"fp8_ff": True}})
    q = mk(torch.bfloat16, {"unet": {"fp8": [r"\.resnets\."]}})             # the conv key alone unmarks the feed-forwards
    assert P.fp8_unet_ff_layers(unet) == [] and len(P.fp8_unet_conv_layers(unet)) == 44 and not q.fp8_unet_ff
    mk(torch.bfloat16)


def test_routing_rule_is_one_function_and_the_modules_ask_it(bf16):
    from omgsr_amd import precision as P
    import json
    # what the library serves
    for rows, C in ((147456, 320), (4096, 320), (64, 1280), (1, 32), (5, 4096)):
        assert P.fp8_unet_ff_served(rows, C)
    for rows, C in ((100, 24), (100, 328), (100, 4128), (0, 320)):
        assert not P.fp8_unet_ff_served(rows, C) and not P.fp8_unet_ff_routed(rows, C)
    # the rule admits exactly the measured classes whose every MXFP8 step beat every bf16 step (profiles/fp8_unet_ff.json)
    prof = json.load(open(os.path.join(ROOT, "profiles", "fp8_unet_ff.json")))
    assert len(prof["layers"]) == 12
    for row in prof["layers"]:
        won = max(row["mxfp8_ms"]) < min(row["bf16_ms"])
        assert won == row["every_mxfp8_step_faster_than_every_bf16_step"] and len(row["mxfp8_ms"]) == len(row["bf16_ms"]) == 9
        assert P.fp8_unet_ff_routed(row["rows"], row["C"]) == won, (row["rows"], row["C"])
    assert sorted((r["rows"], r["C"]) for r in prof["layers"] if P.fp8_unet_ff_routed(r["rows"], r["C"])) == \
        [(2304, 1280), (2304, 1280), (9216, 640), (9216, 1280), (36864, 640)]
    unet = _meta_unet()
    blk = unet.get_submodule("mid_block.attentions.0.transformer_blocks.0")     # C = 1280
    assert not blk.ff.fp8_routed(9216)                                      # unmarked
    P.set_fp8_unet_ff(unet, True)
    assert blk.ff.fp8_routed(9216) and not blk.ff.fp8_routed(576)
    assert not unet.get_submodule(BLOCKS[0]).ff.fp8_routed(147456)          # C = 320: no class of it won
    bf16.setattr(P, "fp8_unet_ff_routed", lambda rows, C: rows >= 8192)     # the module asks the rule at call time
    assert not blk.ff.fp8_routed(4096) and blk.ff.fp8_routed(8192)
    bf16.undo()
    P.clear_fp8_unet_ff(unet)
    src = open(os.path.join(ROOT, "omgsr_amd", "diffusers_api", "unet_2d_condition.py")).read()
    assert src.count("fp8_unet_ff_routed") == 3                             # the import and the call in FeedForward.fp8_routed, one docstring


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------

def _c_args(decl: str) -> list:
    """Parameter kinds of a C declaration's argument list: 'P' pointer, 'I' int32, 'L' int64, 'F' float."""
    out = []
    for a in decl.split(","):
        a = a.strip()
        out.append("P" if "*" in a else "L" if a.startswith("int64_t") else "I" if a.startswith("int32_t") else "F" if a.startswith("float") else "?")
    return out


def test_symbols_under_abi_v22_match_the_binding():
    import ctypes as C
    from omgsr_amd import _lib
    assert _lib.ABI_VERSION == 22
    hdr = open(os.path.join(ROOT, "include", "omgsr_hip.h")).read()
    lib_src = open(os.path.join(ROOT, "omgsr_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"omgsr_abi_version\(void\)\s*\{\s*return 22;", lib_src)        # additive: no struct changed, the version stays
    kinds = {C.c_void_p: "P", C.c_int32: "I", C.c_int64: "L", C.c_float: "F", C.POINTER(_lib.IgemmArgs): "P"}
    for sym in SYMBOLS:
        assert sym in _lib.SIGNATURES, sym
        m = re.search(rf"^(int32_t|int) {sym}\(([^;]*?)\);", hdr, flags=re.M | re.S)
        assert m, f"{sym} is not declared in the header"
        res, args = _lib.SIGNATURES[sym]
        assert res == (C.c_int32 if m.group(1) == "int32_t" else C.c_int)
        assert [kinds[a] for a in args] == _c_args(m.group(2)), sym
    # the padded LayerNorm takes omgsr_layernorm_mxfp8's arguments
    assert _lib.SIGNATURES["omgsr_layernorm_mxfp8_pad"] == _lib.SIGNATURES["omgsr_layernorm_mxfp8"]
    assert _lib.SIGNATURES["omgsr_igemm_geglu_mxfp8"] == _lib.SIGNATURES["omgsr_igemm_out_mxfp8"]
    assert re.search(r"\b28 mxfp8_gemm_geglu_kernel\b", hdr)
    own = open(GEGLU_SRC).read()
    assert re.search(r"ts\.rec\.variant = 28;", own) and "OMGSR_TK_IGEMM" in own and "mxfp8_gemm_body<OUT8>" in own
    import dyadic_probe as dp
    assert 28 not in dp.variant_ids(open(os.path.join(ROOT, "omgsr_amd", "csrc", "igemm.hip")).read())      # the dispatcher's own ids stay what they were
    # the existing predicate keeps refusing GEGLU and K % 128, in its source
    old = open(os.path.join(ROOT, "omgsr_amd", "csrc", "gemm_mxfp8.hip")).read()
    assert "(a.Cin % BK) == 0" in old and "a.act != OMGSR_ACT_GEGLU" in old
    epi = open(os.path.join(ROOT, "omgsr_amd", "csrc", "igemm.hip")).read()
    assert re.search(r"omgsr_igemm_out_mxfp8\(.*?a\.act == OMGSR_ACT_GEGLU\)\s*return OMGSR_E_SHAPE;", epi, flags=re.S)
    assert not os.path.basename(GEGLU_SRC).startswith("igemm_") and "void igemm_" not in own


# ---- resources ---------------------------------------------------------------------------------------------------------------------------------

# layernorm_kernel<T, MAXCH, RPW, XF32, YEL> at the parent commit: (VGPRs, waves per SIMD); no AGPRs, spills, scratch or LDS in any of them
PARENT_LAYERNORM = {
    "bf16,1,4,0,0": (82, 5), "bf16,1,4,0,2": (82, 5), "bf16,1,4,0,5": (86, 5), "bf16,1,4,1,0": (82, 5), "bf16,1,4,1,2": (82, 5), "bf16,1,4,1,3": (0, 8),
    "bf16,2,4,0,0": (124, 4), "bf16,2,4,0,2": (124, 4), "bf16,2,4,0,5": (134, 3), "bf16,2,4,1,0": (124, 4), "bf16,2,4,1,2": (124, 4), "bf16,2,4,1,3": (0, 8),
    "bf16,3,2,0,0": (122, 4), "bf16,3,2,0,2": (122, 4), "bf16,3,2,0,5": (128, 4), "bf16,3,2,1,0": (122, 4), "bf16,3,2,1,2": (122, 4), "bf16,3,2,1,3": (0, 8),
    "fp16,1,4,0,0": (84, 5), "fp16,1,4,0,2": (84, 5), "fp16,1,4,1,0": (82, 5), "fp16,1,4,1,2": (82, 5), "fp16,1,4,1,3": (84, 5),
    "fp16,2,4,0,0": (124, 4), "fp16,2,4,0,2": (124, 4), "fp16,2,4,1,0": (124, 4), "fp16,2,4,1,2": (124, 4), "fp16,2,4,1,3": (128, 4),
    "fp16,3,2,0,0": (122, 4), "fp16,3,2,0,2": (122, 4), "fp16,3,2,1,0": (122, 4), "fp16,3,2,1,2": (122, 4), "fp16,3,2,1,3": (126, 4),
}
# the MXFP8 token GEMM's three kernels at the parent commit: (VGPRs, SGPR spills); two workgroups per CU, no VGPR spills, no scratch
PARENT_GEMM = {"mxfp8_gemm_kernel": (249, 0, "gemm_mxfp8.hip"), "mxfp8_gemm_out8_kernel": (249, 3, "gemm_mxfp8_out8.hip"),
               "mxfp8_gemm_multi_kernel": (249, 0, "gemm_mxfp8_multi.hip")}
LN_PAD = 105        # norm.hip's LN_MXFP8_PAD: the new instantiations' YEL


def test_kernel_resources():
    """mxfp8_gemm_geglu_kernel (both output forms): at most 256 registers, no spills, no scratch, two workgroups per CU, from its own translation
    unit; the existing MXFP8 GEMM kernels and every layernorm_kernel instantiation of the parent commit keep the parent's figures."""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import SOURCES, kernel_resources
    assert "gemm_mxfp8_geglu.hip" in SOURCES
    res = kernel_resources()
    ks = {name: v for name, v in res.items() if "mxfp8_gemm_geglu" in name}
    assert sorted(ks) == ["mxfp8_gemm_geglu_kernel<0>", "mxfp8_gemm_geglu_kernel<1>"], sorted(ks)
    for name, k in ks.items():
        print(name, k)
        assert k["source"] == "gemm_mxfp8_geglu.hip"
        assert k["vgpr"] + k.get("agpr", 0) <= 256 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["scratch"] == 0 and k["occupancy"] == 2, (name, k)
    # the register budget of two 512-thread workgroups per CU (256 per lane), like the kernels whose body it instantiates
    assert "__launch_bounds__(512, 2) void mxfp8_gemm_geglu_kernel" in open(GEGLU_SRC).read()
    for name, (vgpr, sspill, source) in PARENT_GEMM.items():
        o = res[name]
        assert (o["vgpr"], o["agpr"], o["spill_vgpr"], o["spill_sgpr"], o["scratch"], o["occupancy"], o["source"]) == (vgpr, 0, 0, sspill, 0, 2, source), (name, o)
    ln = {name[len("layernorm_kernel<"):-1]: v for name, v in res.items() if name.startswith("layernorm_kernel<")}
    old = {k: v for k, v in ln.items() if not k.endswith(f",{LN_PAD}")}
    assert sorted(old) == sorted(PARENT_LAYERNORM), sorted(set(old) ^ set(PARENT_LAYERNORM))
    for k, (vgpr, occ) in PARENT_LAYERNORM.items():
        o = old[k]
        assert (o["vgpr"], o["agpr"], o["spill_vgpr"], o["spill_sgpr"], o["scratch"], o["occupancy"], o["lds"], o["source"]) == (vgpr, 0, 0, 0, 0, occ, 0, "norm.hip"), (k, o)
    new = sorted(k for k in ln if k.endswith(f",{LN_PAD}"))
    assert new == [f"bf16,1,4,0,{LN_PAD}", f"bf16,2,4,0,{LN_PAD}", f"bf16,3,2,0,{LN_PAD}"], new
    for k in new:
        o = ln[k]
        assert o["spill_vgpr"] == 0 and o["spill_sgpr"] == 0 and o["scratch"] == 0, (k, o)


# ---- the saturated gate of the GPU probe ---------------------------------------------------------------------------------------------------------

def gelu_erf_f32(x: torch.Tensor) -> torch.Tensor:
    """csrc/common.hip.h's gelu_erf_f restated in fp32 operation by operation (fused multiply-adds as single roundings through fp64: a product
    of two fp32 values is exact there, and the one rounding of the sum to fp32 differs from fmaf's only by double rounding, which the
    saturated range never reaches: the polynomial's value is multiplied by an exponential below 2^-46)."""
    f = lambda v: v.to(torch.float32)                                       # noqa: E731
    fma = lambda a, b, c: f(a.double() * b.double() + c.double())           # noqa: E731
    c = lambda v: torch.tensor(v, dtype=torch.float32)                      # noqa: E731
    z = f(x.abs() * c(0.70710678118654752440))
    t = f(1.0 / fma(c(0.3275911), z, c(1.0)))
    poly = fma(c(1.061405429), t, c(-1.453152027))
    poly = fma(poly, t, c(1.421413741))
    poly = fma(poly, t, c(-0.284496736))
    poly = fma(poly, t, c(0.254829592))
    e = f(c(1.0) - f(f(poly * t) * torch.exp(f(-(z * z)))))
    return f(f(c(0.5) * x) * f(c(1.0) + torch.copysign(e, x)))


def test_saturated_gelu_is_the_identity_or_zero():
    """For a dyadic g with |g| >= 8 the kernel's GELU is exactly g (g > 0) or exactly +-0 (g < 0): exp(-g^2 / 2) <= e^-32 vanishes under
    1 - ... in fp32. Every multiple of 1/2 with 8 <= |g| <= 256 - the GPU probe's gate pre-activations are among them - and the rcp / exp
    approximations of the device cannot change it: any t in (0, 1] and any exponential below 2^-25 give e = 1."""
    g = torch.arange(16, 513, dtype=torch.float32) / 2
    assert float(g.min()) == 8.0 and float(g.max()) == 256.0
    pos, neg = gelu_erf_f32(g), gelu_erf_f32(-g)
    assert torch.equal(pos, g)
    assert torch.equal(neg, torch.zeros_like(g)) and bool(torch.signbit(neg).all())          # -0: 0.5 g (1 - 1)
    assert float(torch.exp(-(g.double() * 0.70710678118654752440) ** 2).max()) < 2.0 ** -46
    # and it is NOT the identity below the saturated range: the probe's |g| >= 8 is what makes the expectation exact
    assert not torch.equal(gelu_erf_f32(torch.tensor([2.0])), torch.tensor([2.0]))
    # the restatement is the exact GELU to the A&S bound on ordinary arguments
    x = torch.randn(1 << 16, generator=torch.Generator().manual_seed(7)) * 3
    ref = 0.5 * x.double() * (1 + torch.erf(x.double() / 2 ** 0.5))
    assert float(x.abs().max()) < 16
    assert float((gelu_erf_f32(x).double() - ref).abs().max()) < 5e-6       # 0.5 |x| (1.5e-7 + a few fp32 roundings of 1 + erf), |x| < 16


# ---- the packer ----------------------------------------------------------------------------------------------------------------------------------

def test_pack_geglu_weight_mxfp8_layout(bf16):
    """Interleave, K pad and row pad on the host: ops.quantize_mxfp8 stands in as omgsr_amd.testing.mxfp8_ref (the quantiser's restatement)."""
    from omgsr_amd import ops
    from omgsr_amd.testing import mxfp8_ref

    def host_quant(w):
        c, s = mxfp8_ref(w)
        return ops.Mxfp8(c, s)
    bf16.setattr(ops, "quantize_mxfp8", host_quant)
    g = torch.Generator().manual_seed(11)
    inner, cin = 160, 320
    w = torch.randn(2 * inner, cin, generator=g).to(torch.bfloat16)
    b = torch.randn(2 * inner, generator=g)
    pw = ops.pack_geglu_weight_mxfp8(w, b)
    assert pw.fp8 and pw.geglu and pw.cout == inner and pw.cin == 384 and pw.w.shape == (512, 384) and pw.w_scale.shape == (512, 12)
    assert pw.bias.dtype == torch.float32 and pw.bias.shape == (512,)
    ref = ops.pack_geglu_weight(w, b)                                       # the bf16 pack: the same interleave
    wc, ws = mxfp8_ref(ref.w[:2 * inner, :cin].float())
    assert torch.equal(pw.w[:2 * inner, :320], wc) and torch.equal(pw.w_scale[:2 * inner, :10], ws)
    assert not pw.w[:, 320:].any() and not pw.w_scale[:, 10:].any() and not pw.w[2 * inner:].any() and not pw.w_scale[2 * inner:].any()
    assert torch.equal(pw.bias[:2 * inner], ref.bias) and not pw.bias[2 * inner:].any()
    # row 0 .. 31 are the value rows 0 .. 31, rows 32 .. 63 the gate rows 0 .. 31
    assert torch.equal(pw.bias[:32], b[:32]) and torch.equal(pw.bias[32:64], b[inner:inner + 32]) and torch.equal(pw.bias[64:96], b[32:64])
    with pytest.raises(ValueError):
        ops.pack_geglu_weight_mxfp8(torch.zeros(2 * 48, 128, dtype=torch.bfloat16), None)       # inner % 32
    bf16.setattr(ops, "_ACT", torch.float16)
    with pytest.raises(ValueError):
        ops.pack_geglu_weight_mxfp8(w, b)
