"""The fp8 tier's fused MXFP8 producers, the parts that need no GPU: the host reference of layer_norm_mxfp8, the function that decides which
producers of a block fuse, the combinations ops.linear(out_mxfp8=...) refuses, and the parsing of OMGSR_FP8_FUSED_QUANT."""
import pytest
import torch


def test_layer_norm_mxfp8_ref_against_fp64_by_hand():
    from omgsr_amd.testing import layer_norm_mxfp8_ref, mxfp8_ref
    g = torch.Generator().manual_seed(17)
    x = (torch.randn(3, 64, generator=g) * torch.tensor([[2.0 ** -9], [1.0], [2.0 ** 11]])).to(torch.bfloat16)
    a, b = torch.randn(64, generator=g) + 1.0, torch.randn(64, generator=g) * 0.25
    eps = 1e-6
    xd = x.double()
    rows = []
    for r in range(3):                                          # by hand: mean, centred variance, affine, one rounding to bf16
        mu = sum(float(v) for v in xd[r]) / 64
        var = sum((float(v) - mu) ** 2 for v in xd[r]) / 64
        rows.append(torch.tensor([(float(v) - mu) / (var + eps) ** 0.5 * float(a[c]) + float(b[c]) for c, v in enumerate(xd[r])], dtype=torch.float64))
    want_c, want_s = mxfp8_ref(torch.stack(rows).to(torch.bfloat16))
    got_c, got_s = layer_norm_mxfp8_ref(x, a, b, eps)
    assert got_c.shape == (3, 64) and got_s.shape == (3, 2) and got_c.dtype == got_s.dtype == torch.uint8
    assert torch.equal(got_s, want_s) and torch.equal(got_c, want_c)
    # no affine: a = 1, b = 0
    plain_c, plain_s = layer_norm_mxfp8_ref(x, None, None, eps)
    ones_c, ones_s = layer_norm_mxfp8_ref(x, torch.ones(64), torch.zeros(64), eps)
    assert torch.equal(plain_c, ones_c) and torch.equal(plain_s, ones_s)


ON = {"layernorm": True, "gemm": True}


def test_producer_selection_on_the_flag_patterns():
    from omgsr_amd.diffusers_api.transformer_flux import fused_quant_plan
    double = lambda v, **kw: {**dict.fromkeys(("to_q", "to_v", "add_q", "add_v", "ff0", "ff2", "ffc0", "ffc2"), v), **kw}
    single = lambda v, **kw: {**dict.fromkeys(("to_q", "to_v", "proj_mlp", "proj_out"), v), **kw}
    # all fp8: everything fuses
    assert fused_quant_plan(double(True), ON) == dict(ln1=True, ln1_ctx=True, ln2=True, ln2_ctx=True, ff=True, ffc=True)
    assert fused_quant_plan(single(True), ON) == dict(ln=True, cat8=True)
    # q / k / v fp8 but proj_mlp not: the LayerNorm has a bf16 reader and proj_mlp writes no MXFP8 - today's path for both
    assert fused_quant_plan(single(True, proj_mlp=False), ON) == dict(ln=False, cat8=False)
    # net[0] fp8 but net[2] not: the LayerNorm in front still fuses (its only reader is net[0]), the hidden stays bf16
    got = fused_quant_plan(double(True, ff2=False), ON)
    assert got == dict(ln1=True, ln1_ctx=True, ln2=True, ln2_ctx=True, ff=False, ffc=True)
    # nothing fp8
    assert not any(fused_quant_plan(double(False), ON).values()) and not any(fused_quant_plan(single(False), ON).values())
    # a mixed q / v set keeps the pass form for that LayerNorm only
    assert fused_quant_plan(double(True, add_v=False), ON)["ln1_ctx"] is False and fused_quant_plan(double(True, add_v=False), ON)["ln1"] is True
    assert fused_quant_plan(single(True, proj_out=False), ON) == dict(ln=True, cat8=False)
    # the switch: each producer kind on its own, and everything off
    assert fused_quant_plan(double(True), {"layernorm": True, "gemm": False}) == dict(ln1=True, ln1_ctx=True, ln2=True, ln2_ctx=True, ff=False, ffc=False)
    assert fused_quant_plan(single(True), {"layernorm": False, "gemm": True}) == dict(ln=False, cat8=True)
    assert not any(fused_quant_plan(double(True), {"layernorm": False, "gemm": False}).values())


def test_producer_selection_reads_the_block_flags():
    """The blocks feed the function their layers' .fp8 flags: a narrowed policy shows up in the plan."""
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api.transformer_flux import fused_quant_plan
    assert set(ops.FP8_FUSED_QUANT) == {"layernorm", "gemm"}
    assert set(fused_quant_plan(dict(to_q=True, to_v=True, proj_mlp=True, proj_out=True))) == {"ln", "cat8"}      # default switch: ops.FP8_FUSED_QUANT


def test_producer_selection_falls_back_on_shape():
    """A width the fused kernels do not take keeps the pass form instead of raising: LayerNorm rows that are no multiple of 128 or wider than
    4096, an MXFP8 hidden / [attn | mlp] operand that is not whole 128-column groups."""
    from omgsr_amd.diffusers_api.transformer_flux import fused_quant_plan
    double = dict.fromkeys(("to_q", "to_v", "add_q", "add_v", "ff0", "ff2", "ffc0", "ffc2"), True)
    single = dict.fromkeys(("to_q", "to_v", "proj_mlp", "proj_out"), True)
    assert all(fused_quant_plan(double, ON, dim=3072, hidden=12288).values()) and all(fused_quant_plan(single, ON, dim=256, hidden=1024).values())
    assert fused_quant_plan(double, ON, dim=5120, hidden=20480) == dict(ln1=False, ln1_ctx=False, ln2=False, ln2_ctx=False, ff=True, ffc=True)
    assert fused_quant_plan(double, ON, dim=320, hidden=1280) == dict(ln1=False, ln1_ctx=False, ln2=False, ln2_ctx=False, ff=True, ffc=True)
    assert fused_quant_plan(double, ON, dim=256, hidden=1056) == dict(ln1=True, ln1_ctx=True, ln2=True, ln2_ctx=True, ff=False, ffc=False)
    assert fused_quant_plan(single, ON, dim=320, hidden=1280) == dict(ln=False, cat8=False)
    assert fused_quant_plan(single, ON, dim=256, hidden=1056) == dict(ln=True, cat8=False)


def test_single_block_plan_is_what_the_workspace_allocation_reads():
    from omgsr_amd.diffusers_api.transformer_flux import FluxSingleTransformerBlock, fused_quant_plan
    blk = FluxSingleTransformerBlock(256, 2, 128)
    assert not any(blk.quant_plan().values())
    for lin in (blk.attn.to_q, blk.attn.to_k, blk.attn.to_v, blk.proj_mlp, blk.proj_out):
        lin.fp8 = True
    assert blk.quant_plan() == fused_quant_plan(dict(to_q=True, to_v=True, proj_mlp=True, proj_out=True), dim=256, hidden=1024)
    blk.proj_out.fp8 = False
    assert blk.quant_plan()["cat8"] is False


def _fp8_weight(cout=256, cin=128):
    from omgsr_amd import ops
    return ops.PackedWeight(torch.zeros(cout, cin, dtype=torch.uint8), torch.zeros(cout), cout, cin, 1, 1,
                            w_scale=torch.zeros(cout, cin // 32, dtype=torch.uint8))


def test_linear_out_mxfp8_refused_combinations():
    from omgsr_amd import ops
    pw8 = _fp8_weight()
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="residual"):
        ops.linear(x, pw8, residual=torch.zeros(4, 256, dtype=torch.bfloat16), out_mxfp8=True)
    with pytest.raises(ValueError, match="gate"):
        ops.linear(x, pw8, gate=torch.zeros(256), out_mxfp8=True)
    pw16 = ops.pack_linear_weight(torch.zeros(256, 128, dtype=torch.bfloat16), None)
    assert not pw16.fp8
    with pytest.raises(ValueError, match="fp8-packed"):
        ops.linear(x, pw16, out_mxfp8=True)
    # the other forms the epilogue does not write, and destinations that do not fit
    with pytest.raises(ValueError):
        ops.linear(x, pw8, out_dtype=ops.OUT_F32, out_mxfp8=True)
    with pytest.raises(ValueError):
        ops.linear(x, pw8, gn_groups=4, out_mxfp8=True)
    dst = ops.Mxfp8(torch.zeros(4, 384, dtype=torch.uint8), torch.zeros(4, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="fit"):
        ops.linear_into(x, pw8, None, 0, 256, out_mxfp8=dst)                      # 256 + 256 > 384
    with pytest.raises(ValueError, match="fit"):
        ops.linear_into(x, pw8, None, 0, 64, out_mxfp8=dst)                       # column offset % 128
    with pytest.raises(ValueError, match="residual"):
        ops.linear_into(x, pw8, None, 0, 128, residual=torch.zeros(4, 256, dtype=torch.bfloat16), out_mxfp8=dst)
    with pytest.raises(ValueError):
        ops.linear_into(x, pw8, torch.zeros(4, 384, dtype=torch.bfloat16), 0, 128, out_mxfp8=dst)      # two destinations


def test_fused_quant_switch_parsing():
    from omgsr_amd import ops
    assert ops.parse_fp8_fused_quant(None) == ops.FP8_FUSED_QUANT_DEFAULT and ops.parse_fp8_fused_quant("") == ops.FP8_FUSED_QUANT_DEFAULT
    assert ops.parse_fp8_fused_quant(None) is not ops.FP8_FUSED_QUANT_DEFAULT           # a copy: the defaults are not edited through it
    assert ops.parse_fp8_fused_quant("0") == {"layernorm": False, "gemm": False}
    assert ops.parse_fp8_fused_quant("1") == {"layernorm": True, "gemm": True}
    assert ops.parse_fp8_fused_quant(" 1 ") == {"layernorm": True, "gemm": True}
    for bad in ("2", "on", "-1"):
        with pytest.raises(ValueError):
            ops.parse_fp8_fused_quant(bad)


def test_quantize_out_col_validation():
    from omgsr_amd import ops
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    dst = ops.Mxfp8(torch.zeros(4, 384, dtype=torch.uint8), torch.zeros(4, 12, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.quantize_mxfp8(x, out_col=0)                                          # no destination
    with pytest.raises(ValueError):
        ops.quantize_mxfp8(x, out=dst, out_col=320)                               # past the end
    with pytest.raises(ValueError):
        ops.quantize_mxfp8(x, out=dst, out_col=32)                                # not a multiple of 128
