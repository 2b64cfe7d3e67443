"""The fp8 tier without a GPU: the MXFP8 format's reference quantiser (include/omgsr_hip.h OMGSR_EL_MXFP8), the layer policy
(precision.set_fp8_linear / FLUX_FP8 on the full-size FLUX.1-dev module tree, built on the meta device), the tier contract's
ValueError cases and the compiler's resource figures of the new GEMM kernel."""
import re

import pytest
import torch

from omgsr_amd.testing import mxfp8_dequant, mxfp8_ref


def test_reference_quantiser_edge_rows():
    K = 128
    x = torch.zeros(6, K)
    x[1, :32] = torch.tensor([2.0 ** e for e in range(-16, 16)])            # exact powers of two, 32 binades in one block
    x[2, :32] = 448.0 * 2.0 ** 3                                            # saturating values: 448 2^s
    x[2, 32:64] = -448.0 * 2.0 ** -20
    x[3, :32] = torch.tensor([(-1) ** i * 1.5 * 2.0 ** (i % 15) for i in range(32)])   # 14+ binades of spread
    x[4, 64:96] = 2.0 ** -130                                               # fp32 subnormals: scale 0
    x[5] = torch.linspace(-3.0, 5.0, K)
    codes, scales = mxfp8_ref(x)
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and scales.shape == (6, K // 32)
    assert int(scales[0].max()) == 0 and int(codes[0].max()) == 0          # all-zero blocks: scale 0, zero codes
    # exact powers of two survive while they are within the e4m3 range under the block's scale (2^15 max -> scale 127 + 15 - 8)
    assert int(scales[1, 0]) == 127 + 15 - 8
    d = mxfp8_dequant(codes, scales)
    x = x.double()
    assert torch.equal(d[1, 23:32], x[1, 23:32])                            # 2^7 .. 2^15 are normal codes under scale 2^7
    # 448 2^s: the block's largest value sits at the top code (0x7e), never NaN (0x7f)
    assert int(scales[2, 0]) == 127 + 3 + 8 - 8 and int(codes[2, 0]) == 0x7E and torch.equal(d[2, :32], x[2, :32])
    assert torch.equal(d[2, 32:64], x[2, 32:64]) and int(codes[2, 32]) == 0xFE
    assert not torch.isnan(d).any()
    assert int(scales[4, 2]) == 0
    # 15 binades under one scale: every value keeps a normal code, relative error <= 2^-4 (here: exact)
    assert ((d[3, :32] - x[3, :32]).abs() / x[3, :32].abs()).max() <= 2.0 ** -4 and bool(((codes[3, :32] & 0x78) != 0).all())


def test_reference_quantiser_relative_error_on_normal_codes():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 256, generator=g) * torch.exp2(torch.randint(-20, 20, (64, 1), generator=g).float())
    codes, scales = mxfp8_ref(x)
    d = mxfp8_dequant(codes, scales)
    q = x.double() / torch.exp2(scales.double() - 127).repeat_interleave(32, dim=1)
    normal = ((codes & 0x78) != 0) & (q.abs() <= 448)                       # normal codes (exponent field != 0), not saturated
    rel = ((d - x.double()).abs() / x.double().abs())[normal]
    assert normal.float().mean() > 0.9 and float(rel.max()) <= 2.0 ** -4
    # the statement of the format (the clamp first: torch does not saturate on this cast)
    s = scales.repeat_interleave(32, dim=1).float()
    want = (x / torch.exp2(s - 127)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(codes, want)


def _meta_flux():
    from omgsr_amd.diffusers_api import FluxTransformer2DModel
    with torch.device("meta"):
        return FluxTransformer2DModel()


def test_flux_fp8_policy_marks_exactly_the_token_linears():
    from omgsr_amd.nn import Linear
    from omgsr_amd.precision import FLUX_FP8, fp8_layers, set_fp8_linear
    m = _meta_flux()
    n = set_fp8_linear(m, FLUX_FP8)
    names = set(fp8_layers(m))
    double = ["attn.to_q", "attn.to_k", "attn.to_v", "attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj", "attn.to_out.0", "attn.to_add_out",
              "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2"]
    single = ["attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp", "proj_out"]
    want = {f"transformer_blocks.{i}.{s}" for i in range(19) for s in double} | {f"single_transformer_blocks.{i}.{s}" for i in range(38) for s in single}
    assert names == want and n == len(want) == 19 * 12 + 38 * 5
    excluded = [name for name, mod in m.named_modules() if isinstance(mod, Linear) and name not in want]
    for must_stay in ("x_embedder", "context_embedder", "proj_out", "norm_out.linear", "transformer_blocks.0.norm1.linear",
                      "single_transformer_blocks.0.norm.linear", "time_text_embed.timestep_embedder.linear_1"):
        assert must_stay in excluded, must_stay
    assert not any(re.search(r"(norm|embed)", x) for x in names)
    # a user list narrows (and a q | k pair moves together: to_q alone moves neither)
    n2 = set_fp8_linear(m, [r"single_transformer_blocks\.\d+\.proj_out$", r"transformer_blocks\.0\.attn\.to_q$", r"^x_embedder$"])
    assert set(fp8_layers(m)) == {f"single_transformer_blocks.{i}.proj_out" for i in range(38)} and n2 == 38


def test_tier_contract_value_errors(monkeypatch):
    from omgsr_amd import ops
    from omgsr_amd.nn import Linear
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    from omgsr_amd.precision import FLUX_FP8, set_fp8_linear
    with pytest.raises(ValueError):
        OMGSR_S_Infer(None, None, 273, "cpu", torch.float8_e4m3fn)
    m = _meta_flux()
    monkeypatch.setattr(ops, "_PRECISE", True)                              # the accurate tier
    with pytest.raises(ValueError):
        set_fp8_linear(m, FLUX_FP8)
    monkeypatch.setattr(ops, "_PRECISE", False)
    set_fp8_linear(m, FLUX_FP8)
    monkeypatch.setattr(ops, "_ACT", torch.float16)                         # fp16: an fp8 layer cannot be packed
    lin = m.transformer_blocks[0].ff.net[2]
    assert isinstance(lin, Linear) and lin.fp8
    with pytest.raises(ValueError):
        lin.packed()


def test_fp8_tier_value_error_for_a_wrong_policy():
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    with pytest.raises(ValueError):
        OMGSR_F_Infer(None, None, "cpu", torch.float8_e4m3fn, precision_policy="all")


def test_mxfp8_kernel_resources():
    import os
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import kernel_resources
    res = kernel_resources()
    k = [v for name, v in res.items() if "mxfp8_gemm_kernel" in name]
    assert len(k) == 1, sorted(res)
    k = k[0]
    assert k["spill_vgpr"] == 0 and k["scratch"] == 0 and k["occupancy"] >= 2, k
    q = [v for name, v in res.items() if "mxfp8_quantize_kernel" in name]
    assert len(q) == 2 and all(v["spill_vgpr"] == 0 and v["scratch"] == 0 for v in q)
