"""Host-side logic of the fused GroupNorm-apply + 1x1 shortcut launch (csrc/norm_shortcut.hip) on CPU, no kernel run: the routing predicate
serves exactly the shapes and forms the kernel has, the 16-bit tiers and the off switch keep the old path, the weight pack is the layout
include/omgsr_hip.h documents, and the shipped precision policy is untouched."""
import itertools

import pytest
import torch


@pytest.fixture()
def tier(monkeypatch):
    """Set the tier's two module globals without the library (ops.set_compute_dtype also calls into it)."""
    from omgsr_amd import ops

    def set_(precise, act):
        monkeypatch.setattr(ops, "_PRECISE", precise)
        monkeypatch.setattr(ops, "_ACT", act)
    monkeypatch.delenv("OMGSR_GN_SHORTCUT_FUSED", raising=False)
    set_(True, torch.float16)
    return set_


def test_predicate_serves_exactly_the_kernel_shapes_and_forms(tier):
    from omgsr_amd import ops
    served = (128, 256, 512)
    for cin, cout, split in itertools.product((64, 128, 192, 256, 320, 512, 640, 1024), (64, 128, 256, 320, 512, 640, 1280), (1, 2, 3, 4, 5)):
        want = cin in served and cout in served and split in (1, 4)
        assert ops.gn_shortcut_ok(torch.float32, (cout, cin, 1, 1), 1, 0, 32, split) is want, (cin, cout, split)
    ok = ((128, 256, 1, 1), 1, 0, 32, 4)
    assert ops.gn_shortcut_ok(torch.float32, *ok)
    assert not ops.gn_shortcut_ok(torch.float16, *ok) and not ops.gn_shortcut_ok(torch.bfloat16, *ok)          # a 16-bit stream tensor
    assert not ops.gn_shortcut_ok(torch.float32, (128, 256, 3, 3), 1, 0, 32, 4)                                   # not a 1x1 kernel
    assert not ops.gn_shortcut_ok(torch.float32, (128, 256, 1, 1), 2, 0, 32, 4)                                   # strided
    assert not ops.gn_shortcut_ok(torch.float32, (128, 256, 1, 1), 1, 1, 32, 4)                                   # padded
    assert not ops.gn_shortcut_ok(torch.float32, (128, 256, 1, 1), 1, 0, 48, 4)                                   # C % G
    assert not ops.gn_shortcut_ok(torch.float32, (128, 256), 1, 0, 32, 4)                                         # a linear weight


def test_16_bit_tiers_range_fallback_and_the_switch_take_the_old_path(tier, monkeypatch):
    from omgsr_amd import ops
    ok = (torch.float32, (256, 128, 1, 1), 1, 0, 32, 1)
    assert ops.gn_shortcut_ok(*ok)
    tier(False, torch.bfloat16)
    assert not ops.gn_shortcut_ok(*ok)
    tier(False, torch.float16)
    assert not ops.gn_shortcut_ok(*ok)
    tier(True, torch.bfloat16)                      # the range-fallback tier: bf16 operands, a form the kernel does not have
    assert not ops.gn_shortcut_ok(*ok)
    tier(True, torch.float16)
    monkeypatch.setenv("OMGSR_GN_SHORTCUT_FUSED", "0")
    assert not ops.gn_shortcut_enabled() and not ops.gn_shortcut_ok(*ok)
    monkeypatch.setenv("OMGSR_GN_SHORTCUT_FUSED", "1")
    assert ops.gn_shortcut_ok(*ok)


def test_shipped_policy_is_unchanged_and_routes_the_four_vae_layers(tier):
    from omgsr_amd import nn as N
    from omgsr_amd import precision as P
    from omgsr_amd.diffusers_api import AutoencoderKL, UNet2DConditionModel
    with torch.device("meta"):
        v, u = AutoencoderKL(), UNet2DConditionModel()
    P.apply_default_policy(vae=v, unet=u)

    def forms(model, kinds):
        out = {}
        for _, m in model.named_modules():
            if isinstance(m, kinds):
                out[(m.op_split, m.w_split)] = out.get((m.op_split, m.w_split), 0) + 1
        return out

    # the counts tests/test_precision_cpu.py pins: the 1x1 shortcuts keep their (3, 2) form - the fused launch is a routing decision at the
    # call sites, not a policy change
    assert forms(v, (N.Conv2d, N.Linear)) == {(4, 2): 33, (3, 2): 4, (1, 1): 18, (2, 2): 17}
    assert forms(u, N.Conv2d) == {(2, 2): 5, (4, 2): 20, (3, 2): 17, (1, 1): 24}

    def routed(model):
        names = []
        for n, b in model.named_modules():
            sc = getattr(b, "conv_shortcut", None)
            if sc is not None:
                x = torch.empty((1, 1, 1, sc.in_channels), device="meta", dtype=torch.float32)
                if sc.gn_shortcut(x, b.norm1, b.conv1.in_split()):
                    names.append(n)
        return names

    four = ["encoder.down_blocks.1.resnets.0", "encoder.down_blocks.2.resnets.0", "decoder.up_blocks.2.resnets.0", "decoder.up_blocks.3.resnets.0"]
    assert routed(v) == four
    assert routed(u) == []                          # the UNet's shortcuts (320 / 640 / 1280 channels) are not served
    tier(False, torch.bfloat16)
    assert routed(v) == []
    tier(True, torch.float16)
    blk = v.decoder.up_blocks[3].resnets[0]
    x16 = torch.empty((1, 1, 1, 256), device="meta", dtype=torch.float16)
    assert not blk.conv_shortcut.gn_shortcut(x16, blk.norm1, blk.conv1.in_split())
    assert not blk.conv_shortcut.gn_shortcut(torch.empty((1, 1, 1, 256), device="meta"), blk.norm1, 2)          # a two-term split conv1 operand
    assert not blk.conv_shortcut.gn_shortcut(torch.empty((1, 1, 1, 256), device="meta"), blk.norm1, 3)          # an OMGSR_EL_MX conv1 operand


def test_weight_pack_layout_and_cache(tier):
    from omgsr_amd import nn as N
    from omgsr_amd import ops
    cout, cin = 128, 256
    g = torch.Generator().manual_seed(3)
    w = torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5
    b = torch.randn(cout, generator=g)
    sw = ops.pack_gn_shortcut_weight(w, b)
    assert sw.w.dtype == torch.float16 and tuple(sw.w.shape) == (cin // 64, 4, cout // 32, 2, 64, 8) and sw.w.is_contiguous()
    assert torch.equal(sw.bias, b) and (sw.cin, sw.cout) == (cin, cout)
    w2 = w.reshape(cout, cin)
    hi = w2.to(torch.float16)
    lo = (w2 - hi.float()).to(torch.float16)
    for chunk, step, tile_, lane, j in [(0, 0, 0, 0, 0), (3, 2, 1, 37, 5), (1, 3, 3, 63, 7), (2, 1, 2, 31, 0), (3, 3, 3, 32, 1)]:
        n, c = 32 * tile_ + (lane & 31), 64 * chunk + 16 * step + 8 * (lane >> 5) + j
        assert sw.w[chunk, step, tile_, 0, lane, j] == hi[n, c] and sw.w[chunk, step, tile_, 1, lane, j] == lo[n, c]
    # hi + lo carries the fp32 weight to 2^-22
    back = (sw.w[:, :, :, 0].float() + sw.w[:, :, :, 1].float()).reshape(cin // 64, 4, cout // 32, 2, 32, 8).permute(2, 4, 0, 1, 3, 5).reshape(cout, cin)
    assert ((back - w2).norm() / w2.norm()).item() < 2.0 ** -20
    with pytest.raises(ValueError):
        ops.pack_gn_shortcut_weight(torch.zeros(128, 256, 3, 3), None)
    # the module's pack is cached under a key of its own and re-packed (with a cache-epoch bump) when the weight changes
    conv = N.Conv2d(cin, cout, 1)
    p1 = conv.packed_gn_shortcut()
    assert conv.packed_gn_shortcut() is p1
    e = N.cache_epoch()
    with torch.no_grad():
        conv.weight.mul_(2.0)
    p2 = conv.packed_gn_shortcut()
    assert p2 is not p1 and N.cache_epoch() > e and torch.equal(p2.w[..., 0, :, :].float(), (conv.weight.detach().reshape(cout, cin).to(torch.float16).float()
                                                                                        .reshape(cout // 32, 32, cin // 64, 4, 2, 8).permute(2, 3, 0, 4, 1, 5).reshape(cin // 64, 4, cout // 32, 64, 8)))
