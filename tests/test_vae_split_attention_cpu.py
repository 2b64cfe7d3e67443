"""The range-fallback tier's fused head_dim-512 attention (vae_attn_full_kernel: every operand a two-term split) without a GPU: the compiler's
resource figures, the routing with the tier's opt-in, the module switch / setter / environment knob, and ops.attention's argument checks."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "vae_attn_full_kernel"


def test_vae_attn_full_kernel_resources():
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import kernel_resources
    res = {name: v for name, v in kernel_resources().items() if KERNEL in name}
    # <compute type, channels per workgroup>: 8 parts per query tile; two stages of [K_hi | K_lo | V^T_hi | V^T_lo] are 149504 B of dynamic LDS
    assert sorted(res) == [f"{KERNEL}<bf16,64>", f"{KERNEL}<fp16,64>"], sorted(res)
    for name, v in res.items():
        print(name, v)
        assert v["source"] == "attention_d512.hip"
        assert v["spill_vgpr"] == 0 and v["scratch"] == 0 and v["occupancy"] >= 1, (name, v)
        assert v["vgpr"] + v["agpr"] <= 512, (name, v)


@pytest.mark.parametrize("L", [1024, 16384, 16385, 65536])
@pytest.mark.parametrize("switch", [None, True, False])
@pytest.mark.parametrize("env", [None, True, False])
def test_routing_opt_in_takes_the_tier_at_every_size(L, switch, env):
    from omgsr_amd.diffusers_api.autoencoder_kl import vae_attention_route
    assert vae_attention_route(L, True, True, switch, env, rf_fused=True) == "fused_split"


def test_routing_opt_in_changes_no_other_tier():
    from omgsr_amd.diffusers_api.autoencoder_kl import vae_attention_route
    from test_vae_fused_attention_cpu import ROUTES
    rows = [r for r in ROUTES if not (r[1] and r[2])]
    assert len(rows) >= 13
    for L, precise, attn_split, switch, env, want in rows:
        assert vae_attention_route(L, precise, attn_split, switch, env, rf_fused=True) == want
        assert vae_attention_route(L, precise, attn_split, switch, env, rf_fused=False) == want


@pytest.mark.parametrize("switch,env", [(None, None), (True, None), (False, None), (None, True)])
def test_routing_without_the_opt_in_is_unchanged(switch, env):
    from omgsr_amd.diffusers_api.autoencoder_kl import vae_attention_route
    for kw in ({}, {"rf_fused": False}):
        assert vae_attention_route(16384, True, True, switch, env, **kw) == "materialised"
        with pytest.raises(ValueError, match="range-fallback VAE attention is limited to 16384 keys"):
            vae_attention_route(16385, True, True, switch, env, **kw)


def test_setter_and_module_default():
    from omgsr_amd import precision
    from omgsr_amd.diffusers_api import AutoencoderKL
    from omgsr_amd.diffusers_api import autoencoder_kl as M
    vae = AutoencoderKL(block_out_channels=[32, 32, 32, 64], layers_per_block=1)
    mids = [m for m in vae.modules() if isinstance(m, M.VaeAttention)]
    assert len(mids) == 2 and all(m.fused_range_fallback is False for m in mids)
    before = precision.policy_epoch()
    vae.set_range_fallback_fused_attention(True)
    assert all(m.fused_range_fallback is True for m in mids) and all(m.fused is None for m in mids)
    assert precision.policy_epoch() != before              # a captured graph is keyed on the epoch: never replayed stale
    vae.set_range_fallback_fused_attention(False)
    assert all(m.fused_range_fallback is False for m in mids)
    for junk in ("1", 1, None):
        with pytest.raises(ValueError):
            vae.set_range_fallback_fused_attention(junk)
    assert all(m.fused_range_fallback is False for m in mids)


@pytest.mark.parametrize("value,want", [("1", "True"), (" 1 ", "True"), ("0", "False"), ("yes", "False"), ("2", "False"), ("", "False"), (None, "False")])
def test_knob_is_read_once_at_import(value, want):
    env = {k: v for k, v in os.environ.items() if k != "OMGSR_VAE_ATTN_FUSED_RF"}
    if value is not None:
        env["OMGSR_VAE_ATTN_FUSED_RF"] = value
    code = ("import os; from omgsr_amd.diffusers_api import autoencoder_kl as M; os.environ['OMGSR_VAE_ATTN_FUSED_RF'] = '1'; "
            "print(M._ENV_FUSED_RF)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == want


def test_attention_argument_checks_at_512_split_vt():
    """Raised in Python, before the library is loaded or a device is touched."""
    from omgsr_amd import ops
    B, L, D = 1, 64, 512
    q = torch.zeros(B, L, 2 * D, dtype=ops.act_dtype())
    vts = torch.zeros(B, 2 * D, L, dtype=ops.act_dtype())
    for kw in ({}, {"p_split": False}, {"q_lo_col": D}, {"k_lo_col": D}):
        with pytest.raises(ValueError, match="split V\\^T comes with split q / k"):
            ops.attention(q, q, vts, 1, D, D ** -0.5, **kw)
    with pytest.raises(ValueError, match="single V\\^T"):
        ops.attention(q, q, vts, 1, D, D ** -0.5, q_lo_col=D, k_lo_col=D, p_split=False)
    with pytest.raises(ValueError, match="out_split 1 or 2"):
        ops.attention(q, q, vts, 1, D, D ** -0.5, q_lo_col=D, k_lo_col=D, p_split=True, out_split=3)
