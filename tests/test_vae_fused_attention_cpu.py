"""The fused head_dim-512 VAE attention without a GPU: the compiler's resource figures of vae_attn_kernel, the routing of VaeAttention as a pure
function of (tokens, tier, switch, environment knob), and ops.attention's argument checks that need no device."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vae_attn_kernel_resources():
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import PINNED_PREFIXES
    finally:
        sys.path.pop(0)
    from omgsr_amd.build import kernel_resources
    res = {name: v for name, v in kernel_resources().items() if "vae_attn_kernel" in name}
    # <compute type, channels per workgroup, two-term-split q / k>
    assert sorted(res) == ["vae_attn_kernel<bf16,128,1>", "vae_attn_kernel<bf16,256,0>", "vae_attn_kernel<fp16,128,1>", "vae_attn_kernel<fp16,256,0>"], sorted(res)
    for name, v in res.items():
        assert v["source"] == "attention_d512.hip"
        assert v["spill_vgpr"] == 0 and v["scratch"] == 0 and v["occupancy"] >= 1, (name, v)
        assert v["vgpr"] + v["agpr"] <= 512, (name, v)
        assert not name.startswith(PINNED_PREFIXES), name


ROUTES = [
    # L, precise, attn_split, module switch, env knob -> path
    (4096, False, False, None, None, "materialised"),
    (16384, False, False, None, None, "materialised"),
    (16385, False, False, None, None, "fused"),
    (20480, False, False, None, None, "fused"),
    (65536, True, False, None, None, "fused"),              # accurate tier (fp16 operands)
    (16384, True, False, None, None, "materialised"),
    (4096, False, False, True, None, "fused"),
    (4096, True, False, True, None, "fused"),
    (20480, False, False, False, None, "materialised"),     # switch off: the softmax kernel refuses the row, as before
    (4096, False, False, None, True, "fused"),              # the knob stands in for an unset switch ...
    (20480, False, False, None, False, "materialised"),
    (4096, False, False, False, True, "materialised"),      # ... and the module's switch wins over it
    (4096, False, False, True, False, "fused"),
    (4096, True, True, None, None, "materialised"),         # range-fallback tier: materialised whatever the switch
    (4096, True, True, True, True, "materialised"),
    (16384, True, True, True, None, "materialised"),
    (20480, False, True, None, None, "fused"),              # attn_split only means something in the accurate tier
]


@pytest.mark.parametrize("L,precise,attn_split,switch,env,want", ROUTES)
def test_routing_table(L, precise, attn_split, switch, env, want):
    from omgsr_amd.diffusers_api.autoencoder_kl import vae_attention_route
    assert vae_attention_route(L, precise, attn_split, switch, env) == want


@pytest.mark.parametrize("switch,env", [(None, None), (True, None), (False, None), (None, True)])
def test_routing_range_fallback_past_the_limit_names_it(switch, env):
    from omgsr_amd.diffusers_api.autoencoder_kl import vae_attention_route
    with pytest.raises(ValueError, match="range-fallback VAE attention is limited to 16384 keys"):
        vae_attention_route(16385, True, True, switch, env)


def test_knob_parsing_and_module_default():
    from omgsr_amd.diffusers_api import AutoencoderKL
    from omgsr_amd.diffusers_api import autoencoder_kl as M
    assert M._parse_fused_knob(None) is None and M._parse_fused_knob("") is None
    assert M._parse_fused_knob("1") is True and M._parse_fused_knob(" 0 ") is False
    for junk in ("yes", "2", "on", "-1", "1.0"):
        assert M._parse_fused_knob(junk) is None                        # malformed: the guarded default (automatic), no exception
    vae = AutoencoderKL(block_out_channels=[32, 32, 32, 64], layers_per_block=1)
    mids = [m for m in vae.modules() if isinstance(m, M.VaeAttention)]
    assert len(mids) == 2 and all(m.fused is None for m in mids)
    vae.set_fused_attention(True)
    assert all(m.fused is True for m in mids)
    vae.set_fused_attention(None)
    assert all(m.fused is None for m in mids)
    with pytest.raises(ValueError):
        vae.set_fused_attention("1")


@pytest.mark.parametrize("value,want", [("1", "True"), ("0", "False"), ("maybe", "None"), (None, "None")])
def test_knob_is_read_once_at_import(value, want):
    env = {k: v for k, v in os.environ.items() if k != "OMGSR_VAE_ATTN_FUSED"}
    if value is not None:
        env["OMGSR_VAE_ATTN_FUSED"] = value
    code = "from omgsr_amd.diffusers_api import autoencoder_kl as M; print(M._ENV_FUSED)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == want


def test_attention_argument_checks_at_512():
    """Raised in Python, before the library is loaded or a device is touched."""
    from omgsr_amd import ops
    B, L, D = 1, 64, 512
    q = torch.zeros(B, L, 2 * D, dtype=ops.act_dtype())
    vt = torch.zeros(B, D, L, dtype=ops.act_dtype())
    with pytest.raises(ValueError, match="out_split 1 or 2"):
        ops.attention(q, q, vt, 1, D, D ** -0.5, out_split=3)
    with pytest.raises(ValueError, match="single V\\^T"):
        ops.attention(q, q, torch.zeros(B, 2 * D, L, dtype=ops.act_dtype()), 1, D, D ** -0.5, q_lo_col=D, k_lo_col=D, p_split=False)
    with pytest.raises(ValueError, match="p_split=False"):
        ops.attention(q, q, vt, 1, D, D ** -0.5, q_lo_col=D, k_lo_col=D)
    with pytest.raises(ValueError, match="head_dim 128"):
        m = ops.Mxfp8(torch.zeros(B, L, D, dtype=torch.uint8), torch.zeros(B, L, D // 32, dtype=torch.uint8))
        ops.attention(m, m, ops.Mxfp8(torch.zeros(B, D, 128, dtype=torch.uint8), torch.zeros(B, D, 4, dtype=torch.uint8)), 1, D, D ** -0.5)
