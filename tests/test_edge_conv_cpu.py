"""CPU checks of the fp32 edge convolution (csrc/conv_edge.hip): its ABI struct and symbol agree between include/omgsr_hip.h, omgsr_amd/_lib.py
and the library; the call sites route fp32 stream tensors with Cout <= 8 to it and the 16-bit tiers to the path they had; hipcc builds the
translation unit for gfx950 without scratch memory (the build's resource remarks)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "omgsr_hip.h")


def test_edge_group_layout_and_symbol_match_the_header(tmp_path):
    from omgsr_amd import _lib
    from omgsr_amd.build import build_library
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(omgsr_edge_group));']
    for fname, _ in _lib.EdgeGroup._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(omgsr_edge_group, {fname}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines() if ln.strip())
    assert int(got.pop("size")) == ctypes.sizeof(_lib.EdgeGroup)
    assert {k: int(v) for k, v in got.items()} == {f: getattr(_lib.EdgeGroup, f).offset for f, _ in _lib.EdgeGroup._fields_}
    # the declaration's parameter list against the ctypes signature: pointers, int32_t, then the stream
    decl = re.search(r"int omgsr_conv_out_gn\(([^;]*)\);", open(HEADER).read()).group(1)
    kinds = [ctypes.c_void_p if "*" in p else ctypes.c_int32 for p in decl.split(",")]
    res, args = _lib.SIGNATURES["omgsr_conv_out_gn"]
    assert res is ctypes.c_int and len(args) == len(kinds)
    assert args[0] is ctypes.POINTER(_lib.EdgeGroup) and list(args[1:]) == kinds[1:]
    assert hasattr(ctypes.CDLL(build_library()), "omgsr_conv_out_gn")


def test_bad_arguments_are_rejected_without_a_gpu():
    from omgsr_amd import _lib
    lib = _lib.load()
    g = (_lib.EdgeGroup * 1)()
    assert lib.omgsr_conv_out_gn(None, 1, 8, 8, 8, 8, 8, 8, 64, 3, 32, 1, None) == -1
    g[0].x, g[0].y, g[0].rows, g[0].H, g[0].W = 8, 8, 1, 4, 4
    assert lib.omgsr_conv_out_gn(g, 9, 8, 8, 8, 8, 8, 8, 64, 3, 32, 1, None) == -1          # more than OMGSR_GN_MAX_GROUPS
    assert lib.omgsr_conv_out_gn(g, 1, 8, 8, 8, 8, 8, 8, 48, 3, 16, 1, None) == -2          # Cin % 32
    assert lib.omgsr_conv_out_gn(g, 1, 8, 8, 8, 8, 8, 8, 64, 9, 32, 1, None) == -2          # Cout > 8
    assert lib.omgsr_conv_out_gn(g, 1, 8, 8, 8, 8, 8, 8, 2048, 3, 32, 1, None) == -2        # Cin > 1024
    g[0].H = g[0].W = 1 << 14
    assert lib.omgsr_conv_out_gn(g, 1, 8, 8, 8, 8, 8, 8, 64, 3, 32, 1, None) == -2          # H W Cin >= 2^31


@pytest.mark.parametrize("dtype,want", [(torch.float32, True), (torch.bfloat16, False), (torch.float16, False)])
def test_routing_predicate(dtype, want):
    from omgsr_amd import ops
    from omgsr_amd.nn import Conv2d, GroupNorm
    assert ops.edge_conv_out_ok(dtype, (3, 128, 3, 3), 1, 1, 32) is want
    norm = GroupNorm(32, 128)
    x = torch.zeros((1, 4, 4, 128), dtype=dtype)
    for cout in (3, 4, 8):
        assert Conv2d(128, cout, 3, padding=1).edge_out(x, norm) is want
    # never, whatever the stream type: wide outputs, other kernels / strides / paddings, channel counts the kernel does not serve
    assert not Conv2d(128, 16, 3, padding=1).edge_out(x, norm)
    assert not Conv2d(128, 4, 1).edge_out(x, norm)
    assert not Conv2d(128, 4, 3, stride=2, padding=1).edge_out(x, norm)
    assert not Conv2d(128, 4, 3, padding=0).edge_out(x, norm)
    assert not Conv2d(48, 4, 3, padding=1).edge_out(torch.zeros((1, 4, 4, 48), dtype=dtype), GroupNorm(16, 48))
    assert not Conv2d(2048, 4, 3, padding=1).edge_out(torch.zeros((1, 2, 2, 2048), dtype=dtype), GroupNorm(32, 2048))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_call_sites_route_by_stream_type(monkeypatch, dtype):
    """nn.norm_silu_conv (the UNet's and the untiled VAE's tail) and VAEHook._run (the tiled VAE's): fp32 stream tensors reach
    ops.conv_out_gn_multi with the un-normalised tensors and the norm's statistics; 16-bit ones reach Conv2d.nhwc / nhwc_multi with the norm."""
    from types import SimpleNamespace
    from omgsr_amd import nn as onn, ops
    from omgsr_amd.pipelines.vaehook import VAEHook
    norm, conv = onn.GroupNorm(32, 64), onn.Conv2d(64, 3, 3, padding=1)
    x = torch.zeros((2, 4, 4, 64), dtype=dtype)
    st = torch.zeros((2, 32))
    calls = []
    monkeypatch.setattr(ops, "conv_out_gn_multi", lambda xs, ew, mean, rstd, g, b, groups: calls.append(("edge", [t.dtype for t in xs], groups)) or list(xs))
    monkeypatch.setattr(onn.Conv2d, "packed_edge_out", lambda self: None)
    monkeypatch.setattr(onn.GroupNorm, "stats", lambda self, t: (st, st, st))
    monkeypatch.setattr(onn.GroupNorm, "spec_stats", lambda self, mean, rstd, act=0: "spec")
    monkeypatch.setattr(onn.Conv2d, "nhwc", lambda self, t, gn=None, **kw: calls.append(("nhwc", gn)) or t)
    monkeypatch.setattr(onn.Conv2d, "nhwc_multi", lambda self, xs, gn=None, **kw: calls.append(("nhwc_multi", gn)) or list(xs))
    monkeypatch.setattr(ops, "group_norm_stats_merged", lambda tensors, tiles, N, G, eps: (st, st, st))
    monkeypatch.setattr(onn.GroupNorm, "apply_stats_multi", lambda self, xs, *a, **kw: calls.append(("apply",)) or list(xs))
    onn.norm_silu_conv(norm, conv, x)
    hook = VAEHook(SimpleNamespace(conv_out=conv), 64, True, False, False, False)
    hook._run([("gn", norm, ops.ACT_SILU, conv, None), ("conv", conv, {})], {(4, 4): x}, {(4, 4): 1}, 2)
    if dtype == torch.float32:
        assert calls == [("edge", [dtype], 32), ("edge", [dtype], 32)]
    else:
        assert calls == [("nhwc", "spec"), ("nhwc_multi", "spec")]


def test_conv_edge_builds_for_gfx950_without_scratch():
    from omgsr_amd.build import kernel_resources
    mine = {k: v for k, v in kernel_resources().items() if v["source"] == "conv_edge.hip"}
    assert mine and all("edge_conv" in k for k in mine), sorted(mine)
    for name, r in mine.items():
        assert not name.startswith(("igemm_", "attn_", "gn_apply")), name
        assert r["scratch"] == 0 and r["spill_vgpr"] == 0, (name, r)
        assert r["agpr"] == 0, (name, r)                     # no MFMA accumulators: plain fp32 FMAs
        assert r["occupancy"] >= 2 and r["lds"] * 3 <= 160 * 1024, (name, r)      # three workgroups per CU by LDS
