"""Host-side checks of the ABI v21 GroupNorm entries: the ctypes mirror of omgsr_gn_apply_group against the header, argument checks that
return before any launch, and the rules by which ops.group_norm_pair takes the two-source path."""
import ctypes
import os
import shutil
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gn_apply_group_layout_matches_header(tmp_path):
    from omgsr_amd._lib import GN_MAX_GROUPS, GnApplyGroup
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "omgsr_hip.h")}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(omgsr_gn_apply_group));', '  printf("max %d\\n", OMGSR_GN_MAX_GROUPS);']
    for fname, _ in GnApplyGroup._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(omgsr_gn_apply_group, {fname}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "probe.c").write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c11", "-o", str(tmp_path / "probe"), str(tmp_path / "probe.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got.pop("size")) == ctypes.sizeof(GnApplyGroup)
    assert int(got.pop("max")) == GN_MAX_GROUPS
    assert {k: int(v) for k, v in got.items()} == {f: getattr(GnApplyGroup, f).offset for f, _ in GnApplyGroup._fields_}


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from omgsr_amd import _lib
    lib = _lib.load()
    g = (_lib.GnApplyGroup * 2)()
    assert lib.omgsr_groupnorm_apply_multi(None, 1, 8, 8, None, None, 64, 32, 0, 1, 1, 0, 0, None, None) == -1
    assert lib.omgsr_groupnorm_apply_multi(g, 9, 8, 8, None, None, 64, 32, 0, 1, 1, 0, 0, None, None) == -1           # more than OMGSR_GN_MAX_GROUPS
    assert lib.omgsr_groupnorm_apply_multi(g, 2, 8, 8, None, None, 64, 32, 0, 1, 1, 0, 0, None, None) == -1           # null tensors
    g[0].x, g[0].y, g[0].HW, g[0].rows = 8, 8, 16, 3
    assert lib.omgsr_groupnorm_apply_multi(g, 1, 8, 8, None, None, 64, 32, 0, 2, 1, 0, 0, None, None) == -1           # rows % stat_rows
    g[0].rows = 2
    assert lib.omgsr_groupnorm_apply_multi(g, 1, 8, 8, None, None, 60, 30, 0, 2, 1, 0, 0, None, None) == -2           # C % 8
    assert lib.omgsr_groupnorm_finalize2(None, 1, 8, 8, 1, 8, 8, 8, None, 1, 2, 1.0, 1e-5, None) == -1
    assert lib.omgsr_groupnorm_finalize2(8, 1, 8, 8, 1, 16, 8, 8, None, 1, 5, 1.0, 1e-5, None) == -2                  # (Ca + Cb) % G
    assert lib.omgsr_groupnorm_apply2(8, None, 8, 8, 8, 8, None, None, 1, 4, 16, 2, 0, 0, None, 0, None, None) == -1  # no second tensor
    assert lib.omgsr_groupnorm_apply2(8, 8, 12, 8, 8, 8, None, None, 1, 4, 32, 2, 0, 0, None, 0, None, None) == -1    # Ca % 8
    assert lib.omgsr_groupnorm_apply2(8, 8, 16, 8, 8, 8, None, None, 1, 4, 16, 2, 0, 0, None, 0, None, None) == -1    # Ca >= C


def test_pair_path_rules():
    """The two-source path needs fp32 stream tensors that both carry a valid per-channel handle; everything else is the old path."""
    from omgsr_amd import ops
    N, C1 = 2, 64
    a, b = torch.zeros(N, 4, 4, C1), torch.zeros(N, 4, 4, C1)
    assert ops.group_norm_pair_stats(a, b, 32, 1e-5) is None                      # no handles
    per_channel = torch.zeros(N, 3, C1, 2)
    per_group = torch.zeros(N, 3, 32, 2)
    a._omgsr_gn = (per_channel, 32, a.data_ptr(), a._version)
    assert ops._fused_gn_channels(a, N) is per_channel and ops._fused_gn(a, 32, N) is per_channel
    assert ops._fused_gn_channels(a, N + 1) is None
    assert ops.group_norm_pair_stats(a, b, 32, 1e-5) is None                      # one side only
    b._omgsr_gn = (per_group, 32, b.data_ptr(), b._version)
    assert ops._fused_gn(b, 32, N) is per_group and ops._fused_gn_channels(b, N) is None     # per-group partials cannot be regrouped
    assert ops.group_norm_pair_stats(a, b, 32, 1e-5) is None
    a.add_(1.0)                                                                   # written since: the handle is stale
    assert ops._fused_gn_channels(a, N) is None
    # a handle made for another group count still serves (per-channel entries), which _fused_gn itself keeps refusing
    c = torch.zeros(N, 4, 4, C1)
    c._omgsr_gn = (per_channel, 16, c.data_ptr(), c._version)
    assert ops._fused_gn_channels(c, N) is per_channel and ops._fused_gn(c, 32, N) is None
    h16 = torch.zeros(N, 4, 4, C1, dtype=torch.float16)
    h16._omgsr_gn = (per_channel, 32, h16.data_ptr(), h16._version)
    assert ops.group_norm_pair_stats(h16, h16, 32, 1e-5) is None                  # 16-bit tiers keep concat_channels
