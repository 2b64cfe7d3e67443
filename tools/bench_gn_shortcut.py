"""The fused GroupNorm-apply + 1x1 shortcut launch (csrc/norm_shortcut.hip) in isolation, against the path it replaces (the apply pass that
also writes an OMGSR_EL_MX twin of x, then the shortcut GEMM on the twin), for the four channel-changing ResnetBlocks of the tiled VAE at the
default benchmark's sizes (OMGSR-S 256 -> 1024, batch 4): HIP-event median of 10 launches after 3 warm-ups, and the achieved bytes per second
on the algorithmic bytes (x once + y + sc).
    python tools/bench_gn_shortcut.py            the four layers
    python tools/bench_gn_shortcut.py --scale 0.1    the same layers with a tenth of the pixels"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omgsr_amd import ops  # noqa: E402

# (name, pixels, Cin, Cout, split of conv1's operand: 1 plain fp16 | 4 MX6)
LAYERS = [("decoder.up_blocks.3.resnets.0", 5_760_000, 256, 128, 1), ("decoder.up_blocks.2.resnets.0", 1_440_000, 512, 256, 1),
          ("encoder.down_blocks.1.resnets.0", 1_480_000, 128, 256, 4), ("encoder.down_blocks.2.resnets.0", 370_000, 256, 512, 4)]


def median_ms(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    ops.set_compute_dtype(torch.float32)
    dev, G, rows = "cuda", 32, 16
    for name, pixels, C, Co, split in LAYERS:
        HW = max(int(pixels * args.scale) // rows, 1)
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(rows, HW, 1, C, device=dev, generator=g) * 1.5 + 0.2
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        w = torch.randn(Co, C, 1, 1, device=dev, generator=g) * C ** -0.5
        b = torch.zeros(Co, device=dev)
        mean, rstd, _ = ops.group_norm_stats(x, G, 1e-6)
        sw = ops.pack_gn_shortcut_weight(w, b)
        pw = ops.pack_conv_weight(w, b, device=dev, cout_multiple=8, split=3)

        def fused():
            return ops.group_norm_shortcut(x, sw, mean, rstd, gamma, beta, G, ops.ACT_SILU, split)

        def apply_twin():
            return ops.group_norm_apply(x, mean, rstd, gamma, beta, G, ops.ACT_SILU, split=split, also_cast=3)

        x3 = apply_twin()[1]

        def gemm():
            return ops.conv2d(x3, pw, pad=0)

        t_f, t_a, t_g = median_ms(fused), median_ms(apply_twin), median_ms(gemm)
        px = rows * HW
        algo = px * (4.0 * C + (4.0 if split == 4 else 2.0) * C + 4.0 * Co)
        print(json.dumps(dict(layer=name, pixels=px, cin=C, cout=Co, y="mx6" if split == 4 else "fp16", fused_ms=round(t_f, 4),
                              apply_twin_ms=round(t_a, 4), shortcut_gemm_ms=round(t_g, 4), old_ms=round(t_a + t_g, 4),
                              algorithmic_gb=round(algo / 1e9, 3), fused_tb_per_s=round(algo / t_f / 1e9, 3))), flush=True)
        del x, x3


if __name__ == "__main__":
    main()
