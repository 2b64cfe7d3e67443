"""The fp32 edge convolution (csrc/conv_edge.hip) in isolation, on one MI355X:
  * silu_f's largest relative error against fp64, measured THROUGH edge_conv_out_kernel (identity statistics and affine, a weight that is 1 at
    the centre tap of channel 0: the output is silu_f(x) in fp32) - the SILU_REL constant of tests/test_edge_conv_gpu.py;
  * the conv_norm_out + conv_out launch at the sizes of the default benchmark (OMGSR-S 256 -> 1024, batch 4, tiled VAE 256 / 64): one launch over
    the tile-shape groups, one launch per group, and the path it replaces (apply pass writing a two-term split operand + ops.conv2d_multi on the
    split weight), HIP-event times of 10 launches after 3 warm-ups, sorted.
    python tools/bench_edge_conv.py [out.json]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omgsr_amd import ops  # noqa: E402

DEV = "cuda"
N, G = 4, 32


def timed(fn, it=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(it):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(round(e0.elapsed_time(e1), 4))
    return sorted(ts)


def silu_error(R=12.0, H=1024, W=2048):
    x = torch.zeros((1, H, W, 32), dtype=torch.float32)
    x[0, :, :, 0] = torch.linspace(-R, R, H * W, dtype=torch.float64).float().view(H, W)
    w = torch.zeros((3, 32, 3, 3))
    w[0, 0, 1, 1] = 1.0
    y = ops.conv_out_gn(x.to(DEV), ops.pack_edge_out_weight(w.to(DEV), None), torch.zeros((1, 32), device=DEV), torch.ones((1, 32), device=DEV),
                        torch.ones(32, device=DEV), torch.zeros(32, device=DEV), 32)
    torch.cuda.synchronize()
    got, xv = y[0, :, :, 0].cpu().double().view(-1), x[0, :, :, 0].double().view(-1)
    ref = xv * torch.sigmoid(xv)
    rel = torch.where(ref != 0, (got - ref).abs() / ref.abs(), torch.zeros_like(ref))
    out = {"range": R, "points": H * W, "rel_max": float(rel.max()), "at_x": float(xv[rel.argmax()])}
    for lo, hi in ((-12, -6), (-6, -2), (-2, 0), (0, 2), (2, 6), (6, 12)):
        out[f"rel_max[{lo},{hi})"] = float(rel[(xv >= lo) & (xv < hi)].max())
    return out


def launch(name, Cin, Cout, shapes, out, gen, old=True):
    xs = [torch.randn(s + (Cin,), device=DEV, generator=gen) for s in shapes]
    mean, rstd = torch.randn((N, G), device=DEV, generator=gen) * 0.1, torch.rand((N, G), device=DEV, generator=gen) + 0.5
    gamma, beta = torch.randn(Cin, device=DEV, generator=gen) * 0.2 + 1.0, torch.randn(Cin, device=DEV, generator=gen) * 0.2
    w, b = torch.randn((Cout, Cin, 3, 3), device=DEV, generator=gen) * 0.03, torch.randn(Cout, device=DEV, generator=gen) * 0.1
    ew = ops.pack_edge_out_weight(w, b)
    px = sum(r * h * wd for r, h, wd in shapes)
    rec = {"pixels": px, "one_launch_ms": timed(lambda: ops.conv_out_gn_multi(xs, ew, mean, rstd, gamma, beta, G))}
    if len(xs) > 1:
        rec["per_group_ms"] = timed(lambda: ops.conv_out_gn_multi(xs, ew, mean, rstd, gamma, beta, G, one_launch=False))
        rec["one_launch_again_ms"] = timed(lambda: ops.conv_out_gn_multi(xs, ew, mean, rstd, gamma, beta, G))
        rec["per_group_again_ms"] = timed(lambda: ops.conv_out_gn_multi(xs, ew, mean, rstd, gamma, beta, G, one_launch=False))
    if old:
        pw = ops.pack_conv_weight(w, b, cout_multiple=8, split=2, w_split=2)
        rec["apply_plus_conv2d_ms"] = timed(lambda: ops.conv2d_multi(ops.group_norm_apply_multi(xs, mean, rstd, gamma, beta, G, ops.ACT_SILU, split=2),
                                                                     pw, stride=1, pad=1), it=5)
    med = sorted(rec.get("one_launch_again_ms", rec["one_launch_ms"]))[5]
    cp = 4 if Cout <= 4 else 8
    rec.update(median_ms=med, TBps=round(px * (4.0 * Cin + 32.0) / (med * 1e-3) / 1e12, 3),
               TFLOPs_useful=round(2.0 * px * Cin * 9 * Cout / (med * 1e-3) / 1e12, 2), TFLOPs_issued=round(2.0 * px * Cin * 9 * cp / (med * 1e-3) / 1e12, 2))
    out[name] = rec


def main():
    ops.set_compute_dtype(torch.float32)
    gen = torch.Generator(device=DEV).manual_seed(3)
    out = {"silu_f": silu_error()}
    print(json.dumps(out["silu_f"]), flush=True)
    # rows = tiles x images of each tile-shape group
    launch("decoder 128->3", 128, 3, [(N, 688, 688), (N, 688, 512), (N, 512, 688), (N, 512, 512)], out, gen)
    launch("encoder 512->8", 512, 8, [(9 * N, 40, 40), (3 * N, 40, 32), (3 * N, 32, 40), (N, 32, 32)], out, gen)
    launch("unet 320->4", 320, 4, [(9 * N, 64, 64)], out, gen)
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
