"""The fp8 tier against the bf16 tier, in one process (bench.py has no fp8 choice and never runs the fp8 code):

  * the OMGSR-F 256 -> 1024 batch-8 step (BASELINE configs[3]'s shape, bench.py's f1024 workload: FLUX.1-dev-shaped DiT with seeded
    weights generated on the device, FLUX VAE), bf16 and fp8 in alternated rounds, each warmed after the switch, device-synchronised;
  * a per-shape GEMM table at the DiT's token-linear shapes: mxfp8_gemm_kernel (MXFP8 x MXFP8) against igemm_p8 (bf16), TFLOP/s and the
    fraction of the dense peaks (fp8 5 PF, bf16 2.5 PF), plus the quantiser's GB/s on the operand it would quantise.

    python tools/bench_fp8_tier.py [--rounds 3] [--steps 3] [--out profiles/fp8_tier.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP8_PEAK_TF, BF16_PEAK_TF = 5000.0, 2500.0
SHAPES = [(3072, 3072), (3072, 6144), (3072, 12288), (12288, 3072), (15360, 3072)]


def _events_ms(fn, iters: int, warm: int = 3) -> float:
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def gemm_table(dev) -> list:
    import torch
    from omgsr_amd import ops
    rows = []
    for M in (8 * 4608, 8 * 512):
        for K, N in SHAPES:
            g = torch.Generator(device=dev).manual_seed(K + N)
            x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
            w = (torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16)
            b = torch.zeros(N, device=dev)
            p16 = ops.pack_linear_weight(w, b)
            p8 = ops.pack_linear_weight_mxfp8(w, b)
            xq = ops.quantize_mxfp8(x)
            iters = 20 if M * K * N > 1e11 else 50
            t16 = _events_ms(lambda: ops.linear(x, p16), iters)
            t8 = _events_ms(lambda: ops.linear(xq, p8), iters)
            tq = _events_ms(lambda: ops.quantize_mxfp8(x), iters)
            fl = 2.0 * M * K * N
            rows.append(dict(M=M, K=K, N=N, bf16_ms=round(t16, 4), fp8_ms=round(t8, 4), speedup=round(t16 / t8, 3),
                             bf16_tflops=round(fl / t16 / 1e9, 1), fp8_tflops=round(fl / t8 / 1e9, 1),
                             bf16_peak_frac=round(fl / t16 / 1e9 / BF16_PEAK_TF, 3), fp8_peak_frac=round(fl / t8 / 1e9 / FP8_PEAK_TF, 3),
                             quant_ms=round(tq, 4), quant_gbps=round(M * K * (2 + 1 + 1 / 32) / tq / 1e6, 1),
                             fp8_plus_quant_speedup=round(t16 / (t8 + tq), 3)))
            print(json.dumps(rows[-1]), flush=True)
            del x, w, p16, p8, xq
            torch.cuda.empty_cache()
    return rows


def step_rounds(dev, rounds: int, steps: int) -> dict:
    import torch
    import bench
    from omgsr_amd.precision import FLUX_FP8, set_fp8_linear
    family, side, B, tile, overlap, _ = bench.WORKLOADS["f1024"]
    pipe, _ = bench.build_f(dev, 0, 1, torch.bfloat16)
    inp = bench.make_inputs(family, side, B, tile, 0, dev, torch.bfloat16)
    pipe.vae.posterior_noise = inp["eps"].to(dev)
    step = bench.make_step(pipe, family, inp, tile, overlap)
    times = {"bf16": [], "fp8": []}
    with torch.no_grad():
        for r in range(rounds):
            for tier in (("bf16", "fp8") if r % 2 == 0 else ("fp8", "bf16")):
                set_fp8_linear(pipe.flux_transformer, FLUX_FP8 if tier == "fp8" else [])
                step()                          # warm: (re-)packs the weights of the tier
                step()
                torch.cuda.synchronize()
                for _ in range(steps):
                    t0 = time.perf_counter()
                    step()
                    torch.cuda.synchronize()
                    times[tier].append(time.perf_counter() - t0)
                print(f"round {r} {tier}: {[round(t * 1e3, 1) for t in times[tier][-steps:]]} ms", flush=True)
    out = {}
    for tier, ts in times.items():
        out[tier] = dict(median_ms=round(statistics.median(ts) * 1e3, 2), min_ms=round(min(ts) * 1e3, 2), max_ms=round(max(ts) * 1e3, 2),
                         samples_ms=[round(t * 1e3, 2) for t in ts])
    out["speedup_median"] = round(out["bf16"]["median_ms"] / out["fp8"]["median_ms"], 3)
    out["spread_ms"] = dict(bf16=round(out["bf16"]["max_ms"] - out["bf16"]["min_ms"], 2), fp8=round(out["fp8"]["max_ms"] - out["fp8"]["min_ms"], 2))
    out["fp8_faster_than_spread"] = out["bf16"]["min_ms"] > out["fp8"]["max_ms"]
    out["shape"] = dict(workload="f1024", side=side, batch=B, tile=tile, overlap=overlap)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per tier per round")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-gemm", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_tier.json"))
    args = ap.parse_args()
    import torch
    from omgsr_amd import _lib, ops
    dev = torch.device("cuda", 0)
    _lib.check(_lib.load().omgsr_check_device(), "omgsr_check_device")
    ops.set_compute_dtype(torch.bfloat16)
    rec = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)
    if not args.no_gemm:
        rec["gemm"] = gemm_table(dev)
    if not args.no_step:
        rec["f1024_b8_step"] = step_rounds(dev, args.rounds, args.steps)
        print(json.dumps({k: v for k, v in rec["f1024_b8_step"].items() if k != "samples_ms"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
