"""The fp8 tier's MXFP8 attention (precision_policy={"flux": {"fp8_attention": True}}) against its bf16 attention, in one process (bench.py
never runs it):

  * per launch at B = 8, H = 24, L = 4608, D = 128 (FLUX's joint attention at F-1024 batch 8): attn_kernel (bf16), mxfp8_attn_kernel alone,
    and mxfp8_attn_kernel plus the V^T quantise pass (q | k come out of RMSNorm + RoPE already quantised), TFLOP/s (4 Lq Lk D per head)
    and the fraction of the 5 PF fp8 peak (an A/B build with OMGSR_EXTRA_DEFS=-DOMGSR_ATTN_FP8_DEFER=8 times the deferred maximum);
  * the OMGSR-F 256 -> 1024 batch-8 step, fp8 tier against fp8 tier + fp8_attention, in alternated rounds, each warmed after the switch,
    device-synchronised.

    python tools/bench_fp8_attention.py [--rounds 3] [--steps 3] [--no-step] [--kernel-only] [--out profiles/fp8_attention.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

FP8_PEAK_TF, BF16_PEAK_TF = 5000.0, 2500.0
B, H, L, D = 8, 24, 4608, 128


def kernel_table(dev, iters: int = 20) -> dict:
    import torch
    from bench_fp8_tier import _events_ms
    from omgsr_amd import ops
    g = torch.Generator(device=dev).manual_seed(7)
    inner = H * D
    qk = (torch.randn(B, L, 2 * inner, generator=g, device=dev) * 1.5).to(torch.bfloat16)
    vt = torch.zeros(B, inner, ops._round_up(L, 128), device=dev, dtype=torch.bfloat16)
    vt[..., :L] = torch.randn(B, inner, L, generator=g, device=dev).to(torch.bfloat16)
    qk8, vt8 = ops.quantize_mxfp8(qk), ops.quantize_mxfp8(vt)
    o = torch.empty(B, L, inner, device=dev, dtype=torch.bfloat16)
    sc = D ** -0.5
    t16 = _events_ms(lambda: ops.attention(qk, qk, vt, H, D, sc, q_col=0, k_col=inner, out=o), iters)
    t8 = _events_ms(lambda: ops.attention(qk8, qk8, vt8, H, D, sc, q_col=0, k_col=inner, out=o), iters)
    tq = _events_ms(lambda: ops.quantize_mxfp8(vt, out=vt8), iters)
    fl = 4.0 * B * H * L * L * D
    rec = dict(shape=dict(B=B, H=H, L=L, D=D), build_defs=os.environ.get("OMGSR_EXTRA_DEFS", ""),
               bf16_ms=round(t16, 4), mxfp8_ms=round(t8, 4), vt_quant_ms=round(tq, 4), mxfp8_plus_vt_quant_ms=round(t8 + tq, 4),
               bf16_tflops=round(fl / t16 / 1e9, 1), mxfp8_tflops=round(fl / t8 / 1e9, 1),
               bf16_frac_of_bf16_peak=round(fl / t16 / 1e9 / BF16_PEAK_TF, 3), mxfp8_frac_of_fp8_peak=round(fl / t8 / 1e9 / FP8_PEAK_TF, 3),
               speedup_kernel=round(t16 / t8, 3), speedup_with_vt_quant=round(t16 / (t8 + tq), 3))
    print(json.dumps(rec), flush=True)
    return rec


def step_rounds(dev, rounds: int, steps: int) -> dict:
    import torch
    import bench
    from omgsr_amd.precision import FLUX_FP8, clear_fp8_attention, set_fp8_attention, set_fp8_linear
    family, side, Bs, tile, overlap, _ = bench.WORKLOADS["f1024"]
    pipe, _ = bench.build_f(dev, 0, 1, torch.bfloat16)
    inp = bench.make_inputs(family, side, Bs, tile, 0, dev, torch.bfloat16)
    pipe.vae.posterior_noise = inp["eps"].to(dev)
    step = bench.make_step(pipe, family, inp, tile, overlap)
    set_fp8_linear(pipe.flux_transformer, FLUX_FP8)
    times = {"fp8": [], "fp8_attention": []}
    with torch.no_grad():
        for r in range(rounds):
            for arm in (("fp8", "fp8_attention") if r % 2 == 0 else ("fp8_attention", "fp8")):
                if arm == "fp8_attention":
                    set_fp8_attention(pipe.flux_transformer, True)
                else:
                    clear_fp8_attention(pipe.flux_transformer)
                step()                          # warm after the switch
                step()
                torch.cuda.synchronize()
                for _ in range(steps):
                    t0 = time.perf_counter()
                    step()
                    torch.cuda.synchronize()
                    times[arm].append(time.perf_counter() - t0)
                print(f"round {r} {arm}: {[round(t * 1e3, 1) for t in times[arm][-steps:]]} ms", flush=True)
        # where the time goes: one step per arm with the library's per-launch timing, summed by (kind, variant)
        from omgsr_amd import _lib
        lib = _lib.load()
        kinds = {1: "igemm", 2: "attention", 3: "groupnorm", 4: "layernorm", 5: "elementwise", 6: "softmax"}
        per_kind = {}
        for arm in ("fp8", "fp8_attention"):
            if arm == "fp8_attention":
                set_fp8_attention(pipe.flux_transformer, True)
            else:
                clear_fp8_attention(pipe.flux_transformer)
            step()
            torch.cuda.synchronize()
            lib.omgsr_timing_enable(1); lib.omgsr_timing_reset()
            step()
            buf = (_lib.TimingEntry * 65536)()
            n = lib.omgsr_timing_collect(buf, 65536)
            lib.omgsr_timing_enable(0)
            agg = {}
            for e in buf[:n]:
                key = f"{kinds.get(e.kind, e.kind)}/{e.variant}"
                a = agg.setdefault(key, [0, 0.0])
                a[0] += 1
                a[1] += e.ms
            per_kind[arm] = {k: dict(launches=c, ms=round(t, 3)) for k, (c, t) in sorted(agg.items())}
            print(f"{arm}: {json.dumps(per_kind[arm])}", flush=True)
    out = {"kernel_ms_by_kind_variant_one_step": per_kind}
    for arm, ts in times.items():
        out[arm] = dict(median_ms=round(statistics.median(ts) * 1e3, 2), min_ms=round(min(ts) * 1e3, 2), max_ms=round(max(ts) * 1e3, 2),
                        samples_ms=[round(t * 1e3, 2) for t in ts])
    out["speedup_median"] = round(out["fp8"]["median_ms"] / out["fp8_attention"]["median_ms"], 3)
    out["every_fp8_attention_step_faster"] = out["fp8"]["min_ms"] > out["fp8_attention"]["max_ms"]
    out["shape"] = dict(workload="f1024", side=side, batch=Bs, tile=tile, overlap=overlap)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per arm per round")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="print the kernel line and exit (no file written)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_attention.json"))
    args = ap.parse_args()
    import torch
    from omgsr_amd import _lib, ops
    dev = torch.device("cuda", 0)
    _lib.check(_lib.load().omgsr_check_device(), "omgsr_check_device")
    ops.set_compute_dtype(torch.bfloat16)
    rec = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)
    rec["kernel"] = kernel_table(dev)
    if args.kernel_only:
        return
    if not args.no_step:
        rec["f1024_b8_step"] = step_rounds(dev, args.rounds, args.steps)
        print(json.dumps({k: v for k, v in rec["f1024_b8_step"].items() if not isinstance(v, dict) or "samples_ms" not in v}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
