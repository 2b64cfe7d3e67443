"""The fp8 tier against the bf16 tier, in one process (bench.py has no fp8 choice and never runs the fp8 code):

  * the OMGSR-F 256 -> 1024 batch-8 step (BASELINE configs[3]'s shape, bench.py's f1024 workload: FLUX.1-dev-shaped DiT with seeded
    weights generated on the device, FLUX VAE), bf16 and fp8 in alternated rounds, each warmed after the switch, device-synchronised;
  * a per-shape GEMM table at the DiT's token-linear shapes: mxfp8_gemm_kernel (MXFP8 x MXFP8) against igemm_p8 (bf16), TFLOP/s and the
    fraction of the dense peaks (fp8 5 PF, bf16 2.5 PF), plus the quantiser's GB/s on the operand it would quantise.

    python tools/bench_fp8_tier.py [--rounds 3] [--steps 3] [--out profiles/fp8_tier.json]

--fused-quant measures the fp8 tier's fused MXFP8 producers instead (writes profiles/fp8_fused_quant.json):
  (a) the kernels alone - layer_norm_mxfp8 against layer_norm + quantize_mxfp8 at [36864, 3072]; the OUT8 GEMM against GEMM + quantise pass at
      36864 x 3072 -> 12288, dense and into the [attn | mlp] slice of a 15360-wide operand;
  (b) the F-1024 batch-8 step of the fp8 tier in four arms - the pass form (what OMGSR_FP8_FUSED_QUANT=0 runs), the LayerNorm kind alone, the
      GEMM kind alone, both - alternated rounds in one process, plus the per-kind launch table of one step per arm;
  (c) the same step on the parent commit's build: --parent-json takes the file this tool wrote when run WITHOUT --fused-quant (--no-gemm) from a
      checkout of that commit in the same visit to the machine; its fp8 arm is recorded as `parent_commit_step`.

--gemm-groups [--batch 1,2,8] measures the fp8 tier's paired launch groups (writes profiles/fp8_gemm_groups.json):
  (a) the four image / text pairs of a double block at batch 1 (4096 and 512 tokens), two launches against one ops.gemm_group;
  (b) the F-1024 full-depth step of the fp8 tier at each batch, groups off and on in alternated rounds in one process, HIP events;
  (c) the same step on the parent commit's build: --parent-json takes the file this tool wrote with --gemm-groups --parent-arm (the step as
      the checkout it runs from builds it, no switch touched) from a checkout of that commit in the same visit to the machine.
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


def fused_quant_kernels(dev) -> dict:
    """(a): each fused producer against the two launches it replaces, device events, same tensors."""
    import torch
    from omgsr_amd import ops
    M, D, H = 8 * 4608, 3072, 12288
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(M, D, generator=g, device=dev).to(torch.bfloat16)
    a, b = torch.randn(D, generator=g, device=dev) * 0.1 + 1.0, torch.randn(D, generator=g, device=dev) * 0.1
    out = {}
    ws = ops._mxfp8_like(x)
    t_ln = _events_ms(lambda: ops.layer_norm(x, a, b, 1e-6), 50)
    t_q = _events_ms(lambda: ops.quantize_mxfp8(x, out=ws), 50)
    t_pass = _events_ms(lambda: ops.quantize_mxfp8(ops.layer_norm(x, a, b, 1e-6), out=ws), 50)
    t_fused = _events_ms(lambda: ops.layer_norm_mxfp8(x, a, b, 1e-6, out=ws), 50)
    out["layer_norm_36864x3072"] = dict(layer_norm_ms=round(t_ln, 4), quantize_ms=round(t_q, 4), pass_form_ms=round(t_pass, 4), fused_ms=round(t_fused, 4),
                                        fused_gbps=round(M * D * (2 + 1 + 1 / 32) / t_fused / 1e6, 1), fused_faster=t_fused < t_pass)
    print(json.dumps(out["layer_norm_36864x3072"]), flush=True)
    w = (torch.randn(H, D, generator=g, device=dev) / D ** 0.5).to(torch.bfloat16)
    pw = ops.pack_linear_weight_mxfp8(w, torch.zeros(H, device=dev))
    xq = ops.quantize_mxfp8(x)
    h16 = torch.empty(M, H, device=dev, dtype=torch.bfloat16)
    h8 = ops._mxfp8_like(h16)
    t_g = _events_ms(lambda: ops.linear(xq, pw, act=ops.ACT_GELU_TANH, out_dtype=ops.OUT_BF16), 20)
    t_hq = _events_ms(lambda: ops.quantize_mxfp8(h16, out=h8), 20)
    t_pass = _events_ms(lambda: ops.quantize_mxfp8(ops.linear(xq, pw, act=ops.ACT_GELU_TANH, out_dtype=ops.OUT_BF16), out=h8), 20)
    t_fused = _events_ms(lambda: ops.linear(xq, pw, act=ops.ACT_GELU_TANH, out_mxfp8=h8), 20)
    fl = 2.0 * M * D * H
    out["gemm_36864x3072_to_12288"] = dict(gemm_bf16_out_ms=round(t_g, 4), quantize_ms=round(t_hq, 4), pass_form_ms=round(t_pass, 4), fused_ms=round(t_fused, 4),
                                           fused_tflops=round(fl / t_fused / 1e9, 1), fused_faster=t_fused < t_pass)
    print(json.dumps(out["gemm_36864x3072_to_12288"]), flush=True)
    del h16, h8
    torch.cuda.empty_cache()
    Kc = D + H                                  # the single block: proj_mlp into columns [D, Kc) of proj_out's operand
    cat = torch.empty(M, Kc, device=dev, dtype=torch.bfloat16)
    cat8 = ops._mxfp8_like(cat)
    t_pass = _events_ms(lambda: (ops.linear_into(xq, pw, cat, 0, D, act=ops.ACT_GELU_TANH), ops.quantize_mxfp8(cat, out=cat8)), 20)
    t_fused = _events_ms(lambda: (ops.linear_into(xq, pw, None, 0, D, act=ops.ACT_GELU_TANH, out_mxfp8=cat8),
                                  ops.quantize_mxfp8(cat[:, :D], out=cat8, out_col=0)), 20)
    out["gemm_into_cat8_slice_Kc15360"] = dict(pass_form_ms=round(t_pass, 4), fused_ms=round(t_fused, 4), fused_faster=t_fused < t_pass,
                                               note="pass form: GEMM into the bf16 concat + one quantise pass over all 15360 columns; fused: OUT8 GEMM into "
                                                    "columns [3072, 15360) + the strided quantiser over the 3072 attention columns")
    print(json.dumps(out["gemm_into_cat8_slice_Kc15360"]), flush=True)
    return out


def _kind_table(step) -> dict:
    """Per-kind launch table of ONE step from the library's timing trace: launches and summed device ms of the elementwise and LayerNorm
    kinds and of the MXFP8 GEMM (igemm, variant 18)."""
    import torch
    from omgsr_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.omgsr_timing_enable(1); lib.omgsr_timing_reset()
    try:
        step()
        torch.cuda.synchronize()
        buf = (_lib.TimingEntry * 65536)()
        n = lib.omgsr_timing_collect(buf, 65536)
    finally:
        lib.omgsr_timing_enable(0)
    kinds = {1: "igemm", 2: "attention", 3: "groupnorm", 4: "layernorm", 5: "elementwise", 6: "softmax"}       # OMGSR_TK_*, as bench.py names them
    table = {}
    for e in buf[:n]:
        name = kinds.get(e.kind, str(e.kind))
        if name == "igemm":
            name = f"igemm/{e.variant}"
        row = table.setdefault(name, dict(launches=0, ms=0.0))
        row["launches"] += 1
        row["ms"] += e.ms
    return {k: dict(launches=v["launches"], ms=round(v["ms"], 3)) for k, v in sorted(table.items())}


def fused_quant_step(dev, rounds: int, steps: int) -> dict:
    """(b): the fp8 tier's F-1024 batch-8 step, fused producers against the pass form, alternated rounds in one process."""
    import torch
    import bench
    from omgsr_amd import ops
    from omgsr_amd.precision import FLUX_FP8, set_fp8_linear
    family, side, B, tile, overlap, _ = bench.WORKLOADS["f1024"]
    pipe, _ = bench.build_f(dev, 0, 1, torch.bfloat16)
    inp = bench.make_inputs(family, side, B, tile, 0, dev, torch.bfloat16)
    pipe.vae.posterior_noise = inp["eps"].to(dev)
    step = bench.make_step(pipe, family, inp, tile, overlap)
    set_fp8_linear(pipe.flux_transformer, FLUX_FP8)
    arms = {"pass": (False, False), "layernorm": (True, False), "gemm": (False, True), "fused": (True, True)}
    times = {name: [] for name in arms}
    kinds = {}
    saved = dict(ops.FP8_FUSED_QUANT)

    def arm(name):
        ops.FP8_FUSED_QUANT.update(layernorm=arms[name][0], gemm=arms[name][1])
    try:
        with torch.no_grad():
            for r in range(rounds):
                for name in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
                    arm(name)
                    step(); step()
                    torch.cuda.synchronize()
                    for _ in range(steps):
                        t0 = time.perf_counter()
                        step()
                        torch.cuda.synchronize()
                        times[name].append(time.perf_counter() - t0)
                    print(f"round {r} {name}: {[round(t * 1e3, 1) for t in times[name][-steps:]]} ms", flush=True)
            for name in arms:
                arm(name)
                step()
                kinds[name] = _kind_table(step)
    finally:
        ops.FP8_FUSED_QUANT.clear(); ops.FP8_FUSED_QUANT.update(saved)
    out = {}
    for name, ts in times.items():
        out[name] = dict(median_ms=round(statistics.median(ts) * 1e3, 2), min_ms=round(min(ts) * 1e3, 2), max_ms=round(max(ts) * 1e3, 2),
                         samples_ms=[round(t * 1e3, 2) for t in ts])
    # the acceptance of DESIGN 3.1, per producer kind alone and for both: every step of the arm faster than every pass-form step
    out["saved_ms_median"] = {name: round(out["pass"]["median_ms"] - out[name]["median_ms"], 2) for name in arms if name != "pass"}
    out["every_step_faster_than_every_pass_step"] = {name: out[name]["max_ms"] < out["pass"]["min_ms"] for name in arms if name != "pass"}
    out["per_kind_one_step"] = {name: {k: v for k, v in kinds[name].items() if k in ("elementwise", "layernorm", "igemm/18")} for name in kinds}
    out["per_kind_one_step_all"] = kinds
    out["shape"] = dict(workload="f1024", side=side, batch=B, tile=tile, overlap=overlap)
    return out


GROUP_PAIRS = {"to_q|k": (3072, 6144), "to_v": (3072, 3072), "to_out/to_add_out": (3072, 3072), "ff.net.2": (12288, 3072)}      # (K, N)


def gemm_group_pairs(dev) -> dict:
    """(a): per pair at batch 1, the image launch (4096 rows) + the text launch (512 rows) against the two as one launch group."""
    import torch
    from omgsr_amd import ops
    out = {}
    for name, (K, N) in GROUP_PAIRS.items():
        g = torch.Generator(device=dev).manual_seed(K + N)
        mk = lambda rows: ops.quantize_mxfp8(torch.randn(rows, K, generator=g, device=dev).to(torch.bfloat16))      # noqa: E731
        pk = lambda: ops.pack_linear_weight_mxfp8((torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16), torch.zeros(N, device=dev))      # noqa: E731
        xi, xt, wi, wt = mk(4096), mk(512), pk(), pk()

        def pair(grouped):
            if grouped:
                with ops.gemm_group():
                    ops.linear(xi, wi); ops.linear(xt, wt)
            else:
                ops.linear(xi, wi); ops.linear(xt, wt)
        off = [_events_ms(lambda: pair(False), 50) for _ in range(3)]
        on = [_events_ms(lambda: pair(True), 50) for _ in range(3)]
        t_img, t_txt = _events_ms(lambda: ops.linear(xi, wi), 50), _events_ms(lambda: ops.linear(xt, wt), 50)
        out[name] = dict(K=K, N=N, image_alone_ms=round(t_img, 4), text_alone_ms=round(t_txt, 4), two_launches_ms=[round(t, 4) for t in off],
                         one_group_ms=[round(t, 4) for t in on], saved_ms_median=round(statistics.median(off) - statistics.median(on), 4))
        print(name, json.dumps(out[name]), flush=True)
        del xi, xt, wi, wt
        torch.cuda.empty_cache()
    return out


def gemm_groups_step(dev, rounds: int, steps: int, batches, parent_arm: bool) -> dict:
    """(b) / (c): the fp8 tier's F-1024 step per batch size. The blocks' `gemm_groups` attribute is what OMGSR_F_Infer.enable_gemm_groups sets;
    parent_arm: one arm, nothing set (a checkout without the feature)."""
    import torch
    import bench
    from omgsr_amd.precision import FLUX_FP8, set_fp8_linear
    family, side, _, tile, overlap, _ = bench.WORKLOADS["f1024"]
    pipe, _ = bench.build_f(dev, 0, 1, torch.bfloat16)
    set_fp8_linear(pipe.flux_transformer, FLUX_FP8)
    arms = ["parent"] if parent_arm else ["off", "on"]
    out = {}
    for B in batches:
        inp = bench.make_inputs(family, side, B, tile, 0, dev, torch.bfloat16)
        pipe.vae.posterior_noise = inp["eps"].to(dev)
        step = bench.make_step(pipe, family, inp, tile, overlap)
        times = {a: [] for a in arms}
        with torch.no_grad():
            for r in range(rounds):
                for a in (arms if r % 2 == 0 else arms[::-1]):
                    if not parent_arm:
                        for blk in pipe.flux_transformer.transformer_blocks:
                            blk.gemm_groups = a == "on"
                    step(); step()
                    torch.cuda.synchronize()
                    for _ in range(steps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        step()
                        e1.record()
                        torch.cuda.synchronize()
                        times[a].append(e0.elapsed_time(e1))
                    print(f"batch {B} round {r} {a}: {[round(t, 2) for t in times[a][-steps:]]} ms", flush=True)
            rec = {a: dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3),
                           samples_ms=[round(t, 3) for t in ts]) for a, ts in times.items()}
            if not parent_arm:
                for blk in pipe.flux_transformer.transformer_blocks:
                    blk.gemm_groups = True
                step()
                kinds = _kind_table(step)
                rec["on_igemm_launches_one_step"] = {k: v for k, v in kinds.items() if k in ("igemm/18", "igemm/24")}
                rec["saved_ms_median"] = round(rec["off"]["median_ms"] - rec["on"]["median_ms"], 3)
                for blk in pipe.flux_transformer.transformer_blocks:
                    blk.gemm_groups = False
        out[f"batch_{B}"] = rec
        print(f"batch {B}", json.dumps({a: {k: v for k, v in rec[a].items() if k != "samples_ms"} for a in arms}), flush=True)
        del inp, step
        torch.cuda.empty_cache()
    out["shape"] = dict(workload="f1024", side=side, tile=tile, overlap=overlap, timer="HIP events around one step", rounds=rounds, steps=steps)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per tier per round")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-gemm", action="store_true")
    ap.add_argument("--fused-quant", action="store_true", help="measure the fused MXFP8 producers (see the module docstring)")
    ap.add_argument("--parent-json", default=None, help="--fused-quant: the parent commit's run of this tool (its fp8 step) to record as (c)")
    ap.add_argument("--gemm-groups", action="store_true", help="measure the paired launch groups (see the module docstring)")
    ap.add_argument("--batch", default="1,2,8", help="--gemm-groups: batch sizes of the step, comma-separated")
    ap.add_argument("--parent-arm", action="store_true", help="--gemm-groups: the step as this checkout builds it, one arm (the parent commit's run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "fp8_gemm_groups.json" if args.gemm_groups else
                                        "fp8_fused_quant.json" if args.fused_quant else "fp8_tier.json")
    import torch
    from omgsr_amd import _lib, ops
    dev = torch.device("cuda", 0)
    _lib.check(_lib.load().omgsr_check_device(), "omgsr_check_device")
    ops.set_compute_dtype(torch.bfloat16)
    rec = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)
    if args.gemm_groups:
        batches = [int(b) for b in args.batch.split(",")]
        if not args.no_gemm and not args.parent_arm:
            rec["pairs_batch_1"] = gemm_group_pairs(dev)
        if not args.no_step:
            rec["f1024_step"] = gemm_groups_step(dev, args.rounds, args.steps, batches, args.parent_arm)
        if args.parent_json:
            with open(args.parent_json) as f:
                parent = json.load(f)["f1024_step"]
            rec["parent_commit_step"] = dict({k: v["parent"] for k, v in parent.items() if k.startswith("batch_")},
                                             note="the parent commit's own build and Python, run on the same machine in the same visit just before this process")
            if "f1024_step" in rec:
                cmp_ = {}
                for k, v in rec["f1024_step"].items():
                    if k.startswith("batch_") and k in parent:
                        p = parent[k]["parent"]
                        cmp_[k] = dict(off_median_minus_parent_ms=round(v["off"]["median_ms"] - p["median_ms"], 3),
                                       on_median_minus_parent_ms=round(v["on"]["median_ms"] - p["median_ms"], 3),
                                       every_grouped_step_faster_than_every_parent_step=v["on"]["max_ms"] < p["min_ms"],
                                       parent_spread_ms=round(p["max_ms"] - p["min_ms"], 3))
                rec["parent_commit_step"]["comparison"] = cmp_
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(f"wrote {args.out}")
        return
    if args.fused_quant:
        if not args.no_gemm:
            rec["kernels_alone"] = fused_quant_kernels(dev)
        if not args.no_step:
            rec["f1024_b8_step"] = fused_quant_step(dev, args.rounds, args.steps)
            print(json.dumps({k: v for k, v in rec["f1024_b8_step"].items() if k != "per_kind_one_step_all"}), flush=True)
        if args.parent_json:
            with open(args.parent_json) as f:
                parent = json.load(f)["f1024_b8_step"]
            rec["parent_commit_step"] = dict(fp8=parent["fp8"], shape=parent["shape"], note="the parent commit's own build and Python, its fp8 tier "
                                             "(every MXFP8 operand from a quantise pass), run on the same machine in the same visit just before this process")
            if "f1024_b8_step" in rec:
                ours = rec["f1024_b8_step"]
                rec["parent_commit_step"]["median_ms_vs_parent"] = {n: round(ours[n]["median_ms"] - parent["fp8"]["median_ms"], 2)
                                                                    for n in ("pass", "layernorm", "gemm", "fused")}
    elif not args.no_gemm:
        rec["gemm"] = gemm_table(dev)
    if not args.no_step and not args.fused_quant:
        rec["f1024_b8_step"] = step_rounds(dev, args.rounds, args.steps)
        print(json.dumps({k: v for k, v in rec["f1024_b8_step"].items() if k != "samples_ms"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
