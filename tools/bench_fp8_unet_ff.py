"""OMGSR-S's opt-in MXFP8 UNet feed-forwards (precision_policy {"unet": {"fp8_ff": ...}} on the bf16 tier) against the bf16 tier, every timed step
kept (the acceptance rule of DESIGN 3.1: every step of the MXFP8 arm faster than every step of the bf16 arm); bench.py never runs them.
Writes profiles/fp8_unet_ff.json. HIP events, 3 alternated rounds x 3 steps. Every leg is a fresh child process with its own time limit; a leg
that fails or runs out of time ends the run.

  * layers: the feed-forward as the pipeline runs it - norm3 + GEGLU projection + net.2 with the bf16 residual - at every (rows, C) of the SD 2.1
    UNet in three workloads: bf16 = LayerNorm -> bf16 GEGLU GEMM -> bf16 net.2; mxfp8 = LayerNorm -> MXFP8 (K padded to 128) ->
    mxfp8_gemm_geglu_kernel -> MXFP8 hidden -> mxfp8_gemm_kernel. A shape class belongs in precision.fp8_unet_ff_routed only if every MXFP8
    step of it is faster than every bf16 step of it;
  * step: OMGSR-S 256 -> 1024, tiled VAE, batch 4 (bench.py's s1024 workload) on the bf16 tier: the key off, fp8_ff on, fp8 + fp8_ff on, in one
    process; --baseline-repo PATH: a checkout of the PARENT commit with its library built, timed first by a child started there, in the same visit;
  * quality: OMGSR-S 256 -> 1024, batch 2, seeded weights, three draws, PSNR and rel-L2 against the accurate tier: the key off, fp8_ff alone,
    fp8 + fp8_ff.

    python tools/bench_fp8_unet_ff.py [--baseline-repo PATH] [--legs layers,step,quality] [--out profiles/fp8_unet_ff.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (workload, rows, C): one transformer block's token matrix per UNet call
SHAPES = ([("s1024 batch 4", r, c) for r, c in ((147456, 320), (36864, 640), (9216, 1280), (2304, 1280))] +
          [("s1024 batch 1", r, c) for r, c in ((36864, 320), (9216, 640), (2304, 1280), (576, 1280))] +
          [("s512 batch 1", r, c) for r, c in ((4096, 320), (1024, 640), (256, 1280), (64, 1280))])
QUALITY_BATCH = 2
ALL_FF = [r"transformer_blocks"]
ALL_CONV = True                                 # precision.UNET_FP8: what {"fp8": True} marks
# the quality leg's rows: the key off, fp8_ff alone, fp8_ff beside {"fp8": True}, and beside the two narrower conv lists of DESIGN 3.5's table
# that lose least (the 32-wide level, the up path) - what to fall back to where the full combination misses the 30 dB target
ROWS = {"bf16_tier": None, "fp8_ff": {"fp8_ff": ALL_FF}, "fp8_and_fp8_ff": {"fp8": ALL_CONV, "fp8_ff": ALL_FF},
        "fp8_level_32_and_fp8_ff": {"fp8": [r"^(down_blocks\.1|up_blocks\.2)\.resnets\."], "fp8_ff": ALL_FF},
        "fp8_up_path_and_fp8_ff": {"fp8": [r"^up_blocks\.[23]\.resnets\."], "fp8_ff": ALL_FF}}
LIMITS = {"layers": 300, "step": 540, "baseline": 420, "quality": 900}      # seconds per leg


def _ms(fn) -> float:
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b), 4)


def _alternate(arms: dict, rounds: int, steps: int, before=None) -> dict:
    """{arm: [ms of every timed step]}: alternated rounds of `steps` single timed calls per arm (before(arm) switches, then two untimed calls)."""
    t = {k: [] for k in arms}
    for r in range(rounds):
        for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            if before is not None:
                before(k)
            arms[k]()
            arms[k]()
            for _ in range(steps):
                t[k].append(_ms(arms[k]))
    return t


def _stats(ms) -> dict:
    return dict(min=min(ms), max=max(ms), median=round(statistics.median(ms), 4))


def _verdict(off, on) -> dict:
    return dict(speedup_median=round(statistics.median(off) / statistics.median(on), 3), every_mxfp8_step_faster_than_every_bf16_step=max(on) < min(off))


def _variants(fn) -> list:
    import torch
    from omgsr_amd import _lib
    lib = _lib.load()
    fn()
    torch.cuda.synchronize()
    lib.omgsr_timing_enable(1)
    lib.omgsr_timing_reset()
    fn()
    buf = (_lib.TimingEntry * 16384)()
    n = lib.omgsr_timing_collect(buf, 16384)
    lib.omgsr_timing_enable(0)
    return sorted(e.variant for e in buf[:n] if e.kind == 1)


def leg_layers(dev, rounds: int, steps: int):
    import torch
    from omgsr_amd import ops
    rows = []
    for workload, M, Cc in SHAPES:
        g = torch.Generator(device=dev).manual_seed(M + Cc)
        y = torch.randn(1, M, Cc, generator=g, device=dev).to(torch.bfloat16)
        w0 = (torch.randn(8 * Cc, Cc, generator=g, device=dev) / Cc ** 0.5).to(torch.bfloat16)
        b0 = torch.randn(8 * Cc, generator=g, device=dev) * 0.1
        w2 = (torch.randn(Cc, 4 * Cc, generator=g, device=dev) / (4 * Cc) ** 0.5).to(torch.bfloat16)
        b2 = torch.randn(Cc, generator=g, device=dev) * 0.1
        gamma, beta = torch.rand(Cc, generator=g, device=dev) + 0.5, torch.randn(Cc, generator=g, device=dev) * 0.1
        p0, p2 = ops.pack_geglu_weight(w0, b0), ops.pack_linear_weight(w2, b2)
        q0, q2 = ops.pack_geglu_weight_mxfp8(w0, b0), ops.pack_linear_weight_mxfp8(w2, b2)

        def bf16():
            h = ops.linear(ops.layer_norm(y, gamma, beta, 1e-5), p0, out_dtype=ops.OUT_BF16)
            return ops.linear(h, p2, residual=y)

        def mxfp8():
            h = ops.linear(ops.layer_norm_mxfp8(y, gamma, beta, 1e-5, pad128=True), q0, out_mxfp8=True)
            return ops.linear(h, q2, residual=y)

        arms = {"bf16": bf16, "mxfp8": mxfp8}
        ran = {k: _variants(fn) for k, fn in arms.items()}
        t = _alternate(arms, rounds, steps)
        fl = 2.0 * M * Cc * 8 * Cc + 2.0 * M * 4 * Cc * Cc
        row = dict(workload=workload, rows=M, C=Cc, variants=ran, bf16_ms=t["bf16"], mxfp8_ms=t["mxfp8"], bf16=_stats(t["bf16"]), mxfp8=_stats(t["mxfp8"]),
                   bf16_tflops=round(fl / statistics.median(t["bf16"]) / 1e9, 1), mxfp8_tflops=round(fl / statistics.median(t["mxfp8"]) / 1e9, 1),
                   **_verdict(t["bf16"], t["mxfp8"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del y, w0, w2, p0, p2, q0, q2
        torch.cuda.empty_cache()
    return rows


def _s1024(dev):
    import torch
    import bench
    family, side, B, tile, overlap, _ = bench.WORKLOADS["s1024"]
    pipe, _ = bench.build_s(dev, 0, 1, torch.bfloat16)
    pipe._init_tiled_vae(encoder_tile_size=256, decoder_tile_size=64)
    inp = bench.make_inputs(family, side, B, tile, 0, dev, torch.bfloat16)
    pipe.vae.posterior_noise = inp["eps"].to(dev)
    return pipe, bench.make_step(pipe, family, inp, tile, overlap), dict(workload="s1024", side=side, batch=B, tile=tile, overlap=overlap, tiled_vae=True)


def leg_step(dev, rounds: int, steps: int):
    import torch
    from omgsr_amd.precision import clear_fp8_unet_conv, clear_fp8_unet_ff, fp8_unet_conv_layers, fp8_unet_ff_layers, set_fp8_unet_conv, set_fp8_unet_ff
    pipe, step, shape = _s1024(dev)

    def switch(arm):
        clear_fp8_unet_conv(pipe.unet)
        clear_fp8_unet_ff(pipe.unet)
        if arm in ("fp8_ff", "fp8_and_fp8_ff"):
            set_fp8_unet_ff(pipe.unet, ALL_FF)
        if arm == "fp8_and_fp8_ff":
            set_fp8_unet_conv(pipe.unet, ALL_CONV)
    with torch.no_grad():
        t = _alternate({"key_off": step, "fp8_ff": step, "fp8_and_fp8_ff": step}, rounds, steps, before=switch)
        switch("fp8_and_fp8_ff")
        marked = dict(ff_blocks=len(fp8_unet_ff_layers(pipe.unet)), convs=len(fp8_unet_conv_layers(pipe.unet)))
        v = _variants(step)
        switch("key_off")
    return dict(shape=shape, marked=marked, launches_per_step=dict(geglu_28=v.count(28), gemm_18=v.count(18), conv_deep_27=v.count(27)),
                key_off_ms=t["key_off"], fp8_ff_ms=t["fp8_ff"], fp8_and_fp8_ff_ms=t["fp8_and_fp8_ff"], key_off=_stats(t["key_off"]), fp8_ff=_stats(t["fp8_ff"]),
                fp8_and_fp8_ff=_stats(t["fp8_and_fp8_ff"]), fp8_ff_vs_key_off=_verdict(t["key_off"], t["fp8_ff"]),
                fp8_and_fp8_ff_vs_key_off=_verdict(t["key_off"], t["fp8_and_fp8_ff"]))


def leg_baseline(dev, rounds: int, steps: int):
    """Run with cwd = a checkout of the parent commit (its package, its library): the bf16 tier's s1024 step."""
    import torch
    pipe, step, shape = _s1024(dev)
    with torch.no_grad():
        step()
        step()
        ms = [_ms(step) for _ in range(rounds * steps)]
        return dict(shape=shape, step_ms=ms, **_stats(ms))


def leg_quality(dev, draws: int):
    import torch
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api import AutoencoderKL, UNet2DConditionModel
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    from omgsr_amd.testing import psnr, rel_l2, seeded_init_, synthetic_lq
    rows = []
    for draw in range(draws):
        vae_sd = seeded_init_(AutoencoderKL(), 101 + 31 * draw, rounded=False).state_dict()
        unet_sd = seeded_init_(UNet2DConditionModel(), 202 + 31 * draw, rounded=False).state_dict()
        g = torch.Generator().manual_seed(4321 + draw)
        x = synthetic_lq(QUALITY_BATCH, 1024, 1024, seed=1234 + draw).to(dev)
        eps = torch.randn(QUALITY_BATCH, 4, 128, 128, generator=torch.Generator().manual_seed(99 + draw)).to(dev)
        prompt = torch.randn(1, 77, 1024, generator=g).to(dev)

        def modules():
            pv, pu = AutoencoderKL(), UNet2DConditionModel()
            pv.load_state_dict(vae_sd)
            pu.load_state_dict(unet_sd)
            return pv, pu

        def run(mods, wd, policy=None):
            pipe = OMGSR_S_Infer(None, None, 273, dev, wd, vae=mods[0], unet=mods[1], precision_policy=policy)
            pipe.vae.posterior_noise = eps
            with torch.no_grad():
                return pipe(x.to(wd), prompt.to(wd), 64, 32)[0].float()

        ref = run(modules(), torch.float32)
        row = dict(draw=draw, batch=QUALITY_BATCH)
        mods = modules()                                    # one set of bf16 modules per draw: only the marks change between the rows
        for name, pol in ROWS.items():
            y = run(mods, torch.bfloat16, None if pol is None else {"unet": pol})
            row[name] = dict(rel_l2=rel_l2(y, ref), psnr_db=round(psnr(y, ref), 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    ops.set_compute_dtype(torch.bfloat16)
    return rows


def _child(leg: str, rounds: int, steps: int, draws: int) -> None:
    import torch
    from omgsr_amd import _lib, ops
    dev = torch.device("cuda", 0)
    _lib.check(_lib.load().omgsr_check_device(), "omgsr_check_device")
    ops.set_compute_dtype(torch.bfloat16)
    out = {"layers": lambda: leg_layers(dev, rounds, steps), "step": lambda: leg_step(dev, rounds, steps),
           "baseline": lambda: leg_baseline(dev, rounds, steps), "quality": lambda: leg_quality(dev, draws)}[leg]()
    print("RESULT " + json.dumps(out), flush=True)


def _run_leg(leg: str, args, cwd: str):
    """A fresh child process per leg, under that leg's time limit; raises when it fails or runs out of time (nothing else is started then)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--rounds", str(args.rounds), "--steps", str(args.steps), "--draws", str(args.draws)]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=LIMITS[leg])
    sys.stdout.write("".join(ln + "\n" for ln in r.stdout.splitlines() if not ln.startswith("RESULT ")))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"leg {leg} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(lines[-1][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="timed calls per arm per round")
    ap.add_argument("--draws", type=int, default=3)
    ap.add_argument("--legs", default="layers,step,quality")
    ap.add_argument("--baseline-repo", default=None, help="a checkout of the parent commit with its library built: its s1024 bf16 step is timed first")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_unet_ff.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.child == "baseline":        # the parent's package: whatever checkout the process was started in
            sys.path[0] = os.getcwd()
        return _child(args.child, args.rounds, args.steps, args.draws)
    import torch
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps": args.steps,
           "note": "seeded synthetic weights and inputs (no real checkpoint exists on the build machines)"}
    if os.path.isfile(args.out):
        out = {**json.load(open(args.out)), **out}
    legs = [v for v in args.legs.split(",") if v]
    if args.baseline_repo and "step" in legs:
        out["parent_build_step"] = _run_leg("baseline", args, args.baseline_repo)
    for leg in legs:
        out[leg] = _run_leg(leg, args, ROOT)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
