"""OMGSR-S's opt-in MXFP8 UNet resnet convolutions (precision_policy {"unet": {"fp8": ...}} on the bf16 tier) against the bf16 tier, every timed
step kept (the acceptance rule of DESIGN 3.1: every step of the fp8 arm faster than every step of the bf16 arm); bench.py never runs them.
Writes profiles/fp8_unet.json. HIP events, 3 alternated rounds x 3 steps. Every leg is a fresh child process with its own time limit; a leg
that fails or runs out of time ends the run.

  * layers: every resnet-conv shape of the SD 2.1 UNet's 64- and 32-wide levels in the s1024 batch-4 workload (36 latent tiles of 64 x 64 in one
    call) - GroupNorm + SiLU + 3x3 conv with the statistics epilogue, as the pipeline runs either arm: bf16 = the halo kernel with the norm
    fused into its patch producer where the library can; fp8 = the apply-to-MXFP8 pass + mxfp8_conv_deep_kernel (the apply pass also timed alone);
  * step: OMGSR-S 256 -> 1024, tiled VAE, batch 4 (bench.py's s1024 workload) on the bf16 tier, the key off against on in one process;
    --baseline-repo PATH: a checkout of the PARENT commit with its library built, timed first by a child started there, in the same visit;
  * quality: OMGSR-S 256 -> 1024, batch 2 (18 latent tiles in one UNet call: at batch 1 the 32-wide level has 180 tiles, under the dispatcher's
    192, and would run in bf16), seeded weights, three draws, against the accurate tier: the key off, every served layer, each level, each path.

    python tools/bench_fp8_unet.py [--baseline-repo PATH] [--legs layers,step,quality] [--out profiles/fp8_unet.json]
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

# (latent side, Cin, Cout, what it is) - the resnet convs of the 64- and 32-wide levels
SHAPES = [(64, 320, 320, "down 0 conv1/conv2, up 3 conv2"), (64, 960, 320, "up 3 resnet 0 conv1"), (64, 640, 320, "up 3 resnets 1-2 conv1"),
          (32, 320, 640, "down 1 resnet 0 conv1"), (32, 640, 640, "down 1 / up 2 conv2, down 1 resnet 1 conv1"), (32, 1920, 640, "up 2 resnet 0 conv1"),
          (32, 1280, 640, "up 2 resnet 1 conv1"), (32, 960, 640, "up 2 resnet 2 conv1")]
TILES = 36
QUALITY_BATCH = 2
# the quality leg's rows: the key off, every served layer, one level, one path (the 64-wide level = down 0 / up 3, the 32-wide = down 1 / up 2)
GROUPS = {"bf16_tier": None, "all_served": [r"^(down_blocks\.[01]|up_blocks\.[23])\."], "level_64": [r"^(down_blocks\.0|up_blocks\.3)\."],
          "level_32": [r"^(down_blocks\.1|up_blocks\.2)\."], "down_path": [r"^down_blocks\.[01]\."], "up_path": [r"^up_blocks\.[23]\."]}
LIMITS = {"layers": 240, "step": 420, "baseline": 420, "quality": 900}      # seconds per leg


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


def _verdict(off, on) -> dict:
    return dict(speedup_median=round(statistics.median(off) / statistics.median(on), 3), every_fp8_step_faster_than_every_bf16_step=max(on) < min(off))


def leg_layers(dev, rounds: int, steps: int):
    import torch
    from omgsr_amd import _lib, ops
    rows = []
    for side, cin, cout, what in SHAPES:
        g = torch.Generator(device=dev).manual_seed(side + cin + cout)
        x = torch.randn(TILES, side, side, cin, generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn(cout, cin, 3, 3, generator=g, device=dev) / (3.0 * cin ** 0.5)).to(torch.bfloat16)
        b = torch.zeros(cout, device=dev)
        p16 = ops.pack_conv_weight(w, b, cout_multiple=8)
        p8 = ops.pack_conv_weight_mxfp8(w, b, cin_multiple=64)
        gamma, beta = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
        mean, rstd, _ = ops.group_norm_stats(x, 32, 1e-5)
        spec = lambda: ops.GnSpec(mean, rstd, gamma, beta, 32, ops.ACT_SILU)      # noqa: E731  (a fresh spec per call: its table is built per call)
        arms = {"bf16": lambda: ops.conv2d(x, p16, gn=spec(), gn_groups=32),
                "fp8": lambda: ops.conv2d(x, p16, gn=spec(), gn_groups=32, fp8_deep_pack=lambda: p8),
                "fp8_apply_only": lambda: ops.group_norm_apply_mxfp8(x, mean, rstd, gamma, beta, 32, ops.ACT_SILU, c64=True)}
        # which kernels each arm runs (kind-1 launches by timing variant)
        lib = _lib.load()
        ran = {}
        for k in ("bf16", "fp8"):
            arms[k]()
            torch.cuda.synchronize()
            lib.omgsr_timing_enable(1)
            lib.omgsr_timing_reset()
            arms[k]()
            buf = (_lib.TimingEntry * 64)()
            n = lib.omgsr_timing_collect(buf, 64)
            lib.omgsr_timing_enable(0)
            ran[k] = sorted(e.variant for e in buf[:n] if e.kind == 1)
        t = _alternate(arms, rounds, steps)
        fl = 2.0 * TILES * side * side * 9 * cin * cout
        row = dict(side=side, cin=cin, cout=cout, tiles=TILES, layers=what, variants=ran, bf16_ms=t["bf16"], fp8_ms=t["fp8"], fp8_apply_ms=t["fp8_apply_only"],
                   bf16_tflops=round(fl / statistics.median(t["bf16"]) / 1e9, 1),
                   fp8_conv_tflops=round(fl / (statistics.median(t["fp8"]) - statistics.median(t["fp8_apply_only"])) / 1e9, 1),
                   fp8_faster_in_every_round=all(max(t["fp8"][r * steps:(r + 1) * steps]) < min(t["bf16"][r * steps:(r + 1) * steps]) for r in range(rounds)),
                   **_verdict(t["bf16"], t["fp8"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, w, p16, p8
        torch.cuda.empty_cache()
    return rows


def _s1024(dev, with_key: bool):
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
    from omgsr_amd import _lib
    from omgsr_amd.precision import clear_fp8_unet_conv, fp8_unet_conv_layers, set_fp8_unet_conv
    pipe, step, shape = _s1024(dev, True)
    lib = _lib.load()

    def switch(arm):
        if arm == "key_off":
            clear_fp8_unet_conv(pipe.unet)
        else:
            set_fp8_unet_conv(pipe.unet, GROUPS["all_served"])
    with torch.no_grad():
        t = _alternate({"key_off": step, "key_on": step}, rounds, steps, before=switch)
        switch("key_on")
        marked = len(fp8_unet_conv_layers(pipe.unet))
        step()
        torch.cuda.synchronize()
        lib.omgsr_timing_enable(1)
        lib.omgsr_timing_reset()
        step()
        buf = (_lib.TimingEntry * 16384)()
        n = lib.omgsr_timing_collect(buf, 16384)
        lib.omgsr_timing_enable(0)
        deep = sum(1 for e in buf[:n] if e.kind == 1 and e.variant == 27)
        clear_fp8_unet_conv(pipe.unet)
    return dict(shape=shape, marked_layers=marked, deep_launches_per_step=deep, key_off_ms=t["key_off"], key_on_ms=t["key_on"], **_verdict(t["key_off"], t["key_on"]))


def leg_baseline(dev, rounds: int, steps: int):
    """Run with cwd = a checkout of the parent commit (its package, its library): the bf16 tier's s1024 step."""
    import torch
    pipe, step, shape = _s1024(dev, False)
    with torch.no_grad():
        step()
        step()
        return dict(shape=shape, step_ms=[_ms(step) for _ in range(rounds * steps)])


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
        for name, pol in GROUPS.items():
            y = run(mods, torch.bfloat16, None if pol is None else {"unet": {"fp8": pol}})
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_unet.json"))
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
