"""The fp8 tier's opt-in VAE convolutions (precision_policy {"vae": {"fp8": ...}}) against the bf16 VAE, in one process (bench.py never runs them):

  * layers: every eligible layer shape of the FLUX VAE at 1024^2, batch 8 - GroupNorm + SiLU + 3x3 conv as the bf16 path runs it (the halo
    kernel with the norm fused into its patch producer, or the apply pass + the halo kernel) against the apply-to-MXFP8 pass + mxfp8_conv_kernel;
    HIP events, alternated rounds. A shape belongs in precision.VAE_FP8 only if the fp8 arm wins in every round;
  * step: VAE encode, VAE decode and the whole OMGSR-F 256 -> 1024 batch-8 step (bench.py's f1024 workload) in the fp8 tier with and without
    the key, same process, alternated rounds;
  * quality (--quality): full depth, OMGSR-F 256 -> 1024, batch 1, seeded draws, the fp8 tier with and without the key against the accurate tier.

  * tiled (--tiled; nothing else runs): the FLUX VAE's TILED decode (VAEHook, decoder tile 64: tile shapes 86 / 64 latents) of a 128 x 128
    latent, batch 8 - the 16-bit tiled decode against the fp8 tiled decode (the marked layers' tile-shape groups through
    gn_apply_mxfp8_multi_kernel + mxfp8_conv_multi_kernel), same process, alternated rounds, HIP events; and the kind-1 launches of one decode
    per arm by timing variant (21 / 22 / others). With --quality: the seeded full-depth draws above with both VAEs tiled (encoder tile 512,
    decoder tile 64), the fp8 tier with and without the key (default list) against the accurate tier.

  * upsample (--upsample; nothing else runs; writes profiles/fp8_vae_upsample.json): precision_policy {"vae": {"fp8_upsample": ...}} on against
    off, every timed step kept (the acceptance rule of DESIGN 3.1: every step of the on arm faster than every step of the off arm) -
    per layer, the decoder's three up-sampler shapes at batch 8 (low-resolution maps 128^2 / 256^2 / 512^2 with 512 / 512 / 256 channels): the
    16-bit phase form against quantize_mxfp8 + mxfp8_conv_up_kernel (the quantise pass counted, and timed alone too); the untiled 1024^2 decode
    and the tiled decode (decoder tile 64) of the {"fp8": True} VAE with the key on against off. 3 alternated rounds x 3 steps, HIP events.
    --baseline-repo PATH: a checkout of the PARENT commit with its library built - its decode and tiled decode ({"fp8": True}) are timed by a
    fresh child process started there, in front of this build's legs, in the same visit.

    python tools/bench_fp8_vae.py [--rounds 3] [--no-step] [--quality] [--tiled] [--out profiles/fp8_vae.json]
    python tools/bench_fp8_vae.py --upsample [--baseline-repo PATH] [--out profiles/fp8_vae_upsample.json]
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

# (map side, Cin, Cout, layers of that shape in encoder + decoder) of the FLUX VAE's resnet conv1 / conv2 at 1024^2
SHAPES = [(1024, 128, 128, 4 + 5), (1024, 256, 128, 1), (512, 128, 256, 1), (512, 256, 256, 3 + 5), (512, 512, 256, 1),
          (256, 256, 512, 1), (256, 512, 512, 3 + 6), (128, 512, 512, 8 + 10)]


def _events_ms(fn, iters: int) -> float:
    import torch
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def layer_table(dev, batch: int, rounds: int) -> list:
    import torch
    from omgsr_amd import ops
    rows = []
    for side, cin, cout, count in SHAPES:
        g = torch.Generator(device=dev).manual_seed(side + cin + cout)
        x = torch.randn(batch, side, side, cin, generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn(cout, cin, 3, 3, generator=g, device=dev) / (3.0 * cin ** 0.5)).to(torch.bfloat16)
        b = torch.zeros(cout, device=dev)
        p16 = ops.pack_conv_weight(w, b)
        p8 = ops.pack_conv_weight_mxfp8(w, b)
        gamma, beta = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
        mean, rstd, _ = ops.group_norm_stats(x, 32, 1e-6)
        spec = lambda: ops.GnSpec(mean, rstd, gamma, beta, 32, ops.ACT_SILU)      # noqa: E731  (a fresh spec per call: its table is built per call)
        arms = {"bf16": lambda: ops.conv2d(x, p16, gn=spec(), gn_groups=32),
                "fp8": lambda: ops.conv2d(x, p16, gn=spec(), gn_groups=32, fp8_pack=lambda: p8),
                "fp8_apply_only": lambda: spec().apply(x, 5)}
        for fn in arms.values():
            for _ in range(2):
                fn()
        iters = 10 if side >= 512 else 30
        t = {k: [] for k in arms}
        for r in range(rounds):
            for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
                t[k].append(_events_ms(arms[k], iters))
        fl = 2.0 * batch * side * side * 9 * cin * cout
        row = dict(side=side, cin=cin, cout=cout, batch=batch, layers=count,
                   bf16_ms=[round(v, 4) for v in t["bf16"]], fp8_ms=[round(v, 4) for v in t["fp8"]], fp8_apply_ms=[round(v, 4) for v in t["fp8_apply_only"]],
                   speedup_median=round(statistics.median(t["bf16"]) / statistics.median(t["fp8"]), 3),
                   fp8_conv_tflops=round(fl / (statistics.median(t["fp8"]) - statistics.median(t["fp8_apply_only"])) / 1e9, 1),
                   bf16_tflops=round(fl / statistics.median(t["bf16"]) / 1e9, 1),
                   fp8_faster_in_every_round=all(a > c for a, c in zip(t["bf16"], t["fp8"])))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, w, p16, p8
        torch.cuda.empty_cache()
    return rows


def step_rounds(dev, rounds: int, steps: int) -> dict:
    import torch
    import bench
    from omgsr_amd import ops
    from omgsr_amd.precision import FLUX_FP8, clear_fp8_conv, fp8_conv_layers, set_fp8_conv, set_fp8_linear
    family, side, B, tile, overlap, _ = bench.WORKLOADS["f1024"]
    pipe, _ = bench.build_f(dev, 0, 1, torch.bfloat16)
    set_fp8_linear(pipe.flux_transformer, FLUX_FP8)
    inp = bench.make_inputs(family, side, B, tile, 0, dev, torch.bfloat16)
    pipe.vae.posterior_noise = inp["eps"].to(dev)
    step = bench.make_step(pipe, family, inp, tile, overlap)
    lq = ops.nchw_to_nhwc(inp["lq"].to(dev, torch.bfloat16).contiguous(), 8)
    z = torch.randn(B, side // 8, side // 8, 16, device=dev).to(torch.bfloat16)
    parts = {"step": step, "encode": lambda: pipe.vae.encode_moments_nhwc(lq), "decode": lambda: pipe.vae.decode_nhwc(z)}
    times = {arm: {k: [] for k in parts} for arm in ("fp8_tier", "fp8_tier_vae_fp8")}
    marked = 0
    with torch.no_grad():
        for r in range(rounds):
            for arm in (list(times) if r % 2 == 0 else list(times)[::-1]):
                if arm == "fp8_tier":
                    clear_fp8_conv(pipe.vae)
                else:
                    marked = set_fp8_conv(pipe.vae, True)
                for k, fn in parts.items():
                    fn(); fn()                      # warm: (re-)packs
                    torch.cuda.synchronize()
                    for _ in range(steps):
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[arm][k].append(time.perf_counter() - t0)
                print(f"round {r} {arm}: " + ", ".join(f"{k} {statistics.median(v[-steps:]) * 1e3:.1f} ms" for k, v in times[arm].items()), flush=True)
        names = fp8_conv_layers(pipe.vae)
        clear_fp8_conv(pipe.vae)
    out = {"marked_layers": marked or len(names)}
    for arm, d in times.items():
        out[arm] = {k: dict(median_ms=round(statistics.median(v) * 1e3, 2), min_ms=round(min(v) * 1e3, 2), max_ms=round(max(v) * 1e3, 2)) for k, v in d.items()}
    out["shape"] = dict(workload="f1024", side=side, batch=B, tile=tile, overlap=overlap)
    return out


# the per-group table of the quality leg: the fp8 tier alone, the whole default list, then encoder / decoder / mid blocks and resolution levels
GROUPS = {"fp8_tier": None, "vae_fp8_true": True, "encoder": [r"^encoder\."], "decoder": [r"^decoder\."], "mid_blocks": [r"mid_block"],
          "decoder_128_256px": [r"^decoder\.up_blocks\.[01]\."], "decoder_512px": [r"^decoder\.up_blocks\.2\."], "decoder_1024px": [r"^decoder\.up_blocks\.3\."],
          "encoder_1024px": [r"^encoder\.down_blocks\.0\."], "encoder_512px_and_below": [r"^encoder\.down_blocks\.[123]\."]}


def quality(dev, draws: int) -> list:
    """Full depth, OMGSR-F 256 -> 1024, batch 1 (tests/test_fp8_gpu.py's full-depth case, per draw): PSNR / rel-L2 against the accurate tier."""
    import torch
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG, FluxTransformer2DModel
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer, prepare_latent_image_ids
    from omgsr_amd.testing import psnr, rel_l2, seeded_init_, seeded_init_device_, synthetic_lq
    rows = []
    for draw in range(draws):
        ops.set_compute_dtype(torch.float32)
        with torch.device("meta"):
            pf = FluxTransformer2DModel()
        pf = pf.to_empty(device=dev)
        seeded_init_device_(pf, 404 + 31 * draw)
        pf.round_timestep_to_weight_dtype = False
        vae_sd = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303 + 31 * draw, rounded=False).state_dict()
        g = torch.Generator().manual_seed(4321 + draw)
        x = synthetic_lq(1, 1024, 1024, seed=1234 + draw).to(dev)
        eps = torch.randn(1, 16, 128, 128, generator=torch.Generator().manual_seed(99 + draw)).to(dev)
        pe, pooled = torch.randn(1, 512, 4096, generator=g).to(dev), torch.randn(1, 768, generator=g).to(dev)
        tids, iids = torch.zeros(512, 3, device=dev), prepare_latent_image_ids(64, 64, dev, torch.float32)

        def run(wd, policy=None):
            pv = AutoencoderKL(**FLUX_VAE_CONFIG)
            pv.load_state_dict(vae_sd)
            pipe = OMGSR_F_Infer(None, None, dev, wd, 244, 1.0, vae=pv, flux_transformer=pf, precision_policy=policy)
            pipe.vae.posterior_noise = eps
            cd = torch.float32 if wd == torch.float32 else torch.bfloat16
            with torch.no_grad():
                return pipe(x.to(cd), pe.to(cd), pooled.to(cd), tids.to(cd), iids.to(cd), 128, 64)[0].float()

        ref = run(torch.float32)
        row = dict(draw=draw)
        for name, pol in GROUPS.items():
            y = run(torch.float8_e4m3fn, None if pol is None else {"vae": {"fp8": pol}})
            row[name] = dict(rel_l2=rel_l2(y, ref), psnr_db=round(psnr(y, ref), 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pf
        torch.cuda.empty_cache()
    ops.set_compute_dtype(torch.bfloat16)
    return rows


def _variant_counts(fn, variants=(21, 22)) -> dict:
    """Kind-1 (conv / GEMM) launches of one fn() call by timing variant: {"21": n, "22": n, "others": n}, and the number of layers they stand for."""
    import torch
    from omgsr_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.omgsr_timing_enable(1)
    lib.omgsr_timing_reset()
    try:
        fn()
        buf = (_lib.TimingEntry * 8192)()
        n = lib.omgsr_timing_collect(buf, 8192)
    finally:
        lib.omgsr_timing_enable(0)
    v = [e.variant for e in buf[:n] if e.kind == 1]
    return {**{str(k): v.count(k) for k in variants}, "others": len(v) - sum(v.count(k) for k in variants)}


def tiled_decode(dev, batch: int, rounds: int, iters: int) -> dict:
    """FLUX VAE tiled decode, 128 x 128 latent, decoder tile 64: one VAE, one hook; the arms differ in the hook's fp8_convs only (the marks and
    both weight packs stay), so they alternate without re-packing."""
    import torch
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
    from omgsr_amd.pipelines.vaehook import VAEHook
    from omgsr_amd.precision import fp8_conv_layers, set_fp8_conv
    from omgsr_amd.testing import seeded_init_
    vae = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303, rounded=False).to(dev, torch.bfloat16).eval()
    marked = set_fp8_conv(vae, True)
    hook = VAEHook(vae.decoder, 64, is_decoder=True, fast_decoder=False, fast_encoder=False, color_fix=False)
    z = torch.randn(batch, 128, 128, 16, generator=torch.Generator().manual_seed(77)).to(dev, torch.bfloat16)
    arms = {"bf16_tiled": False, "fp8_tiled": True}
    t = {k: [] for k in arms}
    counts = {}
    with torch.no_grad():
        for k, on in arms.items():
            hook.fp8_convs = on
            hook(z); hook(z)                        # warm: packs, code objects
            counts[k] = _variant_counts(lambda: hook(z))
        for r in range(rounds):
            for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
                hook.fp8_convs = arms[k]
                hook(z)
                t[k].append(_events_ms(lambda: hook(z), iters))
            print(f"round {r}: " + ", ".join(f"{k} {t[k][-1]:.2f} ms" for k in arms), flush=True)
    out = dict(shape=dict(latent=128, batch=batch, decoder_tile=64, tile_shapes=[86, 64]), marked_layers=marked, layers=fp8_conv_layers(vae),
               iters_per_round=iters, bf16_tiled_ms=[round(v, 3) for v in t["bf16_tiled"]], fp8_tiled_ms=[round(v, 3) for v in t["fp8_tiled"]],
               speedup_median=round(statistics.median(t["bf16_tiled"]) / statistics.median(t["fp8_tiled"]), 3),
               fp8_faster_in_every_round=all(a > c for a, c in zip(t["bf16_tiled"], t["fp8_tiled"])),
               kind1_launches_by_variant=counts)
    return out


def tiled_quality(dev, draws: int) -> list:
    """quality()'s seeded draws with both VAEs tiled (encoder tile 512: the 1024^2 input splits into 2 x 2 tiles; decoder tile 64), default list."""
    import torch
    from omgsr_amd import ops
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG, FluxTransformer2DModel
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer, prepare_latent_image_ids
    from omgsr_amd.testing import psnr, rel_l2, seeded_init_, seeded_init_device_, synthetic_lq
    rows = []
    for draw in range(draws):
        ops.set_compute_dtype(torch.float32)
        with torch.device("meta"):
            pf = FluxTransformer2DModel()
        pf = pf.to_empty(device=dev)
        seeded_init_device_(pf, 404 + 31 * draw)
        pf.round_timestep_to_weight_dtype = False
        vae_sd = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303 + 31 * draw, rounded=False).state_dict()
        g = torch.Generator().manual_seed(4321 + draw)
        x = synthetic_lq(1, 1024, 1024, seed=1234 + draw).to(dev)
        eps = torch.randn(1, 16, 128, 128, generator=torch.Generator().manual_seed(99 + draw)).to(dev)
        pe, pooled = torch.randn(1, 512, 4096, generator=g).to(dev), torch.randn(1, 768, generator=g).to(dev)
        tids, iids = torch.zeros(512, 3, device=dev), prepare_latent_image_ids(64, 64, dev, torch.float32)

        def run(wd, policy=None):
            pv = AutoencoderKL(**FLUX_VAE_CONFIG)
            pv.load_state_dict(vae_sd)
            pipe = OMGSR_F_Infer(None, None, dev, wd, 244, 1.0, vae=pv, flux_transformer=pf, precision_policy=policy)
            pipe._init_tiled_vae(encoder_tile_size=512, decoder_tile_size=64, fp8_convs=policy is not None)
            pipe.vae.posterior_noise = eps
            cd = torch.float32 if wd == torch.float32 else torch.bfloat16
            with torch.no_grad():
                return pipe(x.to(cd), pe.to(cd), pooled.to(cd), tids.to(cd), iids.to(cd), 128, 64)[0].float()

        ref = run(torch.float32)
        row = dict(draw=draw)
        for name, pol in (("fp8_tier_tiled", None), ("vae_fp8_true_tiled", {"vae": {"fp8": True}})):
            y = run(torch.float8_e4m3fn, pol)
            row[name] = dict(rel_l2=rel_l2(y, ref), psnr_db=round(psnr(y, ref), 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pf
        torch.cuda.empty_cache()
    ops.set_compute_dtype(torch.bfloat16)
    return rows


# ---- --upsample ----------------------------------------------------------------------------------------------------------------------------
# (low-resolution map side, channels) of decoder.up_blocks.{0, 1, 2}.upsamplers.0.conv at 1024^2
UP_SHAPES = [(128, 512), (256, 512), (512, 256)]


def _alternate(arms: dict, rounds: int, steps: int, before=None) -> dict:
    """{arm: [ms of every timed step]}: `rounds` alternated rounds of `steps` single timed calls per arm (before(arm) switches the arm, then one
    untimed call)."""
    t = {k: [] for k in arms}
    for r in range(rounds):
        for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            if before is not None:
                before(k)
            arms[k]()
            for _ in range(steps):
                t[k].append(round(_events_ms(arms[k], 1), 4))
    return t


def _verdict(off, on) -> dict:
    return dict(speedup_median=round(statistics.median(off) / statistics.median(on), 3), every_on_step_faster_than_every_off_step=max(on) < min(off))


def upsample_layers(dev, batch: int, rounds: int, steps: int) -> list:
    import torch
    from omgsr_amd import ops
    rows = []
    for side, ch in UP_SHAPES:
        g = torch.Generator(device=dev).manual_seed(side + ch)
        x = torch.randn(batch, side, side, ch, generator=g, device=dev).to(torch.bfloat16)
        w = (torch.randn(ch, ch, 3, 3, generator=g, device=dev) / (3.0 * ch ** 0.5)).to(torch.bfloat16)
        b = torch.zeros(ch, device=dev)
        p16 = ops.pack_conv_weight(w, b, cout_multiple=8, upsample_phases=True)
        p8 = ops.pack_conv_weight_mxfp8_up(w, b)
        arms = {"bf16_phase_form": lambda: ops.conv2d(x, p16, upsample=True, gn_groups=32),
                "quantize_plus_mxfp8_up": lambda: ops.conv2d(x, p16, upsample=True, gn_groups=32, fp8_up_pack=lambda: p8),
                "quantize_only": lambda: ops.quantize_mxfp8(x)}
        for fn in arms.values():
            fn(); fn()
        counts = _variant_counts(arms["quantize_plus_mxfp8_up"], (25,))
        t = _alternate(arms, rounds, steps)
        fl = 2.0 * batch * 4 * side * side * 9 * ch * ch          # algorithmic (nine taps on the up-sampled map); the phase form runs 4 / 9 of it
        row = dict(low_res_side=side, channels=ch, batch=batch, served=counts["25"] == 1, ms=t,
                   bf16_tflops=round(fl / statistics.median(t["bf16_phase_form"]) / 1e9, 1),
                   mxfp8_conv_alone_tflops=round(fl / (statistics.median(t["quantize_plus_mxfp8_up"]) - statistics.median(t["quantize_only"])) / 1e9, 1),
                   **_verdict(t["bf16_phase_form"], t["quantize_plus_mxfp8_up"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, w, p16, p8
        torch.cuda.empty_cache()
    return rows


# What a checkout WITHOUT the key can run (the parent commit): the {"fp8": True} VAE's untiled and tiled decode, every step's time as JSON.
_BASELINE_CHILD = r"""
import json, sys, torch
sys.path.insert(0, ".")
from omgsr_amd import _lib, ops
from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
from omgsr_amd.pipelines.vaehook import VAEHook
from omgsr_amd.precision import set_fp8_conv
from omgsr_amd.testing import seeded_init_
batch, rounds, steps = (int(v) for v in sys.argv[1:4])
dev = torch.device("cuda", 0)
_lib.check(_lib.load().omgsr_check_device(), "omgsr_check_device")
ops.set_compute_dtype(torch.bfloat16)
vae = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303, rounded=False).to(dev, torch.bfloat16).eval()
set_fp8_conv(vae, True)
hook = VAEHook(vae.decoder, 64, is_decoder=True, fast_decoder=False, fast_encoder=False, color_fix=False)
hook.fp8_convs = True
z = torch.randn(batch, 128, 128, 16, generator=torch.Generator().manual_seed(77)).to(dev, torch.bfloat16)
def ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return round(a.elapsed_time(b), 4)
out = {}
with torch.no_grad():
    for name, fn in (("decode", lambda: vae.decode_nhwc(z)), ("tiled_decode", lambda: hook(z))):
        fn(); fn()
        out[name] = [ms(fn) for _ in range(rounds * steps)]
print("BASELINE " + json.dumps(out))
"""


def upsample_baseline(repo: str, batch: int, rounds: int, steps: int) -> dict:
    """The parent commit's build, timed by a fresh child process in its own checkout (its package, its library)."""
    import subprocess
    r = subprocess.run([sys.executable, "-c", _BASELINE_CHILD, str(batch), str(rounds), str(steps)], cwd=repo, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("BASELINE ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"baseline run in {repo} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(lines[-1][len("BASELINE "):])


def upsample_decodes(dev, batch: int, rounds: int, steps: int) -> dict:
    """The {"fp8": True} FLUX VAE, 128 x 128 latent: untiled decode and tiled decode (decoder tile 64, fp8_convs hooks), fp8_upsample on against off."""
    import torch
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
    from omgsr_amd.pipelines.vaehook import VAEHook
    from omgsr_amd.precision import clear_fp8_upsample, set_fp8_conv, set_fp8_upsample
    from omgsr_amd.testing import seeded_init_
    vae = seeded_init_(AutoencoderKL(**FLUX_VAE_CONFIG), 303, rounded=False).to(dev, torch.bfloat16).eval()
    set_fp8_conv(vae, True)
    hook = VAEHook(vae.decoder, 64, is_decoder=True, fast_decoder=False, fast_encoder=False, color_fix=False)
    hook.fp8_convs = True
    z = torch.randn(batch, 128, 128, 16, generator=torch.Generator().manual_seed(77)).to(dev, torch.bfloat16)

    def switch(arm):
        if arm == "on":
            set_fp8_upsample(vae, True)
        else:
            clear_fp8_upsample(vae)

    out = {}
    with torch.no_grad():
        for name, fn in (("decode", lambda: vae.decode_nhwc(z)), ("tiled_decode", lambda: hook(z))):
            arms = {"off": fn, "on": fn}
            counts = {}
            for k in arms:
                switch(k)
                fn(); fn()                              # warm: packs, code objects
                counts[k] = _variant_counts(fn, (21, 22, 25, 26))
            t = _alternate(arms, rounds, steps, before=switch)
            out[name] = dict(ms=t, kind1_launches_by_variant=counts, **_verdict(t["off"], t["on"]))
            print(name, json.dumps(out[name]), flush=True)
    clear_fp8_upsample(vae)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="timed calls per arm per round")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--quality", action="store_true", help="also the full-depth quality draws (minutes)")
    ap.add_argument("--draws", type=int, default=3)
    ap.add_argument("--tiled", action="store_true", help="the tiled VAE decode legs only (with --quality: the tiled full-depth draws)")
    ap.add_argument("--iters", type=int, default=5, help="--tiled: decodes per timed window")
    ap.add_argument("--upsample", action="store_true", help="the fp8_upsample legs only (default --out profiles/fp8_vae_upsample.json)")
    ap.add_argument("--baseline-repo", default=None, help="--upsample: a checkout of the parent commit with its library built, timed first")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "fp8_vae_upsample.json" if args.upsample else "fp8_vae.json")
    import torch
    from omgsr_amd import _lib, ops
    dev = torch.device("cuda", 0)
    _lib.check(_lib.load().omgsr_check_device(), "omgsr_check_device")
    ops.set_compute_dtype(torch.bfloat16)
    rec = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)
    if os.path.isfile(args.out):                    # sections measured by an earlier call stay
        with open(args.out) as f:
            rec = {**json.load(f), **rec}
    if args.upsample:
        if args.baseline_repo:
            rec["parent_build_fp8_true_b%d" % args.batch] = dict(ms=upsample_baseline(args.baseline_repo, args.batch, args.rounds, args.steps))
            print(json.dumps(rec["parent_build_fp8_true_b%d" % args.batch]), flush=True)
        rec["layers_b%d" % args.batch] = upsample_layers(dev, args.batch, args.rounds, args.steps)
        rec["decodes_b%d" % args.batch] = upsample_decodes(dev, args.batch, args.rounds, args.steps)
        base = rec.get("parent_build_fp8_true_b%d" % args.batch)
        if base:                                        # the same rule against the parent's build, run just before
            for name, d in rec["decodes_b%d" % args.batch].items():
                d["against_parent_build"] = _verdict(base["ms"][name], d["ms"]["on"])
                d["off_arm_against_parent_build"] = dict(median_ratio=round(statistics.median(d["ms"]["off"]) / statistics.median(base["ms"][name]), 3))
        args.no_layers = args.no_step = True
        args.quality = args.tiled = False
    if args.tiled:
        rec["tiled_decode_b%d" % args.batch] = tiled_decode(dev, args.batch, args.rounds, args.iters)
        print(json.dumps(rec["tiled_decode_b%d" % args.batch]), flush=True)
        if args.quality:
            rec["tiled_full_depth_quality"] = tiled_quality(dev, args.draws)
        args.no_layers = args.no_step = True
        args.quality = False
    if not args.no_layers:
        rec["layers"] = layer_table(dev, args.batch, args.rounds)
    if not args.no_step:
        rec["f1024_b8"] = step_rounds(dev, args.rounds, args.steps)
        print(json.dumps(rec["f1024_b8"]), flush=True)
    if args.quality:
        rec["full_depth_quality"] = quality(dev, args.draws)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
