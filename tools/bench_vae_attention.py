"""The VAE mid block's attention (one head of 512) per `VaeAttention.attend` call: the fused kernel (vae_attn_kernel, one launch) against the
materialised path (the k padding / [hi | hi | lo] copy, the score GEMM, the row softmax, the PV GEMM), on the same q / k / V^T operands. The
projections, which both paths share, are left out.

  (N, L) = (8, 16384) bf16 and accurate   OMGSR-F 256 -> 1024, batch 8: the default workload's encode / decode
           (16, 4096) bf16                OMGSR-S 1024 tiled decode: tile groups
           (1, 20480), (1, 65536) bf16    1280 x 1024 and 2048^2 untiled: fused only (the materialised path stops at 16384 keys)

--tier range-fallback (fp32 stream, bf16 operands, every operand a two-term split): the fused full-split kernel (vae_attn_full_kernel, the
opt-in route "fused_split") against the tier's materialised chain, both from q / k as their projections wrote them and V as its projection's
fp32 output (each path transposes and splits it itself), written to profiles/vae_fused_attention_rf.json

  (N, L) = (4, 4096), (1, 16384)          the sizes both run
           (1, 20480)                     fused only

HIP-event timing, 3 alternated rounds, torch.cuda.max_memory_allocated of each path on top of the operands. Every case runs in a child process
of its own under a time limit; the first failure ends the run.

    python tools/bench_vae_attention.py [--rounds 3] [--out profiles/vae_fused_attention.json]
    python tools/bench_vae_attention.py --tier range-fallback [--rounds 3] [--out profiles/vae_fused_attention_rf.json]
    python tools/bench_vae_attention.py --case 8x16384_bf16          # one case, one JSON line
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

C = 512
CASES = {       # name: (N, L, tier, with the materialised path, timed launches per sample, time limit in seconds)
    "8x16384_bf16": (8, 16384, "bf16", True, 5, 240),
    "8x16384_accurate": (8, 16384, "accurate", True, 3, 300),
    "16x4096_bf16": (16, 4096, "bf16", True, 10, 180),
    "1x20480_bf16": (1, 20480, "bf16", False, 10, 180),
    "1x65536_bf16": (1, 65536, "bf16", False, 3, 240),
    "4x4096_rf": (4, 4096, "range-fallback", True, 5, 180),
    "1x16384_rf": (1, 16384, "range-fallback", True, 3, 240),
    "1x20480_rf": (1, 20480, "range-fallback", False, 3, 180),
}
OUT = {"fast-accurate": "vae_fused_attention.json", "range-fallback": "vae_fused_attention_rf.json"}


def run_case(name: str, rounds: int) -> dict:
    import torch
    from bench_fp8_tier import _events_ms
    from omgsr_amd import _lib, ops
    N, L, tier, with_mat, iters, _ = CASES[name]
    dev = torch.device("cuda", 0)
    _lib.check(_lib.load().omgsr_check_device(), "omgsr_check_device")
    full = tier == "range-fallback"
    if full:
        ops.set_compute_dtype(torch.float32, operand_dtype=torch.bfloat16)
    else:
        ops.set_compute_dtype(torch.float32 if tier == "accurate" else torch.bfloat16)
    dt, split = ops.act_dtype(), tier != "bf16"               # accurate tier: q / k as two-term splits (precision.VAE_QK_SPLIT), out_split 2
    g = torch.Generator(device=dev).manual_seed(11)
    Lp = ops._round_up(L, 128)
    mk = lambda: torch.randn(N, L, C, generator=g, device=dev) * 1.5           # noqa: E731
    sp = lambda t: torch.cat([t.to(dt), (t - t.to(dt).float()).to(dt)], -1) if split else t.to(dt)      # noqa: E731
    q, k = sp(mk()), sp(mk())
    if full:
        v32 = torch.randn(N, L, C, generator=g, device=dev)
    else:
        vt = torch.zeros(N, C, Lp, device=dev, dtype=dt)
        vt[..., :L] = torch.randn(N, C, L, generator=g, device=dev).to(dt)
    osp = 2 if split else 1
    scale = C ** -0.5

    def fused():
        if full:            # VaeAttention.attend, route "fused_split"
            return ops.attention(q, k, ops.transpose_split(v32, ops._round_up(L, 8)), 1, C, scale, out_split=2, q_lo_col=C, k_lo_col=C, p_split=True)
        return ops.attention(q, k, vt, 1, C, scale, Lk=L, out_split=osp, q_lo_col=C if split else None, k_lo_col=C if split else None, p_split=False)

    def materialised():
        if split:
            kk = ops.split_rows_hhl(k, Lp)
        elif Lp != L:
            kk = torch.zeros((N, Lp, C), device=dev, dtype=dt)
            kk[:, :L] = k
        else:
            kk = k
        s = ops.bmm_nt(q, kk, alpha=scale, out_dtype=ops.OUT_F32, both_split=split)
        if full:
            vts = ops.transpose_split(v32, Lp)
            vt3 = torch.cat([vts[:, :C], vts[:, :C], vts[:, C:]], dim=-1)
            p = ops.softmax_rows(s, valid=L, split=True)
            del s, vts
            return ops.bmm_nt(p, vt3, out_split=2, both_split=True)
        p = ops.softmax_rows(s, valid=L)
        del s
        return ops.bmm_nt(p, vt, out_split=osp)

    arms = {"fused": fused, **({"materialised": materialised} if with_mat else {})}
    ms = {a: [] for a in arms}
    peak = {}
    for r in range(rounds):
        for a in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            ms[a].append(_events_ms(arms[a], iters, warm=2))
    for a, fn in arms.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak[a] = torch.cuda.max_memory_allocated() - base
        del out
    flops = 4.0 * N * L * L * C
    rec = dict(case=name, N=N, L=L, tier=tier, operand=str(dt).replace("torch.", ""), split_qk=split, algorithmic_tflop=round(flops / 1e12, 3))
    for a in arms:
        med = statistics.median(ms[a])
        rec[a] = dict(median_ms=round(med, 3), samples_ms=[round(t, 3) for t in ms[a]], tflops=round(flops / med / 1e9, 1),
                      peak_bytes_above_operands=int(peak[a]))
    if with_mat:
        rec["fused_over_materialised_time"] = round(rec["fused"]["median_ms"] / rec["materialised"]["median_ms"], 3)
        rec["fused_faster_in_every_round"] = max(ms["fused"]) < min(ms["materialised"])
        a, b = fused().float(), materialised().float()
        if full:            # hi + lo: the two routes may round a value's hi half to different neighbours
            a, b = a[..., :C] + a[..., C:], b[..., :C] + b[..., C:]
        rec["fused_vs_materialised_rel_l2"] = float(((a[..., :C] - b[..., :C]).norm() / b[..., :C].norm()).item())
    if full:
        rec["mfma_work_over_algorithmic"] = 13.5          # (96 score + 12 PV MFMAs per 32-key tile and wave) x 8 parts, against 64
    ops.set_compute_dtype(torch.bfloat16)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--case", choices=sorted(CASES), help="run this case in this process and print its JSON line")
    ap.add_argument("--tier", choices=sorted(OUT), default="fast-accurate", help="which leg a run without --case covers")
    ap.add_argument("--out", help="default: profiles/vae_fused_attention.json, or profiles/vae_fused_attention_rf.json for --tier range-fallback")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", OUT[args.tier])
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.rounds)), flush=True)
        return 0
    rec = dict(cases=[])
    for name, spec in CASES.items():            # one child process per case, each under its own time limit; stop at the first failure
        if (spec[2] == "range-fallback") != (args.tier == "range-fallback"):
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=spec[5])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"case {name} failed (exit status {r.returncode}); nothing further is started", file=sys.stderr)
            return 1
        rec["cases"].append(json.loads(line[-1][7:]))
        print(line[-1][7:], flush=True)
    import torch
    rec["device"], rec["torch"] = torch.cuda.get_device_name(0), torch.__version__
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
