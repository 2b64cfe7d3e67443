"""Synthetic weights / inputs / metrics shared by tests, bench.py and __graft_entry__.smoke().

There are no checkpoints on the GPU box (and no network), so every model runs with seeded random
weights at the real architecture shapes. All values are bf16-representable so the
fp32 CPU oracle and the bf16 HIP path start from bit-identical parameters.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn


@torch.no_grad()
def seeded_init_(model: nn.Module, seed: int = 0, device=None, rounded: bool = True) -> nn.Module:
    """Fan-in scaled normal weights, small random biases, norm affines near (1, 0). Deterministic per parameter NAME (not
    traversal order), generated on CPU. rounded=True: values rounded to bf16-representable ones (every tier then starts from
    bit-identical parameters); rounded=False: full fp32 mantissas - what a real checkpoint looks like after an fp32 LoRA merge
    (infer/omgsr_s_infer_model.py:16-23), the case the accurate tier's weight-side split exists for."""
    for name, p in model.named_parameters():
        g = torch.Generator().manual_seed((hash_name(name) + seed) & 0x7FFFFFFF)
        shape = tuple(p.shape)
        if p.dim() >= 2:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            v = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        elif name.endswith("weight"):       # norm scale / RMSNorm weight
            v = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:                               # biases
            v = 0.05 * torch.randn(shape, generator=g)
        if rounded:
            v = v.to(torch.bfloat16)
        p.copy_(v.to(p.dtype).to(p.device))
    return model


@torch.no_grad()
def seeded_init_device_(model: nn.Module, seed: int = 0) -> nn.Module:
    """Same recipe as seeded_init_ but generated ON the parameter's device (FLUX.1-dev has 11.9 B parameters:
    a CPU randn of that size takes minutes). Values differ from the CPU recipe; use only where no CPU twin
    of the model is needed (throughput benchmarks)."""
    for name, p in model.named_parameters():
        g = torch.Generator(device=p.device).manual_seed((hash_name(name) + seed) & 0x7FFFFFFF)
        shape = tuple(p.shape)
        if p.dim() >= 2:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            p.copy_(torch.randn(shape, generator=g, device=p.device, dtype=torch.float32).mul_(1.0 / math.sqrt(fan_in)))
        elif name.endswith("weight"):
            p.copy_(torch.randn(shape, generator=g, device=p.device).mul_(0.1).add_(1.0))
        else:
            p.copy_(torch.randn(shape, generator=g, device=p.device).mul_(0.05))
    return model


def hash_name(name: str) -> int:
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def synthetic_lq(batch: int, height: int, width: int, seed: int = 1234) -> torch.Tensor:
    """[B,3,H,W] fp32 in [-1,1]: low-passed random field upsampled x4 (mimics the x4-upscaled LQ image the
    reference feeds the model, infer/infer_omgsr_s.py:81-84)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(batch, 3, height // 4, width // 4, generator=g)
    for _ in range(3):
        u = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(u, (1, 1, 1, 1), mode="replicate"), 3, stride=1)
    x = torch.nn.functional.interpolate(u, size=(height, width), mode="bicubic", align_corners=False)
    x = (x - x.amin(dim=(1, 2, 3), keepdim=True)) / (x.amax(dim=(1, 2, 3), keepdim=True) - x.amin(dim=(1, 2, 3), keepdim=True))
    return (x * 2 - 1).to(torch.bfloat16).float()


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-20)).item()


def psnr(got: torch.Tensor, ref: torch.Tensor, peak: float = 2.0) -> float:
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    mse = (got - ref).pow(2).mean().item()
    return float("inf") if mse == 0 else 10.0 * math.log10(peak * peak / mse)


def mxfp8_ref(x: torch.Tensor):
    """Reference OMGSR_EL_MXFP8 quantiser (include/omgsr_hip.h) on the host: x [..., K] (K % 32 == 0) -> (codes uint8 [..., K],
    scales uint8 [..., K / 32]). scale = max(0, biased exponent of the block's largest |v| - 8); code = (v / 2^(scale - 127)).clamp(-448, 448)
    as e4m3fn (the clamp first: torch does not saturate on this cast). The division is done as the exact multiplication by 2^(127 - scale)."""
    x = x.float()
    K = x.shape[-1]
    blk = x.reshape(*x.shape[:-1], K // 32, 32)
    e = (blk.abs().amax(-1).view(torch.int32) >> 23) & 0xFF
    s = (e - 8).clamp(min=0)
    q = (blk * torch.exp2((127 - s).float())[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.reshape(x.shape), s.to(torch.uint8)


def layer_norm_mxfp8_ref(x: torch.Tensor, a: Optional[torch.Tensor], b: Optional[torch.Tensor], eps: float):
    """Reference of ops.layer_norm_mxfp8 (omgsr_layernorm_mxfp8): mxfp8_ref of the LayerNorm (x - mean) rstd a + b computed in fp32 (two-pass
    variance, as the kernel) and rounded to bf16. x [..., C] (C % 32 == 0), a / b fp32 [C] or None -> (codes, scales)."""
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    d = xf - mu
    y = d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    if a is not None:
        y = y * a.float()
    if b is not None:
        y = y + b.float()
    return mxfp8_ref(y.to(torch.bfloat16))


def mxfp8_dequant(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """The values an MXFP8 (codes, scales) pair stands for, in float64 (exact)."""
    lut = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).double().to(codes.device)
    v = lut[codes.long()]
    K = v.shape[-1]
    s = torch.exp2(scales.double() - 127)
    return (v.reshape(*v.shape[:-1], K // 32, 32) * s[..., None]).reshape(v.shape)


def mxfp8_attention_ref(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, scale: float, Lk: Optional[int] = None, stats: Optional[dict] = None):
    """Torch restatement of mxfp8_attn_kernel's arithmetic (attention_mxfp8.hip), in float64: q [..., Lq, D], k [..., >= Lk, D], vt [..., D, >= Lk]
    are the DEQUANTISED operands (mxfp8_dequant). The keys are walked in the kernel's 64-key tiles with an exact running maximum; the
    probabilities enter the PV product as e4m3(P 2^8) 2^-8 (round to nearest even), and the row sum adds those dequantised values. Keys >= Lk
    are masked. stats (optional dict) receives the largest code value seen ("max_code")."""
    Lk = k.shape[-2] if Lk is None else Lk
    q, k, vt = q.double(), k.double(), vt.double()
    sc = scale * math.log2(math.e)
    m = torch.full(q.shape[:-1], -math.inf, dtype=torch.float64, device=q.device)
    l = torch.zeros_like(m)
    o = torch.zeros(*q.shape[:-1], vt.shape[-2], dtype=torch.float64, device=q.device)
    top = 0.0
    for k0 in range(0, Lk, 64):
        k1 = min(k0 + 64, Lk)
        s = q @ k[..., k0:k1, :].transpose(-1, -2)
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.exp2((m - m_new) * sc)                                # m = -inf on the first tile: alpha = 0
        o, l, m = o * alpha[..., None], l * alpha, m_new
        p = torch.exp2((s - m[..., None]) * sc + 8.0)
        pq = p.float().to(torch.float8_e4m3fn).double()                     # the code's value (P 2^8, in [0, 256])
        top = max(top, float(pq.max()))
        l = l + pq.sum(-1)
        o = o + (pq @ vt[..., :, k0:k1].transpose(-1, -2)) * 2.0 ** -8
    if stats is not None:
        stats["max_code"] = top
    return o / (l[..., None] * 2.0 ** -8)
