"""Bit-exact probes for the GEMM / conv kernels (not a test module: imported by tests/test_dyadic_probes_*.py).

Operands are dyadic - small signed integers times powers of two - with exponents that vary per row, per channel and per 32-channel block,
so a value paired with the wrong row, channel or block changes by a power of two rather than by nothing. With a bounded bit budget every
product and every partial sum is exact in fp32, whatever the summation order, split-K partition or MFMA-internal grouping; the one rounding
left is the documented output conversion, so a correct kernel matches the float64 restatement below bit for bit.

Budget: for every output, sum |product| + |bias| + |residual| in units of the finest product quantum must stay below 2^22 (fp32 holds 2^24),
and every product must be a normal fp32 value. `Budget` asserts it before a probe's kernel runs: a probe that cannot be exact is a test bug.

Restatements decode the BYTES a kernel reads - the packed weight (`PackedWeight.w` / `w_ph`) and the operand tensor - in the documented forms
(include/omgsr_hip.h, ops.pack_conv_weight):
  16-bit         [a] x [w]
  split          [a_hi | a_lo] x [w_hi | w_hi], optionally + a third segment [w_lo] that wraps back to a_hi (w_split 2)
  MX fp8         [a_hi fp16 | a_lo' e4m3 | a_hi' e4m3] x [w_hi fp16 | w_hi' e4m3 | w_lo' e4m3], the fp8 segments scaled by 2^(mx_scale_* - 127)
  MX6            the same row with e2m3 codes and one E8M0 scale byte per 32-channel block inside the data
  MXFP8          e4m3fn codes x 2^(E8M0 scale - 127) per 32 K values (omgsr_amd.testing.mxfp8_dequant)
and compute the contraction in float64 (on whatever device the tensors are on: the data are exact, so the device result equals the host's).
"""
from __future__ import annotations

import math
import re
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

LIMIT = 2 ** 22          # quanta per output (fp32 carries 2^24: two bits of margin)
MIN_NORMAL = 2.0 ** -126


# ---- generators ------------------------------------------------------------------------------------------------------------------

def signed_ints(gen: torch.Generator, shape, lo: int, hi: int) -> torch.Tensor:
    """Integers with |v| in [lo, hi] and a random sign (float32)."""
    mag = torch.randint(lo, hi + 1, shape, generator=gen).float()
    return mag * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)


def exponents(gen: torch.Generator, rows: int, cols: int, row=(0, 0), col=(0, 0), block: int = 1) -> torch.Tensor:
    """[rows, cols] integer exponents: one per row plus one per `block` consecutive columns (per channel: 1; per 32-channel block: 32)."""
    re_ = torch.randint(row[0], row[1] + 1, (rows, 1), generator=gen)
    ce = torch.randint(col[0], col[1] + 1, (1, (cols + block - 1) // block), generator=gen).repeat_interleave(block, 1)[:, :cols]
    return (re_ + ce).float()


def dyadic(gen: torch.Generator, e: torch.Tensor, mant=(1, 7)) -> torch.Tensor:
    """m 2^e with m a signed integer, |m| in mant."""
    return signed_ints(gen, tuple(e.shape), *mant) * torch.exp2(e)


def two_term(gen: torch.Generator, e: torch.Tensor) -> torch.Tensor:
    """x = hi + lo with hi = m 2^e (|m| in 4 .. 7: the top bit is fixed, so hi's fp16 half-ulp is 2^(e - 9)) and lo = +-2^(e - 11): exact in fp32,
    fp16(x) = hi and x - hi = lo, both nonzero. The low term is a power of two, exact in e4m3 (after MX's 2^11), e2m3 and fp16."""
    return dyadic(gen, e, (4, 7)) + signed_ints(gen, tuple(e.shape), 1, 1) * torch.exp2(e - 11)


def sparse_mask(gen: torch.Generator, rows: int, k: int, nnz: int) -> torch.Tensor:
    """bool [rows, k] with nnz True per row at positions that differ between rows; rows * nnz >= k covers every position."""
    perm = torch.randperm(k, generator=gen)
    idx = (torch.arange(rows)[:, None] * nnz + torch.arange(nnz)[None, :]) % k
    m = torch.zeros(rows, k, dtype=torch.bool)
    m.scatter_(1, perm[idx], True)
    return m


# ---- bit budget --------------------------------------------------------------------------------------------------------------------

def pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k (float64) for integer k >= -1022, built from its bits (torch.ldexp / exp2 need not be exact on every device)."""
    return ((k.to(torch.int64).clamp(min=-1022) + 1023) << 52).view(torch.float64)


def quantum(x: torch.Tensor) -> torch.Tensor:
    """Finest power of two dividing each element (float64); +inf for zeros. (Values below 2^-1022 count as 2^-1022: conservative.)"""
    x = x.double()
    m, e = torch.frexp(x)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = mi & (-mi)
    q = low.double() * pow2(e.to(torch.int64) - 53)
    return torch.where(x == 0, torch.full_like(q, float("inf")), q)


class Budget:
    """Per-output bit budget of a contraction fed as (A [M, k], W [N, k]) segments (one call per segment: the quantum bound is per segment,
    so the a_lo x w_lo product a split form never computes does not count), then the epilogue terms."""

    def __init__(self, M: int, N: int, device):
        self.tot = torch.zeros(M, N, dtype=torch.float64, device=device)
        self.unit = torch.full((M, N), float("inf"), dtype=torch.float64, device=device)

    def add(self, A: torch.Tensor, W: torch.Tensor) -> None:
        self.tot += A.abs() @ W.abs().T
        qa, qw = quantum(A).amin(1), quantum(W).amin(1)
        self.unit = torch.minimum(self.unit, qa[:, None] * qw[None, :])

    def scale(self, g: torch.Tensor) -> None:
        """Multiply by a per-column gate of powers of two (exact)."""
        g = g.double().abs()
        assert torch.equal(quantum(g), g), "gate values must be powers of two"
        self.tot *= g
        self.unit *= g

    def term(self, t: torch.Tensor) -> None:
        t = t.double().expand_as(self.tot)
        self.tot += t.abs()
        self.unit = torch.minimum(self.unit, quantum(t))

    def counts(self) -> torch.Tensor:
        live = self.tot > 0
        return torch.where(live, self.tot / self.unit, torch.zeros_like(self.tot))

    def check(self, limit: float = LIMIT) -> float:
        live = self.tot > 0
        worst = float(self.counts().max())
        assert worst < limit, f"probe over its bit budget: {worst:.3g} quanta > {limit:.3g}"
        if bool(live.any()):
            assert float(self.unit[live].min()) >= MIN_NORMAL and float(self.tot.max()) < 2.0 ** 100, "products outside the normal fp32 range"
        return worst


# ---- byte decoders -----------------------------------------------------------------------------------------------------------------

def e4m3(codes: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3fn codes -> float64 values."""
    lut = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).double().to(codes.device)
    return lut[codes.long()]


_E2M3 = [(m / 8.0) if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1) for e in range(4) for m in range(8)]


def e2m3_third(raw: torch.Tensor) -> torch.Tensor:
    """uint8 [..., C] (C % 64 == 0): one correction third of an OMGSR_EL_MX6 row -> float64 [..., C]. Per 64-byte group, block h owns bytes
    [16h, 16h + 16) and [32 + 16h, 40 + 16h) (channel i at bits [6i, 6i + 6) of that little-endian 192-bit string) and its scale byte 40 + 16h."""
    lead, C = raw.shape[:-1], raw.shape[-1]
    g = raw.reshape(-1, C // 64, 64).long()
    lut = torch.tensor(_E2M3, dtype=torch.float64, device=raw.device)
    bit = torch.arange(32, device=raw.device) * 6
    by, sh = bit // 8, bit % 8
    out = []
    for h in (0, 1):
        st = torch.cat([g[..., 16 * h:16 * h + 16], g[..., 32 + 16 * h:40 + 16 * h]], -1)
        st = torch.cat([st, torch.zeros_like(st[..., :1])], -1)
        code = ((st[..., by] | (st[..., by + 1] << 8)) >> sh) & 63
        val = torch.where((code & 32) != 0, -1.0, 1.0).double() * lut[code & 31]
        out.append(val * torch.exp2(g[..., 40 + 16 * h].double() - 127)[..., None])
    return torch.stack(out, -2).reshape(*lead, C)


def _mx_split(raw: torch.Tensor, C: int, fmt: int, s_hi8: int, s_lo8: int) -> torch.Tensor:
    """4C bytes [fp16 (2C) | third (C) | third (C)] -> float64 [.., 3C]; fmt 8: e4m3 thirds times 2^(s - 127), fmt 6: e2m3 blocks."""
    hi = raw[..., :2 * C].contiguous().view(torch.float16).double()
    if fmt == 6:
        t1, t2 = e2m3_third(raw[..., 2 * C:3 * C]), e2m3_third(raw[..., 3 * C:])
    else:
        t1 = e4m3(raw[..., 2 * C:3 * C]) * 2.0 ** (s_hi8 - 127)
        t2 = e4m3(raw[..., 3 * C:]) * 2.0 ** (s_lo8 - 127)
    return torch.cat([hi, t1, t2], -1)


def operand_values(x: torch.Tensor, pw) -> torch.Tensor:
    """An operand tensor as the kernel reads it against `pw` -> float64 [..., K of one tap] (the wrap of a w_split weight included)."""
    if pw.mx is not None:
        C = pw.cin // 2
        raw = x.contiguous().view(torch.uint8)
        _, a1, _, a2 = pw.mx[1:]
        v = _mx_split(raw, C, pw.mx_fmt or 8, a1, a2)
    else:
        v = x.double()
    if v.shape[-1] < _tap_k(pw):                       # w_split 2: the last segment re-reads the operand's first (hi) half
        v = torch.cat([v, v[..., :_tap_k(pw) - v.shape[-1]]], -1)
    return v


def _tap_k(pw) -> int:
    return 3 * (pw.cin // 2) if pw.mx is not None else pw.cin


def weight_values(pw) -> torch.Tensor:
    """Packed weight bytes -> float64 [Cout_pad, R * S, K of one tap]."""
    taps = pw.R * pw.S
    if pw.mx is not None:
        C = pw.cin // 2
        raw = pw.w.contiguous().view(torch.uint8)[:, :taps * 4 * C].reshape(pw.cout_pad, taps, 4 * C)
        w1, _, w2, _ = pw.mx[1:]
        return _mx_split(raw, C, pw.mx_fmt or 8, w1, w2)
    return pw.w[:, :taps * pw.cin].double().reshape(pw.cout_pad, taps, pw.cin)


def phase_weight_values(pw) -> torch.Tensor:
    """`w_ph` [4][Kslots/32][4][Cout_pad][32] -> float64 [4 phases (2a + b), 4 taps (2dy + dx), Cout_pad, K of one tap]."""
    ks = pw.w_ph.shape[1] * 32
    w = pw.w_ph.permute(0, 2, 3, 1, 4).reshape(4, 4, pw.cout_pad, ks)
    if pw.mx is not None:
        C = pw.cin // 2
        w1, _, w2, _ = pw.mx[1:]
        return _mx_split(w.contiguous().view(torch.uint8), C, pw.mx_fmt or 8, w1, w2)
    return w.double()


def segments(pw) -> list:
    """(start, end) ranges of one tap's K whose products share a quantum scale: hi x hi, lo x hi, hi x lo."""
    if pw.mx is not None:
        C = pw.cin // 2
        return [(0, C), (C, 2 * C), (2 * C, 3 * C)]
    nseg = pw.split + pw.w_split - 1
    c = pw.cin // nseg
    return [(i * c, (i + 1) * c) for i in range(nseg)]


def mxfp8_values(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    lut = e4m3(codes)
    K = codes.shape[-1]
    return (lut.reshape(*codes.shape[:-1], K // 32, 32) * torch.exp2(scales.double() - 127)[..., None]).reshape(lut.shape)


def host_operand(x: torch.Tensor, form: str, dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """The documented operand forms of an fp32 tensor x [..., C], made on the host: "16" (one rounding to `dtype`), "split" ([hi | lo]),
    "mx" ([hi fp16 | e4m3((x - hi) 2^11) | e4m3(hi)], both clamped to +-448) and "mx6" ([hi fp16 | e2m3 blocks of x - hi | of hi])."""
    from omgsr_amd import ops
    if form == "16":
        return x.to(dtype)
    hi = x.to(torch.float16)
    lo = x - hi.float()
    if form == "split":
        return torch.cat([hi, lo.to(torch.float16)], -1)
    C = x.shape[-1]
    hib = hi.contiguous().view(torch.uint8).reshape(*x.shape[:-1], 2 * C)
    if form == "mx":
        f8 = lambda t: t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)      # noqa: E731
        parts = [hib, f8(lo * 2.0 ** ops.MX_LO_SHIFT), f8(hi.float())]
    else:
        parts = [hib, ops._e2m3_blocks(lo), ops._e2m3_blocks(hi.float())]
    return torch.cat(parts, -1).contiguous().view(torch.float16)


# ---- references --------------------------------------------------------------------------------------------------------------------

def _epilogue(acc: torch.Tensor, bud: Budget, bias, gate, residual, alpha: float, cout: int, check: bool = True) -> torch.Tensor:
    """acc [M, Cout_pad] float64 -> (acc alpha + bias) gate + residual over the logical columns (the kernels' order)."""
    assert alpha == 2.0 ** round(math.log2(alpha)), "alpha must be a power of two"
    acc, bud.tot, bud.unit = acc[:, :cout] * alpha, bud.tot[:, :cout] * alpha, bud.unit[:, :cout] * alpha
    if bias is not None:
        acc = acc + bias.double()[:cout]
        bud.term(bias[:cout])
    if gate is not None:
        acc = acc * gate.double()[:cout]
        bud.scale(gate[:cout])
    if residual is not None:
        r = residual.double().reshape(acc.shape)
        acc = acc + r
        bud.term(r)
    if check:
        bud.check()
    return acc


def conv_ref(a: torch.Tensor, pw, *, stride: int = 1, pad=(1, 1, 1, 1), upsample: bool = False, bias=None, gate=None, residual=None,
             alpha: float = 1.0, weights: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """Exact result of omgsr_igemm's gather form for the operand `a` [N, H, W, row channels] and the packed weight `pw`: float64
    [N, Ho, Wo, cout]. The budget is asserted on the way (check=False: a deliberately perturbed restatement, test_dyadic_probes_cpu.py).
    weights: decoded weights to use instead of pw's (same layout as weight_values)."""
    av = operand_values(a, pw)
    w = weight_values(pw) if weights is None else weights
    if upsample:
        av = av.repeat_interleave(2, 1).repeat_interleave(2, 2)
    N, Hv, Wv, K = av.shape
    pt, pb, pl, pr = pad
    Ho = (Hv + pt + pb - pw.R) // stride + 1
    Wo = (Wv + pl + pr - pw.S) // stride + 1
    ap = F.pad(av, (0, 0, pl, max(0, (Wo - 1) * stride + pw.S - Wv - pl), pt, max(0, (Ho - 1) * stride + pw.R - Hv - pt)))
    M = N * Ho * Wo
    acc = torch.zeros(M, w.shape[0], dtype=torch.float64, device=av.device)
    bud = Budget(M, w.shape[0], av.device)
    for r in range(pw.R):
        for s in range(pw.S):
            A = ap[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride, :].reshape(M, K)
            Wt = w[:, r * pw.S + s, :]
            acc += A @ Wt.T
            for k0, k1 in segments(pw):
                bud.add(A[:, k0:k1], Wt[:, k0:k1])
    return _epilogue(acc, bud, bias, gate, residual, alpha, pw.cout, check).reshape(N, Ho, Wo, pw.cout)


def phase_conv_ref(a: torch.Tensor, pw, *, bias=None) -> torch.Tensor:
    """Exact result of the phase-decomposed upsampling conv (weight_ph): output (2y + pa, 2x + pb) = sum over dy, dx of
    a[y - 1 + pa + dy, x - 1 + pb + dx] x w_ph[2 pa + pb][2 dy + dx]. float64 [N, 2H, 2W, cout]."""
    av = operand_values(a, pw)
    w = phase_weight_values(pw)
    N, H, W, K = av.shape
    ap = F.pad(av, (0, 0, 1, 1, 1, 1))
    M = N * H * W
    accs, buds = [], []
    for pa in (0, 1):
        for pb in (0, 1):
            acc = torch.zeros(M, w.shape[2], dtype=torch.float64, device=av.device)
            bud = Budget(M, w.shape[2], av.device)
            for dy in (0, 1):
                for dx in (0, 1):
                    A = ap[:, pa + dy:pa + dy + H, pb + dx:pb + dx + W, :].reshape(M, K)
                    Wt = w[2 * pa + pb, 2 * dy + dx]
                    acc += A @ Wt.T
                    for k0, k1 in segments(pw):
                        bud.add(A[:, k0:k1], Wt[:, k0:k1])
            accs.append(_epilogue(acc, bud, bias, None, None, 1.0, pw.cout).reshape(N, H, W, pw.cout))
    out = torch.stack(accs, 0).reshape(2, 2, N, H, W, pw.cout).permute(2, 3, 0, 4, 1, 5)
    return out.reshape(N, 2 * H, 2 * W, pw.cout)


def gemm_ref(A: torch.Tensor, W: torch.Tensor, *, alpha: float = 1.0, bias=None, gate=None, residual=None) -> torch.Tensor:
    """Exact A [M, K] x W [N, K]^T (16-bit operands, one segment) with the epilogue: float64 [M, N]."""
    A, W = A.double(), W.double()
    bud = Budget(A.shape[0], W.shape[0], A.device)
    bud.add(A, W)
    return _epilogue(A @ W.T, bud, bias, gate, residual, alpha, W.shape[0])


# v_mfma_scale_f32_32x32x64_f8f6f4 (measured on MI355X): the products of each 8-wide K group (k = 8g ... 8g + 7) are aligned to
# the group's largest one and a product 2^14 or more below it is dropped (2^13 below is kept). An exact probe keeps every group inside that window.
MFMA_F8_GROUP, MFMA_F8_WINDOW = 8, 2.0 ** 13


def mxfp8_ref(a_codes, a_scales, w_codes, w_scales, cout: int, *, bias=None, gate=None, residual=None, check: bool = True) -> torch.Tensor:
    """Exact MXFP8 x MXFP8 GEMM: float64 [M, cout]; the budget is kept per 32-wide K block (each block has its own scale pair), and every
    8-wide K group of every output must span less than MFMA_F8_WINDOW (largest / smallest nonzero |product|)."""
    A = mxfp8_values(a_codes, a_scales).reshape(-1, a_codes.shape[-1])
    W = mxfp8_values(w_codes, w_scales)
    acc = A @ W.T
    bud = Budget(A.shape[0], W.shape[0], A.device)
    for k0 in range(0, A.shape[1], 32):
        bud.add(A[:, k0:k0 + 32], W[:, k0:k0 + 32])
    if check:
        for k0 in range(0, A.shape[1], MFMA_F8_GROUP):
            p = (A[:, None, k0:k0 + MFMA_F8_GROUP] * W[None, :cout, k0:k0 + MFMA_F8_GROUP]).abs()
            lo = torch.where(p > 0, p, torch.full_like(p, float("inf"))).amin(-1)
            span = torch.where(torch.isfinite(lo), p.amax(-1) / lo, torch.ones_like(lo))
            assert float(span.max()) <= MFMA_F8_WINDOW, f"K group {k0 // MFMA_F8_GROUP} spans {float(span.max()):.3g} > 2^13: the instruction drops products"
    return _epilogue(acc, bud, bias, gate, residual, 1.0, cout, check)


def rounded(y: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The one documented output rounding: the exact value (fp32-representable by the budget) to `dtype`, round to nearest even."""
    y32 = y.float()
    assert torch.equal(y32.double(), y), "reference is not exact in fp32: the probe is over budget"
    return y32 if dtype == torch.float32 else y32.to(dtype)


def split_rounded(y: torch.Tensor, dtype: torch.dtype):
    """out_split 2: hi = round(y), lo = round(y - hi) (y - hi is exact in fp32)."""
    y32 = rounded(y, torch.float32)
    hi = y32.to(dtype)
    return hi, (y32 - hi.float()).to(dtype)


# ---- GroupNorm statistics (tests/test_gn_stats_probes_*.py) --------------------------------------------------------------------------
# Every producer keeps (sum, sum of squares) of the fp32 values it stores in fp32 partials - per lane, per wave, per 32-row block or per
# pixel chunk - and the finalisers fold the partials in double. When every value of an (image, group) is an integer multiple of one quantum q
# and the largest run of values one fp32 partial can cover (`slot_elems`) keeps sum |v| / q and sum v^2 / q^2 below 2^24, every partial sum is
# an exact integer times q (q^2) in ANY summation order, so the folded partials equal the float64 sums below bit for bit.

def stats_act(gen: torch.Generator, shape, img_e=(0, 1), mant=(1, 3)) -> torch.Tensor:
    """Activations [N, ..., C] = +-m 2^(e[n]): ONE exponent per image (consecutive images alternate inside img_e, so a value credited to the
    neighbouring image is off by a power of two) and none per channel, so the products of one output group share one quantum."""
    N = shape[0]
    e = img_e[0] + (torch.arange(N) + int(torch.randint(0, 2, (1,), generator=gen))) % (img_e[1] - img_e[0] + 1)
    return signed_ints(gen, tuple(shape), *mant) * torch.exp2(e.float()).reshape(N, *([1] * (len(shape) - 1)))


def group_exponents(gen: torch.Generator, groups: int, channels: int, span=(-2, 2)) -> torch.Tensor:
    """[channels] exponents, one integer per group of channels / groups consecutive channels and none per channel inside a group; neighbouring
    groups always differ (a channel credited to the group next door moves by a power of two, and one group keeps one quantum)."""
    n = span[1] - span[0] + 1
    assert n >= 2 and channels % groups == 0
    return (span[0] + torch.randint(1, n, (groups,), generator=gen).cumsum(0) % n).float().repeat_interleave(channels // groups)


def stats_wt(gen: torch.Generator, ce: torch.Tensor, cin: int, R: int = 3, S: int = 3, nnz: int = 2, mant=(1, 3), alt_sign: bool = False) -> torch.Tensor:
    """[Cout, Cin, R, S]: +-m 2^(ce[output channel]) at nnz (tap, channel) positions per output channel, zero elsewhere. alt_sign: the sign
    alternates with the output channel instead (for operands of one sign: the group's mean stays small against its spread)."""
    cout = ce.numel()
    v = signed_ints(gen, (cout, cin * R * S), *mant) * torch.exp2(ce)[:, None]
    if alt_sign:
        v = v.abs() * (1 - 2 * (torch.arange(cout) % 2).float())[:, None]
    return (v * sparse_mask(gen, cout, cin * R * S, nnz)).reshape(cout, cin, R, S)


def stats_bias(gen: torch.Generator, ce: torch.Tensor, img_e0: int = 0) -> torch.Tensor:
    """An odd multiple (+-1, +-3) of HALF the finest product quantum 2^(ce + img_e0) per channel: every output is then an odd multiple of
    q / 2 - never zero - so dropping or double-counting any single value changes the sum of squares."""
    n = ce.numel()
    return (torch.randint(0, 2, (n,), generator=gen).float() * 2 + 1) * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1) * torch.exp2(ce + img_e0 - 1)


def stats_residual(gen: torch.Generator, shape, ce: torch.Tensor, img_e0: int = 0) -> torch.Tensor:
    """A residual [N, ..., C] of +-{1..3} whole product quanta 2^(ce + img_e0)."""
    return signed_ints(gen, tuple(shape), 1, 3) * torch.exp2(ce + img_e0)


def stats_values(gen: torch.Generator, shape, ce: torch.Tensor, img_e=(0, 1)) -> torch.Tensor:
    """A tensor [N, P, C] for the statistics read pass: {1, 3} 2^(ce[channel] + e[image]) with the sign alternating over pixels and channels -
    nonzero odd multiples of one quantum per (image, group), and a mean that stays below the spread even in a group of five values."""
    N, P, C = shape
    e = img_e[0] + (torch.arange(N) + int(torch.randint(0, 2, (1,), generator=gen))) % (img_e[1] - img_e[0] + 1)
    odd = (torch.randint(0, 2, tuple(shape), generator=gen).float() * 2 + 1) * (1 - 2 * ((torch.arange(P)[:, None] + torch.arange(C)[None, :]) % 2).float())
    return odd * torch.exp2(ce) * torch.exp2(e.float()).reshape(N, 1, 1)


def group_sums(y: torch.Tensor, G: int):
    """y [N, ..., C] exact values -> (S, Q) float64 [N, G]: sum and sum of squares per (image, group of C / G consecutive channels)."""
    y = y.double()
    N, C = y.shape[0], y.shape[-1]
    v = y.reshape(N, -1, G, C // G)
    return v.sum((1, 3)), (v * v).sum((1, 3))


class StatsBudget:
    """Asserted before a statistics probe launches: per (image, group) every value is a nonzero multiple of one quantum q (the finest of the
    group), a normal fp32 value exactly representable in the stored type `dtype`, and the largest run of values one fp32 partial can cover
    stays exact: max |v| slot_elems < 2^24 q and max v^2 slot_elems < 2^24 q^2 (the fold over slots is in double: no budget there, beyond the
    2^53 the float64 reference itself needs)."""

    def __init__(self, y: torch.Tensor, G: int, slot_elems: int, dtype: torch.dtype):
        y = y.double()
        N, C = y.shape[0], y.shape[-1]
        assert C % G == 0
        v = y.reshape(N, -1, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1)
        self.nonzero = bool((v != 0).all())
        self.stored = torch.equal(y.to(dtype).double(), y)
        self.q = quantum(v).amin(-1)
        self.amax = v.abs().amax(-1)
        self.count = v.shape[-1]
        self.slot_elems = min(int(slot_elems), self.count)
        S, Q = v.sum(-1), (v * v).sum(-1)
        m = S / self.count
        self.m2, self.var = m * m, Q / self.count - m * m

    def check(self) -> float:
        assert self.nonzero, "a statistics probe must not hold an exactly-zero output: a dropped or doubled value could go unseen"
        assert self.stored, "the exact output is not representable in the stored type: what is stored and what is summed would differ"
        k = self.amax / self.q
        worst = float((k * k * self.slot_elems).max())
        assert worst < 2.0 ** 24 and float((k * self.slot_elems).max()) < 2.0 ** 24, \
            f"statistics probe over its bit budget: max v^2 x slot = {worst:.3g} q^2 >= 2^24 (mixed quanta in a group, or too many bits)"
        assert float((k * k * self.count).max()) < 2.0 ** 53, "the float64 reference would not be exact"
        assert float(self.q.min()) ** 2 >= MIN_NORMAL and float(self.amax.max()) ** 2 * self.slot_elems < 2.0 ** 100, "values outside the normal fp32 range"
        assert bool((self.m2 <= self.var).all()), "mean^2 > variance: the subtraction q / count - m^2 would amplify a last-bit difference"
        return worst


def finalize_ref(S: torch.Tensor, Q: torch.Tensor, count: float, eps: float):
    """float64 restatement of gn_finalize_kernel: (mean, var, rstd) from the folded sums; eps enters as the fp32 value the kernel is handed."""
    m = S.double() / float(count)
    v = (Q.double() / float(count) - m * m).clamp(min=0.0)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    return m, v, 1.0 / torch.sqrt(v + eps32)


def merged_ref(parts, eps: float):
    """float64 restatement of omgsr_groupnorm_finalize_merged (include/omgsr_hip.h): parts = [(S [T, N, G], Q, count, weight)] per tile-shape
    group; mean = sum over (group, tile) of weight m, var = sum of weight max(q / count - m^2, 0), weight as the fp32 value the library holds."""
    mm = vv = 0.0
    for S, Q, count, weight in parts:
        w32 = float(torch.tensor(weight, dtype=torch.float32))
        m, v, _ = finalize_ref(S, Q, count, eps)
        mm = mm + (w32 * m).sum(0)
        vv = vv + (w32 * v).sum(0)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    return mm, vv, 1.0 / torch.sqrt(vv + eps32)


def fold_partials(partial: torch.Tensor, G: int):
    """A producer's raw partials [N, nslot, entries, 2] -> (S, Q) float64 [N, G]: over the slots, and over the entries / G entries of a group."""
    p = partial.double()
    N, _, entries, _ = p.shape
    assert entries % G == 0, f"{entries} entries do not fold into {G} groups"
    f = p.sum(1).reshape(N, G, entries // G, 2).sum(2)
    return f[..., 0], f[..., 1]


def halo_partials_ref(y: torch.Tensor, G: int, per_channel: bool) -> torch.Tensor:
    """What the halo-tile kernel's spatial form leaves for an exact output y [N, H, W, C] (igemm_halo_body.hip.h): float32
    [N, 2 ceil(H / 8) ceil(W / 32), entries, 2], slot = (tile row-major, upper / lower four tile rows), entries = G or C. Pixels outside the
    map add nothing. (The emulated partials of tests/test_gn_stats_probes_cpu.py's negative controls.)"""
    N, H, W, C = y.shape
    ty, tx = (H + 7) // 8, (W + 31) // 32
    v = F.pad(y.double(), (0, 0, 0, tx * 32 - W, 0, ty * 8 - H)).reshape(N, ty, 2, 4, tx, 32, C)
    s = torch.stack([v.sum((3, 5)), (v * v).sum((3, 5))], -1)                # [N, ty, wm, tx, C, 2]
    s = s.permute(0, 1, 3, 2, 4, 5).reshape(N, ty * tx * 2, C, 2)
    if not per_channel:
        s = s.reshape(N, ty * tx * 2, G, C // G, 2).sum(3)
    return s.float()


def ulps32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in fp32 steps between two fp32 tensors of finite values."""
    def ordered(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (ordered(a) - ordered(b)).abs()


# ---- the dispatcher's variant ids ----------------------------------------------------------------------------------------------------

def variant_ids(source: str) -> set:
    """Every id a `ts.rec.variant = ...` assignment in igemm.hip can record: integer literals, both arms of ternaries included."""
    ids = set()
    for rhs in re.findall(r"ts\.rec\.variant\s*=\s*([^;]+);", source):
        rhs = re.sub(r"//.*", "", rhs)
        rhs = re.sub(r"\b\w+\s*(==|!=|>=|<=|>|<)\s*\w+", "", rhs)        # drop the comparisons of the conditions
        ids.update(int(v) for v in re.findall(r"(?<![\w.])(\d+)(?![\w.])", rhs))
    return ids


def variant_of_probe(name: str) -> int:
    return int(name.split("_", 1)[0][1:])


def probe_names(source: str) -> Sequence[str]:
    """Names of the probes a test file declares in its PROBES table (`"v<id>_<what>"` strings)."""
    return re.findall(r'^\s*"(v\d+_\w+)"\s*:', source, flags=re.M)
