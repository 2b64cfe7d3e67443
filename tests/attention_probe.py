"""Bit-exact probes for the head_dim 64 / 128 attention kernel, attn_kernel<T, D, DMA, SPLIT> in omgsr_amd/csrc/attention.hip (not a test module:
imported by tests/test_attention_probes_*.py). Everything here runs on any device.

The construction, called with scale = 1:
  q     row i of image b is 16 e_c, c = (a (i + 37 b) + b0) mod D                          (one-hot: a score is one k element times 16)
  k     k[bk, j, h D + c] = 0 if ((j + m c + 11 h + 5 bk) mod Lk) < n_live else -16        (score 0 = live, -256 = dead)
  V     V[bk, j, h D + d] = (integer in -7 .. 7) 2^e(d), e(d) = (d mod 5) - 2, the rows of a head pairwise distinct
In the kernel's base-2 domain a dead key sits at 2^-369 of a live one: its probability is an exact 0 in fp32 (and so in bf16 / fp16), the live
ones are exact 1s, l = n_live is a power of two, the PV sums are small integers times 2^e(d), and O = (sum of the live V rows) / n_live is
exactly representable in bf16 and fp16: a correct kernel matches it with torch.equal, and with n_live = 1 a wrong result names the key read.
The live set of column c is the cyclic window of n_live keys that starts at (-m c - 11 h - 5 bk) mod Lk.

`pick` chooses (m, a, b0) per configuration and `preconditions` asserts what makes the probe trustworthy (tests/test_attention_probes_cpu.py
runs it for every configuration; the GPU probes for the one they launch). `emulate` restates the kernel's tile loop - 64-key tiles, the
deferred running maximum, the per-wave `__any` rescale, the split passes - in fp32 on the host, with switches for deliberate defects.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

Q_VAL, DEAD = 16.0, -16.0
DEAD_SCORE = Q_VAL * DEAD                  # -256
LOG2E = 1.4426950408889634
TILE, WAVE = 64, 32
LQ = 150                                   # 2 workgroups of 128 queries: four full waves, one of 22 rows, three idle


@dataclass(frozen=True)
class Case:
    D: int
    Lk: int
    n_live: int
    H: int = 2
    B: int = 1
    Bk: int = 1
    Lq: int = LQ

    @property
    def dma(self) -> bool:
        """The LDS-DMA instantiation (omgsr_attention: Lk % 64 == 0); otherwise the register-staged one."""
        return self.Lk % TILE == 0

    @property
    def inner(self) -> int:
        return self.H * self.D

    @property
    def ld(self) -> int:
        return (self.Lk + 7) // 8 * 8

    @property
    def prefix_attainable(self) -> bool:
        """Can a row have no live key among the first 64? Its window of n_live consecutive keys must fit into [64, Lk)."""
        return self.Lk - TILE >= self.n_live

    @property
    def id(self) -> str:
        tail = "" if (self.H, self.B, self.Bk) == (2, 1, 1) else f"-H{self.H}B{self.B}Bk{self.Bk}"
        return f"D{self.D}-Lk{self.Lk}-{'dma' if self.dma else 'reg'}-live{self.n_live}{tail}"


DMA_LK, REG_LK, N_LIVE = (64, 128, 320), (40, 77, 100, 136), (1, 16, 32)
KEY_CASES = [Case(D, Lk, n) for D in (64, 128) for Lk in DMA_LK + REG_LK for n in N_LIVE]
ADDRESS_CASES = [Case(D, Lk, 16, H=3, B=2, Bk=Bk) for D in (64, 128) for Lk in (128, 77) for Bk in (1, 2)]
SPLIT_CASES = [Case(64, Lk, n, H=2) for Lk in (128, 100) for n in (1, 16)]
LOLO_CASES = [Case(64, Lk, 1) for Lk in (32, 64, 128)]            # information in q_lo and k_lo only: the mean over ALL keys, exact in fp32
ALL_CASES = list(dict.fromkeys(KEY_CASES + ADDRESS_CASES + SPLIT_CASES + LOLO_CASES))


# ---- the index maps --------------------------------------------------------------------------------------------------------------------

def q_column(case: Case, a: int, b0: int) -> torch.Tensor:
    """c(b, i): int64 [B, Lq]."""
    i = torch.arange(case.Lq)[None, :] + 37 * torch.arange(case.B)[:, None]
    return (a * i + b0) % case.D


def window_start(case: Case, m: int) -> torch.Tensor:
    """First key of the live window of (bk, h, c): int64 [Bk, H, D]."""
    bk, h, c = torch.arange(case.Bk)[:, None, None], torch.arange(case.H)[None, :, None], torch.arange(case.D)[None, None, :]
    return (-(m * c + 11 * h + 5 * bk)) % case.Lk


def live_mask(case: Case, m: int) -> torch.Tensor:
    """bool [Bk, H, D, Lk]: key j is live for column c of head h."""
    j = torch.arange(case.Lk)
    return ((j - window_start(case, m)[..., None]) % case.Lk) < case.n_live


def row_start(case: Case, m: int, a: int, b0: int) -> torch.Tensor:
    """First live key of query (b, h, i): int64 [B, H, Lq]."""
    st = window_start(case, m)
    st = st if case.Bk == case.B else st.expand(case.B, -1, -1)
    return torch.gather(st, 2, q_column(case, a, b0)[:, None, :].expand(-1, case.H, -1))


def dead_prefix_rows(case: Case, m: int, a: int, b0: int) -> torch.Tensor:
    """bool [B, H, Lq]: no live key among the first 64 (the window does not wrap and starts at 64 or later)."""
    st = row_start(case, m, a, b0)
    return (st >= TILE) & (st + case.n_live <= case.Lk)


def _waves(x: torch.Tensor) -> list:
    """[..., Lq] -> the slices a wave owns: 32 consecutive rows of a 128-row workgroup (the last one may be short)."""
    return [x[..., r:r + WAVE] for r in range(0, x.shape[-1], WAVE)]


def _admissible(case: Case, m: int, a: int, b0: int) -> bool:
    if math.gcd(m, case.Lk) != 1 or math.gcd(a, case.D) != 1:
        return False
    if case.Lk > TILE and case.prefix_attainable:
        dp = dead_prefix_rows(case, m, a, b0)
        if not all(bool(w.any(-1).all()) and bool((~w).any(-1).all()) for w in _waves(dp)):
            return False
    if not case.dma:                       # some query's window holds the last key of the ragged tile
        st = row_start(case, m, a, b0)
        if not bool((((case.Lk - 1 - st) % case.Lk) < case.n_live).any()):
            return False
    return True


@functools.lru_cache(maxsize=None)
def pick(case: Case) -> tuple:
    """(m, a, b0): the first choice, in a fixed order that starts at the plain m = 7, c(i) = 5 i + 3, that meets `preconditions`."""
    for a, b0 in ((5, 3), (3, 1), (7, 5), (9, 2), (11, 7), (13, 0), (15, 4), (17, 6), (19, 9), (21, 10), (23, 11), (25, 12)):
        for m in [7] + [x for x in range(3, case.Lk) if x != 7]:
            if _admissible(case, m, a, b0):
                return m, a, b0
    raise AssertionError(f"{case.id}: no (m, a, b0) meets the probe's preconditions")


# ---- operands --------------------------------------------------------------------------------------------------------------------------

@dataclass
class Operands:
    case: Case
    m: int
    a: int
    b0: int
    q: torch.Tensor                        # [B, Lq, inner] float32
    k: torch.Tensor                        # [Bk, Lk, inner]
    v: torch.Tensor                        # [Bk, Lk, inner]

    def vt(self, dtype: torch.dtype, poison: bool = True) -> torch.Tensor:
        """V^T [Bk, inner, ld], ld = Lk rounded up to 8; the pad columns hold 0xFF bytes (NaN) unless poison=False (zeros)."""
        return transposed(self.v, self.case.ld, dtype, poison)


def transposed(v: torch.Tensor, ld: int, dtype: torch.dtype, poison: bool = True) -> torch.Tensor:
    from guard_bands import poison_tail
    Lk = v.shape[1]
    vt = torch.zeros(v.shape[0], v.shape[2], ld, dtype=dtype)
    vt[:, :, :Lk] = v.transpose(1, 2).to(dtype)
    return poison_tail(vt, 2, Lk) if poison else vt


def values(gen: torch.Generator, Bk: int, Lk: int, H: int, D: int) -> torch.Tensor:
    """V [Bk, Lk, H D]: (integer in -7 .. 7) 2^e(d), the Lk rows of every (image, head) pairwise distinct."""
    e = (torch.arange(D) % 5 - 2).float()
    v = torch.randint(-7, 8, (Bk, Lk, H, D), generator=gen).float() * torch.exp2(e)
    return v.reshape(Bk, Lk, H * D)


def build(case: Case, seed: int = 0) -> Operands:
    m, a, b0 = pick(case)
    c = q_column(case, a, b0)
    q = torch.zeros(case.B, case.Lq, case.H, case.D)
    q.scatter_(3, c[:, :, None, None].expand(-1, -1, case.H, 1), Q_VAL)
    k = torch.where(live_mask(case, m), 0.0, DEAD).permute(0, 3, 1, 2)                      # [Bk, Lk, H, D]
    v = values(torch.Generator().manual_seed(1000 + seed), case.Bk, case.Lk, case.H, case.D)
    return Operands(case, m, a, b0, q.reshape(case.B, case.Lq, case.inner), k.reshape(case.Bk, case.Lk, case.inner).contiguous(), v)


def expected(ops_: Operands) -> torch.Tensor:
    """The exact result, float64 [B, Lq, inner]: the mean of the live V rows of each query, straight from the index maps."""
    case = ops_.case
    live = live_mask(case, ops_.m)                                                            # [Bk, H, D, Lk]
    live = live if case.Bk == case.B else live.expand(case.B, -1, -1, -1)
    c = q_column(case, ops_.a, ops_.b0)                                                       # [B, Lq]
    rows = torch.gather(live, 2, c[:, None, :, None].expand(-1, case.H, -1, case.Lk)).double()      # [B, H, Lq, Lk]
    vh = ops_.v.double().reshape(case.Bk, case.Lk, case.H, case.D).permute(0, 2, 1, 3).expand(case.B, -1, -1, -1)
    return (rows @ vh / case.n_live).permute(0, 2, 1, 3).reshape(case.B, case.Lq, case.inner)


def softmax_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, H: int, scale: float = 1.0) -> torch.Tensor:
    """Plain float64 softmax attention: q [B, Lq, H D], k / v [Bk, Lk, H D] (Bk = 1 broadcasts) -> [B, Lq, H D]."""
    B, Lq, inner = q.shape
    D = inner // H
    qh = q.double().reshape(B, Lq, H, D).transpose(1, 2)
    kh = k.double().reshape(k.shape[0], -1, H, D).transpose(1, 2).expand(B, -1, -1, -1)
    vh = v.double().reshape(v.shape[0], -1, H, D).transpose(1, 2).expand(B, -1, -1, -1)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    return (p @ vh).transpose(1, 2).reshape(B, Lq, inner)


SPLIT_FORMS = ("k_lo", "q_lo", "lo_lo")


def split_form(ops_: Operands, form: str):
    """(q_hi, q_lo, k_hi, k_lo) for the SPLIT kernel's three score passes K_lo Q_hi + K_hi Q_lo + K_hi Q_hi:
    "k_lo"   the -16 pattern only in k_lo (k_hi = 0), the one-hot in q_hi: only the first pass carries the scores
    "q_lo"   the one-hot only in q_lo (q_hi = 0), the pattern in k_hi: only the second
    "lo_lo"  both only in the low halves: there is no lo x lo pass, every score is 0 and O is the mean over all keys."""
    zq, zk = torch.zeros_like(ops_.q), torch.zeros_like(ops_.k)
    return {"k_lo": (ops_.q, zq, zk, ops_.k), "q_lo": (zq, ops_.q, ops_.k, zk), "lo_lo": (zq, ops_.q, zk, ops_.k)}[form]


def mean_of_all_keys(ops_: Operands) -> torch.Tensor:
    """float64 [B, Lq, inner]: what uniform probabilities give."""
    return ops_.v.double().mean(1, keepdim=True).expand(ops_.case.B, ops_.case.Lq, -1).contiguous()


def split_rounded(y: torch.Tensor, dtype: torch.dtype):
    """out_split 2: hi = round(y), lo = round(y - hi), from a float64 value that fp32 holds exactly."""
    y32 = y.float()
    assert torch.equal(y32.double(), y), "reference is not exact in fp32"
    hi = y32.to(dtype)
    return hi, (y32 - hi.float()).to(dtype)


# ---- preconditions ---------------------------------------------------------------------------------------------------------------------

def preconditions(ops_: Operands) -> torch.Tensor:
    """Assert what makes a probe exact and able to see a wrong map; returns the expected result (float64).

    The live sets of the D columns of a head are pairwise distinct when D <= Lk. A head has only Lk windows of n_live consecutive keys
    (Lk singletons with n_live = 1), so with Lk < D that is out of reach for any construction; there every run of Lk consecutive columns
    is pairwise distinct, i.e. all Lk windows are in use and two columns share one only when they differ by a multiple of Lk."""
    case, m = ops_.case, ops_.m
    B, H, D, Lk, Lq = case.B, case.H, case.D, case.Lk, case.Lq
    assert case.n_live & (case.n_live - 1) == 0 and 0 < case.n_live < Lk, "n_live must be a power of two below Lk"
    assert math.gcd(m, Lk) == 1 and math.gcd(ops_.a, D) == 1
    s = torch.einsum("bqhd,bkhd->bhqk", ops_.q.double().reshape(B, Lq, H, D), ops_.k.double().reshape(case.Bk, Lk, H, D).expand(B, -1, -1, -1))
    assert bool(((s == 0) | (s == DEAD_SCORE)).all()), "scores other than 0 and -256"
    assert bool(((s == 0).sum(-1) == case.n_live).all()), "a query row without exactly n_live live keys"
    assert DEAD_SCORE * LOG2E < -150, "a dead key's probability is not an exact fp32 zero (the smallest subnormal is 2^-149)"
    st = window_start(case, m)
    for run0 in range(0, max(1, D - Lk + 1)):
        run = st[..., run0:run0 + min(D, Lk)]
        assert bool((run.sort(-1).values.diff(dim=-1) != 0).all()), "two columns of a head share a live set"
    vh = ops_.v.reshape(case.Bk, Lk, H, D).permute(0, 2, 1, 3).reshape(case.Bk * H, Lk, D)
    same = (vh[:, :, None, :] == vh[:, None, :, :]).all(-1)
    assert int(same.sum()) == case.Bk * H * Lk, "two V rows of a head are equal"
    want = expected(ops_)
    ref = softmax_ref(ops_.q, ops_.k, ops_.v, H)
    assert torch.equal(ref.float().double(), want), "float64 softmax attention differs from the mean of the live rows"
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(want.to(dt).double(), want), f"the exact result does not survive {dt}"
        for t in (ops_.q, ops_.k, ops_.v):
            assert torch.equal(t.to(dt).float(), t), f"an operand is not exact in {dt}"
    if Lk > TILE and case.prefix_attainable:
        dp = dead_prefix_rows(case, m, ops_.a, ops_.b0)
        assert torch.equal(dp, ~(s[..., :TILE] == 0).any(-1)), "dead_prefix_rows disagrees with the scores"
        for w in _waves(dp):
            assert bool(w.any(-1).all()) and bool((~w).any(-1).all()), "a wave without both a dead-prefix row and a live-prefix row"
    elif Lk > TILE:
        assert not bool((s[..., :TILE] == 0).any(-1).logical_not().any())                    # (cannot happen: the window does not fit)
    if not case.dma:
        assert bool((s[..., Lk - 1] == 0).any()), "no query has the last ragged key live"
    return want


# ---- host emulation of the kernel's tile loop --------------------------------------------------------------------------------------------

def emulate(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, H: int, dtype: torch.dtype, *, scale: float = 1.0, defer: float = 8.0,
            q_lo: Optional[torch.Tensor] = None, k_lo: Optional[torch.Tensor] = None, v_lo: Optional[torch.Tensor] = None, p_split: bool = False,
            skip_prefix_rescale: bool = False, k_lo_reads_hi: bool = False, k_hi_reads_lo: bool = False, q_lo_reads_hi: bool = False,
            v_lo_reads_hi: bool = False, v_hi_reads_lo: bool = False, drop_p_lo: bool = False, l_misses_rescale: bool = False) -> torch.Tensor:
    """attn_kernel's arithmetic in fp32 on the host: [B, Lq, H D] float32, before the output rounding. 64-key tiles; S = K_lo Q_hi + K_hi Q_lo +
    K_hi Q_hi; the running maximum moves, and O / l are rescaled, for a whole wave of 32 rows when one of them saw (m_new - m_run) sc > defer;
    P is rounded to `dtype` (P_lo = round(p - P_hi) with p_split); O += V P_lo + V_lo P_hi + V P_hi; O / l.
    Defects: skip_prefix_rescale (a row that had only seen smaller scores keeps its accumulated O and l when the maximum jumps so far that
    alpha is 0), x_lo_reads_hi / x_hi_reads_lo (one tile or fragment of a two-term split read through the other's offset), drop_p_lo,
    l_misses_rescale (alpha applied to O but not to l)."""
    B, Lq, inner = q.shape
    D, Lk = inner // H, k.shape[1]
    sc = scale * LOG2E
    pad = (-Lq) % WAVE
    heads = lambda t: None if t is None else t.float().reshape(t.shape[0], t.shape[1], H, D).permute(0, 2, 1, 3).expand(B, -1, -1, -1)    # noqa: E731
    rows = lambda t: None if t is None else torch.cat([t, t[:, :, -1:].expand(-1, -1, pad, -1)], 2)                                      # noqa: E731
    qh, ql, kh, kl, vh, vl = rows(heads(q)), rows(heads(q_lo)), heads(k), heads(k_lo), heads(v), heads(v_lo)
    ql = qh if (q_lo_reads_hi and ql is not None) else ql
    kh, kl = (kl if (k_hi_reads_lo and kl is not None) else kh), (kh if (k_lo_reads_hi and kl is not None) else kl)
    vh, vl = (vl if (v_hi_reads_lo and vl is not None) else vh), (vh if (v_lo_reads_hi and vl is not None) else vl)
    R = Lq + pad
    m_run = torch.full((B, H, R), float("-inf"))
    l_run = torch.zeros(B, H, R)
    o = torch.zeros(B, H, R, D)
    for t0 in range(0, Lk, TILE):
        t1 = min(t0 + TILE, Lk)
        s = torch.zeros(B, H, R, t1 - t0)
        if kl is not None:
            s = s + qh @ kl[:, :, t0:t1].transpose(-1, -2)
            s = s + ql @ kh[:, :, t0:t1].transpose(-1, -2)
        s = s + qh @ kh[:, :, t0:t1].transpose(-1, -2)
        m_new = torch.maximum(m_run, s.amax(-1))
        grow = torch.where(torch.isinf(m_run), torch.full_like(m_run, float("inf")), (m_new - m_run) * sc)
        move = (grow > defer).reshape(B, H, R // WAVE, WAVE).any(-1, keepdim=True).expand(-1, -1, -1, WAVE).reshape(B, H, R)
        alpha = torch.where(torch.isinf(m_run), torch.zeros_like(m_run), torch.exp2((m_run - m_new) * sc))
        if skip_prefix_rescale:
            alpha = torch.where(torch.isfinite(m_run) & (alpha == 0), torch.ones_like(alpha), alpha)
        alpha = torch.where(move, alpha, torch.ones_like(alpha))
        l_run, o = (l_run if l_misses_rescale else l_run * alpha), o * alpha[..., None]
        m_run = torch.where(move, m_new, m_run)
        p = torch.exp2(s * sc - (m_run * sc)[..., None])
        l_run = l_run + p.sum(-1)
        p_hi = p.to(dtype).float()
        if p_split and not drop_p_lo:
            o = o + (p - p_hi).to(dtype).float() @ vh[:, :, t0:t1]
        if vl is not None:
            o = o + p_hi @ vl[:, :, t0:t1]
        o = o + p_hi @ vh[:, :, t0:t1]
    out = o / l_run[..., None]
    return out[:, :, :Lq].permute(0, 2, 1, 3).reshape(B, Lq, inner)


# ---- the P_lo tolerance probe ------------------------------------------------------------------------------------------------------------

# Non-trivial probabilities cannot be exact, so the P_lo lane map gets the bound of test_lane_map_p_lo_identity_v (the 512-wide kernel's twin of
# this probe): 2^-13 relative on EVERY element. What a correct kernel leaves: p_hi + p_lo and o_hi + o_lo carry 16 (bf16) / 22 (fp16) significant
# bits, 2^-16 each at worst; the scores miss the q_lo k_lo products, at most 2^-16 of sum |q_i k_i| D^-1/2 (about 1.3 for these draws) - an
# absolute 2e-5 on an exponent; v_exp_f32 and the fp32 sums add a few 2^-23. Together under 2^-14, half the bound. A dropped or misplaced P_lo
# leaves P with a single rounding: up to 2^-8 (bf16) / 2^-11 (fp16) on an element, 31 / 4 times the bound.
# q and k are 0.5 N(0, 1): scores spread by +-1.5, every probability within 2^-5 of the row's largest and above 2^-12 after the division
# by l <= 64 - clear of fp16's subnormals (2^-14), where a low half would lose bits for reasons that have nothing to do with the lane map.
P_LO_BOUND = 2.0 ** -13


def p_lo_operands(Lk: int, dtype: torch.dtype, seed: int = 0):
    """(q [1, LQ, 128], k [1, Lk, 128], V^T [1, 64, ld]): q and k as [hi | lo] two-term splits of one head of 64 channels; V^T = the identity
    over the Lk <= 64 keys (pad columns poisoned), so O[i, d] is the probability of key d."""
    from guard_bands import poison_tail
    D = 64
    assert Lk <= D
    g = torch.Generator().manual_seed(2000 + seed)
    sp = lambda t: torch.cat([t.to(dtype), (t - t.to(dtype).float()).to(dtype)], -1)          # noqa: E731
    q, k = 0.5 * torch.randn(1, LQ, D, generator=g), 0.5 * torch.randn(1, Lk, D, generator=g)
    ld = (Lk + 7) // 8 * 8
    vt = torch.zeros(1, D, ld, dtype=dtype)
    vt[0, :Lk, :Lk] = torch.eye(Lk)
    return sp(q), sp(k), poison_tail(vt, 2, Lk)


def p_lo_reference(qq: torch.Tensor, kk: torch.Tensor, Lk: int) -> torch.Tensor:
    """float64 softmax rows [1, LQ, Lk] of the hi + lo operands."""
    D = 64
    q, k = qq[..., :D].double() + qq[..., D:].double(), kk[..., :D].double() + kk[..., D:].double()
    return torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1)


# ---- the normalisation property --------------------------------------------------------------------------------------------------------

# V constant per channel: softmax weights sum to one, so o = c_d whatever the scores. The kernel rounds P per element to the compute type for
# the PV product while l sums the unrounded values, and rounds the output once: |o / c - 1| <= u_P + u_out + fp32 noise. c_d has three
# significant bits, so p c is exact in the fp32 accumulator; the noise term is the fp32 sums over Lk keys and P's below-normal tail in fp16,
# a few 2^-20 together. The asserted bounds are 2^-8 x 1.01 (bf16) and 2^-10 x 1.01 (fp16). For fp16 (11 significant bits, u = 2^-11) that is
# u_P + u_out plus 1 %. For bf16 (8 significant bits, u = 2^-8) the worst case of the two roundings is 2^-7, so 2^-8 x 1.01 is the stricter
# statement that at most ONE of them shows. It is not a worst-case bound there: it rests on a row's error being the p-weighted MEAN of the signed
# per-key rounding errors, far below u_P over hundreds of keys, after which o rounds back to c itself (observed: exactly 0 everywhere). A row
# that one key dominates through a DEFERRED maximum carries that key's weight as a rounded exp2(delta); if the bf16 figure is ever missed by
# less than a factor of two, look for such a row before looking for a kernel defect.
NORM_BOUND = {torch.bfloat16: 2.0 ** -8 * 1.01, torch.float16: 2.0 ** -10 * 1.01}
NORM_LQ = 512


def norm_operands(D: int, Lk: int):
    """(q [1, 512, D], k [1, Lk, D], c [D]) float32, bf16-representable: N(0, 1) draws with the spiked keys of test_attention_spiked_max - two
    that force a rescale above the deferred threshold (2^8 in the scaled base-2 domain) late in the sweep, one late maximum below it (p > 1,
    no rescale) - and the per-channel constant c_d = +-(1 .. 7) 2^e."""
    g = torch.Generator().manual_seed(29)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).float()                   # noqa: E731
    q, k = rnd(1, NORM_LQ, D), rnd(1, Lk, D)
    k[0, 300] = q[0, 5] * 4.0
    k[0, Lk - 12] = q[0, 70] * 6.0
    k[0, 400] = q[0, 9] * 0.6 * (64 / D) ** 0.5
    d = torch.arange(D)
    c = (1 + d % 7).float() * torch.exp2((d % 5 - 2).float()) * (1 - 2 * (d % 2)).float()
    return q, k.to(torch.bfloat16).float(), c
