"""Bit-exact lane-map probes for attn_kernel<T, D, DMA, SPLIT> (omgsr_amd/csrc/attention.hip: head_dim 64 and 128, every UNet self- and
cross-attention and FLUX joint attention in the 16-bit tiers). The construction and its preconditions are in tests/attention_probe.py, the
host-side proof that the probes see what they are for in tests/test_attention_probes_cpu.py. One-hot queries against a 0 / -16 key pattern
give scores of exactly 0 or -256 at scale 1: dead keys have probability 0, live ones 1, l is a power of two and V is dyadic, so the
result equals the mean of the live V rows bit for bit, whatever the tile order, the deferred maximum or the MFMA's internal grouping.

Which instantiation a case reaches follows from Lk % 64 alone (omgsr_attention): "dma" in a test id = LDS-DMA staging (attn_kernel<T, D, true, *>),
"reg" = register staging with the masked last tile (attn_kernel<T, D, false, *>). The DMA-named cases skip when OMGSR_ATTN_VARIANT=0 forces
the register-staged form everywhere."""
import functools
import os

import pytest
import torch

import attention_probe as ap

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.0


def _ops():
    from omgsr_amd import ops
    return ops


@pytest.fixture(autouse=True, params=["bf16", "fp16"])
def compute_dtype(request):
    """Every probe runs in both 16-bit modes; the data are exact in both. Yields the operand dtype."""
    ops = _ops()
    dt = torch.bfloat16 if request.param == "bf16" else torch.float16
    ops.set_compute_dtype(dt)
    yield dt
    ops.set_compute_dtype(torch.bfloat16)


def _cases(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


def _needs_dma(dma: bool):
    if dma and os.environ.get("OMGSR_ATTN_VARIANT", "").startswith("0"):
        pytest.skip("OMGSR_ATTN_VARIANT=0: the LDS-DMA instantiation is not reachable")


@functools.lru_cache(maxsize=None)
def _built(case):
    """(operands, exact result), built and checked once per configuration and never modified."""
    ops_ = ap.build(case)
    return ops_, ap.preconditions(ops_)


@functools.lru_cache(maxsize=None)
def _plain(case, dt):
    """The kernel's output for the plain call on a configuration (fast tier of type dt, set by the fixture): [B, Lq, inner] on the host."""
    ops_, _ = _built(case)
    o = _ops().attention(ops_.q.to(dt).to(DEV), ops_.k.to(dt).to(DEV), ops_.vt(dt).to(DEV), case.H, case.D, 1.0, Lk=case.Lk)
    assert o.dtype == dt and tuple(o.shape) == (case.B, case.Lq, case.inner)
    return o.cpu()


def _explain(got, want, ops_) -> str:
    """Name the first wrong query and, where the row it holds is a V row of its head (n_live = 1), the key that was read."""
    case = ops_.case
    g, w = got.double().reshape(case.B, case.Lq, case.H, case.D), want.reshape(case.B, case.Lq, case.H, case.D)
    bad = (g != w).any(-1).nonzero()
    if not len(bad):
        return "equal"
    b, i, h = (int(x) for x in bad[0])
    vh = ops_.v.double().reshape(case.Bk, case.Lk, case.H, case.D)
    hits = [(bk, j, hh) for bk in range(case.Bk) for hh in range(case.H) for j in range(case.Lk) if torch.equal(vh[bk, j, hh], g[b, i, h])]
    st = int(ap.row_start(case, ops_.m, ops_.a, ops_.b0)[b, h, i])
    return (f"{len(bad)} of {case.B * case.Lq * case.H} (image, query, head) rows differ; first: image {b} query {i} head {h}, whose live keys are "
            f"{st} .. +{case.n_live} (mod {case.Lk}); it holds the V row of (image, key, head) {hits or 'none'}; got {g[b, i, h, :6].tolist()} "
            f"want {w[b, i, h, :6].tolist()}")


def _assert_exact(got, want, ops_, dt):
    assert torch.isfinite(got.float()).all(), "non-finite output (a poisoned pad column or row reached the result)"
    assert torch.equal(got.cpu(), want.to(dt)), _explain(got.cpu(), want, ops_)


# ---- 1, 2: the key map and the PV sum map ------------------------------------------------------------------------------------------------------

@_cases([c for c in ap.KEY_CASES if c.n_live == 1])
def test_key_map(case, compute_dtype):
    """One live key per query: O[b, i, h D + d] is that key's V row, bit for bit - through the transposed S / O, the contraction-slot permutation
    of the PV product and, for "dma" ids, the bit-2 / bit-3 K row swap and the XOR-swizzled 16-byte slots (attn_kernel<T, D, true, false>); for
    "reg" ids the ragged last tile with both masks, V^T pad columns poisoned (attn_kernel<T, D, false, false>). The V rows of a head are
    pairwise distinct, so a failure names the key that was read."""
    _needs_dma(case.dma)
    ops_, want = _built(case)
    _assert_exact(_plain(case, compute_dtype), want, ops_, compute_dtype)


@_cases([c for c in ap.KEY_CASES if c.n_live > 1])
def test_pv_sum_map(case, compute_dtype):
    """16 / 32 live keys per query, as a cyclic window that crosses lane halves, 8-key fragments, 32-key blocks and tiles: O is the exact average.
    "dma" ids: attn_kernel<T, D, true, false>; "reg" ids: attn_kernel<T, D, false, false>."""
    _needs_dma(case.dma)
    ops_, want = _built(case)
    _assert_exact(_plain(case, compute_dtype), want, ops_, compute_dtype)


# ---- 3: the rescale from a dead-only prefix ----------------------------------------------------------------------------------------------------

@_cases([c for c in ap.KEY_CASES if c.Lk > 64 and c.prefix_attainable])
def test_rescale_from_dead_only_prefix(case, compute_dtype):
    """The data of probes 1 and 2 at Lk > 64. A row without a live key in the first tile starts with m = -256 and p = 1 on 64 dead keys; when
    its first live key arrives, alpha = exp2(-369) = 0 must wipe that sum and that l. Every wave holds such rows next to rows that found a
    live key at once (alpha = 1 under the same wave-wide `__any`). Both instantiations, by id. The two row classes are asserted apart, and a
    result that equals the emulation with the rescale skipped is named as that."""
    _needs_dma(case.dma)
    ops_, want = _built(case)
    dt = compute_dtype
    got = _plain(case, dt).double().reshape(case.B, case.Lq, case.H, case.D)
    w = want.reshape(case.B, case.Lq, case.H, case.D)
    dp = ap.dead_prefix_rows(case, ops_.m, ops_.a, ops_.b0).permute(0, 2, 1)
    assert bool(dp.any()) and bool((~dp).any())
    if not torch.equal(got[dp], w[dp]):
        skipped = ap.emulate(ops_.q, ops_.k, ops_.v, case.H, dt, skip_prefix_rescale=True).to(dt).double().reshape(w.shape)
        how = "exactly as if the rescale were skipped" if torch.equal(got[dp], skipped[dp]) else "not as a plain skipped rescale"
        raise AssertionError(f"{int((got[dp] != w[dp]).any(-1).sum())} of {int(dp.sum())} dead-prefix rows are wrong, {how}")
    assert torch.equal(got[~dp], w[~dp]), "rows with a live key in the first tile are wrong (rescaled with another row's alpha?)"


# ---- 4: addressing ---------------------------------------------------------------------------------------------------------------------------

@_cases(ap.ADDRESS_CASES)
def test_addressing(case, compute_dtype):
    """H = 3 with the live pattern shifted per head, B = 2 with one broadcast K / V (Bk = 1) or two that differ (Bk = 2), q and k read from one
    fused buffer through q_col / k_col with ld > 2 H D (the gaps and the k rows >= Lk hold NaN), the output written into `out=` at
    o_col > 0. 2 query tiles x 3 heads x 2 images = 12 workgroups, not a multiple of 8: xcd_remap's remainder branch.
    Lk 128: attn_kernel<T, D, true, false>; Lk 77: attn_kernel<T, D, false, false>."""
    _needs_dma(case.dma)
    ops, dt = _ops(), compute_dtype
    ops_, want = _built(case)
    inner, Lq, Lk = case.inner, case.Lq, case.Lk
    q_col, k_col, o_col = 8, inner + 16, 12
    fused = torch.full((case.B, max(Lq, Lk), 2 * inner + 24), float("nan"), dtype=dt)
    fused[:, :Lq, q_col:q_col + inner] = ops_.q.to(dt)
    fused[:case.Bk, :Lk, k_col:k_col + inner] = ops_.k.to(dt)
    fused = fused.to(DEV)
    out = torch.full((case.B, Lq, inner + 24), SENTINEL, dtype=dt, device=DEV)
    ret = ops.attention(fused, fused[:case.Bk], ops_.vt(dt).to(DEV), case.H, case.D, 1.0, q_col=q_col, k_col=k_col, Lk=Lk, out=out, o_col=o_col)
    assert ret is out
    got = out.cpu()
    _assert_exact(got[..., o_col:o_col + inner].contiguous(), want, ops_, dt)
    assert bool((got[..., :o_col] == SENTINEL).all()) and bool((got[..., o_col + inner:] == SENTINEL).all()), "columns outside the window were written"
    # ... and the same bits from dense operands
    dense = ops.attention(ops_.q.to(dt).to(DEV), ops_.k.to(dt).to(DEV), ops_.vt(dt).to(DEV), case.H, case.D, 1.0, Lk=Lk)
    assert torch.equal(dense.cpu(), got[..., o_col:o_col + inner])


# ---- 5: the SPLIT operand maps ---------------------------------------------------------------------------------------------------------------

def _split_call(ops, dt, qh, ql, kh, kl, vt, case, **kw):
    inner = case.inner
    qq = torch.cat([qh, ql], -1).to(dt).to(DEV)
    kk = torch.cat([kh, kl], -1).to(dt).to(DEV)
    return ops.attention(qq, kk, vt.to(DEV), case.H, case.D, 1.0, Lk=case.Lk, out_split=2, q_lo_col=inner, k_lo_col=inner, **kw)


def _assert_split_exact(o, want, ops_, dt, zero_lo=True):
    inner = ops_.case.inner
    hi, lo = ap.split_rounded(want, dt)
    _assert_exact(o[..., :inner].contiguous(), hi.double(), ops_, dt)
    assert torch.equal(o[..., inner:].cpu(), lo), "low output halves differ"
    if zero_lo:
        assert bool((o[..., inner:] == 0).all()), "low output halves are not exact zeros"


@_cases(ap.SPLIT_CASES)
@pytest.mark.parametrize("form", ["k_lo", "q_lo"])
def test_split_score_passes(case, form, compute_dtype):
    """The accurate tier with operand type bf16 / fp16 (where test_attention_two_term_split_q_k_p runs the split form; exact running maximum),
    out_split = 2. "k_lo": the -16 pattern only in k_lo, k_hi = 0, the one-hot in q_hi - the K_lo Q_hi pass, i.e. the K_lo tile behind K_hi in
    LDS, carries every score. "q_lo": the one-hot only in q_lo, q_hi = 0, the pattern in k_hi - the K_hi Q_lo pass and the q_lo fragments.
    Each with and without split probabilities (P_lo = 0 here); the low output halves are exact zeros; once more through out= with o_col and
    o_lo_col. Lk 128: attn_kernel<T, 64, true, true>; Lk 100: attn_kernel<T, 64, false, true>."""
    _needs_dma(case.dma)
    ops, dt = _ops(), compute_dtype
    ops.set_compute_dtype(torch.float32, operand_dtype=dt)
    ops_, want = _built(case)
    qh, ql, kh, kl = ap.split_form(ops_, form)
    inner = case.inner
    for p_split in (True, False):
        o = _split_call(ops, dt, qh, ql, kh, kl, ops_.vt(dt), case, p_split=p_split)
        assert tuple(o.shape) == (case.B, case.Lq, 2 * inner)
        _assert_split_exact(o, want, ops_, dt)
    o_col, o_lo_col = 8, inner + 24
    out = torch.full((case.B, case.Lq, 2 * inner + 40), SENTINEL, dtype=dt, device=DEV)
    _split_call(ops, dt, qh, ql, kh, kl, ops_.vt(dt), case, out=out, o_col=o_col, o_lo_col=o_lo_col)
    got = out.cpu()
    _assert_exact(got[..., o_col:o_col + inner].contiguous(), want, ops_, dt)
    assert bool((got[..., o_lo_col:o_lo_col + inner] == 0).all()), "low output halves at o_lo_col are not exact zeros"
    keep = torch.ones(got.shape[-1], dtype=torch.bool)
    keep[o_col:o_col + inner] = False
    keep[o_lo_col:o_lo_col + inner] = False
    assert bool((got[..., keep] == SENTINEL).all()), "columns outside the two windows were written"


@_cases(ap.LOLO_CASES)
def test_split_has_no_lo_lo_pass(case, compute_dtype):
    """Information only in q_lo and k_lo: no pass multiplies the two, every score is 0 and O is the mean over all keys - exact in fp32 for
    Lk = 32, 64, 128 and written as a two-term split whose low half is NOT zero (the sum of up to 128 values needs more than 8 bits).
    Lk 64, 128: attn_kernel<T, 64, true, true>; Lk 32: attn_kernel<T, 64, false, true>."""
    _needs_dma(case.dma)
    ops, dt = _ops(), compute_dtype
    ops.set_compute_dtype(torch.float32, operand_dtype=dt)
    ops_, _ = _built(case)
    qh, ql, kh, kl = ap.split_form(ops_, "lo_lo")
    want = ap.mean_of_all_keys(ops_)
    for p_split in (True, False):
        _assert_split_exact(_split_call(ops, dt, qh, ql, kh, kl, ops_.vt(dt), case, p_split=p_split), want, ops_, dt, zero_lo=False)


@_cases(ap.SPLIT_CASES)
@pytest.mark.parametrize("p_split", [True, False], ids=["p-split", "p-single"])
def test_split_v_lo_map(case, p_split, compute_dtype):
    """V^T as [2 inner, ld] with V_hi = 0 and V_lo = V (pad columns of both halves poisoned): the V^T_lo tile behind V^T_hi and the V_lo P_hi
    pass carry the whole result. Scores from the "k_lo" form. Lk 128: attn_kernel<T, 64, true, true>; Lk 100: attn_kernel<T, 64, false, true>."""
    _needs_dma(case.dma)
    ops, dt = _ops(), compute_dtype
    ops.set_compute_dtype(torch.float32, operand_dtype=dt)
    ops_, want = _built(case)
    qh, ql, kh, kl = ap.split_form(ops_, "k_lo")
    vt = ops_.vt(dt)
    vt2 = torch.cat([ap.transposed(torch.zeros_like(ops_.v), case.ld, dt), vt], 1)
    assert tuple(vt2.shape) == (case.Bk, 2 * case.inner, case.ld)
    _assert_split_exact(_split_call(ops, dt, qh, ql, kh, kl, vt2, case, p_split=p_split), want, ops_, dt)
    # V_hi = V, V_lo = 0: the same result, nothing read from the lo tile's place
    vt3 = torch.cat([vt, ap.transposed(torch.zeros_like(ops_.v), case.ld, dt)], 1)
    _assert_split_exact(_split_call(ops, dt, qh, ql, kh, kl, vt3, case, p_split=p_split), want, ops_, dt)


# ---- 6: the P_lo map (a tolerance probe) ----------------------------------------------------------------------------------------------------

# Measured on an MI355X (worst relative error of a probability over 150 x Lk elements; bound attention_probe.P_LO_BOUND = 2^-13 = 1.221e-4):
#   bf16  Lk 64: 1.423e-5   Lk 44: 1.228e-5      with p_split=False (P a single 16-bit value): 3.848e-3, 3.836e-3
#   fp16  Lk 64: 4.213e-6   Lk 44: 2.545e-6                                                     4.835e-4, 4.827e-4
# The host emulation (attention_probe.emulate, tests/test_attention_probes_cpu.py) gives the same figures to the digits shown.


@pytest.mark.parametrize("Lk", [64, 44], ids=["Lk64-dma", "Lk44-reg"])
def test_p_lo_map_identity_v(Lk, compute_dtype):
    """V^T = identity over the keys (D = 64, one head), q and k random two-term splits, p_split: o_hi + o_lo is the probability row itself,
    p_hi + p_lo. Within 2^-13 relative of float64 softmax of the hi + lo operands on EVERY element - the bound and derivation of
    test_lane_map_p_lo_identity_v (tests/test_vae_split_attention_gpu.py), restated for this kernel at attention_probe.P_LO_BOUND; a P_lo
    fragment paired with the wrong V^T slots, or dropped, leaves up to 2^-8 (bf16) / 2^-11 (fp16). Output channels >= Lk are exact zeros.
    Lk 64: attn_kernel<T, 64, true, true>; Lk 44 (ld 48, four poisoned pad columns): attn_kernel<T, 64, false, true>."""
    _needs_dma(Lk % 64 == 0)
    ops, dt, D = _ops(), compute_dtype, 64
    ops.set_compute_dtype(torch.float32, operand_dtype=dt)
    qq, kk, vt = ap.p_lo_operands(Lk, dt)
    ref = ap.p_lo_reference(qq, kk, Lk)
    worst = {}
    for p_split in (True, False):
        o = ops.attention(qq.to(DEV), kk.to(DEV), vt.to(DEV), 1, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=D, k_lo_col=D, p_split=p_split).cpu()
        assert torch.isfinite(o.float()).all()
        got = o[..., :D].double() + o[..., D:].double()
        assert bool((got[..., Lk:] == 0).all()), "channels without a key are not exact zeros"
        worst[p_split] = float(((got[..., :Lk] - ref).abs() / ref).max())
    print(f"P_lo lane map, {dt}, Lk {Lk}: worst relative error of a probability {worst[True]:.3e} (bound 2^-13 = {ap.P_LO_BOUND:.3e}); "
          f"with a single P {worst[False]:.3e}")
    assert worst[True] <= ap.P_LO_BOUND
    assert worst[False] > ap.P_LO_BOUND, "p_split=False is as accurate as the split: the probe cannot see P_lo"


# ---- 7: normalisation ------------------------------------------------------------------------------------------------------------------------

# Worst |o / c - 1| observed on an MI355X: 0 in all six cases (bf16 and fp16; D 64 / Lk 512, D 128 / Lk 512, D 64 / Lk 500) - every output
# rounds back to c itself. Bounds: 2^-8 x 1.01 = 3.945e-3 for bf16, 2^-10 x 1.01 = 9.863e-4 for fp16.


@pytest.mark.parametrize("D,Lk", [(64, 512), (128, 512), (64, 500)], ids=["D64-Lk512-dma", "D128-Lk512-dma", "D64-Lk500-reg"])
def test_normalisation_of_constant_v(D, Lk, compute_dtype):
    """Random q and k with the spiked keys of test_attention_spiked_max (two that force a rescale above the deferred threshold late in the sweep,
    one late maximum below it: p > 1, no rescale) and V constant per channel, c_d = +-(1 .. 7) 2^e: softmax weights sum to one, so o = c_d
    whatever the scores. The kernel rounds P per element to the compute type for the PV product while l sums the unrounded values:
    |o / c - 1| <= u_P + u_out + fp32 noise; asserted per element at 2^-8 x 1.01 (bf16) / 2^-10 x 1.01 (fp16), see attention_probe.NORM_BOUND. A rescale
    applied to O but not to l (or the reverse), a lane's l left out of the final sum, or a tile counted twice in either breaks it by far more.
    Fast tiers (deferred maximum 2^8). Lk 512: attn_kernel<T, D, true, false>; Lk 500: attn_kernel<T, 64, false, false>."""
    _needs_dma(Lk % 64 == 0)
    ops, dt = _ops(), compute_dtype
    q, k, c = ap.norm_operands(D, Lk)
    ld = (Lk + 7) // 8 * 8
    vt = ap.transposed(c.expand(1, Lk, D), ld, dt)
    o = ops.attention(q.to(dt).to(DEV), k.to(dt).to(DEV), vt.to(DEV), 1, D, D ** -0.5, Lk=Lk).cpu()
    assert torch.isfinite(o.float()).all()
    worst = float((o.double() / c.double() - 1).abs().max())
    bound = ap.NORM_BOUND[dt]
    print(f"normalisation, {dt}, D {D}, Lk {Lk}: worst |o / c - 1| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound
