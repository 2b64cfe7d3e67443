"""The attention probes of tests/test_attention_probes_gpu.py, checked without a GPU: every configuration's operands are built on the host and
held to the preconditions that make the probe exact (attention_probe.preconditions), the host emulation of the kernel's tile loop reproduces
the exact result in both 16-bit types and with both maximum rules, and deliberate mis-maps - the defects the probes are for - each change
at least one output element in every configuration they apply to."""
import functools

import pytest
import torch

import attention_probe as ap

CASES = pytest.mark.parametrize("case", ap.ALL_CASES, ids=[c.id for c in ap.ALL_CASES])


@functools.lru_cache(maxsize=None)
def _built(case):
    """(operands, exact result): built and checked once per configuration, never modified."""
    ops_ = ap.build(case)
    return ops_, ap.preconditions(ops_)


def _changed(got, want):
    return not torch.equal(got.double(), want)


def _key_perm(Lk, fn):
    j = torch.arange(Lk)
    p = fn(j)
    return torch.where(p < Lk, p, j)


def _swap_bits_2_3(j):
    return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1)


@CASES
def test_preconditions(case):
    ops_, want = _built(case)
    assert want.shape == (case.B, case.Lq, case.inner) and want.dtype == torch.float64
    assert ops_.vt(torch.bfloat16).shape == (case.Bk, case.inner, case.ld) and case.ld % 8 == 0 and case.ld >= case.Lk


def test_the_table_covers_what_the_probes_are_for():
    keys = {(c.D, c.Lk, c.n_live) for c in ap.KEY_CASES}
    assert keys == {(D, Lk, n) for D in (64, 128) for Lk in (64, 128, 320, 40, 77, 100, 136) for n in (1, 16, 32)}
    assert all(c.dma == (c.Lk in (64, 128, 320)) for c in ap.KEY_CASES)
    assert all(c.Lq == 150 and c.Lk <= 320 and c.H <= 3 and c.B <= 2 for c in ap.ALL_CASES)
    # 150 queries = 2 query tiles; with H = 3 and B = 2 that is 12 workgroups: not a multiple of the 8 XCDs (xcd_remap's remainder branch)
    assert all(-(-c.Lq // 128) * c.H * c.B == 12 for c in ap.ADDRESS_CASES)
    assert {c.Bk for c in ap.ADDRESS_CASES} == {1, 2} and {c.dma for c in ap.ADDRESS_CASES} == {True, False}
    assert {c.dma for c in ap.SPLIT_CASES} == {True, False} and all(c.D == 64 for c in ap.SPLIT_CASES + ap.LOLO_CASES)
    # the rescale from a dead-only prefix is exercised wherever a window fits behind the first tile, and that includes ragged and DMA shapes
    pre = [c for c in ap.KEY_CASES if c.Lk > 64 and c.prefix_attainable]
    assert {c.dma for c in pre} == {True, False} and {c.n_live for c in pre} == {1, 16, 32} and {c.D for c in pre} == {64, 128}
    # the plain choice of the construction where it is admissible
    assert ap.pick(ap.Case(64, 64, 1)) == (7, 5, 3)
    assert ap.pick(ap.Case(64, 77, 1))[0] % 7 != 0 and ap.pick(ap.Case(64, 77, 1))[0] % 11 != 0


@CASES
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("defer", [0.0, 8.0])
def test_emulation_reproduces_the_exact_result(case, dt, defer):
    """The tile loop as the kernel runs it - dead-only first tiles, the wave-wide rescale, the ragged last tile - lands on the exact mean."""
    ops_, want = _built(case)
    assert torch.equal(ap.emulate(ops_.q, ops_.k, ops_.v, case.H, dt, defer=defer).double(), want)


@CASES
def test_key_mis_maps_are_seen(case):
    ops_, want = _built(case)
    q, k, v, H, Lk = ops_.q, ops_.k, ops_.v, case.H, case.Lk
    # bits 2 and 3 of the key index swapped inside a 32-key block (the LDS-DMA K row permutation applied to K but not to V^T, or the reverse)
    assert _changed(ap.softmax_ref(q, k[:, _key_perm(Lk, _swap_bits_2_3)], v, H), want)
    assert _changed(ap.softmax_ref(q, k, v[:, _key_perm(Lk, _swap_bits_2_3)], H), want)
    # the two lane halves (keys +4) exchanged
    assert _changed(ap.softmax_ref(q, k[:, _key_perm(Lk, lambda j: j ^ 4)], v, H), want)
    if not case.dma:
        # the last ragged key dropped, and attributed to its neighbour
        assert _changed(ap.softmax_ref(q, k[:, :-1], v[:, :-1], H), want)
        k2, v2 = k.clone(), v.clone()
        k2[:, -1], v2[:, -1] = k[:, -2], v[:, -2]
        assert _changed(ap.softmax_ref(q, k2, v2, H), want)
        v3 = v.clone()
        v3[:, -1] = v[:, -2]
        assert _changed(ap.softmax_ref(q, k, v3, H), want)
        # ... and one key past the end let in as a live one (a mask that stops one short)
        k4 = torch.cat([k, torch.zeros_like(k[:, :1])], 1)
        v4 = torch.cat([v, torch.full_like(v[:, :1], 8.0)], 1)
        assert _changed(ap.softmax_ref(q, k4, v4, H), want)


@CASES
def test_head_and_batch_mis_maps_are_seen(case):
    ops_, want = _built(case)
    q, k, v, H, D = ops_.q, ops_.k, ops_.v, case.H, case.D
    roll = lambda t: t.reshape(*t.shape[:2], H, D).roll(1, 2).reshape(t.shape)                # noqa: E731  heads rotated by one
    assert _changed(ap.softmax_ref(q, roll(k), roll(v), H), want)
    assert _changed(ap.softmax_ref(q, roll(k), v, H), want)
    assert _changed(ap.softmax_ref(q, k, roll(v), H), want)
    if case.B > 1:
        assert _changed(ap.softmax_ref(q.flip(0), k, v, H), want)                           # image 1's queries answered with image 0's
    if case.Bk > 1:
        v2 = v.clone()
        v2[1] = v[0]                                                                         # batch 1 reading batch 0's V
        assert _changed(ap.softmax_ref(q, k, v2, H), want)
        k2 = k.clone()
        k2[1] = k[0]
        assert _changed(ap.softmax_ref(q, k2, v, H), want)


@pytest.mark.parametrize("case", [c for c in ap.ALL_CASES if c.Lk > 64 and c.prefix_attainable],
                         ids=[c.id for c in ap.ALL_CASES if c.Lk > 64 and c.prefix_attainable])
@pytest.mark.parametrize("defer", [0.0, 8.0])
def test_a_skipped_prefix_rescale_is_seen(case, defer):
    """Dead-prefix rows that keep the 64 dead keys they accumulated with p = 1 (their sum and their l): every such row comes out wrong,
    and the rows of the same wave that had a live key in the first tile do not."""
    ops_, want = _built(case)
    got = ap.emulate(ops_.q, ops_.k, ops_.v, case.H, torch.bfloat16, defer=defer, skip_prefix_rescale=True).double()
    dp = ap.dead_prefix_rows(case, ops_.m, ops_.a, ops_.b0).permute(0, 2, 1)                  # [B, Lq, H]
    wrong = (got != want).reshape(case.B, case.Lq, case.H, case.D).any(-1)
    assert bool(dp.any()) and torch.equal(wrong, dp)


SPLITS = pytest.mark.parametrize("case", ap.SPLIT_CASES, ids=[c.id for c in ap.SPLIT_CASES])


@SPLITS
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_split_forms_and_lo_for_hi(case, dt):
    """Each split arrangement is exact in the emulation (defer = 0: the tier that runs the split kernel), and reading a lo tile through the hi
    tile's offsets - K_lo, V^T_lo - changes it."""
    ops_, want = _built(case)
    for form in ("k_lo", "q_lo"):
        qh, ql, kh, kl = ap.split_form(ops_, form)
        for p_split in (False, True):
            assert torch.equal(ap.emulate(qh, kh, ops_.v, case.H, dt, defer=0.0, q_lo=ql, k_lo=kl, p_split=p_split).double(), want)
        for defect in {"k_lo": ("k_lo_reads_hi",), "q_lo": ("q_lo_reads_hi", "k_hi_reads_lo")}[form]:
            assert _changed(ap.emulate(qh, kh, ops_.v, case.H, dt, defer=0.0, q_lo=ql, k_lo=kl, **{defect: True}), want), defect
    qh, ql, kh, kl = ap.split_form(ops_, "k_lo")
    zv = torch.zeros_like(ops_.v)
    for p_split in (False, True):
        assert torch.equal(ap.emulate(qh, kh, zv, case.H, dt, defer=0.0, q_lo=ql, k_lo=kl, v_lo=ops_.v, p_split=p_split).double(), want)
        for defect in ("v_lo_reads_hi", "v_hi_reads_lo"):
            got = ap.emulate(qh, kh, zv, case.H, dt, defer=0.0, q_lo=ql, k_lo=kl, v_lo=ops_.v, p_split=p_split, **{defect: True})
            assert _changed(got, want), defect


@pytest.mark.parametrize("case", ap.LOLO_CASES, ids=[c.id for c in ap.LOLO_CASES])
def test_lo_lo_is_the_mean_of_all_keys(case):
    ops_, _ = _built(case)
    qh, ql, kh, kl = ap.split_form(ops_, "lo_lo")
    want = ap.mean_of_all_keys(ops_)
    got = ap.emulate(qh, kh, ops_.v, case.H, torch.bfloat16, defer=0.0, q_lo=ql, k_lo=kl, p_split=True)
    assert torch.equal(got.double(), want)
    for dt in (torch.bfloat16, torch.float16):
        hi, lo = ap.split_rounded(want, dt)
        assert torch.equal(hi.double() + lo.double(), want), "the mean over all keys is not exact as a two-term split"
    # a lo x lo pass, if the kernel had one, would bring the pattern back
    assert _changed(ap.softmax_ref(ops_.q, ops_.k, ops_.v, case.H), want)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("Lk", [64, 44])
def test_p_lo_probe_bound_separates(dt, Lk):
    """Probe 6 on the host: with V^T = identity the emulated o_hi + o_lo is the probability row, within 2^-13 relative of float64 softmax on
    every element; with P_lo dropped the worst element is beyond it."""
    qq, kk, vt = ap.p_lo_operands(Lk, dt)
    ref = ap.p_lo_reference(qq, kk, Lk)
    D = 64
    v = vt[:, :, :Lk].transpose(1, 2).float()
    args = dict(scale=D ** -0.5, defer=0.0, q_lo=qq[..., D:], k_lo=kk[..., D:], p_split=True)
    worst = {}
    for drop in (False, True):
        o = ap.emulate(qq[..., :D], kk[..., :D], v, 1, dt, drop_p_lo=drop, **args)
        hi, lo = ap.split_rounded(o.double(), dt)
        got = (hi.double() + lo.double())[..., :Lk]
        worst[drop] = float(((got - ref).abs() / ref).max())
    print(f"P_lo probe on the host, {dt}, Lk {Lk}: worst relative error {worst[False]:.3e}, with P_lo dropped {worst[True]:.3e}")
    assert worst[False] <= ap.P_LO_BOUND < worst[True]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D,Lk", [(64, 512), (64, 500)])
def test_normalisation_probe_bound_separates(D, Lk, dt):
    """Probe 7 on the host: the emulated kernel keeps o = c within the derived bound under both maximum rules, the spiked rows do rescale late
    in the sweep, and a rescale that reaches O but not l leaves them far outside."""
    q, k, c = ap.norm_operands(D, Lk)
    v = c.expand(1, Lk, D)
    for defer in (0.0, 8.0):
        o = ap.emulate(q, k, v, 1, dt, scale=D ** -0.5, defer=defer).to(dt)
        assert float((o.double() / c.double() - 1).abs().max()) <= ap.NORM_BOUND[dt]
        bad = ap.emulate(q, k, v, 1, dt, scale=D ** -0.5, defer=defer, l_misses_rescale=True).to(dt)
        err = (bad.double() / c.double() - 1).abs().amax(-1)[0]
        assert float(err[5]) > 0.5 and float(err[70]) > 0.5, "the spiked rows did not rescale"
