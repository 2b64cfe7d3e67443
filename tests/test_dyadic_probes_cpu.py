"""Host side of the dyadic probes (tests/dyadic_probe.py, tests/test_dyadic_probes_gpu.py): every kernel variant the dispatcher can record
has a probe or a stated exclusion, every probe fits its bit budget, the budget check rejects what cannot be exact, the restatements decode
the documented byte forms, and the probe data are sensitive to the defects the GPU equality is meant to catch."""
import contextlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dyadic_probe as dp  # noqa: E402
import test_dyadic_probes_gpu as gpu_probes  # noqa: E402

ROOT = os.path.dirname(HERE)
# variants deliberately without a dyadic probe: none. (The GroupNorm-fused variants 10 / 11 apply SiLU in their prologue; their probes use data
# on which it is the identity in fp32 - test_dyadic_probes_gpu.gn_fused_case - and the tolerance tests keep the nonlinear range.)
EXCLUDED = {}


def _src(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@contextlib.contextmanager
def _tier(act: torch.dtype, precise: bool):
    """The packing rules of a tier without the library (ops reads these two module globals)."""
    from omgsr_amd import ops
    saved = ops._ACT, ops._PRECISE
    ops._ACT, ops._PRECISE = act, precise
    try:
        yield ops
    finally:
        ops._ACT, ops._PRECISE = saved


# ---- coverage ------------------------------------------------------------------------------------------------------------------------

def test_variant_parser_reads_both_arms_of_ternaries():
    src = "ts.rec.variant = ng == 1 ? (mode == 1 ? 6 : 3) : (mode == 1 ? 8 : 7);  // 7 / 8\n ts.rec.variant = a.mx_fmt == 6 ? 15 : 12;\n" \
          "ts.rec.variant = 18;"
    assert dp.variant_ids(src) == {3, 6, 7, 8, 12, 15, 18}


def test_every_dispatcher_variant_has_a_probe():
    ids = dp.variant_ids(_src("omgsr_amd", "csrc", "igemm.hip"))
    assert {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18} <= ids, f"parser lost ids: {sorted(ids)}"
    names = dp.probe_names(_src("tests", "test_dyadic_probes_gpu.py"))
    assert sorted(names) == sorted(gpu_probes.PROBES)
    probed = {dp.variant_of_probe(n) for n in names}
    missing = ids - probed - set(EXCLUDED)
    assert not missing, f"kernel variants without a dyadic probe: {sorted(missing)} (add one to tests/test_dyadic_probes_gpu.py)"
    assert not (set(EXCLUDED) & probed) and set(EXCLUDED) <= ids
    assert probed <= ids, f"probes name variants the dispatcher no longer records: {sorted(probed - ids)}"


@pytest.mark.parametrize("name", list(gpu_probes.PROBES))
def test_probe_fits_its_bit_budget(name):
    """Each probe built on the host with its tier's packing rules: the reference is computed and the budget asserted (the launch is skipped)."""
    gpu_probes.dry_run(name)


# ---- the budget check --------------------------------------------------------------------------------------------------------------

def test_budget_rejects_what_cannot_be_exact():
    A = torch.tensor([[2.0 ** 22, 1.0]], dtype=torch.float64)
    W = torch.tensor([[1.0, 1.0]], dtype=torch.float64)
    b = dp.Budget(1, 1, "cpu")
    b.add(A, W)
    with pytest.raises(AssertionError, match="budget"):
        b.check()
    A20 = torch.tensor([[2.0 ** 20, 1.0]], dtype=torch.float64)
    ok = dp.Budget(1, 1, "cpu")
    ok.add(A20, W)
    assert ok.check() == 2.0 ** 20 + 1
    # the finest quantum can come from an epilogue term
    t = dp.Budget(1, 1, "cpu")
    t.add(A20, W)
    t.term(torch.tensor([[2.0 ** -3]]))
    with pytest.raises(AssertionError, match="budget"):
        t.check()
    # products below the normal fp32 range
    tiny = dp.Budget(1, 1, "cpu")
    tiny.add(torch.tensor([[2.0 ** -70]], dtype=torch.float64), torch.tensor([[2.0 ** -70]], dtype=torch.float64))
    with pytest.raises(AssertionError, match="normal"):
        tiny.check()
    # a gate that is not a power of two cannot be folded exactly
    with pytest.raises(AssertionError):
        ok.scale(torch.tensor([3.0]))
    # segments: the a_lo x w_lo product a split form never computes does not count
    seg = dp.Budget(1, 1, "cpu")
    seg.add(torch.tensor([[4.0]], dtype=torch.float64), torch.tensor([[2.0 ** -20]], dtype=torch.float64))
    seg.add(torch.tensor([[2.0 ** -20]], dtype=torch.float64), torch.tensor([[4.0]], dtype=torch.float64))
    assert seg.check() == 2.0


def test_mxfp8_probe_must_fit_the_instruction_window():
    """A product 2^14 below the largest of its 8-wide K group is dropped by the block-scaled MFMA: the MXFP8 reference refuses
    probe data that would depend on it, whatever the bit budget says."""
    f8 = lambda v: torch.tensor([float(v)]).to(torch.float8_e4m3fn).view(torch.uint8)[0]      # noqa: E731
    a = torch.zeros(1, 128, dtype=torch.uint8)
    w = torch.zeros(1, 128, dtype=torch.uint8)
    a[0, 0], w[0, 0], w[0, 1] = f8(32.0), f8(32.0), f8(1.0)
    s = torch.full((1, 4), 127, dtype=torch.uint8)
    a[0, 1] = f8(2.0 ** -3)                                               # 2^10 vs 2^-3: 13 bits, inside the window
    assert float(dp.mxfp8_ref(a, s, w, s, 1)[0, 0]) == 1024 + 2.0 ** -3
    a[0, 1] = f8(2.0 ** -4)                                               # 14 bits: dropped by the instruction
    with pytest.raises(AssertionError, match="group"):
        dp.mxfp8_ref(a, s, w, s, 1)
    a[0, 1], a[0, 8], w[0, 8] = 0, f8(2.0 ** -4), f8(2.0 ** -4)           # 18 bits across two groups is fine
    assert float(dp.mxfp8_ref(a, s, w, s, 1)[0, 0]) == 1024 + 2.0 ** -8


def test_quantum():
    x = torch.tensor([0.0, 1.0, -3.0, 6.0, 0.375, 2.0 ** -60 * 5, 448.0], dtype=torch.float64)
    q = dp.quantum(x)
    assert q[0] == float("inf")
    assert q[1:].tolist() == [1.0, 1.0, 2.0, 0.125, 2.0 ** -60, 64.0]


def test_generators():
    g = torch.Generator().manual_seed(0)
    e = dp.exponents(g, 64, 128, row=(-3, 3), col=(0, 1), block=32)
    assert torch.equal(e[:, :32], e[:, :1].expand(64, 32))          # one exponent per 32-channel block
    x = dp.two_term(g, e)
    hi = x.to(torch.float16).float()
    lo = x - hi
    assert bool((lo != 0).all()) and torch.equal(lo.abs(), torch.exp2(e - 11))
    assert torch.equal(lo.to(torch.float16).float(), lo)
    m = dp.sparse_mask(g, 40, 576, 16)
    assert bool((m.sum(1) == 16).all()) and bool(m.any(0).all())     # 40 x 16 >= 576: every K position is exercised


# ---- restatements vs the documented forms ------------------------------------------------------------------------------------------

def test_mxfp8_restatement_is_mxfp8_dequant():
    from omgsr_amd.testing import mxfp8_dequant
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 256, (7, 256), generator=g, dtype=torch.int64).to(torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0                                   # no NaN codes
    scales = torch.randint(80, 175, (7, 8), generator=g, dtype=torch.int64).to(torch.uint8)
    assert torch.equal(dp.mxfp8_values(codes, scales), mxfp8_dequant(codes, scales))


def test_split_weight_restatement_is_the_documented_segments():
    g = torch.Generator().manual_seed(2)
    with _tier(torch.float16, True) as ops:
        w = gpu_probes._wt(g, 16, 32, nnz=20, chan=(0, 0), split=True)
        pw = ops.pack_conv_weight(w, None, device="cpu", split=2, w_split=2)
        assert pw.cin == 96 and dp.segments(pw) == [(0, 32), (32, 64), (64, 96)]
        wt = w.permute(0, 2, 3, 1).reshape(16, 9, 32)
        hi = wt.to(torch.float16).double()
        want = torch.cat([hi, hi, wt.double() - hi], -1)                 # [w_hi | w_hi | w_lo] per tap
        assert torch.equal(dp.weight_values(pw)[:16], want)
        assert not bool(dp.weight_values(pw)[16:].any())                # padded rows
        x = dp.two_term(g, torch.zeros(5, 32))
        av = dp.operand_values(dp.host_operand(x, "split"), pw)
        xh = x.to(torch.float16).double()
        assert torch.equal(av, torch.cat([xh, x.double() - xh, xh], -1))     # [a_hi | a_lo] and the wrap back to a_hi


def test_mx_restatements_are_the_documented_byte_forms():
    g = torch.Generator().manual_seed(3)
    with _tier(torch.float16, True) as ops:
        for fmt, split in ((8, 3), (6, 4)):
            w = gpu_probes._wt(g, 24, 64, nnz=30, chan=(0, 1), block=32, split=True)
            pw = ops.pack_conv_weight(w, None, device="cpu", split=split)
            wt = w.permute(0, 2, 3, 1).reshape(24, 9, 64).double()
            hi = wt.to(torch.float16).double()
            assert torch.equal(dp.weight_values(pw)[:24], torch.cat([hi, hi, wt - hi], -1)), fmt      # [w_hi | w_hi' | w_lo'] decoded
            x = dp.two_term(g, dp.exponents(g, 6, 64, row=(0, 1), col=(0, 1), block=32))
            xh = x.to(torch.float16).double()
            av = dp.operand_values(dp.host_operand(x, "mx" if fmt == 8 else "mx6"), pw)
            assert torch.equal(av, torch.cat([xh, x.double() - xh, xh], -1)), fmt                   # [a_hi | a_lo' | a_hi'] decoded
            if fmt == 6:          # the decoder reads the bytes ops._e2m3_blocks writes, scale byte and bit positions included
                v = dp.dyadic(g, dp.exponents(g, 4, 128, row=(-20, 20), col=(0, 0), block=32), (1, 7))
                assert torch.equal(dp.e2m3_third(ops._e2m3_blocks(v)), v.double())


def test_phase_restatement_sums_the_taps():
    g = torch.Generator().manual_seed(4)
    with _tier(torch.bfloat16, False) as ops:
        w = gpu_probes._wt(g, 8, 32, nnz=200)
        pw = ops.pack_conv_weight(w, None, device="cpu", upsample_phases=True)
        ph = ops._phase_kernels(w.permute(0, 2, 3, 1)).reshape(4, 8, 4, 32).permute(0, 2, 1, 3).double()      # [phase][tap][cout][c]
        assert torch.equal(dp.phase_weight_values(pw)[:, :, :8], ph)
        x = dp.dyadic(g, dp.exponents(g, 2 * 5 * 6, 32, row=(-2, 2), col=(0, 1))).reshape(2, 5, 6, 32).to(torch.bfloat16)
        assert torch.equal(dp.phase_conv_ref(x, pw), dp.conv_ref(x, pw, upsample=True))


# ---- sensitivity: the defects the GPU equality must see change the reference --------------------------------------------------------

def _mx_probe(g, ops):
    x = dp.host_operand(dp.two_term(g, dp.exponents(g, 2 * 6 * 7, 64, row=(0, 1), col=(0, 0))).reshape(2, 6, 7, 64), "mx")
    pw = ops.pack_conv_weight(gpu_probes._wt(g, 16, 64, nnz=16, chan=(0, 0), split=True), None, device="cpu", split=3)
    return x, pw


def test_dropping_one_correction_block_changes_the_reference():
    g = torch.Generator().manual_seed(5)
    with _tier(torch.float16, True) as ops:
        x, pw = _mx_probe(g, ops)
        ref = dp.conv_ref(x, pw)
        for k0 in (64, 96, 128, 160):          # each 32-channel block of the a_lo' x w_hi' and a_hi' x w_lo' segments
            w = dp.weight_values(pw).clone()
            w[:, :, k0:k0 + 32] = 0
            assert not torch.equal(dp.conv_ref(x, pw, weights=w, check=False), ref), k0


def test_shifting_one_scale_byte_changes_the_reference():
    g = torch.Generator().manual_seed(6)
    ac, asc, wc, wsc, _, _ = gpu_probes._mxfp8_pair(g, 12, 16, 256, 1 / 2)
    ref = dp.mxfp8_ref(ac, asc, wc, wsc, 16)
    for row, blk in ((3, 0), (7, 5), (11, 7)):
        bumped = asc.clone()
        bumped[row, blk] += 1
        got = dp.mxfp8_ref(ac, bumped, wc, wsc, 16, check=False)
        assert not torch.equal(got[row], ref[row]) and torch.equal(got[:row], ref[:row])
        swapped = asc.clone()                  # a scale byte taken from the neighbouring block
        swapped[row, blk] = asc[row, (blk + 1) % 8]
        assert not torch.equal(dp.mxfp8_ref(ac, swapped, wc, wsc, 16, check=False)[row], ref[row])
    wb = wsc.clone()
    wb[9, 2] -= 1
    assert not torch.equal(dp.mxfp8_ref(ac, asc, wc, wb, 16, check=False)[:, 9], ref[:, 9])


def test_dropping_one_border_tap_changes_the_reference():
    """Output column 0 of a 3x3 conv reads input columns 0 and 1 through taps s = 1, 2 (s = 0 is the zero padding). Every probe output there
    whose weights meet that tap would move if the kernel lost it: the contribution is nonzero for the probe data."""
    g = torch.Generator().manual_seed(7)
    with _tier(torch.bfloat16, False) as ops:
        x = dp.dyadic(g, dp.exponents(g, 2 * 9 * 11, 64, row=(-2, 2), col=(0, 1))).reshape(2, 9, 11, 64).to(torch.bfloat16)
        pw = ops.pack_conv_weight(gpu_probes._wt(g, 32, 64, nnz=64), None, device="cpu")
        ref = dp.conv_ref(x, pw)
        w = dp.weight_values(pw)
        for r in range(3):
            for s in (1, 2):
                tap = x.double()[:, :, s - 1]                        # input column s - 1 at output column 0, rows y - 1 + r
                rows = torch.nn.functional.pad(tap, (0, 0, 1, 1))[:, r:r + 9]
                contrib = rows @ w[:32, 3 * r + s].T
                assert bool(contrib.any()), (r, s)
                dropped = ref.clone()
                dropped[:, :, 0] -= contrib
                assert not torch.equal(dropped, ref)
