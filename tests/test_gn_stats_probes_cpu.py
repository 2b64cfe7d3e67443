"""Host side of the GroupNorm statistics probes (tests/test_gn_stats_probes_gpu.py, helpers in tests/dyadic_probe.py): every probe dry-runs to
its launch with its budgets asserted, StatsBudget rejects data that cannot be exact, the exact-sum assertion fires on each defect it is meant
to catch (emulated partials), and the float64 restatements of the finalisers agree with torch's GroupNorm."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dyadic_probe as dp  # noqa: E402
import guard_bands as gb  # noqa: E402
import test_gn_stats_probes_gpu as probes  # noqa: E402


@pytest.mark.parametrize("name", list(probes.PROBES))
def test_probe_dry_runs_to_its_launch_inside_its_budgets(name):
    """Data, restatement, the contraction's bit budget and the StatsBudget of every probe, with the tier's packing rules; the launch is skipped."""
    probes.dry_run(name)


def test_every_documented_producer_has_a_probe():
    """One probe at least per producer, group-size regime and finaliser named in the GPU module's docstring."""
    need = ["s3_spatial_gsz4", "s3_flat_gsz4", "s3_spatial_gsz8", "s3_spatial_gsz16", "s3_spatial_gsz64", "s3_spatial_gsz10_per_channel",
            "s3_spatial_gsz1_per_channel", "s3_split", "s3_mx", "s13_mx6", "s6_phase", "s16_phase", "s7_multi", "s8_multi_phase", "s1_stride2_gsz4",
            "s1_stride2_ragged_no_handle", "s2_conv1x1", "s1_linear", "s2_linear", "s4_splitk_no_handle", "s5_p8", "s21_mxfp8_conv", "s22_mxfp8_conv_multi",
            "s25_mxfp8_up", "s27_mxfp8_deep_c320", "s27_mxfp8_deep_c960", "s10_gn_fused", "s11_gn_fused_multi", "f2_pair_halo_gemm", "f2_pair_gemm_halo",
            "fm_merged", "r_bf16_", "r_fp16_", "r_fp32_"]
    for prefix in need:
        assert any(n.startswith(prefix) for n in probes.PROBES), prefix
    hw = sorted({v[0] for v in list(probes.READ_16.values()) + list(probes.READ_32.values())})
    assert {probes.gn_ppc(h) for h in hw} == {16, 32, 128, 256}, "every pixels-per-chunk regime of the read pass"
    assert any(h % probes.gn_ppc(h) for h in hw) and any(h < 256 // min(c // 8, 256) for h, c, _ in probes.READ_16.values())
    assert {v[1] for v in list(probes.READ_16.values()) + list(probes.READ_32.values())} >= {32, 320, 512, 2304}


def test_gn_ppc_restates_the_kernel_source():
    with open(os.path.join(os.path.dirname(HERE), "omgsr_amd", "csrc", "norm.hip")) as f:
        src = f.read()
    assert "return HW >= 32768 ? GN_PPC : (HW >= 8192 ? 128 : (HW >= 2048 ? 32 : 16));" in src and "constexpr int GN_PPC = 256;" in src
    assert [probes.gn_ppc(h) for h in (1, 2047, 2048, 8191, 8192, 32767, 32768)] == [16, 16, 32, 32, 128, 128, 256]


# ---- the generators ------------------------------------------------------------------------------------------------------------------

def _case(seed=3, N=3, H=11, W=40, Cin=32, C=40, G=4, residual=True):
    """A small halo-shaped case built like the GPU probes': exact output float64 [N, H, W, C], residual, per-channel exponents."""
    g = torch.Generator().manual_seed(seed)
    ce = dp.group_exponents(g, G, C)
    x = dp.stats_act(g, (N, H, W, Cin))
    w = dp.stats_wt(g, ce, Cin)
    r = dp.stats_residual(g, (N, H, W, C), ce) if residual else None
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), dp.stats_bias(g, ce).double(), padding=1).permute(0, 2, 3, 1)
    return (y + r.double() if residual else y).contiguous(), r, ce


def test_generators_keep_one_quantum_per_image_and_group():
    y, _, ce = _case()
    N, H, W, C = y.shape
    G = 4
    assert bool((y != 0).all())
    q = dp.quantum(y).reshape(N, H * W, G, C // G)
    per = q.amin((1, 3))
    assert torch.equal(q, per[:, None, :, None].expand_as(q)), "every output is an ODD multiple of its (image, group)'s quantum"
    e = ce.reshape(G, -1)
    assert torch.equal(e, e[:, :1].expand_as(e)) and bool((e[1:, 0] != e[:-1, 0]).all()), "one exponent per group, neighbours differ"
    x = dp.stats_act(torch.Generator().manual_seed(1), (4, 5, 8))
    m = x.abs().amax((1, 2))
    assert bool((x != 0).all()) and m[0] != m[1] and m[0] == m[2], "the exponent alternates between consecutive images"
    v = dp.stats_values(torch.Generator().manual_seed(2), (2, 9, C), ce)
    assert bool((v != 0).all()) and torch.equal(dp.quantum(v), v.abs().double() / torch.where(v.abs() / dp.quantum(v).float() == 3, 3.0, 1.0))


def test_group_sums_and_fold_partials():
    y, _, _ = _case()
    G = 4
    S, Q = dp.group_sums(y, G)
    N, _, _, C = y.shape
    for n in range(N):
        for g in range(G):
            blk = y[n, :, :, g * (C // G):(g + 1) * (C // G)]
            assert float(S[n, g]) == float(blk.sum()) and float(Q[n, g]) == float((blk * blk).sum())
    for per_channel in (False, True):
        part = dp.halo_partials_ref(y, G, per_channel)
        assert part.shape == (N, 2 * 2 * 2, C if per_channel else G, 2)
        s, q = dp.fold_partials(part, G)
        assert torch.equal(s, S) and torch.equal(q, Q)
        probes.assert_exact_sums(part, G, S, Q, "emulated partials")


# ---- StatsBudget ---------------------------------------------------------------------------------------------------------------------

def test_stats_budget_accepts_the_probe_data_and_rejects_what_cannot_be_exact():
    y, _, _ = _case()
    G = 4
    worst = dp.StatsBudget(y, G, 128 * 10, torch.bfloat16).check()
    assert 0 < worst < 2.0 ** 24
    # too many bits: the same data with a slot so large that a partial sum of squares passes 2^24 quanta
    with pytest.raises(AssertionError, match="bit budget"):
        dp.StatsBudget(y, G, 1 << 22, torch.bfloat16).check()
    big = y.clone()
    big[0, 0, 0, 0] *= 2.0 ** 12                      # one value of 2^12 and more quanta: its square alone is 2^24
    with pytest.raises(AssertionError, match="bit budget"):
        dp.StatsBudget(big, G, 128 * 10, torch.float32).check()
    # mixed quanta in a group: one value 2^-20 finer than the others
    mixed = y.clone()
    mixed[1, 2, 3, 5] += dp.quantum(y)[1, 2, 3, 5] * 2.0 ** -20
    with pytest.raises(AssertionError, match="mixed quanta"):
        dp.StatsBudget(mixed, G, 128 * 10, torch.float32).check()
    # a zero output
    zero = y.clone()
    zero[2, 10, 39, 39] = 0.0
    with pytest.raises(AssertionError, match="zero"):
        dp.StatsBudget(zero, G, 128 * 10, torch.bfloat16).check()
    # not representable in the stored type: 9 significant bits in bf16
    wide = y.clone()
    wide[0, 0, 0, 0] = 257.0 * float(dp.quantum(y)[0, 0, 0, 0])
    with pytest.raises(AssertionError, match="stored type"):
        dp.StatsBudget(wide, G, 128 * 10, torch.bfloat16).check()
    # a group whose mean dominates its spread
    g = torch.Generator().manual_seed(5)
    onesided = (32.0 + 2.0 * torch.randint(0, 4, (2, 6, 7, 8), generator=g).double()) + 1.0      # odd integers 33 .. 39
    with pytest.raises(AssertionError, match="mean"):
        dp.StatsBudget(onesided, 2, 16, torch.float32).check()
    # values whose squares leave the normal fp32 range
    with pytest.raises(AssertionError, match="normal"):
        dp.StatsBudget(y * 2.0 ** -70, G, 128 * 10, torch.float32).check()


# ---- negative controls: each defect makes the exact-sum assertion fire ----------------------------------------------------------------

def _emulated(per_channel, C=40, G=4):
    y, r, _ = _case(C=C, G=G)
    S, Q = dp.group_sums(y, G)
    part = dp.halo_partials_ref(y, G, per_channel)
    probes.assert_exact_sums(part, G, S, Q, "untouched")
    return y, r, S, Q, part


def _add(part, n, slot, entry, v, sign=1.0):
    part[n, slot, entry, 0] += sign * float(v)
    part[n, slot, entry, 1] += sign * float(v) ** 2


@pytest.mark.parametrize("per_channel", [False, True])
def test_dropping_one_border_pixel_is_seen(per_channel):
    y, _, S, Q, part = _emulated(per_channel)
    N, H, W, C = y.shape
    G = 4
    # the last pixel of the ragged last tile (row 10 of 11: tile row 1, upper half; column 39 of 40: tile column 1), one channel of it is enough
    n, yy, xx, c = 1, H - 1, W - 1, 17
    slot = ((yy // 8) * 2 + xx // 32) * 2 + (yy % 8) // 4
    for chans in ([c], range(C)):                     # one channel of the pixel, then the whole pixel
        p = part.clone()
        for ch in chans:
            _add(p, n, slot, ch if per_channel else ch // (C // G), y[n, yy, xx, ch], -1.0)
        with pytest.raises(AssertionError, match="differ from the exact sums"):
            probes.assert_exact_sums(p, G, S, Q, "dropped pixel")
    # ... and a pixel counted twice
    p = part.clone()
    _add(p, n, slot, c if per_channel else c // (C // G), y[n, yy, xx, c])
    with pytest.raises(AssertionError, match="differ from the exact sums"):
        probes.assert_exact_sums(p, G, S, Q, "doubled pixel")


@pytest.mark.parametrize("per_channel", [False, True])
def test_counting_one_padded_column_is_seen(per_channel):
    """Cout 40 is packed as Cout_pad 128. Column 40 holds no weight and no bias: an epilogue that did not stop at Cout would compute 0 + the
    residual it reads there - row-major, the NEXT pixel's channel 0 - and credit it to the last entry it has."""
    y, r, S, Q, part = _emulated(per_channel)
    C, G = y.shape[-1], 4
    n, yy, xx = 0, 3, 7
    v = r[n, yy, xx + 1, 0]
    assert float(v) != 0.0
    p = part.clone()
    _add(p, n, ((yy // 8) * 2 + xx // 32) * 2 + (yy % 8) // 4, C - 1 if per_channel else G - 1, v)
    with pytest.raises(AssertionError, match="differ from the exact sums"):
        probes.assert_exact_sums(p, G, S, Q, "padded column")


@pytest.mark.parametrize("per_channel", [False, True])
def test_crediting_one_channel_to_the_neighbouring_group_is_seen(per_channel):
    y, _, S, Q, part = _emulated(per_channel)
    N, H, W, C = y.shape
    G = 4
    c = C // G - 1                                    # the last channel of group 0, credited to group 1
    p = part.clone()
    if per_channel:                                   # the per-channel entries of channels c and c + 1 swapped in every slot
        p[:, :, [c, c + 1]] = part[:, :, [c + 1, c]]
    else:
        col = dp.halo_partials_ref(y[..., c:c + 1].contiguous(), 1, False)          # [N, slots, 1, 2]: channel c alone
        p[:, :, 0] -= col[:, :, 0]
        p[:, :, 1] += col[:, :, 0]
    with pytest.raises(AssertionError, match="differ from the exact sums"):
        probes.assert_exact_sums(p, G, S, Q, "channel in the wrong group")
    # one image's partials credited to its neighbour
    p = part.clone()
    p[[0, 1]] = part[[1, 0]]
    with pytest.raises(AssertionError, match="differ from the exact sums"):
        probes.assert_exact_sums(p, G, S, Q, "wrong image")


@pytest.mark.parametrize("per_channel", [False, True])
def test_one_slot_left_at_the_fence_pattern_is_seen(per_channel):
    """fenced_outputs pre-fills the partials buffer: a slot the kernel never writes holds pattern bytes, not zeros. The same defect passes
    unnoticed on a zero-filled buffer when the slot's true sums are zero - which no probe allows (no zero outputs) - and here."""
    y, _, S, Q, part = _emulated(per_channel)
    G = 4
    with gb.fenced_outputs(host=True):
        buf = torch.empty(part.shape, device="cpu", dtype=torch.float32)
        fence = buf.clone()
        buf.copy_(part)
        probes.assert_exact_sums(buf, G, S, Q, "every slot written")
        buf[2, 5] = fence[2, 5]                       # slot 5 of image 2 never written
    assert not torch.equal(buf[2, 5], torch.zeros_like(buf[2, 5]))
    with pytest.raises(AssertionError, match="differ from the exact sums"):
        probes.assert_exact_sums(buf, G, S, Q, "unwritten slot")
    one = part.clone()                                # a single entry of a single slot is enough
    one[0, 1, 0] = fence[0, 1, 0]
    with pytest.raises(AssertionError, match="differ from the exact sums"):
        probes.assert_exact_sums(one, G, S, Q, "unwritten entry")


# ---- the finalisers' restatements ------------------------------------------------------------------------------------------------------

def test_finalize_ref_is_group_norm_in_float64():
    g = torch.Generator().manual_seed(11)
    N, C, H, W, G = 3, 24, 7, 9, 6
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 3 + 0.5
    eps = 1e-5
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    S, Q = dp.group_sums(x.permute(0, 2, 3, 1), G)
    m, v, r = dp.finalize_ref(S, Q, H * W * (C // G), eps)
    xg = x.reshape(N, G, -1)
    assert torch.allclose(m, xg.mean(-1), rtol=1e-13, atol=1e-13) and torch.allclose(v, xg.var(-1, unbiased=False), rtol=1e-11)
    want = F.group_norm(x, G, eps=eps32)
    got = (x - m.repeat_interleave(C // G, 1)[:, :, None, None]) * r.repeat_interleave(C // G, 1)[:, :, None, None]
    assert torch.allclose(got, want, rtol=1e-11, atol=1e-12)
    # the clamp: a constant group has variance 0, whatever the rounding of q / count - m^2 says
    c = torch.full((1, 5, 8), 0.1, dtype=torch.float64)
    _, v0, r0 = dp.finalize_ref(*dp.group_sums(c, 1), 40, eps)
    assert float(v0) >= 0.0 and abs(float(r0) - eps32 ** -0.5) < 1e-3


def test_merged_ref_is_the_weighted_fold_of_per_tile_statistics():
    g = torch.Generator().manual_seed(12)
    N, C, G = 2, 16, 4
    shapes, tiles = [(8, 8), (4, 8)], [2, 4]
    tot = float(sum(h * w * t for (h, w), t in zip(shapes, tiles)))
    parts, mm, vv = [], 0.0, 0.0
    for (h, w), t in zip(shapes, tiles):
        x = torch.randn(t * N, h * w, C, generator=g, dtype=torch.float64)
        S, Q = dp.group_sums(x, G)
        parts.append((S.reshape(t, N, G), Q.reshape(t, N, G), h * w * (C // G), h * w / tot))
        xg = x.reshape(t, N, h * w, G, C // G).permute(0, 1, 3, 2, 4).reshape(t, N, G, -1)
        mm = mm + (h * w / tot) * xg.mean(-1).sum(0)
        vv = vv + (h * w / tot) * xg.var(-1, unbiased=False).sum(0)
    m, v, r = dp.merged_ref(parts, 1e-6)
    assert torch.allclose(m, mm, rtol=1e-12, atol=1e-14) and torch.allclose(v, vv, rtol=1e-11)
    assert torch.allclose(r, (v + float(torch.tensor(1e-6, dtype=torch.float32))) ** -0.5, rtol=1e-14)
    # one shape group of one tile with weight 1 is the plain finaliser
    S, Q, count, _ = parts[0]
    a = dp.merged_ref([(S[:1], Q[:1], count, 1.0)], 1e-6)
    b = dp.finalize_ref(S[0], Q[0], count, 1e-6)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_ulps32():
    a = torch.tensor([1.0, 1.0, -1.0, 2.0 ** -140, 0.0])
    b = torch.tensor([1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, -1.0 - 2.0 ** -22, -(2.0 ** -140), -0.0])
    assert dp.ulps32(a, b).tolist() == [1, 1, 2, 2 * 2 ** 9, 0]


def test_halo_partials_ref_drops_the_padding():
    y = torch.ones(1, 9, 33, 8, dtype=torch.float64)
    p = dp.halo_partials_ref(y, 2, False)
    assert p.shape == (1, 8, 2, 2)
    # tile (0, 0): 4 x 32 pixels x 4 channels per half; tile (0, 1): 4 x 1; tile row 1 holds one map row in its upper half only
    assert p[0, :, 0, 0].tolist() == [512.0, 512.0, 16.0, 16.0, 128.0, 0.0, 4.0, 0.0]
