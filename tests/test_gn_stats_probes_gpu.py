"""Bit-exact probes for the GroupNorm statistics of every producer and finaliser.

Every GroupNorm takes its mean and variance from (sum, sum of squares) partials: left by the igemm epilogue (gn_flush, igemm_epilogue.hip.h:
one slot per wave tile of the halo-tile kernel, one per 32-row block of the GEMM-shaped kernels; one entry per group for group sizes
4 / 8 / 16 / 32 / 64, one per channel otherwise), by the MXFP8 conv kernels (the same epilogue behind their own tile maps), by the
GroupNorm-fused halo producer, or by the stand-alone read pass (gn_partial_kernel, norm.hip), and folded in double by gn_finalize_kernel,
gn_finalize2_kernel (a channel concatenation) or omgsr_groupnorm_finalize_merged (tile-shape groups). The tolerance tests cannot see one
miscounted pixel, one counted Cout_pad column or one ragged row counted twice (a relative 1 / (HW cpg)); these probes can: the data are dyadic
inside dyadic_probe.StatsBudget, so every fp32 partial is an exact integer times a quantum in any summation order.

Each probe asserts, in this order:
  1. the output equals the exact restatement after its one rounding, and the expected kernel variant ran;
  2. the producer's raw partials, folded in float64 over slots and entries, equal the exact sums (torch.equal), the handle being present
     exactly where the producer is documented to leave one;
  3. ops.group_norm_stats against dyadic_probe.finalize_ref: mean bit-equal (one correctly rounded double division, one conversion), var and
     rstd within 1 fp32 ulp (the device may contract q / count - m m into an FMA, and double sqrt / division may differ in the last double
     ulp: either can move one fp32 rounding boundary, nothing more; StatsBudget asserts m^2 <= var so the subtraction does not amplify that);
  4. the producer once more inside guard_bands.fenced_outputs(): the partials buffer is then pre-filled with the fence pattern, so a slot the
     kernel never writes cannot pass by holding zeros.

slot_elems (the largest run of values ONE fp32 partial can cover, from the kernels):
  halo-tile kernel, MXFP8 convs   a wave tile is 4 tile rows x 32 pixels (igemm_halo_body.hip.h: FM = 4 row blocks per wave, TW = 32; the FLAT
                                   form: 4 runs of 32 positions; the phase form: 4 x 32 low-resolution pixels of one phase): 128 x group size
                                   for one entry per group, 128 for per-channel entries
  GEMM-shaped kernels             one 32-row block (gn_howo): 32 x group size, or 32 per channel
  read pass                       one pixel chunk of gn_ppc(HW) = 16 / 32 / 128 / 256 pixels x the group's channels
The accurate-tier probes feed plain dyadic values through the split / MX / fp6 operand forms (their low halves are zero: a two-term value's
2^-11 tail would put 2^22 between the quantum and the magnitude of an output); what they pin is the fp32 epilogue - fp32 stores, fp32
residual - behind those instantiations. The GroupNorm-fused producer (variants 10 / 11) applies SiLU and nothing else (omgsr_igemm refuses any
other gn_act), so its probes keep every normalised value at 32 or more: exp(-v) < 2^-46 there, 1 + exp(-v) rounds to 1.0f, v_rcp_f32(1) is 1
and silu_f(v) = v * 1 is v itself - the producer's x * scale + shift, one rounding to the compute type and its zero padding are then exact."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyadic_probe as dp  # noqa: E402
import guard_bands as gb  # noqa: E402
import test_dyadic_probes_gpu as base  # noqa: E402  (_launch, _eq, _g, the dry-run launcher, the v10 / v11 output probes)

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
WAVE_PIXELS = 128          # halo-tile kernel and MXFP8 convs: pixels of one wave tile
BLOCK_ROWS = 32            # GEMM-shaped kernels: rows of one statistics slot


def _ops():
    from omgsr_amd import ops
    return ops


_launch = base._launch          # (variant None: no igemm launch at all; a tuple: one variant of these)


def gn_ppc(HW: int) -> int:
    """norm.hip gn_ppc: pixels per chunk of the statistics read pass."""
    return 256 if HW >= 32768 else 128 if HW >= 8192 else 32 if HW >= 2048 else 16


def _hw(y):
    return y.numel() // (y.shape[0] * y.shape[-1])


# ---- the assertions ------------------------------------------------------------------------------------------------------------------

def assert_exact_sums(partial, G, S, Q, what):
    """Assertion 2: the raw partials folded over slots and entries equal the exact sums, bit for bit."""
    s, q = dp.fold_partials(partial, G)
    S, Q = S.to(s.device), Q.to(s.device)
    if torch.equal(s, S) and torch.equal(q, Q):
        return
    bad = ((s != S) | (q != Q)).nonzero()
    n, g = bad[0].tolist()
    epg = partial.shape[2] // G
    slots = partial[n, :, g * epg:(g + 1) * epg].double().sum(1)          # [nslot, 2]
    odd = (~torch.isfinite(slots).all(-1)).nonzero().flatten().tolist()[:8]
    raise AssertionError(f"{what}: the folded partials differ from the exact sums in {bad.shape[0]} of {S.numel()} (image, group) pairs, first at "
                         f"{bad[:4].tolist()}: sum {float(s[n, g])!r} (exact {float(S[n, g])!r}), squares {float(q[n, g])!r} (exact {float(Q[n, g])!r}); "
                         f"{partial.shape[1]} slots x {partial.shape[2]} entries, non-finite slots of that group: {odd}")


def assert_finalised(stats, S, Q, count, what, ref=None):
    """Assertion 3: (mean, rstd, var) of a finaliser against the float64 restatement: mean bit-equal, var and rstd within 1 fp32 ulp."""
    mean, rstd, var = stats
    m, v, r = ref if ref is not None else dp.finalize_ref(S, Q, count, EPS)
    m, v, r = (t.to(mean.device).float() for t in (m, v, r))
    if ref is None:
        base._eq(mean, m, f"{what}: mean")
    else:
        assert int(dp.ulps32(mean, m).max()) <= 1, f"{what}: mean is {int(dp.ulps32(mean, m).max())} fp32 ulps from the restatement"
    assert bool((v > 0).all()) and bool(torch.isfinite(var).all()) and bool(torch.isfinite(rstd).all())
    dv, dr = int(dp.ulps32(var, v).max()), int(dp.ulps32(rstd, r).max())
    print(f"{what}: var {dv} ulp, rstd {dr} ulp from the float64 restatement")
    assert dv <= 1, f"{what}: var is {dv} fp32 ulps from the float64 restatement (the derived bound is 1)"
    assert dr <= 1, f"{what}: rstd is {dr} fp32 ulps from the float64 restatement (the derived bound is 1)"


def _budget(exact, G, slot_elems, dtype, handle):
    """StatsBudget for the producer's own partials and, where the read pass serves the tensor instead, for that pass's chunks."""
    dp.StatsBudget(exact, G, slot_elems, dtype).check()
    if not handle:
        dp.StatsBudget(exact, G, gn_ppc(_hw(exact)) * (exact.shape[-1] // G), dtype).check()


def probe_producer(launch, variant, producer, exacts, G, slot_elems, dtype, what, handle=True, entries=None):
    """Assertions 1 - 4 for a producer() that returns one tensor or a list of them; `exacts`: the float64 restatement(s) before the output rounding.
    handle=False: the producer is documented to leave NO partials; the read pass over the tensor then gives the exact statistics.
    entries: "group" | "channel" - the form of the entries the producer must write."""
    ops = _ops()
    many = isinstance(exacts, (list, tuple))
    exacts = list(exacts) if many else [exacts]
    for ex in exacts:
        _budget(ex, G, slot_elems, dtype, handle)
    sums = [dp.group_sums(ex, G) for ex in exacts]
    run = (lambda: list(producer())) if many else (lambda: [producer()])
    ys = launch(variant, run)
    for k, (y, ex, (S, Q)) in enumerate(zip(ys, exacts, sums)):
        tag = f"{what}[{k}]" if many else what
        base._eq(y, dp.rounded(ex, dtype), tag)
        h = getattr(y, "_omgsr_gn", None)
        count = float(_hw(ex) * (ex.shape[-1] // G))
        if handle:
            assert h is not None, f"{tag}: the producer left no statistics handle"
            assert h.groups == G and h.partial.shape[0] == y.shape[0]
            if entries is not None:
                want = G if entries == "group" else y.shape[-1]
                assert h.partial.shape[2] == want, f"{tag}: {h.partial.shape[2]} entries per slot, expected {want} (one per {entries})"
            print(f"{tag}: partials {tuple(h.partial.shape)}")
            assert_exact_sums(h.partial, G, S, Q, tag)
        else:
            assert h is None, f"{tag}: this producer is documented to leave no statistics, it left {tuple(h.partial.shape)}"
            assert_exact_sums(ops.group_norm_partial(y, G), G, S, Q, f"{tag} (read pass)")
        assert_finalised(ops.group_norm_stats(y, G, EPS), S, Q, count, tag)
    with gb.fenced_outputs():
        ys2 = run()
        parts = [getattr(y, "_omgsr_gn").partial if handle else ops.group_norm_partial(y, G) for y in ys2]
    for k, (y, ex, (S, Q), part) in enumerate(zip(ys2, exacts, sums, parts)):
        base._eq(y, dp.rounded(ex, dtype), f"{what}[{k}] (fenced outputs)")
        assert_exact_sums(part, G, S, Q, f"{what}[{k}] (partials pre-filled with the fence pattern)")
    return ys


# ---- conv / GEMM producers through omgsr_igemm ----------------------------------------------------------------------------------------------

_SPLIT = {"16": (1, 1), "split": (2, 2), "mx": (3, 1), "mx6": (4, 1)}


def _conv_data(g, dev, shape, Cout, G, *, R=3, nnz=2, wmant=(1, 3), form="16", phases=False, ce=None):
    """Statistics-friendly conv operands: x [N, H, W, Cin] with one exponent per image, w with one per output group (dyadic_probe.stats_*),
    bias an odd multiple of half the product quantum. Returns (operand on dev, packed weight, per-channel exponents)."""
    ops = _ops()
    ce = dp.group_exponents(g, G, Cout) if ce is None else ce
    x = dp.stats_act(g, shape)
    w = dp.stats_wt(g, ce, shape[-1], R, R, nnz, wmant)
    split, w_split = _SPLIT[form]
    pw = ops.pack_conv_weight(w, dp.stats_bias(g, ce), device=dev, split=split, w_split=w_split, upsample_phases=phases)
    return dp.host_operand(x, form, ops.act_dtype()).to(dev), pw, ce


def _planned(x, pw, G, *, stride=1, pad=1, upsample=False, residual=False):
    """(slots, entries) omgsr_igemm plans for the statistics of this 16-bit conv problem, as ops._conv_gn asks: host-side code that reads the
    geometry only (no pointer is followed), so the dry run checks it too."""
    from omgsr_amd import _lib
    ops = _ops()
    a = _lib.IgemmArgs()
    ops._fill_weight(a, pw, x.data_ptr())
    a.weight_ph = pw.w_ph.data_ptr() if upsample and pw.w_ph is not None else None
    N, H, W, _ = x.shape
    pt, pb, pl, pr = (pad,) * 4 if isinstance(pad, int) else pad
    Hv, Wv = (2 * H, 2 * W) if upsample else (H, W)
    a.N, a.H, a.W, a.Ho, a.Wo = N, H, W, (Hv + pt + pb - pw.R) // stride + 1, (Wv + pl + pr - pw.S) // stride + 1
    a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample = pw.R, pw.S, stride, pt, pl, int(upsample)
    a.out, a.out_dtype, a.alpha, a.batch, a.sample_rows, a.gn_groups = x.data_ptr(), ops.OUT_BF16, 1.0, 1, a.Ho * a.Wo, G
    if residual:
        a.residual, a.res_el = x.data_ptr(), ops.EL_16
    lib = _lib.load()
    if lib.omgsr_igemm_workspace_bytes(C.byref(a)) > 0:
        return 0, 0
    return lib.omgsr_igemm_gn_slots(C.byref(a)), lib.omgsr_igemm_gn_entries(C.byref(a))


def _halo(dev, launch, variant, shape, Cout, G, seed, *, residual=False, nnz=2, wmant=(1, 3), form="16", slots=None, entries="group"):
    """One 3x3 stride-1 conv on the halo-tile kernel (spatial or FLAT form, told by `slots` per image)."""
    ops = _ops()
    g = base._g(seed)
    N, H, W, _ = shape
    x, pw, ce = _conv_data(g, dev, shape, Cout, G, nnz=nnz, wmant=wmant, form=form)
    r = dp.stats_residual(g, (N, H, W, Cout), ce).to(dev, ops.stream_dtype()) if residual else None
    exact = dp.conv_ref(x, pw, bias=pw.bias, residual=r)
    gsz = Cout // G
    if slots is not None and form == "16":
        want = {"spatial": 2 * -(-W // 32) * -(-H // 8), "flat": 2 * -(-(H * (W + 2)) // 256)}[slots]
        got = _planned(x, pw, G, residual=residual)
        assert got == (want, G if entries == "group" else Cout), f"the library plans {got} (slots, entries), the {slots} form has {want}"
    probe_producer(launch, variant, lambda: ops.conv2d(x, pw, pad=1, residual=r, gn_groups=G), exact, G,
                   WAVE_PIXELS * (gsz if entries == "group" else 1), ops.stream_dtype(), f"halo {shape} -> {Cout}, G {G}", entries=entries)


def s3_spatial_gsz4_ragged(dev, launch):
    """bf16; 11 maps of 43 x 86 (3 x 6 tiles each, ragged both ways), 64 -> 128, G 32: group size 4, two groups per lane octet; residual."""
    _halo(dev, launch, 3, (11, 43, 86, 64), 128, 32, 9301, residual=True, slots="spatial")


def s3_flat_gsz4_ragged(dev, launch):
    """fp16; 12 maps of 86 x 43: the FLAT form (16 runs of 256 padded positions per image, the last partial), 64 -> 128, G 32, no residual."""
    _halo(dev, launch, 3, (12, 86, 43, 64), 128, 32, 9302, slots="flat")


def s3_spatial_gsz8(dev, launch):
    """bf16; Cout 256, G 32: group size 8 (one lane octet per group, no butterfly step), two column tiles; residual."""
    _halo(dev, launch, 3, (6, 43, 86, 64), 256, 32, 9303, residual=True, slots="spatial")


def s3_spatial_gsz16(dev, launch):
    """fp16; Cout 512, G 32: group size 16 (one butterfly step, the even octet writes), four column tiles."""
    _halo(dev, launch, 3, (3, 43, 86, 64), 512, 32, 9304, slots="spatial")


def s3_spatial_gsz64(dev, launch):
    """bf16; Cout 512, G 8: group size 64 (three butterfly steps: a whole 64-column wave tile is one group); residual. One nonzero tap of +-1 per
    output keeps 128 x 64 values inside the budget."""
    _halo(dev, launch, 3, (3, 43, 86, 64), 512, 8, 9305, residual=True, nnz=1, wmant=(1, 1), slots="spatial")


def s3_spatial_gsz10_per_channel(dev, launch):
    """bf16; Cout 320 (Cout_pad 384: the last column tile is half padding), G 32: group size 10, per-channel entries folded ten at a time; residual."""
    _halo(dev, launch, 3, (4, 43, 86, 64), 320, 32, 9306, residual=True, slots="spatial", entries="channel")


def s3_spatial_gsz1_per_channel(dev, launch):
    """fp16; Cout 128, G 128: group size 1 - per channel IS per group (the epilogue takes its per-channel branch)."""
    _halo(dev, launch, 3, (11, 43, 86, 64), 128, 128, 9307, slots="spatial", entries="channel")


def s3_split_fp32_residual(dev, launch):
    """Accurate tier; two-term split operand and weight, fp32 output with an fp32 residual (the RES32 epilogue), group size 4."""
    _halo(dev, launch, 3, (11, 43, 86, 64), 128, 32, 9308, residual=True, form="split")


def s3_mx_fp32_residual(dev, launch):
    """Accurate tier; MX fp8 operand (144 tiles: above the halo split-K's 128), fp32 output and residual, group size 4."""
    _halo(dev, launch, 3, (8, 43, 86, 128), 128, 32, 9309, residual=True, form="mx")


def s13_mx6_fp32_residual_per_channel(dev, launch):
    """Accurate tier; fp6 correction chunks, Cout 320 / G 32: per-channel entries from the fp32 epilogue; fp32 residual."""
    _halo(dev, launch, 13, (3, 43, 86, 128), 320, 32, 9310, residual=True, form="mx6", entries="channel")


# ---- phase form and launch groups (variants 6, 7, 8, 16) ---------------------------------------------------------------------------------

def _phase(dev, launch, variant, shape, Cout, G, seed, form="16"):
    ops = _ops()
    g = base._g(seed)
    x, pw, _ = _conv_data(g, dev, shape, Cout, G, form=form, phases=True)
    exact = dp.phase_conv_ref(x, pw, bias=pw.bias)
    N, H, W, _ = shape
    if form == "16":
        assert _planned(x, pw, G, upsample=True) == (8 * -(-W // 32) * -(-H // 8), G), "one slot per (wave tile, phase)"
    probe_producer(launch, variant, lambda: ops.conv2d(x, pw, pad=1, upsample=True, gn_groups=G), exact, G, WAVE_PIXELS * (Cout // G),
                   ops.stream_dtype(), f"phase {shape} -> {Cout}", entries="group")


def s6_phase_ragged(dev, launch):
    """bf16; the phase form on two 43 x 150 low-resolution maps (240 phase tiles, ragged both ways), 64 -> 128, G 32: [tile][wm][4 phases] slots."""
    _phase(dev, launch, 6, (2, 43, 150, 64), 128, 32, 9601)


def s16_phase_mx6(dev, launch):
    """Accurate tier; fp6 chunks in the phase form, fp32 output."""
    _phase(dev, launch, 16, (1, 32, 48, 128), 128, 32, 9602, form="mx6")


def _multi(dev, launch, variant, groups, Cin, Cout, G, ups, seed, residual=False):
    ops = _ops()
    g = base._g(seed)
    ce = dp.group_exponents(g, G, Cout)
    pw = ops.pack_conv_weight(dp.stats_wt(g, ce, Cin), dp.stats_bias(g, ce), device=dev, upsample_phases=ups)
    xs, rs, exacts = [], [], []
    for n, h, w in groups:
        x = dp.stats_act(g, (n, h, w, Cin)).to(dev, ops.act_dtype())
        r = dp.stats_residual(g, (n, h, w, Cout), ce).to(dev, ops.stream_dtype()) if residual else None
        exacts.append(dp.phase_conv_ref(x, pw, bias=pw.bias) if ups else dp.conv_ref(x, pw, bias=pw.bias, residual=r))
        xs.append(x), rs.append(r)
    probe_producer(launch, variant, lambda: ops.conv2d_multi(xs, pw, pad=1, upsample=ups, residuals=rs if residual else None, gn_groups=G),
                   exacts, G, WAVE_PIXELS * (Cout // G), ops.stream_dtype(), f"launch group {groups}", entries="group")


def s7_multi_ragged_groups(dev, launch):
    """bf16; the four tile-shape groups of a tiled-VAE layer in one launch (the group plans the FLAT form: 40- and 32-wide maps), residual; every
    row of every member is an image of its own for the statistics."""
    _multi(dev, launch, 7, [(36, 40, 40), (12, 40, 32), (12, 32, 40), (4, 32, 32)], 64, 128, 32, False, 9701, residual=True)


def s8_multi_phase_ragged_groups(dev, launch):
    """bf16; the phase form over three unequal groups in one launch (43-row maps: the last tile row holds 3 of 8 rows), Cout 256: group size 8."""
    _multi(dev, launch, 8, [(4, 43, 32), (4, 32, 32), (2, 43, 64)], 64, 256, 32, True, 9801)


# ---- GEMM-shaped kernels: one slot per 32-row block ----------------------------------------------------------------------------------------

def s1_stride2_gsz4(dev, launch):
    """bf16; a stride-2 conv (asymmetric pad) on the register-staged kernel: Ho Wo = 256 per image, eight 32-row slots, group size 4; residual."""
    ops = _ops()
    g = base._g(9101)
    N, Cout, G = 2, 128, 32
    x, pw, ce = _conv_data(g, dev, (N, 32, 32, 128), Cout, G)
    r = dp.stats_residual(g, (N, 16, 16, Cout), ce).to(dev, ops.stream_dtype())
    exact = dp.conv_ref(x, pw, stride=2, pad=(0, 1, 0, 1), bias=pw.bias, residual=r)
    assert _planned(x, pw, G, stride=2, pad=(0, 1, 0, 1), residual=True) == (8, G)
    probe_producer(launch, 1, lambda: ops.conv2d(x, pw, stride=2, pad=(0, 1, 0, 1), residual=r, gn_groups=G), exact, G, BLOCK_ROWS * 4,
                   ops.stream_dtype(), "stride-2 conv", entries="group")


def s1_stride2_ragged_no_handle(dev, launch):
    """fp16; the same conv on 33 x 35 maps: Ho Wo = 16 x 17 = 272 is no multiple of 32, a row block would straddle images - NO handle; the read
    pass (272 pixels: 17 chunks of 16) gives the exact statistics."""
    ops = _ops()
    g = base._g(9102)
    N, Cout, G = 3, 128, 32
    x, pw, _ = _conv_data(g, dev, (N, 33, 35, 64), Cout, G)
    exact = dp.conv_ref(x, pw, stride=2, pad=(0, 1, 0, 1), bias=pw.bias)
    assert tuple(exact.shape) == (N, 16, 17, Cout) and _planned(x, pw, G, stride=2, pad=(0, 1, 0, 1)) == (0, 0)
    probe_producer(launch, 1, lambda: ops.conv2d(x, pw, stride=2, pad=(0, 1, 0, 1), gn_groups=G), exact, G, BLOCK_ROWS * 4, ops.stream_dtype(),
                   "ragged stride-2 conv", handle=False)


def _linear(dev, launch, variant, B, L, K, Cout, G, seed, *, residual=False, form="16", handle=True, entries="channel", nnz=2):
    """ops.linear on [B, L, K]: B images of L rows."""
    ops = _ops()
    g = base._g(seed)
    ce = dp.group_exponents(g, G, Cout)
    x = dp.host_operand(dp.stats_act(g, (B, L, K)), form, ops.act_dtype()).to(dev)
    split, w_split = _SPLIT[form]
    pw = ops.pack_linear_weight(dp.stats_wt(g, ce, K, 1, 1, nnz)[:, :, 0, 0], dp.stats_bias(g, ce), device=dev, split=split, w_split=w_split)
    r = dp.stats_residual(g, (B, L, Cout), ce).to(dev, ops.stream_dtype()) if residual else None
    exact = dp.conv_ref(x.reshape(1, 1, B * L, x.shape[-1]), pw, pad=(0, 0, 0, 0), bias=pw.bias,
                        residual=None if r is None else r.reshape(B * L, Cout)).reshape(B, L, Cout)
    gsz = Cout // G
    probe_producer(launch, variant, lambda: ops.linear(x, pw, residual=r, gn_groups=G), exact, G,
                   BLOCK_ROWS * (gsz if entries == "group" else 1), ops.stream_dtype(), f"linear [{B}, {L}, {K}] -> {Cout}, G {G}",
                   handle=handle, entries=entries if handle else None)


def s2_conv1x1_residual_gsz10(dev, launch):
    """bf16; a 1x1 conv with a residual (the attention block's proj_out shape) on [2, 16, 16, 320] -> 320, G 32: per-channel entries, group size 10;
    512 rows of K = 320: the LDS-DMA kernel."""
    ops = _ops()
    g = base._g(9103)
    N, H, W, Cc, G = 2, 16, 16, 320, 32
    x, pw, ce = _conv_data(g, dev, (N, H, W, Cc), Cc, G, R=1)
    r = dp.stats_residual(g, (N, H, W, Cc), ce).to(dev, ops.stream_dtype())
    exact = dp.conv_ref(x, pw, pad=(0, 0, 0, 0), bias=pw.bias, residual=r)
    assert _planned(x, pw, G, pad=0, residual=True) == (H * W // 32, Cc)
    probe_producer(launch, 2, lambda: ops.conv2d(x, pw, pad=0, residual=r, gn_groups=G), exact, G, BLOCK_ROWS, ops.stream_dtype(),
                   "1x1 conv + residual", entries="channel")


def s1_linear_gsz1(dev, launch):
    """fp16; linear on [3, 96, 64] -> 64 with G 64: group size 1, three slots per image."""
    _linear(dev, launch, 1, 3, 96, 64, 64, 64, 9104, residual=True)


def s2_linear_gsz2_partial_tile(dev, launch):
    """bf16; the LDS-DMA kernel on [5, 224, 320] -> 128 with G 64: group size 2 (per-channel entries, two per group); M = 1120 rows: the last
    256-row tile holds 96."""
    _linear(dev, launch, 2, 5, 224, 320, 128, 64, 9201)


def s4_splitk_no_handle(dev, launch):
    """bf16; [2, 160, 2048] -> 256: split over K - the reduce pass leaves NO handle (160 % 32 == 0, so only the split decides); read pass."""
    _linear(dev, launch, 4, 2, 160, 2048, 256, 32, 9401, residual=True, handle=False, nnz=4)


def s5_p8_gsz2_partial_tile(dev, launch):
    """bf16; the ping-pong kernel: 3 images of 10976 rows (343 row blocks each; M = 32928: the 129th 256-row tile holds 160), K 640 -> 256, G 128:
    group size 2; residual."""
    _linear(dev, launch, 5, 3, 10976, 640, 256, 128, 9501, residual=True)


def s5_p8_mx_gsz8(dev, launch):
    """Accurate tier; the MX fp8 operand through the ping-pong kernel, fp32 output and residual, G 32 of 256: group size 8, one entry per group."""
    _linear(dev, launch, 5, 3, 10976, 320, 256, 32, 9502, residual=True, form="mx", entries="group")


# ---- MXFP8 convs (bf16 tier) ---------------------------------------------------------------------------------------------------------------

def _f8(v):
    return v.to(torch.float8_e4m3fn).view(torch.uint8)


def _mx_planes(g, shapes, Cin, Cout, G, nnz=2):
    """Statistics-friendly MXFP8 planes: operand codes +-{1..3} (dense) with ONE scale byte 127 + e[image], weight codes +-{1..3} at nnz
    (tap, channel) positions per output with ONE scale byte 127 + ce[cout]: every product of an 8-wide K group lies within a factor 9 (the
    instruction's 2^13 window), every output is an integer times 2^(e + ce). Returns ([(codes, scales)], wc [Cout, 9, Cin], wsc, ce)."""
    ce = dp.group_exponents(g, G, Cout)
    xs = []
    for shape in shapes:
        x = dp.stats_act(g, (*shape, Cin), img_e=(0, 0))
        e = (torch.arange(shape[0]) + int(torch.randint(0, 2, (1,), generator=g))) % 2
        xs.append((_f8(x), (127 + e).reshape(-1, 1, 1, 1).expand(*shape, Cin // 32).contiguous().to(torch.uint8)))
    w = dp.stats_wt(g, torch.zeros(Cout), Cin, 3, 3, nnz).permute(0, 2, 3, 1).reshape(Cout, 9, Cin)
    wsc = (127 + ce).reshape(Cout, 1, 1).expand(Cout, 9, Cin // 32).contiguous().to(torch.uint8)
    return xs, _f8(w), wsc, ce


def _mx_window_by_construction(codes, scales, rows):
    """One scale byte per operand pixel / weight row and code magnitudes in 1 .. 3: the products of any K group lie within a factor 9."""
    mag = dp.e4m3(codes).abs()
    assert float(mag.max()) <= 3.0 and float(mag[mag > 0].min()) >= 1.0
    sc = scales.reshape(-1, scales.shape[-1]) if scales.dim() == 4 and rows is None else scales[:rows].reshape(rows, -1)
    assert bool((sc == sc[:, :1]).all()), "one scale byte per row"


def _mx_exact(V, xq, pw, Cout, r):
    """The exact conv from the bytes (test_fp8_vae_gpu.conv_mxfp8_ref) without its per-K-group window scan (hundreds of [M, Cout, 8] tensors at
    these sizes): the 2^13 window holds by construction, asserted above; an output sums at most two products of at most 9 quanta."""
    uc, us = V.unpack_planes(pw)
    _mx_window_by_construction(xq.codes, xq.scales, None)
    _mx_window_by_construction(uc, us, Cout)
    return V.conv_mxfp8_ref(xq.codes, xq.scales, uc, us, Cout, bias=pw.bias, residual=r, check=False)


def _mx_conv(dev, launch, variant, shapes, Cin, Cout, G, seed, *, deep=False, residual=False, entries="group"):
    import test_fp8_vae_gpu as V
    ops = _ops()
    g = base._g(seed)
    planes, wc, wsc, ce = _mx_planes(g, shapes, Cin, Cout, G)
    pw = V.pack_planes(wc, wsc, dp.stats_bias(g, ce), dev)
    xqs = [ops.Mxfp8(c.to(dev), s.to(dev)) for c, s in planes]
    rs = [dp.stats_residual(g, (*shape, Cout), ce).to(dev, torch.bfloat16) if residual else None for shape in shapes]
    exacts = [_mx_exact(V, xq, pw, Cout, r) for xq, r in zip(xqs, rs)]
    slot = WAVE_PIXELS * ((Cout // G) if entries == "group" else 1)
    if len(shapes) == 1:
        probe_producer(launch, variant, lambda: ops.conv2d_mxfp8(xqs[0], pw, residual=rs[0], gn_groups=G, deep=deep), exacts[0], G, slot,
                       torch.bfloat16, f"mxfp8 conv {shapes[0]} x {Cin} -> {Cout}", entries=entries)
    else:
        probe_producer(launch, variant, lambda: ops.conv2d_mxfp8_multi(xqs, pw, residuals=rs if residual else None, gn_groups=G), exacts, G, slot,
                       torch.bfloat16, f"mxfp8 conv group {shapes} x {Cin} -> {Cout}", entries=entries)


def s21_mxfp8_conv(dev, launch):
    """bf16 tier; mxfp8_conv_kernel on six ragged 45 x 86 maps, 128 -> 256 (216 tiles), G 32: group size 8; bf16 residual."""
    _mx_conv(dev, launch, 21, [(6, 45, 86)], 128, 256, 32, 9211, residual=True)


def s22_mxfp8_conv_multi(dev, launch):
    """bf16 tier; four tile-shape groups served as ONE launch of mxfp8_conv_multi_kernel where none is served alone (200 tiles)."""
    _mx_conv(dev, launch, 22, [(2, 45, 86), (2, 45, 64), (2, 32, 86), (2, 32, 64)], 128, 256, 32, 9221)


def s27_mxfp8_deep_c320(dev, launch):
    """bf16 tier; the deep-K kernel at 320 -> 320 (five 64-channel chunks, Cout_pad 384), G 32: group size 10, per-channel entries; residual."""
    _mx_conv(dev, launch, 27, [(4, 45, 86)], 320, 320, 32, 9271, deep=True, residual=True, entries="channel")


def s27_mxfp8_deep_c960(dev, launch):
    """bf16 tier; the deep-K kernel at 320 -> 960 (eight column tiles, the last half padding), G 32: group size 30, per-channel entries."""
    _mx_conv(dev, launch, 27, [(2, 45, 86)], 320, 960, 32, 9272, deep=True, entries="channel")


def s25_mxfp8_up(dev, launch):
    """bf16 tier; mxfp8_conv_up_kernel (phase form) on ragged 44 x 72 low-resolution maps, 128 -> 256, G 32: the 16-bit phase form's slot layout.
    The four phase kernels are given directly as planes (codes +-{1..3} at two (tap, channel) positions per (phase, output))."""
    import test_fp8_vae_upsample_gpu as U
    ops = _ops()
    g = base._g(9251)
    Cin, Cout, G = 128, 256, 32
    N, H, W = U.served_shape(Cin, Cout)
    ce = dp.group_exponents(g, G, Cout)
    x = dp.stats_act(g, (N, H, W, Cin), img_e=(0, 0))
    e = (torch.arange(N) + 1) % 2
    xq = ops.Mxfp8(_f8(x).to(dev), (127 + e).reshape(N, 1, 1, 1).expand(N, H, W, Cin // 32).contiguous().to(torch.uint8).to(dev))
    wc = torch.stack([_f8(dp.stats_wt(g, torch.zeros(Cout), Cin, 2, 2).permute(0, 2, 3, 1).reshape(Cout, 4, Cin)) for _ in range(4)])
    wsc = (127 + ce).reshape(1, Cout, 1, 1).expand(4, Cout, 4, Cin // 32).contiguous().to(torch.uint8)
    pw = U.pack_up_planes(wc, wsc, dp.stats_bias(g, ce), Cout, dev)
    uc, us = U.unpack_up_planes(pw)
    _mx_window_by_construction(xq.codes, xq.scales, None)
    A, Sc = U._phase_operands(xq.codes), U._phase_operands(xq.scales, 127)
    phases = []
    for ph in range(4):           # U.mxfp8_phase_ref without the per-K-group window scan (by construction, as in _mx_exact)
        _mx_window_by_construction(uc[ph], us[ph], Cout)
        phases.append(dp.mxfp8_ref(torch.cat([A[(ph, t)] for t in range(4)], -1), torch.cat([Sc[(ph, t)] for t in range(4)], -1),
                                   uc[ph].reshape(uc.shape[1], -1), us[ph].reshape(us.shape[1], -1), Cout, bias=pw.bias, check=False))
    exact = U._interleave(phases, N, H, W, Cout)
    probe_producer(launch, 25, lambda: ops.conv2d_mxfp8_up(xq, pw, gn_groups=G), exact, G, WAVE_PIXELS * (Cout // G), torch.bfloat16,
                   f"mxfp8 up-sampling conv {(N, H, W)} x {Cin} -> {Cout}", entries="group")


# ---- the GroupNorm-fused producer (variants 10 / 11) ------------------------------------------------------------------------------------------

def s10_gn_fused(dev, launch):
    """bf16; the normalising patch producer: base.v10_gn_fused_identity_silu's output probe plus the statistics its epilogue leaves."""
    x, pw, spec, exact, G = base.gn_fused_case(dev, [(4, 96, 160)], 2, 1002)
    ops = _ops()
    probe_producer(launch, 10, lambda: ops.conv2d(x[0], pw, pad=1, gn=spec(), gn_groups=G), exact[0], G, WAVE_PIXELS * (pw.cout // G),
                   ops.stream_dtype(), "GroupNorm-fused conv", entries="group")


def s11_gn_fused_multi(dev, launch):
    """bf16; the same producer in a launch group of two tile shapes."""
    xs, pw, spec, exacts, G = base.gn_fused_case(dev, [(2, 96, 160), (2, 96, 128)], 2, 1102)
    ops = _ops()
    probe_producer(launch, 11, lambda: ops.conv2d_multi(xs, pw, pad=1, gn=spec(), gn_groups=G), exacts, G, WAVE_PIXELS * (pw.cout // G),
                   ops.stream_dtype(), "GroupNorm-fused launch group", entries="group")


# ---- the read pass ----------------------------------------------------------------------------------------------------------------------------------

def _read_pass(dev, launch, N, HW, Cc, G, seed, f32):
    """ops.group_norm_stats on a tensor without a handle: gn_partial_kernel's chunks and thread map, then gn_finalize_kernel."""
    ops = _ops()
    g = base._g(seed)
    dtype = torch.float32 if f32 else ops.act_dtype()
    ce = dp.group_exponents(g, G, Cc)
    exact = dp.stats_values(g, (N, HW, Cc), ce).double()
    ppc = gn_ppc(HW)
    dp.StatsBudget(exact, G, ppc * (Cc // G), dtype).check()
    S, Q = dp.group_sums(exact, G)
    y = exact.to(dtype).to(dev)
    what = f"read pass [{N}, {HW}, {Cc}] G {G} ({'fp32' if f32 else '16-bit'}; {ppc} pixels per chunk, {-(-HW // ppc)} chunks)"
    part = launch(None, lambda: ops.group_norm_partial(y.clone(), G))
    assert tuple(part.shape) == (N, -(-HW // ppc), G, 2)
    assert_exact_sums(part, G, S, Q, what)
    assert_finalised(ops.group_norm_stats(y.clone(), G, EPS), S, Q, float(HW * (Cc // G)), what)
    with gb.fenced_outputs():
        part = ops.group_norm_partial(y, G)
    assert_exact_sums(part, G, S, Q, what + " (partials pre-filled with the fence pattern)")


# (HW, C, G): every pixels-per-chunk regime, HW below the pixel lanes P = 256 / min(C / 8, 256), idle threads at C = 320, the octet loop at C > 2048
READ_16 = {
    "hw5_c32_g32": (5, 32, 32),              # P = 64 pixel lanes, five pixels; G = C
    "hw100_c320_g32": (100, 320, 32),        # 16 per chunk, the last chunk holds 4; TP = 40, P = 6: 16 idle threads
    "hw2065_c512_g32": (2065, 512, 32),      # 32 per chunk, the last holds 17
    "hw8192_c256_g256": (8192, 256, 256),    # 128 per chunk; G = C = 256 (the most groups the pass takes)
    "hw2048_c2304_g32": (2048, 2304, 32),    # C > 2048: every thread walks two octets
}
READ_32 = {
    "hw70_c2304_g32": (70, 2304, 32),        # fp32 rows, the octet loop, 16 per chunk with 6 left over
    "hw32773_c32_g32": (32773, 32, 32),      # 256 per chunk, the last holds 5; G = C
    "hw9000_c320_g32": (9000, 320, 32),      # 128 per chunk, the last holds 40
}


def _read_probe(HW, Cc, G, seed, f32):
    return lambda dev, launch: _read_pass(dev, launch, 2, HW, Cc, G, seed, f32)


# ---- finalisers ---------------------------------------------------------------------------------------------------------------------------------------

def _pair(dev, launch, kinds, seed):
    """group_norm_pair_stats over [a | b] with (Ca, Cb) = (640, 320), G 32: 30 channels per group, group 21 straddles the seam (630 .. 659).
    The exponent is per group of the CONCATENATION, so the straddling group keeps one quantum across both tensors."""
    ops = _ops()
    g = base._g(seed)
    N, H, W, Ca, Cb, G = 16, 32, 32, 640, 320, 32
    ce = dp.group_exponents(g, G, Ca + Cb)

    def halo(Cin, c):
        x, pw, _ = _conv_data(g, dev, (N, H, W, Cin), c.numel(), G, ce=c)
        return (lambda: ops.conv2d(x, pw, pad=1, gn_groups=G)), dp.conv_ref(x, pw, bias=pw.bias)

    def gemm(Cin, c):
        x = dp.stats_act(g, (N, H * W, Cin)).to(dev, ops.act_dtype())
        pw = ops.pack_linear_weight(dp.stats_wt(g, c, Cin, 1, 1)[:, :, 0, 0], dp.stats_bias(g, c), device=dev)
        r = dp.stats_residual(g, (N, H * W, c.numel()), c).to(dev, ops.stream_dtype())
        exact = dp.conv_ref(x.reshape(1, 1, N * H * W, Cin), pw, pad=(0, 0, 0, 0), bias=pw.bias, residual=r.reshape(N * H * W, -1))

        def run():
            y = ops.linear(x, pw, residual=r, gn_groups=G)
            return ops.carry_gn(y, y.reshape(N, H, W, c.numel()))
        return run, exact.reshape(N, H, W, c.numel())

    make = {"halo": halo, "gemm": gemm}
    ka, kb = kinds.split("|")
    run_a, ex_a = make[ka](32, ce[:Ca])
    run_b, ex_b = make[kb](32, ce[Ca:])
    exact = torch.cat([ex_a, ex_b], -1)
    # every fp32 partial is per channel: 128 pixels of a wave tile or 32 rows of a row block
    dp.StatsBudget(exact, G, WAVE_PIXELS, torch.float32).check()
    S, Q = dp.group_sums(exact, G)
    want = {"halo": 3, "gemm": (1, 2, 5)}
    a = launch(want[ka], run_a)
    b = launch(want[kb], run_b)
    base._eq(a, dp.rounded(ex_a, torch.float32), "a")
    base._eq(b, dp.rounded(ex_b, torch.float32), "b")
    for t in (a, b):
        assert t._omgsr_gn.partial.shape[2] == t.shape[-1], "the producer should have left per-channel statistics"
    # the seam: fold a's and b's per-channel partials into the concatenation's groups
    pa, pb = a._omgsr_gn.partial.double().sum(1), b._omgsr_gn.partial.double().sum(1)
    cat = torch.cat([pa, pb], 1).reshape(N, G, (Ca + Cb) // G, 2).sum(2)
    assert torch.equal(cat[..., 0], S.to(cat.device)) and torch.equal(cat[..., 1], Q.to(cat.device)), "per-channel partials of the pair differ from the exact sums"
    st = ops.group_norm_pair_stats(a, b, G, EPS)
    assert st is not None, "the two-source path must be taken"
    assert_finalised(st, S, Q, float(H * W * (Ca + Cb) // G), f"pair {kinds}")


def f2_pair_halo_gemm(dev, launch):
    """Accurate tier; finalize2 over a halo-tile producer (640 channels) and a GEMM-shaped one (320, with residual)."""
    _pair(dev, launch, "halo|gemm", 9901)


def f2_pair_gemm_halo(dev, launch):
    """Accurate tier; the other producer order: slot counts and layouts differ between a and b."""
    _pair(dev, launch, "gemm|halo", 9902)


def fm_merged_two_tile_shapes(dev, launch):
    """bf16; group_norm_stats_merged over two tile-shape groups, 2 tiles of 32 x 32 and 4 of 16 x 32 for each of N = 2 images (tile-major rows), group
    size 4: the pixel weights 1024 / 4096 and 512 / 4096 and the per-tile counts 4096 and 2048 are powers of two. Against the float64 restatement
    of the merge formula (include/omgsr_hip.h): mean = sum over (shape, tile) of weight m, var = sum of weight max(q / count - m^2, 0); <= 1 fp32
    ulp on all three (the sums run in a different order in double). Both tensors' partials come from the read pass."""
    ops = _ops()
    g = base._g(9903)
    N, Cc, G = 2, 128, 32
    shapes, tiles = [(32, 32), (16, 32)], [2, 4]
    ce = dp.group_exponents(g, G, Cc)
    ys, parts = [], []
    tot = float(sum(h * w * t for (h, w), t in zip(shapes, tiles)))
    for (h, w), t in zip(shapes, tiles):
        exact = dp.stats_values(g, (t * N, h * w, Cc), ce).double()
        dp.StatsBudget(exact, G, gn_ppc(h * w) * (Cc // G), ops.act_dtype()).check()
        S, Q = dp.group_sums(exact, G)
        parts.append((S.reshape(t, N, G), Q.reshape(t, N, G), float(h * w * (Cc // G)), h * w / tot))
        ys.append(exact.to(ops.act_dtype()).reshape(t * N, h, w, Cc))
    ref = dp.merged_ref(parts, EPS)
    assert bool((ref[1] > 0).all())
    ys = [y.to(dev) for y in ys]
    st = launch(None, lambda: ops.group_norm_stats_merged(ys, tiles, N, G, EPS))
    assert_finalised(st, None, None, None, "merged statistics", ref=ref)
    with gb.fenced_outputs():
        st2 = ops.group_norm_stats_merged(ys, tiles, N, G, EPS)
    assert all(torch.equal(a, b) for a, b in zip(st, st2)), "merged statistics moved with the fenced partials"


def fm_merged_per_channel_handles(dev, launch):
    """bf16; the same fold over partials that PRODUCERS left, per channel: each tile-shape group is an ops.linear on [tiles N, h w, 64] -> 64 with
    G 32 (group size 2: per-channel entries, which the merge folds two at a time; 32 and 16 row-block slots per row). Counts 2048 and 1024 and
    the weights 1 / 4 and 1 / 8 are powers of two."""
    ops = _ops()
    g = base._g(9904)
    N, K, Cc, G = 2, 64, 64, 32
    shapes, tiles = [(32, 32), (16, 32)], [2, 4]
    ce = dp.group_exponents(g, G, Cc)
    pw = ops.pack_linear_weight(dp.stats_wt(g, ce, K, 1, 1)[:, :, 0, 0], dp.stats_bias(g, ce), device=dev)
    tot = float(sum(h * w * t for (h, w), t in zip(shapes, tiles)))
    xs, parts, sums = [], [], []
    for (h, w), t in zip(shapes, tiles):
        x = dp.stats_act(g, (t * N, h * w, K)).to(dev, ops.act_dtype())
        exact = dp.conv_ref(x.reshape(1, 1, t * N * h * w, K), pw, pad=(0, 0, 0, 0), bias=pw.bias).reshape(t * N, h * w, Cc)
        dp.StatsBudget(exact, G, BLOCK_ROWS, ops.stream_dtype()).check()
        S, Q = dp.group_sums(exact, G)
        parts.append((S.reshape(t, N, G), Q.reshape(t, N, G), float(h * w * (Cc // G)), h * w / tot))
        xs.append(x), sums.append((S, Q))
    ref = dp.merged_ref(parts, EPS)
    ys = []
    for x, (h, w), (S, Q) in zip(xs, shapes, sums):
        y = launch((1, 2), lambda: ops.linear(x, pw, gn_groups=G))
        assert y._omgsr_gn.partial.shape[1:] == (h * w // 32, Cc, 2), "one slot per 32-row block, one entry per channel"
        assert_exact_sums(y._omgsr_gn.partial, G, S, Q, f"linear producer of the {h} x {w} tiles")
        ys.append(ops.carry_gn(y, y.reshape(y.shape[0], h, w, Cc)))
    assert_finalised(ops.group_norm_stats_merged(ys, tiles, N, G, EPS), None, None, None, "merged statistics from per-channel handles", ref=ref)


# name -> (tier, probe). "s<id>_": a producer probe asserting kernel variant <id>; "r_": the read pass; "f2_" / "fm_": the pair / merged finalisers.
PROBES = {
    "s3_spatial_gsz4_ragged": ("bf16", s3_spatial_gsz4_ragged),
    "s3_flat_gsz4_ragged": ("fp16", s3_flat_gsz4_ragged),
    "s3_spatial_gsz8": ("bf16", s3_spatial_gsz8),
    "s3_spatial_gsz16": ("fp16", s3_spatial_gsz16),
    "s3_spatial_gsz64": ("bf16", s3_spatial_gsz64),
    "s3_spatial_gsz10_per_channel": ("bf16", s3_spatial_gsz10_per_channel),
    "s3_spatial_gsz1_per_channel": ("fp16", s3_spatial_gsz1_per_channel),
    "s3_split_fp32_residual": ("fp32", s3_split_fp32_residual),
    "s3_mx_fp32_residual": ("fp32", s3_mx_fp32_residual),
    "s13_mx6_fp32_residual_per_channel": ("fp32", s13_mx6_fp32_residual_per_channel),
    "s6_phase_ragged": ("bf16", s6_phase_ragged),
    "s16_phase_mx6": ("fp32", s16_phase_mx6),
    "s7_multi_ragged_groups": ("bf16", s7_multi_ragged_groups),
    "s8_multi_phase_ragged_groups": ("bf16", s8_multi_phase_ragged_groups),
    "s1_stride2_gsz4": ("bf16", s1_stride2_gsz4),
    "s1_stride2_ragged_no_handle": ("fp16", s1_stride2_ragged_no_handle),
    "s2_conv1x1_residual_gsz10": ("bf16", s2_conv1x1_residual_gsz10),
    "s1_linear_gsz1": ("fp16", s1_linear_gsz1),
    "s2_linear_gsz2_partial_tile": ("bf16", s2_linear_gsz2_partial_tile),
    "s4_splitk_no_handle": ("bf16", s4_splitk_no_handle),
    "s5_p8_gsz2_partial_tile": ("bf16", s5_p8_gsz2_partial_tile),
    "s5_p8_mx_gsz8": ("fp32", s5_p8_mx_gsz8),
    "s21_mxfp8_conv": ("bf16", s21_mxfp8_conv),
    "s22_mxfp8_conv_multi": ("bf16", s22_mxfp8_conv_multi),
    "s25_mxfp8_up": ("bf16", s25_mxfp8_up),
    "s27_mxfp8_deep_c320": ("bf16", s27_mxfp8_deep_c320),
    "s27_mxfp8_deep_c960": ("bf16", s27_mxfp8_deep_c960),
    "s10_gn_fused": ("bf16", s10_gn_fused),
    "s11_gn_fused_multi": ("bf16", s11_gn_fused_multi),
    "f2_pair_halo_gemm": ("fp32", f2_pair_halo_gemm),
    "f2_pair_gemm_halo": ("fp32", f2_pair_gemm_halo),
    "fm_merged_two_tile_shapes": ("bf16", fm_merged_two_tile_shapes),
    "fm_merged_per_channel_handles": ("bf16", fm_merged_per_channel_handles),
}
for _i, (_name, (_hw_, _c, _g_)) in enumerate(READ_16.items()):
    PROBES[f"r_bf16_{_name}"] = ("bf16", _read_probe(_hw_, _c, _g_, 9700 + _i, False))
    PROBES[f"r_fp16_{_name}"] = ("fp16", _read_probe(_hw_, _c, _g_, 9720 + _i, False))
for _i, (_name, (_hw_, _c, _g_)) in enumerate(READ_32.items()):
    PROBES[f"r_fp32_{_name}"] = ("fp32", _read_probe(_hw_, _c, _g_, 9740 + _i, True))


def dry_run(name: str) -> None:
    """Build probe `name` on the host with its tier's packing rules up to the launch: the restatement is computed, the contraction's bit budget
    and the StatsBudget asserted (tests/test_gn_stats_probes_cpu.py)."""
    from omgsr_amd import ops
    tier, fn = PROBES[name]
    dt = base._TIER[tier]
    saved = ops._ACT, ops._PRECISE
    ops._ACT, ops._PRECISE = (torch.bfloat16 if dt == torch.bfloat16 else torch.float16), dt == torch.float32
    try:
        fn("cpu", base._DryLaunch())
    except base._DryRun:
        pass
    else:
        raise AssertionError(f"probe {name} never reached a launch")
    finally:
        ops._ACT, ops._PRECISE = saved


@pytest.fixture
def tier():
    from omgsr_amd import ops
    yield lambda t: ops.set_compute_dtype(base._TIER[t])
    ops.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("name", list(PROBES))
def test_gn_stats_probe(name, tier):
    t, fn = PROBES[name]
    tier(t)
    with torch.no_grad():
        fn(DEV, _launch)
