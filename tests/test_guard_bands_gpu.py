"""Guard-band tests (tests/guard_bands.py): every kernel must stay inside the tensors it is handed.

READ side, the same assertion for every op: the result of the call on dense operands is finite and the call with EVERY operand embedded
between bands of 0xFF bytes (NaN in every format the library reads) returns the same bytes. No CPU reference and no tolerance: the kernels are
bit-repeatable and dispatch does not look at addresses, so the shapes are the ones that select a kernel form.
WRITE side: the same call once more inside fenced_outputs() (every tensor the op allocates - result, split-K workspace, GroupNorm partials -
lives in a Fence), and an explicit Fence with a window for the entry points that write into a caller's buffer.
Two negative controls show that both assertions bite while every access stays inside the test's own allocations."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as gb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from omgsr_amd import ops
    return ops


@pytest.fixture(autouse=True, params=["bf16", "fp16"])
def compute_dtype(request):
    """Every test runs in both 16-bit modes, like tests/test_kernels_gpu.py; a test marked `accurate` / `bf16_only` below overrides the list."""
    ops = _ops()
    ops.set_compute_dtype(torch.bfloat16 if request.param == "bf16" else torch.float16)
    yield request.param
    ops.overflow_seen(); ops.mx_saturation_seen()
    ops.set_compute_dtype(torch.bfloat16)


bf16_only = pytest.mark.parametrize("compute_dtype", ["bf16"], indirect=True)       # the fp8 tier's kernels
fp16_only = pytest.mark.parametrize("compute_dtype", ["fp16"], indirect=True)       # the MX / fp6 forms of the accurate tier


@pytest.fixture
def accurate(compute_dtype):
    """The accurate tier (fp32 stream tensors) with operands of the mode the test runs in; the autouse fixture restores the tier."""
    ops = _ops()
    ops.set_compute_dtype(torch.float32, operand_dtype=torch.bfloat16 if compute_dtype == "bf16" else torch.float16)
    ops.overflow_seen(); ops.mx_saturation_seen()
    return ops


def rnd(*shape, seed=0, scale=1.0, dtype=None):
    """Device tensor of normal values in `dtype` (default: the compute type). No reference is computed from them, so nothing is pre-rounded."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype or _ops().act_dtype())


def f32(*shape, seed=0, scale=1.0):
    return rnd(*shape, seed=seed, scale=scale, dtype=torch.float32)


def dense(t):
    return t


def _launches(fn):
    """fn() with the per-launch timing on: (result, [(kind, variant)] of its launches) - the pattern of tests/test_fp8_vae_gpu.py."""
    from omgsr_amd import _lib
    lib = _lib.load()
    lib.omgsr_timing_enable(1)
    lib.omgsr_timing_reset()
    try:
        out = fn()
        torch.cuda.synchronize()
        buf = (_lib.TimingEntry * 4096)()
        n = lib.omgsr_timing_collect(buf, 4096)
    finally:
        lib.omgsr_timing_enable(0)
    return out, [(e.kind, e.variant) for e in buf[:n]]


def _tensors(x):
    """The tensors of a result (a tensor, an Mxfp8, or a tuple / list of those), in order."""
    if x is None:
        return []
    if isinstance(x, torch.Tensor):
        return [x]
    if hasattr(x, "codes"):
        return [x.codes, x.scales]
    return [t for y in x for t in _tensors(y)]


def _finite(x):
    """Float tensors: finite. MXFP8 bytes: no NaN code (0x7F / 0xFF) and no NaN scale (0xFF)."""
    if hasattr(x, "codes"):
        return bool(((x.codes & 0x7F) != 0x7F).all()) and bool((x.scales != 0xFF).all())
    return all(bool(torch.isfinite(t.float()).all()) for t in _tensors(x) if t.dtype.is_floating_point)


def assert_same_bytes(got, want, what):
    g, w = _tensors(got), _tensors(want)
    assert len(g) == len(w), what
    for i, (a, b) in enumerate(zip(g, w)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: output {i} is {tuple(a.shape)} {a.dtype}, the dense call's {tuple(b.shape)} {b.dtype}"
        a8, b8 = a.contiguous().view(torch.uint8).reshape(-1), b.contiguous().view(torch.uint8).reshape(-1)
        if not torch.equal(a8, b8):
            d = (a8 != b8).nonzero()
            bad = a.dtype.is_floating_point and not bool(torch.isfinite(a.float()).all())
            raise AssertionError(f"{what}: output {i} differs from the dense call's in {d.numel()} bytes, the first at byte offset {int(d[0])} "
                                 f"(element {int(d[0]) // a.element_size()} of {tuple(a.shape)}){'; it holds non-finite values' if bad else ''}")


def guard(call, finite=_finite, kind=1, need=None, allowed=None):
    """The read-side and the fenced-outputs assertions for one op. call(E) runs it with E applied to every operand (E = dense | gb.embed) and
    returns everything it computes. need / allowed: kernel variants (omgsr_timing `variant` of the kind-`kind` launches) that must / may run."""
    want, v = _launches(lambda: call(dense))
    assert finite(want), "the dense call's result is not finite"
    got, v1 = _launches(lambda: call(gb.embed))
    assert_same_bytes(got, want, "embedded operands")
    with gb.fenced_outputs():
        fenced, v2 = _launches(lambda: call(dense))
    assert_same_bytes(fenced, want, "fenced outputs")
    ran = sorted({var for k, var in v if k == kind})
    print(f"variants ran: {ran}")
    assert v1 == v and v2 == v, f"dispatch moved with the addresses: {v} / {v1} / {v2}"
    if need is not None:
        allowed = set(allowed or need)
        assert set(need) <= set(ran) <= allowed, f"expected kernel variant(s) {sorted(need)} (allowed {sorted(allowed)}), the library ran {ran}"
    return want


# ---- conv2d 3x3: one case per kernel form -------------------------------------------------------------------------------------------------------
# variants (ts.rec.variant in igemm.hip): 1 register-staged gather igemm, 2 LDS-DMA, 3 halo-tile kernel (spatial / FLAT / narrow), 4 LDS-DMA split-K,
# 5 ping-pong, 6 halo phase form, 7 / 8 halo multi launch (nine taps / phase), 10 GroupNorm-fused halo, 12 halo split-K, 13 halo with fp6 chunks.
# The halo-tile kernel takes a problem only with >= 192 workgroup tiles (use_halo / use_halo_phase), so four shapes as they stand in CONV_CASES
# (one image of 86 x 43, two of 20 x 50, twelve of 50 x 46, one 43 x 150 upsampling) run the gather kernel: they stay here with the variant the
# dispatcher gives them, and the SAME ragged extents with the smallest N that reaches 192 tiles cover the form they were written for.
# A dispatcher change that moves any case off the kernel named here fails the case.
# name: (N, Cin, Cout, H, W, dict of options, variants needed, form of the halo tile grid or None)
CONV = {
    "gather-ragged-k-tail": (1, 40, 72, 9, 7, dict(bias=False), {1}, None),                       # K = 360 < K_pad = 384
    "one-86x43-image": (1, 64, 128, 86, 43, dict(), {1}, None),                                    # 16 FLAT tiles: gather; both borders adjoin a band
    "halo-flat-86x43": (12, 64, 128, 86, 43, dict(), {3}, "flat"),                                 # 12 x 16 tiles, 22-piece patch (W <= 45)
    "halo-spatial-43x86": (11, 64, 128, 43, 86, dict(), {3}, "spatial"),                           # 11 x 3 x 6 tiles, W > 80: spatial form, ragged both ways
    "two-20x50-residual-silu": (2, 128, 256, 20, 50, dict(res=True, act=1), {1}, None),            # 20 tiles: gather
    "halo-20x50-residual-silu": (20, 128, 256, 20, 50, dict(res=True, act=1), {3}, "flat"),        # 20 x 5 x 2 tiles
    "halo-narrow-cout": (2, 128, 3, 128, 192, dict(), {3}, None),                                  # Cout <= 32, exactly 192 tiles
    "halo-flat": (30, 128, 256, 38, 38, dict(res=True, act=1), {3}, "flat"),
    "twelve-50x46": (12, 64, 128, 50, 46, dict(res=True), {1}, None),                              # 120 tiles: gather
    "halo-flat-27-piece": (20, 64, 128, 50, 46, dict(res=True), {3}, "flat"),                      # 20 x 10 tiles, W in 46 .. 80
    "upsample-gather": (1, 256, 256, 12, 20, dict(ups=True), {4}, None),                           # nine taps on the virtual map, split over K (LDS-DMA kernel)
    "one-43x150-upsample": (1, 64, 128, 43, 150, dict(ups=True, phases=True, bias=False), {1}, None),       # 120 phase tiles: gather
    "upsample-phase": (2, 64, 128, 43, 150, dict(ups=True, phases=True, bias=False), {6}, None),   # 240 phase tiles
    "stride-2": (2, 128, 128, 32, 32, dict(stride=2, pad=(0, 1, 0, 1)), {1}, None),
    # (no 3x3 conv reaches the ping-pong kernel - igemm_p8_ok takes GEMM-shaped problems only; test_linear below runs it with a partial last tile)
    "stride-2-ragged-split-k": (9, 192, 256, 118, 122, dict(stride=2, act=1), {4}, None),          # 32 391 rows = 254 tiles of 256 x 128: split over K
    "stride-2-ragged-lds-dma": (10, 192, 256, 118, 122, dict(stride=2, act=1), {2}, None),         # 35 990 rows: the LDS-DMA kernel, last row tile partial
}


def _conv_operands(N, Cin, Cout, H, W, bias=True, res=False, ups=False, phases=False, stride=1, pad=1, seed=1, **pack):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g) if bias else None
    pw = ops.pack_conv_weight(w, b, device=DEV, upsample_phases=phases, **pack)
    x = rnd(N, H, W, Cin, seed=seed + 1, dtype=ops.stream_dtype())
    pt, pb, pl, pr = (pad,) * 4 if isinstance(pad, int) else pad
    Hv, Wv = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = (Hv + pt + pb - 3) // stride + 1, (Wv + pl + pr - 3) // stride + 1
    r = rnd(N, Ho, Wo, pw.cout, seed=seed + 2, dtype=ops.stream_dtype()) if res else None
    return x, pw, r


def _halo_form(x, pw, r, act, expect):
    """The tile grid the halo kernel plans for this problem, told by the number of GroupNorm-partial slots it would leave: two per workgroup tile of
    an image - ceil(W / 32) ceil(H / 8) spatial tiles, or ceil(H (W + 2) / 256) runs of the flattened padded map (FLAT)."""
    from omgsr_amd import _lib
    ops = _ops()
    a = _lib.IgemmArgs()
    ops._conv_args(a, x, pw, 1, 1, False, act, r, None, ops.OUT_STREAM, 1.0, None, 1, 0)
    a.gn_groups = 32
    _, H, W, _ = x.shape
    slots = {"spatial": 2 * -(-W // 32) * -(-H // 8), "flat": 2 * -(-(H * (W + 2)) // 256)}
    assert slots["spatial"] != slots["flat"]
    assert _lib.load().omgsr_igemm_gn_slots(C.byref(a)) == slots[expect], f"the halo kernel does not plan the {expect} form for this shape"


@pytest.mark.parametrize("name", list(CONV))
def test_conv3x3_every_form(name):
    ops = _ops()
    N, Cin, Cout, H, W, opt, need, form = CONV[name]
    opt = dict(opt)
    act = opt.pop("act", 0)
    x, pw, r = _conv_operands(N, Cin, Cout, H, W, **opt)
    kw = dict(stride=opt.get("stride", 1), pad=opt.get("pad", 1), upsample=opt.get("ups", False), act=act)
    if form:
        _halo_form(x, pw, r, act, form)
    guard(lambda E: ops.conv2d(E(x), E(pw), residual=E(r), **kw), need=need)


def _gn_spec(E, mean, rstd, gamma, beta, G, channels):
    """A GnSpec over embedded statistics and affine whose (scale, shift) table - made by the library from them - is embedded too."""
    ops = _ops()
    spec = ops.GnSpec(E(mean), E(rstd), E(gamma), E(beta), G, ops.ACT_SILU)
    spec._table = E(spec.table(channels))
    return spec


def test_conv3x3_groupnorm_fused_patch_producer():
    """The smallest fusable entry of GN_CONV_CASES (four rows sharing two images' statistics, 32 channels: ONE chunk, normalised in the prologue)."""
    ops = _ops()
    N, nimg, Cin, Cout, H, W, G = 4, 2, 32, 128, 96, 160, 32
    x, pw, _ = _conv_operands(N, Cin, Cout, H, W, seed=11)
    mean, rstd = 0.25 + 0.1 * f32(nimg, G, seed=16), (1.0 + 0.1 * f32(nimg, G, seed=17)).abs()
    gamma, beta = 1.0 + 0.2 * f32(Cin, seed=14), 0.3 * f32(Cin, seed=15)

    def call(E):
        y = ops.conv2d(E(x), E(pw), pad=1, gn=_gn_spec(E, mean, rstd, gamma, beta, G, Cin), gn_groups=32)
        return y, ops.group_norm_stats(y, 32, 1e-6)                # ... and the statistics its epilogue left (finalize over the partials)
    guard(call, need={10})


MULTI = {      # tests/test_kernels_gpu.py MULTI_CASES[0] and [2]
    "gather": (128, 128, False, True, [(36, 40, 40), (12, 40, 32), (12, 32, 40), (4, 32, 32)], {7}, {7}),
    # the 43-wide groups of the upsampling layer are too ragged for the phase form and run the nine-tap form; the forms alternate in the list,
    # so every problem is a launch of its own (3 / 6) - the next entry keeps the phase problems together
    "phase-alternating": (256, 256, True, False, [(4, 43, 43), (4, 43, 32), (4, 32, 43), (4, 32, 32)], {3, 6}, {3, 6}),
    "phase": (256, 256, True, False, [(4, 43, 32), (4, 32, 32), (2, 43, 64)], {8}, {8}),
}


@pytest.mark.parametrize("name", list(MULTI))
def test_conv_multi_launch(name):
    ops = _ops()
    Cin, Cout, ups, use_res, groups, need, allowed = MULTI[name]
    g = torch.Generator().manual_seed(2)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    pw = ops.pack_conv_weight(w, torch.randn(Cout, generator=g), device=DEV, cout_multiple=8, upsample_phases=ups)
    xs = [rnd(n, h, wd, Cin, seed=10 + i) for i, (n, h, wd) in enumerate(groups)]
    s = 2 if ups else 1
    rs = [rnd(n, s * h, s * wd, Cout, seed=20 + i) for i, (n, h, wd) in enumerate(groups)] if use_res else None
    guard(lambda E: ops.conv2d_multi([E(x) for x in xs], E(pw), pad=1, upsample=ups, residuals=None if rs is None else [E(r) for r in rs], gn_groups=32),
          need=need, allowed=allowed)


@fp16_only
@pytest.mark.parametrize("form", ["mx", "fp6", "fp6-out"])
def test_conv3x3_accurate_tier_forms(accurate, form):
    """The halo-tile kernel's mixed-precision instantiations (fp16 chunks + block-scaled fp8 / fp6 correction chunks; an epilogue that writes the
    fp6 operand form), one pass each (144 tiles: above the halo split-K's 128), ragged map, fp32 stream input and residual."""
    ops = accurate
    N, H, W, Cc, Cout = 8, 43, 86, 128, 128
    x, pw, r = _conv_operands(N, Cc, Cout, H, W, res=True, seed=8, split=3 if form == "mx" else 4)
    assert x.dtype == torch.float32 and pw.row_channels == 2 * Cc
    if form == "fp6-out":
        xo = ops.to_operand(x, 4)
        # the result is an operand: fp16 third, then fp6 codes and scale bytes (not numbers: compared as bytes, the fp16 third checked for finiteness)
        guard(lambda E: ops.conv2d(E(xo), E(pw), pad=1, residual=E(r), out_dtype=ops.OUT_BF16, out_split=4), need={13},
              finite=lambda y: bool(torch.isfinite(y[..., :Cout].float()).all()))
    else:
        guard(lambda E: ops.conv2d(E(x), E(pw), pad=1, residual=E(r), gn_groups=32), need={3 if form == "mx" else 13})


# ---- linear ---------------------------------------------------------------------------------------------------------------------------------------

def _linear_operands(B, M, K, Nout, seed=5, geglu=False, bias=True):
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(2 * Nout if geglu else Nout, K, generator=g) / math.sqrt(K)
    b = torch.randn(w.shape[0], generator=g) if bias else None
    pw = (ops.pack_geglu_weight if geglu else ops.pack_linear_weight)(w, b, device=DEV)
    return rnd(B, M, K, seed=seed + 1), pw


@pytest.mark.parametrize("B,M,K,Nout,need", [(2, 77, 1024, 640, None), (2, 1000, 1280, 1280, None), (2, 33, 1280, 320, None), (2, 65, 256, 10240, None),
                                            (1, 100, 328, 200, None),                 # a K tail: 328 = 10 chunks of 32 + 8
                                            (1, 36900, 1536, 1024, {5})])             # ping-pong kernel, 145 row tiles, the last one partial
def test_linear(B, M, K, Nout, need):
    ops = _ops()
    x, pw = _linear_operands(B, M, K, Nout)
    r = rnd(B, M, Nout, seed=9) if need else None
    guard(lambda E: ops.linear(E(x), E(pw), residual=E(r)), need=need)


def test_linear_epilogues_geglu_transposed():
    ops = _ops()
    x, pw = _linear_operands(1, 333, 256, 384, seed=8)
    gate, r = f32(384, seed=11), rnd(1, 333, 384, seed=12)
    guard(lambda E: (ops.linear(E(x), E(pw), act=ops.ACT_GELU_TANH, gate=E(gate), residual=E(r)),
                     ops.linear(E(x), E(pw), out_dtype=ops.OUT_F32, alpha=0.125)))
    xg, pg = _linear_operands(1, 200, 320, 1280, seed=13, geglu=True)
    guard(lambda E: ops.linear(E(xg), E(pg)))
    xt, pt = _linear_operands(2, 77, 1024, 320, seed=16, bias=False)
    yt = guard(lambda E: ops.linear_t(E(xt), E(pt), 77))
    assert yt.shape == (2, 320, 80) and bool((yt[:, :, 77:] == 0).all())
    xr, pr = _linear_operands(2, 300, 256, 384, seed=18)           # a row range of every image's sequence
    rr = rnd(2, 200, 384, seed=19)
    guard(lambda E: ops.linear_rows(E(xr), 60, 200, E(pr), residual=E(rr)))


def test_linear_split_k():
    """The shapes of test_split_k_paths: fp32 partial tiles in a workspace (fenced too) and the reduce pass with the full epilogue."""
    ops = _ops()
    x, pw = _linear_operands(1, 300, 3072, 384, seed=70)
    gate, r = f32(384, seed=73), rnd(1, 300, 384, seed=74)
    guard(lambda E: ops.linear(E(x), E(pw), act=ops.ACT_GELU_TANH, gate=E(gate), residual=E(r)), need={4})
    guard(lambda E: ops.linear(E(x), E(pw), out_dtype=ops.OUT_F32, alpha=0.5), need={4})
    xg, pg = _linear_operands(1, 200, 2048, 640, seed=75, geglu=True)
    guard(lambda E: ops.linear(E(xg), E(pg)), need={4})


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------

def _attn_operands(B, Bk, H, D, Lq, Lk, seed=26, extra_rows=5):
    """q, k with rows past Lk, V^T with ld = round_up(Lk, 8) + 8: every K row >= Lk and every V^T column >= Lk holds 0xFF bytes (NaN)."""
    inner = H * D
    q = rnd(B, Lq, inner, seed=seed)
    k = gb.poison_tail(rnd(Bk, Lk + extra_rows, inner, seed=seed + 1), 1, Lk)
    vt = gb.poison_tail(rnd(Bk, inner, (Lk + 7) // 8 * 8 + 8, seed=seed + 2), 2, Lk)
    return q, k, vt


@pytest.mark.parametrize("B,H,D,Lq,Lk,bcast", [(1, 5, 64, 100, 77, False), (1, 2, 128, 200, 136, False), (2, 5, 64, 256, 128, True), (1, 4, 128, 320, 320, False)])
def test_attention(B, H, D, Lq, Lk, bcast):
    ops = _ops()
    q, k, vt = _attn_operands(B, 1 if bcast else B, H, D, Lq, Lk)
    guard(lambda E: ops.attention(E(q), E(k), E(vt), H, D, D ** -0.5, Lk=Lk), kind=2)


def test_attention_fused_qk_buffer():
    ops = _ops()
    B, H, D, L = 2, 5, 64, 200
    inner = H * D
    qk = rnd(B, L, 2 * inner, seed=32)
    vt = gb.poison_tail(rnd(B, inner, L + 8, seed=33), 2, L)
    guard(lambda E: (lambda b: ops.attention(b, b, E(vt), H, D, D ** -0.5, q_col=0, k_col=inner, Lk=L))(E(qk)), kind=2)


@pytest.mark.parametrize("Lq,Lk", [(300, 77), (200, 192)])
def test_attention_two_term_split(accurate, Lq, Lk):
    """q, k as [hi | lo] at q_lo_col / k_lo_col, the probabilities split in registers, V^T as the transposed two-term split, split output."""
    ops = accurate
    B, H, D = 2, 5, 64
    inner = H * D
    q, k = rnd(B, Lq, 2 * inner, seed=90), gb.poison_tail(rnd(B, Lk + 3, 2 * inner, seed=91), 1, Lk)
    ld = (Lk + 7) // 8 * 8 + 8
    vts = guard(lambda E: ops.transpose_split(E(f32(B, Lk, inner, seed=92)), ld))
    assert bool((vts[..., Lk:] == 0).all())
    vts = gb.poison_tail(vts.clone(), 2, Lk)
    vt1 = vts[:, :inner].contiguous()
    kw = dict(Lk=Lk, out_split=2, q_lo_col=inner, k_lo_col=inner)
    guard(lambda E: (ops.attention(E(q), E(k), E(vts), H, D, D ** -0.5, **kw), ops.attention(E(q), E(k), E(vt1), H, D, D ** -0.5, p_split=False, **kw)), kind=2)


# ---- norms ----------------------------------------------------------------------------------------------------------------------------------------

def _gn_operands(N, Cc, H, W, seed=20, dtype=None):
    return (rnd(N, H, W, Cc, seed=seed, scale=2.0, dtype=dtype) + 0.5, 1.0 + f32(Cc, seed=seed + 1), f32(Cc, seed=seed + 2))


@pytest.mark.parametrize("N,Cc,H,W", [(1, 320, 16, 16), (1, 512, 24, 40), (2, 1920, 8, 8)])
def test_group_norm(N, Cc, H, W):
    ops = _ops()
    x, gamma, beta = _gn_operands(N, Cc, H, W)

    def call(E):
        ex = E(x)
        mean, rstd, var = ops.group_norm_stats(ex, 32, 1e-6)
        return mean, rstd, var, ops.group_norm_apply(ex, E(mean), E(rstd), E(gamma), E(beta), 32, ops.ACT_SILU)
    guard(call)


def test_group_norm_tiled_vae_forms():
    """Tile-major rows sharing per-image statistics: apply_shared, apply_multi, the merged statistics of several tile shapes, and
    group_norm_pair (in the 16-bit tiers: concat_channels + statistics + apply)."""
    ops = _ops()
    N, Cc, G = 2, 64, 32
    shapes = [(3, 20, 24), (2, 20, 9), (1, 7, 9)]                  # (tiles, h, w)
    xs = [rnd(t * N, h, w, Cc, seed=100 + i, scale=1.0 + i) for i, (t, h, w) in enumerate(shapes)]
    tiles = [t for t, _, _ in shapes]
    gamma, beta = 1.0 + f32(Cc, seed=110), f32(Cc, seed=111)

    def call(E):
        exs = [E(x) for x in xs]
        mean, rstd, var = ops.group_norm_stats_merged(exs, tiles, N, G, 1e-6)
        em, er, eg, eb = E(mean), E(rstd), E(gamma), E(beta)
        return (mean, rstd, var, [ops.group_norm_apply_shared(x, em, er, eg, eb, G, ops.ACT_SILU) for x in exs],
                ops.group_norm_apply_multi(exs, em, er, eg, eb, G, ops.ACT_SILU))
    guard(call)
    a, b = rnd(2, 9, 11, 64, seed=120), rnd(2, 9, 11, 32, seed=121)
    g2, b2 = 1.0 + f32(96, seed=122), f32(96, seed=123)
    guard(lambda E: ops.group_norm_pair(E(a), E(b), E(g2), E(b2), 32, 1e-5, ops.ACT_SILU))


def test_norms_accurate_tier(accurate):
    """fp32 stream tensors: the GroupNorm apply pass with its second output (also_cast), split operands, the two-source apply pass and statistics fold
    of group_norm_pair, LayerNorm and softmax_rows writing two-term splits."""
    ops = accurate
    x, gamma, beta = _gn_operands(2, 320, 16, 12, dtype=torch.float32)

    def gn(E):
        ex = E(x)
        mean, rstd, _ = ops.group_norm_stats(ex, 32, 1e-6)
        args = (E(mean), E(rstd), E(gamma), E(beta), 32, ops.ACT_SILU)
        return ops.group_norm_apply(ex, *args, also_cast=1), ops.group_norm_apply(ex, *args, split=2, also_cast=2)
    guard(gn)
    # group_norm_pair's two-source form: per-channel partials of both producers -> statistics (finalize2), then the apply pass over the two tensors
    a, b = f32(2, 8, 8, 64, seed=130), f32(2, 8, 8, 32, seed=131)
    pa, pb = f32(2, 3, 64, 2, seed=132).abs() + 1.0, f32(2, 2, 32, 2, seed=133).abs() + 1.0       # (sum, sum of squares) per slot and channel
    pa[..., 1] += 400.0; pb[..., 1] += 400.0                         # sums of squares large enough for a positive variance
    g2, b2 = 1.0 + f32(96, seed=134), f32(96, seed=135)

    def pair(E):
        ea, eb = E(a), E(b)
        ea._omgsr_gn, eb._omgsr_gn = (E(pa), 32, ea.data_ptr(), ea._version), (E(pb), 32, eb.data_ptr(), eb._version)
        st = ops.group_norm_pair_stats(ea, eb, 32, 1e-5)
        assert st is not None, "the two-source fold must be taken"
        return st, ops.group_norm_apply_pair(ea, eb, E(st[0]), E(st[1]), E(g2), E(b2), 32, ops.ACT_SILU, split=2, also_cast=1)
    guard(pair)
    xl, al, bl = f32(33, 3072, seed=23, scale=3.0), 1.0 + f32(3072, seed=24), f32(3072, seed=25)
    guard(lambda E: (ops.layer_norm(E(xl), E(al), E(bl), 1e-5, split=2), ops.layer_norm(E(xl), None, None, 1e-6)))
    s = f32(5, 1664, seed=36, scale=4.0)
    guard(lambda E: ops.softmax_rows(E(s), valid=1600, split=True))
    guard(lambda E: ops.to_operand(E(xl), 2))


@pytest.mark.parametrize("rows,Cc", [(100, 320), (50, 1280), (33, 3072), (1, 640)])
def test_layer_norm(rows, Cc):
    ops = _ops()
    x, a, b = rnd(rows, Cc, seed=23, scale=3.0) + 1.0, 1.0 + f32(Cc, seed=24), f32(Cc, seed=25)
    guard(lambda E: (ops.layer_norm(E(x), E(a), E(b), 1e-5), ops.layer_norm(E(x), None, None, 1e-6)))


@pytest.mark.parametrize("rows,L,valid", [(37, 1000, None), (5, 1664, 1600), (3, 16384, None)])
def test_softmax_rows(rows, L, valid):
    ops = _ops()
    s = f32(rows, L, seed=34, scale=4.0)
    p = guard(lambda E: ops.softmax_rows(E(s), valid=valid))
    assert valid is None or bool((p[:, valid:] == 0).all())


@bf16_only
def test_mxfp8_producers():
    """quantize_mxfp8 (both source types) and the GroupNorm apply pass that writes MXFP8."""
    ops = _ops()
    xb, xf = rnd(3, 37, 256, seed=50, scale=3.0), f32(37, 384, seed=51, scale=3.0)
    guard(lambda E: (ops.quantize_mxfp8(E(xb)), ops.quantize_mxfp8(E(xf))))
    x, gamma, beta = _gn_operands(4, 128, 9, 13, seed=52)
    mean, rstd = 0.5 + 0.1 * f32(2, 32, seed=55), (0.5 + 0.1 * f32(2, 32, seed=56)).abs()
    guard(lambda E: ops.group_norm_apply_mxfp8(E(x), E(mean), E(rstd), E(gamma), E(beta), 32, ops.ACT_SILU))


# ---- layout and tile ops --------------------------------------------------------------------------------------------------------------------------

def test_layout_and_latent_ops():
    ops = _ops()
    x32, x16 = f32(2, 3, 20, 12, seed=38), rnd(2, 3, 20, 12, seed=39)
    xh = guard(lambda E: (ops.nchw_to_nhwc(E(x32)), ops.nchw_to_nhwc(E(x16))))[0]          # 3 -> 8 channels, both source types
    assert xh.shape == (2, 20, 12, 8) and bool((xh[..., 3:] == 0).all())
    guard(lambda E: (ops.nhwc_to_nchw(E(xh), channels=3, dtype=torch.float32, clamp=(-1.0, 1.0)), ops.nhwc_to_nchw(E(xh), channels=3)))
    a, b = rnd(2, 5, 7, 16, seed=40), rnd(2, 5, 7, 24, seed=41)
    guard(lambda E: ops.concat_channels(E(a), E(b)))
    t = rnd(2, 9, 11, 8, seed=45)
    guard(lambda E: ops.crop_nhwc(E(t), 2, 3, 4, 5))
    guard(lambda E: ops.crop_nhwc(E(t), 5, 6, 4, 5))                                     # the window ends at the last row and column
    mom, eps = rnd(2, 6, 5, 8, seed=42), f32(2, 6, 5, 4, seed=43)
    guard(lambda E: ops.vae_sample(E(mom), E(eps), 4, 0.1159, 0.3611))
    u, v = rnd(1000, seed=43), rnd(1000, seed=44)
    guard(lambda E: (ops.axpby(E(u), E(v), 1.0 / 0.797, -0.6035 / 0.797, 0.0, 1.0 / 0.18215), ops.axpby(E(u), None, 2.0, 0.0)))
    lat = rnd(2, 8, 12, 16, seed=46)
    tok = guard(lambda E: ops.flux_pack(E(lat), 16))
    guard(lambda E: (ops.flux_unpack(E(tok), 8, 12), ops.flux_unpack(E(tok), 8, 12, ld=24)))
    acc, wsum = f32(2, 12, 10, 4, seed=47), f32(1, 12, 10, 1, seed=48).abs() + 0.1
    guard(lambda E: ops.tile_normalise(E(acc), E(wsum)))
    big = rnd(2, 37, 41, 8, seed=49)
    guard(lambda E: ops.resize_nearest_exact(E(big), 12 / 41))


def test_to_operand_and_transpose_split(accurate):
    ops = accurate
    x = f32(3, 37, 72, seed=60)                                       # ragged L and C
    guard(lambda E: (ops.to_operand(E(x)), ops.transpose_split(E(x)), ops.transpose_split(E(x), 48)))


# ---- WRITE side: entry points that write into a caller's buffer -----------------------------------------------------------------------------------

def _fence(shape, dtype=None):
    return gb.Fence(shape, dtype or _ops().act_dtype(), DEV)


def test_conv2d_into_a_callers_tensor():
    ops = _ops()
    N, Cin, Cout, H, W = 20, 64, 128, 50, 46
    x, pw, r = _conv_operands(N, Cin, Cout, H, W, res=True)
    want = ops.conv2d(x, pw, pad=1, residual=r)
    f = _fence((N, H, W, Cout), ops.stream_dtype())
    ops.conv2d(x, pw, pad=1, residual=r, out=f.out)
    f.check()
    assert_same_bytes(f.out, want, "conv2d(out=)")
    # a two-term split operand [hi | lo] at the front of wider rows: the 16 columns behind it are not the conv's
    want2 = ops.conv2d(x, pw, pad=1, out_dtype=ops.OUT_BF16, out_split=2)
    f = _fence((N, H, W, 2 * Cout + 16)).window(Ellipsis, slice(0, 2 * Cout))
    ops.conv2d(x, pw, pad=1, out_dtype=ops.OUT_BF16, out_split=2, out=f.out)
    f.check()
    assert_same_bytes(f.out[..., :2 * Cout], want2, "conv2d(out=, out_split=2)")


def _into_plain(shape, fn):
    """The same call into a plainly allocated buffer: the dense result a fenced window must equal."""
    buf = torch.full(shape, 7.0, device=DEV, dtype=_ops().act_dtype())
    fn(buf)
    return buf


def test_linear_into_windows():
    ops = _ops()
    M, K, Nout, rows, ld, row0, col0 = 200, 256, 384, 260, 2 * 384 + 64, 24, 384 + 8
    x, pw = _linear_operands(1, M, K, Nout, seed=60)
    x = x[0]
    for kw in (dict(act=ops.ACT_GELU_TANH), dict(sample_rows=100)):          # (sample_rows: the caller flattened two images into M)
        call = lambda buf: ops.linear_into(x, pw, buf, row0, col0, **kw)     # noqa: E731
        f = _fence((rows, ld)).window(slice(row0, row0 + M), slice(col0, col0 + Nout))
        call(f.out)
        f.check()
        assert_same_bytes(f.out[row0:row0 + M, col0:col0 + Nout], _into_plain((rows, ld), call)[row0:row0 + M, col0:col0 + Nout], "linear_into")
    # two-term split output: the low halves at lo_col0, away from the high halves
    lo = 16
    call = lambda buf: ops.linear_into(x, pw, buf, row0, col0, out_split=2, lo_col0=lo)      # noqa: E731
    with pytest.raises(ValueError):
        call(_fence((rows, ld)).out)                                   # (the low halves must lie behind the high ones)
    ld2, col0, lo = 3 * Nout + 64, 8, 2 * Nout + 8
    call = lambda buf: ops.linear_into(x, pw, buf, row0, col0, out_split=2, lo_col0=lo)      # noqa: E731
    f = _fence((rows, ld2)).window(slice(row0, row0 + M), slice(col0, col0 + Nout)).window(slice(row0, row0 + M), slice(lo, lo + Nout))
    call(f.out)
    f.check()
    plain = _into_plain((rows, ld2), call)
    for c in (col0, lo):
        assert_same_bytes(f.out[row0:row0 + M, c:c + Nout], plain[row0:row0 + M, c:c + Nout], "linear_into(out_split=2)")
    # batched: image b's rows land in out[b]
    xb, _ = _linear_operands(3, 50, K, Nout, seed=60)
    call = lambda buf: ops.linear_into(xb, pw, buf, 7, 16)              # noqa: E731
    f = _fence((3, 64, Nout + 32)).window(slice(None), slice(7, 57), slice(16, 16 + Nout))
    call(f.out)
    f.check()
    assert_same_bytes(f.out[:, 7:57, 16:16 + Nout], _into_plain((3, 64, Nout + 32), call)[:, 7:57, 16:16 + Nout], "linear_into(batched)")


def test_linear_t_into_window():
    ops = _ops()
    for L, key0 in ((77, 24), (96, 32)):                                 # the scalar and the whole-block column path of the transposed epilogue
        x, pw = _linear_operands(2, L, 320, 200, seed=62)
        ld = (L + 64 + 7) // 8 * 8
        call = lambda buf: ops.linear_t_into(x, pw, buf, key0)           # noqa: E731
        f = _fence((2, 200, ld)).window(Ellipsis, slice(key0, key0 + L))
        call(f.out)
        f.check()
        assert_same_bytes(f.out[..., key0:key0 + L], _into_plain((2, 200, ld), call)[..., key0:key0 + L], "linear_t_into")


@pytest.mark.parametrize("H,D,Lq,Lk", [(5, 64, 100, 77), (2, 128, 200, 136), (1, 512, 100, 77), (1, 512, 200, 136)])
def test_attention_into_a_callers_buffer(H, D, Lq, Lk):
    """out=, o_col: the heads' columns of wider rows; Lq is ragged, so the last query tile is partial. out_split 2: low halves at o_lo_col."""
    ops = _ops()
    B, inner = 2, H * D
    q, k, vt = _attn_operands(B, B, H, D, Lq, Lk)
    o_col, ld = 64, 2 * inner + 192
    want = ops.attention(q, k, vt, H, D, D ** -0.5, Lk=Lk)
    f = _fence((B, Lq, ld)).window(Ellipsis, slice(o_col, o_col + inner))
    ops.attention(q, k, vt, H, D, D ** -0.5, Lk=Lk, out=f.out, o_col=o_col)
    f.check()
    assert_same_bytes(f.out[..., o_col:o_col + inner], want, "attention(out=, o_col)")
    want2 = ops.attention(q, k, vt, H, D, D ** -0.5, Lk=Lk, out_split=2)
    lo = o_col + inner + 64
    f = _fence((B, Lq, ld)).window(Ellipsis, slice(o_col, o_col + inner)).window(Ellipsis, slice(lo, lo + inner))
    ops.attention(q, k, vt, H, D, D ** -0.5, Lk=Lk, out=f.out, o_col=o_col, out_split=2, o_lo_col=lo)
    f.check()
    assert_same_bytes(f.out[..., o_col:o_col + inner], want2[..., :inner], "attention(out_split=2) high halves")
    assert_same_bytes(f.out[..., lo:lo + inner], want2[..., inner:], "attention(out_split=2) low halves")


@bf16_only
def test_mxfp8_attention_and_producers_into_callers_buffers():
    ops = _ops()
    B, H, D, Lq, Lk = 2, 2, 128, 200, 136
    inner = H * D
    q, k = rnd(B, Lq, inner, seed=70, scale=1.5), rnd(B, Lk + 4, inner, seed=71, scale=1.5)
    vt = torch.zeros(B, inner, 256, device=DEV, dtype=torch.bfloat16)
    vt[..., :Lk] = rnd(B, inner, Lk, seed=72)
    mq, mk, mvt = ops.quantize_mxfp8(q), ops.quantize_mxfp8(k), ops.quantize_mxfp8(vt)
    gb.poison_tail(mk.codes, 1, Lk); gb.poison_tail(mk.scales, 1, Lk)             # K rows >= Lk: NaN codes and scales
    gb.poison_tail(mvt.codes, 2, Lk); gb.poison_tail(mvt.scales, 2, (Lk + 31) // 32)   # V^T codes >= Lk; the scales of blocks wholly past Lk
    want = guard(lambda E: ops.attention(E(mq), E(mk), E(mvt), H, D, D ** -0.5, Lk=Lk), kind=2, need={19})
    f = _fence((B, Lq, inner + 256)).window(Ellipsis, slice(128, 128 + inner))
    ops.attention(mq, mk, mvt, H, D, D ** -0.5, Lk=Lk, out=f.out, o_col=128)
    f.check()
    assert_same_bytes(f.out[..., 128:128 + inner], want, "attention(MXFP8, out=, o_col)")
    # quantize_mxfp8(out=) and rmsnorm_rope_mxfp8(out=): codes and scales of a workspace
    x = rnd(3, 37, 256, seed=73, scale=3.0)
    wantq = ops.quantize_mxfp8(x)
    fc, fs = _fence((3, 37, 256), torch.uint8), _fence((3, 37, 8), torch.uint8)
    ops.quantize_mxfp8(x, out=ops.Mxfp8(fc.out, fs.out))
    fc.check(); fs.check()
    assert_same_bytes((fc.out, fs.out), wantq, "quantize_mxfp8(out=)")
    Bx, L, Hh = 1, 3, 3                                                   # nine (row, head) pairs: less than one block's 16
    xr = rnd(Bx, L, 2 * Hh * D, seed=74, scale=3.0)
    w, cos, sin = 1.0 + f32(Hh, D, seed=75), f32(L + 2, D, seed=76), f32(L + 2, D, seed=77)
    written = lambda m: ops.Mxfp8(m.codes[..., :Hh * D], m.scales[..., :Hh * D // 32])      # noqa: E731  (the other columns are not the call's)
    wantr = guard(lambda E: written(ops.rmsnorm_rope_mxfp8(E(xr), E(w), E(cos), E(sin), Hh, D, pos0=2)))
    fc = _fence((Bx, L, 2 * Hh * D), torch.uint8).window(Ellipsis, slice(0, Hh * D))          # the first heads * head_dim columns only
    fs = _fence((Bx, L, 2 * Hh * D // 32), torch.uint8).window(Ellipsis, slice(0, Hh * D // 32))
    ops.rmsnorm_rope_mxfp8(xr, w, cos, sin, Hh, D, pos0=2, out=ops.Mxfp8(fc.out, fs.out))
    fc.check(); fs.check()
    assert_same_bytes((fc.out[..., :Hh * D], fs.out[..., :Hh * D // 32]), wantr, "rmsnorm_rope_mxfp8(out=)")


def test_rmsnorm_rope_in_place_window():
    """B, L, H = 1, 3, 3 at col0 = H D of a 2 H D wide row: nine (row, head) pairs, less than one block's 16; columns [0, col0) keep their bytes."""
    ops = _ops()
    B, L, H, D = 1, 3, 3, 128
    col0 = H * D
    x = rnd(B, L, 2 * H * D, seed=36)
    w, cos, sin = 1.0 + f32(H, D, seed=37), f32(L + 8, D, seed=38), f32(L + 8, D, seed=39)
    want = ops.rmsnorm_rope_(x.clone(), w, cos, sin, H, D, col0=col0, pos0=8)
    assert bool(torch.isfinite(want.float()).all()) and torch.equal(want[..., :col0], x[..., :col0])
    f = _fence((B, L, 2 * H * D)).window(Ellipsis, slice(col0, 2 * col0))
    f.out[..., col0:] = x[..., col0:]
    ops.rmsnorm_rope_(f.out, gb.embed(w), gb.embed(cos), gb.embed(sin), H, D, col0=col0, pos0=8)
    f.check()
    assert_same_bytes(f.out[..., col0:], want[..., col0:], "rmsnorm_rope_ window")
    ex = gb.embed(x)                                                      # read side: the rows themselves between NaN bands
    assert_same_bytes(ops.rmsnorm_rope_(ex, w, cos, sin, H, D, col0=col0, pos0=8), want, "rmsnorm_rope_ embedded")


def test_paste_and_tile_accumulate_windows():
    ops = _ops()
    src = rnd(2, 9, 11, 8, seed=80)
    call = lambda buf: ops.paste_nhwc(src, buf, 2, 3, 4, 5, 5, 6)         # noqa: E731  dst[:, 4:9, 5:11] = src[:, 2:7, 3:9]
    f = _fence((2, 12, 14, 8)).window(slice(None), slice(4, 9), slice(5, 11))
    call(f.out)
    f.check()
    assert_same_bytes(f.out[:, 4:9, 5:11], src[:, 2:7, 3:9], "paste_nhwc")
    f = _fence((2, 12, 14, 8)).window(slice(None), slice(4, 9), slice(5, 11))
    ops.paste_nhwc(gb.embed(src), f.out, 4, 5, 4, 5, 5, 6)                # the source window ends at the source's last row and column
    f.check()
    assert_same_bytes(f.out[:, 4:9, 5:11], src[:, 4:9, 5:11], "paste_nhwc from an embedded source")
    # tile_accumulate at an interior window of the accumulator, and of the weight-sum plane
    N, H, W, Cc, th, tw, y0, x0 = 2, 12, 10, 4, 6, 5, 3, 2
    tile, wt, acc0 = rnd(N, th, tw, 8, seed=81), f32(th, tw, seed=82).abs() + 0.1, f32(N, H, W, Cc, seed=83)
    want = acc0.clone()
    ops.tile_accumulate(tile, wt, want, y0, x0)
    f = _fence((N, H, W, Cc), torch.float32).window(slice(None), slice(y0, y0 + th), slice(x0, x0 + tw))
    f.out[:, y0:y0 + th, x0:x0 + tw] = acc0[:, y0:y0 + th, x0:x0 + tw]
    ops.tile_accumulate(gb.embed(tile), gb.embed(wt), f.out, y0, x0)
    f.check()
    assert_same_bytes(f.out[:, y0:y0 + th, x0:x0 + tw], want[:, y0:y0 + th, x0:x0 + tw], "tile_accumulate")
    f = _fence((1, H, W, 1), torch.float32).window(slice(None), slice(y0, y0 + th), slice(x0, x0 + tw))
    f.out[:, y0:y0 + th, x0:x0 + tw] = 0.0
    ops.tile_accumulate(None, wt, f.out, y0, x0)
    f.check()
    assert_same_bytes(f.out[0, y0:y0 + th, x0:x0 + tw, 0], wt, "tile_accumulate(weights alone)")


# ---- negative controls: both assertions bite (every access inside the test's own allocations) ---------------------------------------------------

def test_negative_control_a_read_past_the_operand_raises():
    """crop_nhwc told that the embedded tensor has one more image row than it has: the crop window reaches that row, which is the band behind it."""
    ops = _ops()
    N, H, W, Cc = 1, 9, 11, 8
    t = torch.zeros(N, H + 1, W, Cc, device=DEV, dtype=ops.act_dtype())
    t[:, :H] = rnd(N, H, W, Cc, seed=45)
    want = ops.crop_nhwc(t, 5, 3, 5, 5)                                   # rows 5 .. 9: the last one is the zero row of a dense allocation
    e = gb.embed(t[:, :H].contiguous())
    assert gb.band_bytes(e.shape, e.element_size()) >= W * Cc * e.element_size()
    taller = e.as_strided((N, H + 1, W, Cc), e.stride())                  # the declared extra row lies wholly inside the band
    got = ops.crop_nhwc(taller, 5, 3, 5, 5)
    assert _finite(want) and not _finite(got)
    with pytest.raises(AssertionError, match="non-finite"):
        assert_same_bytes(got, want, "embedded operands")
    assert_same_bytes(got[:, :4], want[:, :4], "rows inside the tensor")


def test_negative_control_a_write_past_the_window_raises():
    ops = _ops()
    src = rnd(2, 9, 11, 8, seed=80)
    f = _fence((2, 12, 14, 8)).window(slice(None), slice(4, 9), slice(5, 11))
    ops.paste_nhwc(src, f.out, 2, 3, 4, 5, 6, 6)                          # one pixel row taller than the declared window (inside the output)
    with pytest.raises(AssertionError, match="outside the window"):
        f.check()
