"""The fp8 tier's fused MXFP8 producers on the MI355X: a producer that writes its MXFP8 output itself (LayerNorm + modulate, the MXFP8 GEMM's
OUT8 epilogue, the strided quantiser) must write THE BYTES of today's chain "producer writes bf16, omgsr_quantize_mxfp8 reads it" - every
comparison here is torch.equal on the code plane and on the scale plane. Then the guard bands around the new kernels, the small OMGSR-F
pipeline with the switch on and off, and a repeat soak per kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as gb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6


@pytest.fixture(autouse=True)
def _bf16_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _eq(got, want_codes, want_scales, what=""):
    """torch.equal on both planes; the mismatch counts are printed first (a failing run leaves the figures in the log)."""
    bad_s = int((got.scales != want_scales).sum())
    bad_c = int((got.codes != want_codes).sum())
    if bad_s or bad_c:
        print(f"{what}: {bad_c} of {got.codes.numel()} codes and {bad_s} of {got.scales.numel()} scale bytes differ")
    assert torch.equal(got.scales, want_scales) and torch.equal(got.codes, want_codes), (what, bad_c, bad_s)


# ---- LayerNorm + modulate -> MXFP8 -----------------------------------------------------------------------------------------------------
# C: every wave-per-rows form (MAXCH 1: 128, 512; 2: 640, 1024; 3: 1536 - a partly filled and a full last chunk each) and the block-per-row
# form with one chunk per thread (1664) and two (3072 partly filled, 4096 full). rows 37 is no multiple of 4 x RPW (16 / 8).
LN_C = [128, 512, 640, 1024, 1536, 1664, 3072, 4096]
_ln_cache = {}


def _ln_case(C, rows):
    """(x bf16, a, b) shared by the tests of one shape: randn rows scaled by 2^-20 ... 2^20, one all-zero row, one row whose 32-value blocks
    have their largest magnitude exactly on a power of two."""
    key = (C, rows)
    if key not in _ln_cache:
        g = torch.Generator().manual_seed(1000 * C + rows)
        x = torch.randn(rows, C, generator=g) * torch.exp2(torch.linspace(-20, 20, rows))[:, None]
        if rows > 8:
            x[5] = 0.0
            row = torch.randn(C, generator=g).clamp(-0.9, 0.9).view(C // 32, 32)
            row[:, 3] = torch.tensor([(-1.0) ** j * 2.0 ** (j % 7 - 3) for j in range(C // 32)])
            x[7] = row.view(C)
        a = (torch.randn(C, generator=g) * 0.5 + 1.0).to(DEV)
        b = (torch.randn(C, generator=g) * 0.3).to(DEV)
        _ln_cache[key] = (x.to(torch.bfloat16).to(DEV), a, b)
    return _ln_cache[key]


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("C", LN_C)
def test_layer_norm_mxfp8_equals_the_pass_form(C, rows, affine):
    from omgsr_amd import ops
    x, a, b = _ln_case(C, rows)
    a, b = (a, b) if affine else (None, None)
    want = ops.quantize_mxfp8(ops.layer_norm(x, a, b, EPS))
    got = ops.layer_norm_mxfp8(x, a, b, EPS)
    assert got.codes.shape == (rows, C) and got.scales.shape == (rows, C // 32)
    _eq(got, want.codes, want.scales, f"layer_norm_mxfp8 C={C} rows={rows} vs pass form")
    # out=: the same bytes in a caller's workspace, which is what comes back
    ws = ops.Mxfp8(torch.full((rows, C), 0xAB, dtype=torch.uint8, device=DEV), torch.full((rows, C // 32), 0xAB, dtype=torch.uint8, device=DEV))
    back = ops.layer_norm_mxfp8(x, a, b, EPS, out=ws)
    assert back.codes.data_ptr() == ws.codes.data_ptr() and back.scales.data_ptr() == ws.scales.data_ptr()
    _eq(ws, want.codes, want.scales, f"layer_norm_mxfp8 C={C} rows={rows} out=")
    # only `a`, only `b`
    if affine and rows == 37:
        for aa, bb in ((a, None), (None, b)):
            w2 = ops.quantize_mxfp8(ops.layer_norm(x, aa, bb, EPS))
            _eq(ops.layer_norm_mxfp8(x, aa, bb, EPS), w2.codes, w2.scales, f"layer_norm_mxfp8 C={C} one affine vector")


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("C", LN_C)
def test_layer_norm_mxfp8_equals_the_host_reference(C, rows, affine):
    from omgsr_amd import ops
    from omgsr_amd.testing import layer_norm_mxfp8_ref
    x, a, b = _ln_case(C, rows)
    a, b = (a, b) if affine else (None, None)
    want_c, want_s = layer_norm_mxfp8_ref(x, a, b, EPS)
    _eq(ops.layer_norm_mxfp8(x, a, b, EPS), want_c, want_s, f"layer_norm_mxfp8 C={C} rows={rows} affine={affine} vs layer_norm_mxfp8_ref")


def test_layer_norm_mxfp8_refuses_what_it_does_not_run():
    from omgsr_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(4, 4224, dtype=torch.bfloat16, device=DEV)
    c, s = torch.zeros(4, 4224, dtype=torch.uint8, device=DEV), torch.zeros(4, 132, dtype=torch.uint8, device=DEV)
    call = lambda C, el, cld, sld: lib.omgsr_layernorm_mxfp8(x.data_ptr(), None, None, 4, C, EPS, el, c.data_ptr(), s.data_ptr(), cld, sld, ops._stream())
    assert call(4224, ops.EL_16, 4224, 132) == -2            # C > 4096
    assert call(192, ops.EL_16, 192, 6) == -2                # C % 128
    assert call(256, ops.EL_F32, 256, 8) == -2               # fp32 input
    assert call(256, ops.EL_16, 128, 8) == -2 and call(256, ops.EL_16, 256, 4) == -2        # pitches shorter than the row
    ops.set_compute_dtype(torch.float16)
    try:
        assert call(256, ops.EL_16, 256, 8) == -2            # fp16 compute type
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    with pytest.raises(ValueError):
        ops.layer_norm_mxfp8(x[:, :192].contiguous(), None, None, EPS)
    with pytest.raises(ValueError):
        ops.layer_norm_mxfp8(x.float(), None, None, EPS)


# ---- MXFP8 out of the MXFP8 GEMM's epilogue (OUT8) -------------------------------------------------------------------------------------

_gemm_cache = {}


def _gemm_problem(M, K, N, cout, bias):
    from omgsr_amd import ops
    key = (M, K, N, cout, bias)
    if key not in _gemm_cache:
        g = torch.Generator(device=DEV).manual_seed(M + 7 * K + 13 * cout + bias)
        # rows scaled over 2^-6 ... 2^6: the output blocks take many different scale bytes
        x = (torch.randn(M, K, generator=g, device=DEV) * torch.exp2(torch.linspace(-6, 6, M, device=DEV))[:, None]).to(torch.bfloat16)
        w = (torch.randn(cout, K, generator=g, device=DEV) / K ** 0.5).to(torch.bfloat16)
        b = torch.randn(cout, generator=g, device=DEV) * 0.5 if bias else None
        pw = ops.pack_linear_weight_mxfp8(w, b)
        assert pw.cout_pad == N
        _gemm_cache[key] = (ops.quantize_mxfp8(x), pw)
    return _gemm_cache[key]


def _pass_form(xq, pw, act):
    """Today's chain: the GEMM writes bf16, the quantiser reads it (Cout padded with zero columns to whole 128s for the quantiser)."""
    from omgsr_amd import ops
    y = ops.linear(xq, pw, act=act, out_dtype=ops.OUT_BF16)
    Kq = -(-pw.cout // 128) * 128
    if Kq != pw.cout:
        y = torch.cat([y, torch.zeros(y.shape[0], Kq - pw.cout, dtype=y.dtype, device=y.device)], 1)
    q = ops.quantize_mxfp8(y.contiguous())
    return q.codes[:, :pw.cout], q.scales[:, :pw.cout // 32]


def _traced(fn):
    """fn() with the library's timing trace on: (result, [(kind, variant)])."""
    from omgsr_amd import _lib
    lib = _lib.load()
    lib.omgsr_timing_enable(1); lib.omgsr_timing_reset()
    try:
        r = fn()
        buf = (_lib.TimingEntry * 8192)()
        n = lib.omgsr_timing_collect(buf, 8192)
    finally:
        lib.omgsr_timing_enable(0)
    return r, [(e.kind, e.variant) for e in buf[:n]]


TK_IGEMM = 1           # OMGSR_TK_IGEMM; the elementwise and LayerNorm kinds are read off the library's own trace (_kinds)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("N,cout", [(256, 256), (512, 480)])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [37, 256 + 37])
def test_gemm_out8_equals_the_pass_form(M, K, N, cout, act, bias):
    from omgsr_amd import ops
    act = ops.ACT_GELU_TANH if act == "gelu" else ops.ACT_NONE
    xq, pw = _gemm_problem(M, K, N, cout, bias)
    (want_c, want_s), tr_pass = _traced(lambda: _pass_form(xq, pw, act))
    assert [v for k, v in tr_pass if k == TK_IGEMM] == [18]
    # dense: a destination of whole 128-column groups (Cout = 480: columns 480 ... 511 are not the GEMM's to write)
    Kw = -(-cout // 128) * 128
    dst = ops.Mxfp8(torch.full((M, Kw), 0xAB, dtype=torch.uint8, device=DEV), torch.full((M, Kw // 32), 0xAB, dtype=torch.uint8, device=DEV))
    got, tr = _traced(lambda: ops.linear(xq, pw, act=act, out_mxfp8=dst))
    assert [(k, v) for k, v in tr] == [(TK_IGEMM, 18)]                        # one launch, the MXFP8 GEMM, nothing else
    assert got is dst
    _eq(ops.Mxfp8(dst.codes[:, :cout], dst.scales[:, :cout // 32]), want_c, want_s, f"OUT8 dense M={M} K={K} Cout={cout}")
    assert bool((dst.codes[:, cout:] == 0xAB).all()) and bool((dst.scales[:, cout // 32:] == 0xAB).all())
    if cout % 128 == 0:
        fresh = ops.linear(xq, pw, act=act, out_mxfp8=True)
        _eq(fresh, want_c, want_s, f"OUT8 out_mxfp8=True M={M} K={K} Cout={cout}")
    # a slice: the small pipeline's cat8 - rows of 1280 codes / 40 scale bytes, the result at column 256
    ld, col0, rows = 1280, 256, M + 3
    cat8 = ops.Mxfp8(torch.full((rows, ld), 0xCD, dtype=torch.uint8, device=DEV), torch.full((rows, ld // 32), 0xCD, dtype=torch.uint8, device=DEV))
    _, tr = _traced(lambda: ops.linear_into(xq, pw, None, 2, col0, act=act, out_mxfp8=cat8))
    assert [(k, v) for k, v in tr] == [(TK_IGEMM, 18)]
    _eq(ops.Mxfp8(cat8.codes[2:2 + M, col0:col0 + cout], cat8.scales[2:2 + M, col0 // 32:(col0 + cout) // 32]), want_c, want_s,
        f"OUT8 slice M={M} K={K} Cout={cout}")
    mc = torch.ones_like(cat8.codes, dtype=torch.bool); mc[2:2 + M, col0:col0 + cout] = False
    ms = torch.ones_like(cat8.scales, dtype=torch.bool); ms[2:2 + M, col0 // 32:(col0 + cout) // 32] = False
    assert bool((cat8.codes[mc] == 0xCD).all()) and bool((cat8.scales[ms] == 0xCD).all())


def test_gemm_out8_refused_by_the_library():
    """omgsr_igemm_out_mxfp8 with a residual, a gate, GroupNorm statistics, out_lo_off, LAYOUT_T or a problem that is not mxf8: OMGSR_E_SHAPE,
    never another kernel; omgsr_igemm itself knows no out_mx = 8."""
    import ctypes as C
    from omgsr_amd import _lib, ops
    from omgsr_amd._lib import IgemmArgs
    xq, pw = _gemm_problem(37, 128, 256, 256, True)
    dst = ops.Mxfp8(torch.zeros(37, 256, dtype=torch.uint8, device=DEV), torch.zeros(37, 8, dtype=torch.uint8, device=DEV))
    other = torch.zeros(37, 256, dtype=torch.float32, device=DEV)

    def args():
        a = IgemmArgs()
        ops._fill_mxfp8(a, xq.codes.data_ptr(), xq.scales.data_ptr(), pw)
        ops._fill_gemm(a, 37)
        scale = ops._fill_out_mxfp8(a, dst, 0, 0)
        a.alpha = 1.0
        return a, scale
    lib = _lib.load()
    go = lambda a, scale: lib.omgsr_igemm_out_mxfp8(C.byref(a), scale[0], scale[1], ops._stream())
    assert go(*args()) == 0
    for field, value in (("residual", other.data_ptr()), ("gate", other.data_ptr()), ("gn_partial", other.data_ptr()), ("out_lo_off", 256),
                         ("out_layout", ops.LAYOUT_T), ("out_dtype", ops.OUT_F32), ("out_ld", 264), ("mxf8", 0), ("out_mx", 1)):
        a, scale = args()
        setattr(a, field, value)
        assert go(a, scale) == -2, field
    a, scale = args()
    assert go(a, (scale[0], 4)) == -2                          # a scale pitch shorter than Cout / 32
    assert go(a, (None, scale[1])) == -1                       # no scale plane
    a.out_mx = 8
    assert lib.omgsr_igemm(C.byref(a), ops._stream()) == -1    # not a value of the argument block


# ---- strided quantiser -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantize_into_columns_equals_dense(dtype):
    from omgsr_amd import ops
    rows, K, Kw, ld = 75, 256, 640, 384
    g = torch.Generator().manual_seed(9)
    src = (torch.randn(3, rows // 3, ld, generator=g) * torch.exp2(torch.randint(-30, 30, (3, rows // 3, 1), generator=g).float())).to(dtype).to(DEV)
    x = src[..., 128:128 + K]                                   # a column window of a dense tensor, as cat[..., :D] is
    want = ops.quantize_mxfp8(x.contiguous())
    for col in range(0, Kw - K + 1, 128):
        out = ops.Mxfp8(torch.full((3, rows // 3, Kw), 0xAB, dtype=torch.uint8, device=DEV), torch.full((3, rows // 3, Kw // 32), 0xAB, dtype=torch.uint8, device=DEV))
        assert ops.quantize_mxfp8(x, out=out, out_col=col) is out
        _eq(ops.Mxfp8(out.codes[..., col:col + K], out.scales[..., col // 32:(col + K) // 32]), want.codes, want.scales, f"quantize out_col={col}")
        out.codes[..., col:col + K] = 0xAB
        out.scales[..., col // 32:(col + K) // 32] = 0xAB
        assert bool((out.codes == 0xAB).all()) and bool((out.scales == 0xAB).all())
        # a dense source too
        out2 = ops.Mxfp8(torch.zeros_like(out.codes), torch.zeros_like(out.scales))
        ops.quantize_mxfp8(x.contiguous(), out=out2, out_col=col)
        _eq(ops.Mxfp8(out2.codes[..., col:col + K], out2.scales[..., col // 32:(col + K) // 32]), want.codes, want.scales, f"quantize dense out_col={col}")


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,rows", [(256, 37), (1536, 5), (3072, 3)])
def test_guard_bands_layer_norm_mxfp8(C, rows):
    from omgsr_amd import ops
    x, a, b = _ln_case(C, 37)
    x = x[:rows].contiguous()
    want = ops.layer_norm_mxfp8(x, a, b, EPS)
    fc, fs = gb.Fence((rows, C), torch.uint8, DEV), gb.Fence((rows, C // 32), torch.uint8, DEV)
    ops.layer_norm_mxfp8(gb.embed(x), gb.embed(a), gb.embed(b), EPS, out=ops.Mxfp8(fc.out, fs.out))
    torch.cuda.synchronize()
    fc.check(); fs.check()
    assert torch.equal(fc.out, want.codes) and torch.equal(fs.out, want.scales)      # a read from a NaN band would have changed the result


@pytest.mark.parametrize("M,cout,N", [(37, 256, 256), (293, 480, 512)])
def test_guard_bands_gemm_out8_slice(M, cout, N):
    """The cat8 slice inside fenced planes: columns outside [256, 256 + Cout), rows past M and the padded columns past Cout keep every byte."""
    from omgsr_amd import ops
    xq, pw = _gemm_problem(M, 384, N, cout, True)
    want_c, want_s = _pass_form(xq, pw, ops.ACT_GELU_TANH)
    rows, ld, col0 = M + 5, 1280, 256
    fc, fs = gb.Fence((rows, ld), torch.uint8, DEV), gb.Fence((rows, ld // 32), torch.uint8, DEV)
    fc.window(slice(1, 1 + M), slice(col0, col0 + cout)); fs.window(slice(1, 1 + M), slice(col0 // 32, (col0 + cout) // 32))
    ops.linear_into(gb.embed(xq), gb.embed(pw), None, 1, col0, act=ops.ACT_GELU_TANH, out_mxfp8=ops.Mxfp8(fc.out, fs.out))
    torch.cuda.synchronize()
    fc.check(); fs.check()
    assert torch.equal(fc.out[1:1 + M, col0:col0 + cout], want_c) and torch.equal(fs.out[1:1 + M, col0 // 32:(col0 + cout) // 32], want_s)


def test_guard_bands_quantize_into_columns():
    from omgsr_amd import ops
    rows, K, Kw = 37, 256, 1280
    g = torch.Generator().manual_seed(4)
    x = torch.randn(rows, K, generator=g).to(torch.bfloat16).to(DEV)
    want = ops.quantize_mxfp8(x)
    fc, fs = gb.Fence((rows, Kw), torch.uint8, DEV), gb.Fence((rows, Kw // 32), torch.uint8, DEV)
    fc.window(slice(None), slice(0, K)); fs.window(slice(None), slice(0, K // 32))
    ops.quantize_mxfp8(gb.embed(x), out=ops.Mxfp8(fc.out, fs.out), out_col=0)
    torch.cuda.synchronize()
    fc.check(); fs.check()
    assert torch.equal(fc.out[:, :K], want.codes) and torch.equal(fs.out[:, :K // 32], want.scales)


# ---- the pipeline: test_fp8_gpu.py's small case (2 double + 2 single blocks, dim 256) ---------------------------------------------------

def _kinds():
    """Timing kinds by what the library itself reports for a known launch (the header's OMGSR_TK_* values are not mirrored in Python)."""
    from omgsr_amd import ops
    x = torch.randn(4, 256, device=DEV).to(torch.bfloat16)
    _, q = _traced(lambda: ops.quantize_mxfp8(x))
    _, l = _traced(lambda: ops.layer_norm(x, None, None, EPS))
    return q[0][0], l[0][0]


def _run_small(fused: bool, policy=None, calls=1, batch_invariant=False, graphs=False, count=False):
    """The small fp8-tier pipeline with the fused producers on / off: (outputs, elementwise launches of the last call)."""
    import test_fp8_gpu as base
    from omgsr_amd import ops
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    vae, flux, inp = base._small_case()
    saved = dict(ops.FP8_FUSED_QUANT)
    ops.FP8_FUSED_QUANT.update(layernorm=fused, gemm=fused)
    try:
        pipe = OMGSR_F_Infer(None, None, DEV, torch.float8_e4m3fn, 244, 1.0, vae=vae, flux_transformer=flux, precision_policy=policy)
        ops.set_batch_invariant(batch_invariant)
        outs, trace = [], []
        with torch.no_grad():
            if graphs:
                pipe.enable_graphs(True)
            for i in range(calls):
                if count and i == calls - 1:
                    y, trace = _traced(lambda: base._call(pipe, inp, inp["xs"][i], inp["ns"][0]))
                else:
                    y = base._call(pipe, inp, inp["xs"][i], inp["ns"][0])
                outs.append(y.clone())
            if batch_invariant:
                outs.append(base._call(pipe, inp, torch.cat(inp["xs"][:2]), torch.cat([inp["ns"][0]] * 2)).clone())
        return outs, trace, pipe
    finally:
        ops.set_batch_invariant(False)
        ops.FP8_FUSED_QUANT.clear(); ops.FP8_FUSED_QUANT.update(saved)


def test_pipeline_fused_equals_pass_form_with_fewer_elementwise_launches():
    """Per double block the fused form drops the quantise passes behind its four LayerNorms and its two feed-forward hiddens (6; the attention
    output keeps its pass). Per single block it drops the pass behind the LayerNorm (1): proj_out's operand still takes one pass, over the
    attention output's D columns instead of the whole [attn | mlp] row. 2 double + 2 single blocks: 2 x 6 + 2 x 1 = 14 launches fewer."""
    tk_elt, tk_ln = _kinds()
    (on,), tr_on, _ = _run_small(True, count=True)
    (off,), tr_off, _ = _run_small(False, count=True)
    assert torch.isfinite(on.float()).all() and torch.equal(on, off)
    n_on, n_off = sum(1 for k, _ in tr_on if k == tk_elt), sum(1 for k, _ in tr_off if k == tk_elt)
    print(f"elementwise launches: fused {n_on}, pass form {n_off}")
    assert n_off - n_on == 2 * 6 + 2 * 1
    assert sum(1 for k, _ in tr_on if k == tk_ln) == sum(1 for k, _ in tr_off if k == tk_ln)            # the LayerNorms are the same launches
    assert sum(1 for k, v in tr_on if k == TK_IGEMM and v == 18) == sum(1 for k, v in tr_off if k == TK_IGEMM and v == 18)


def test_pipeline_fused_batch_invariant_and_graph_replay():
    outs, _, _ = _run_small(True, calls=2, batch_invariant=True)
    a, b, ab = outs
    assert torch.equal(ab[0:1], a) and torch.equal(ab[1:2], b)
    eager, _, _ = _run_small(True, calls=3)
    got, _, pipe = _run_small(True, calls=3, graphs=True)
    assert pipe.graphs.captures == 1 and pipe.graphs.replays == 2
    for e, g in zip(eager, got):
        assert torch.equal(e, g)


def test_pipeline_narrowed_policy_equals_switch_off():
    """proj_mlp left in bf16: the single blocks' LayerNorm has a bf16 reader and there is no MXFP8 hidden to write - that producer takes today's
    path; the double blocks still fuse. Bit for bit the same policy with the switch off."""
    from omgsr_amd.precision import FP8_ELIGIBLE, fp8_layers
    narrowed = [p for p in FP8_ELIGIBLE if "proj_mlp" not in p] + [r"^single_transformer_blocks\.\d+\.proj_out$"]
    policy = {"flux": {"fp8": narrowed}}
    tk_elt, _ = _kinds()
    (on,), tr_on, pipe = _run_small(True, policy=policy, count=True)
    assert len(fp8_layers(pipe.flux_transformer)) == 2 * 12 + 2 * 4
    (off,), tr_off, _ = _run_small(False, policy=policy, count=True)
    assert torch.equal(on, off)
    assert sum(1 for k, _ in tr_off if k == tk_elt) - sum(1 for k, _ in tr_on if k == tk_elt) == 2 * 6          # the double blocks only


# ---- repeat soak: 50 launches, the same bytes ------------------------------------------------------------------------------------------

def _soak(fn):
    first = fn()
    c0, s0 = first.codes.clone(), first.scales.clone()
    for _ in range(49):
        r = fn()
        assert torch.equal(r.codes, c0) and torch.equal(r.scales, s0)


@pytest.mark.parametrize("C", [1536, 3072])
def test_soak_layer_norm_mxfp8(C):
    from omgsr_amd import ops
    x, a, b = _ln_case(C, 37)
    _soak(lambda: ops.layer_norm_mxfp8(x, a, b, EPS))


def test_soak_gemm_out8():
    from omgsr_amd import ops
    xq, pw = _gemm_problem(293, 384, 512, 480, True)

    def go():
        dst = ops.Mxfp8(torch.zeros(293, 512, dtype=torch.uint8, device=DEV), torch.zeros(293, 16, dtype=torch.uint8, device=DEV))
        return ops.linear(xq, pw, act=ops.ACT_GELU_TANH, out_mxfp8=dst)
    _soak(go)


def test_soak_quantize_into_columns():
    from omgsr_amd import ops
    x = torch.randn(293, 256, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)

    def go():
        dst = ops.Mxfp8(torch.zeros(293, 1280, dtype=torch.uint8, device=DEV), torch.zeros(293, 40, dtype=torch.uint8, device=DEV))
        return ops.quantize_mxfp8(x, out=dst, out_col=256)
    _soak(go)
