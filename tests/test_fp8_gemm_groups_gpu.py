"""The fp8 tier's launch groups of MXFP8 token GEMMs (omgsr_igemm_mxfp8_multi, mxfp8_gemm_multi_kernel, ops.gemm_group, timing variant 24).

What a group promises is that nothing but the number of launches changes: every problem's output holds the bytes of its own omgsr_igemm call
(variant 18), so the checks here are torch.equal - against separate calls, against the float64 restatement of dyadic operands
(tests/dyadic_probe.py), between two launches of one group, and between the small seeded pipeline with the groups on and off."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyadic_probe as dp  # noqa: E402
import guard_bands as gb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TK_IGEMM = 1            # OMGSR_TK_IGEMM
E_SHAPE = -2            # OMGSR_E_SHAPE

# (M, N, K): a ragged last row tile; one K-tile; an odd K-tile count (3) with ragged M; ten row tiles (an M-group of 8 and a remainder of 2,
# and 6 filler blocks behind its 10 tiles)
SHAPES = [(520, 512, 256), (256, 256, 128), (100, 768, 384), (2344, 256, 128)]


@pytest.fixture(autouse=True)
def _bf16_tier():
    from omgsr_amd import ops
    ops.set_compute_dtype(torch.bfloat16)
    yield
    ops.set_compute_dtype(torch.bfloat16)


def _traced(fn):
    """fn() with the library's timing trace on: (result, [variant of every igemm launch])."""
    from omgsr_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.omgsr_timing_enable(1); lib.omgsr_timing_reset()
    try:
        r = fn()
        buf = (_lib.TimingEntry * 8192)()
        n = lib.omgsr_timing_collect(buf, 8192)
    finally:
        lib.omgsr_timing_enable(0)
    return r, [e.variant for e in buf[:n] if e.kind == TK_IGEMM]


def _rand(g, *shape, dtype=torch.bfloat16, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


_CACHE = {}


def _layer(shape_id, cout=None):
    """(operand Mxfp8 [M, K], fp8-packed weight with bias) of SHAPES[shape_id], made once; cout < N leaves padded weight rows (Cout_pad = N)."""
    from omgsr_amd import ops
    key = (shape_id, cout)
    if key not in _CACHE:
        M, N, K = SHAPES[shape_id]
        g = torch.Generator().manual_seed(100 + shape_id)
        xq = ops.quantize_mxfp8(_rand(g, M, K))
        pw = ops.pack_linear_weight_mxfp8(_rand(g, cout or N, K, scale=K ** -0.5), _rand(g, cout or N, dtype=torch.float32))
        _CACHE[key] = (xq, pw)
    return _CACHE[key]


def _fill(shape, dtype=torch.bfloat16):
    """A destination buffer with known finite contents (what a slice write must leave alone)."""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, device=DEV) % 251).float() / 16 - 7).to(dtype).reshape(shape)


# ---- the four epilogue kinds of the issue; each returns the tensor(s) the launch writes --------------------------------------------------

def _p_bias_gelu(sid):
    from omgsr_amd import ops
    xq, pw = _layer(sid)
    return ops.linear(xq, pw, act=ops.ACT_GELU_TANH, out_dtype=ops.OUT_BF16)


def _p_gate_res32(sid):
    from omgsr_amd import ops
    xq, pw = _layer(sid)
    M, N, _ = SHAPES[sid]
    g = torch.Generator().manual_seed(200 + sid)
    return ops.linear(xq, pw, gate=_rand(g, N, dtype=torch.float32), residual=_rand(g, M, N, dtype=torch.float32), out_dtype=ops.OUT_F32)


def _p_t_slice(sid, cout=None):
    from omgsr_amd import ops
    xq, pw = _layer(sid, cout)
    M, N, _ = SHAPES[sid]
    out_t = _fill((cout or N, M + 24))
    ops.linear_t_into(xq, pw, out_t, 16)
    return out_t


def _batched(sid):
    """Two images of SHAPES[sid]'s M // 2 rows each (the operand's rows split in two)."""
    from omgsr_amd import ops
    xq, pw = _layer(sid)
    M, _, K = SHAPES[sid]
    m = M // 2
    return ops.Mxfp8(xq.codes[:2 * m].reshape(2, m, K), xq.scales[:2 * m].reshape(2, m, K // 32)), pw, m


def _p_into_b2(sid):
    from omgsr_amd import ops
    xb, pw, m = _batched(sid)
    out = _fill((2, m + 9, SHAPES[sid][1] + 128))
    ops.linear_into(xb, pw, out, 5, 64)
    return out


def _p_t_b2(sid):
    from omgsr_amd import ops
    xb, pw, m = _batched(sid)
    out_t = _fill((2, SHAPES[sid][1], m + 16))
    ops.linear_t_into(xb, pw, out_t, 8)
    return out_t


def _p_rows_b2(sid):
    from omgsr_amd import ops
    xb, pw, m = _batched(sid)
    g = torch.Generator().manual_seed(300 + sid)
    N = SHAPES[sid][1]
    return ops.linear_rows(xb, 3, m - 7, pw, gate=_rand(g, N, dtype=torch.float32), residual=_rand(g, 2, m - 7, N))


GROUPS = {
    "two": [(_p_bias_gelu, 0), (_p_gate_res32, 1)],
    "three_t_first": [(_p_t_slice, 3), (_p_bias_gelu, 2), (_p_gate_res32, 0)],
    "four": [(_p_gate_res32, 3), (_p_t_slice, 2), (_p_bias_gelu, 1), (_p_bias_gelu, 0)],
    "grid_z_2": [(_p_into_b2, 2), (_p_t_b2, 1), (_p_rows_b2, 0)],
    "grid_z_2_pair": [(_p_rows_b2, 3), (_p_into_b2, 0)],
}


def _p_t_slice_c300(sid):
    """Cout = 300 under the weight's 512 padded rows (SHAPES[0]): room for the Cout_pad = 384 refusal to be about Cout_pad alone."""
    return _p_t_slice(sid, cout=300)


def _separate(members):
    return [fn(sid) for fn, sid in members]


def _grouped(members):
    from omgsr_amd import ops
    with ops.gemm_group():
        outs = [fn(sid) for fn, sid in members]
    return outs


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_group_equals_separate_calls(name):
    members = GROUPS[name]
    want, tr_w = _traced(lambda: _separate(members))
    got, tr_g = _traced(lambda: _grouped(members))
    assert tr_w == [18] * len(members)
    assert tr_g == [24], f"one launch of variant 24 and none of variant 18 expected, the trace shows {tr_g}"
    for i, (w, y) in enumerate(zip(want, got)):
        assert torch.isfinite(w.float()).all()
        assert w.dtype == y.dtype and torch.equal(w, y), f"{name}: member {i} differs from its own launch"


def test_group_is_repeatable():
    a = _grouped(GROUPS["four"])
    b = _grouped(GROUPS["four"])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_launch_counting():
    """A group of one is mxfp8_gemm_kernel's launch; five problems run as 4 + 1."""
    one, tr1 = _traced(lambda: _grouped([(_p_bias_gelu, 0)]))
    assert tr1 == [18]
    five = [(_p_bias_gelu, 0), (_p_gate_res32, 1), (_p_t_slice, 2), (_p_bias_gelu, 3), (_p_gate_res32, 0)]
    got, tr5 = _traced(lambda: _grouped(five))
    assert tr5 == [24, 18]
    want = _separate(five)
    assert all(torch.equal(w, y) for w, y in zip(want, got)) and torch.equal(one[0], want[0])


# ---- dyadic operands: bit for bit against the float64 restatement ------------------------------------------------------------------------

def test_dyadic_group_matches_the_exact_restatement():
    """Three problems with their own scale patterns (seed, spread, density), sizes and epilogues in one launch: a tile that read another
    problem's operand, weight, scales or epilogue terms is off by powers of two."""
    import test_dyadic_probes_gpu as probes
    from omgsr_amd import ops
    specs = [dict(seed=2401, M=300, N=256, K=384, density=1 / 2, spread=40, out=torch.float32),
             dict(seed=2402, M=37, N=200, K=128, density=1.0, spread=12, out=torch.bfloat16),
             dict(seed=2403, M=2100, N=512, K=256, density=1 / 4, spread=25, out=torch.float32)]
    built = []
    for s in specs:
        g = probes._g(s["seed"])
        ac, asc, wc, wsc, r_e, t = probes._mxfp8_pair(g, s["M"], s["N"], s["K"], s["density"], spread=s["spread"])
        pw = probes._mxfp8_weight(DEV, wc, wsc, probes._scaled(g, t[0]))
        xq = ops.Mxfp8(ac.to(DEV), asc.to(DEV))
        if s["out"] == torch.bfloat16:
            gate = probes._gate(g, s["N"]).to(DEV)
            res = probes._scaled(g, r_e + t).to(DEV, torch.bfloat16)
        else:
            gate = res = None
        want = dp.rounded(dp.mxfp8_ref(xq.codes, xq.scales, pw.w, pw.w_scale, s["N"], bias=pw.bias, gate=gate, residual=res), s["out"])
        built.append((xq, pw, gate, res, want, s))

    def run():
        with ops.gemm_group():
            return [ops.linear(xq, pw, gate=gate, residual=res, out_dtype=ops.OUT_F32 if s["out"] == torch.float32 else ops.OUT_STREAM)
                    for xq, pw, gate, res, _, s in built]
    ys, tr = _traced(run)
    assert tr == [24]
    for y, (_, _, _, _, want, s) in zip(ys, built):
        probes._eq(y, want, f"dyadic group member M={s['M']} N={s['N']} K={s['K']}")


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------

def test_guard_bands_around_every_operand_and_output():
    """Operands, scale planes, weights and biases between NaN bands, outputs inside fences: ragged rows (M = 100, 520), Cout = 200 under
    Cout_pad = 256, a slice of a wider buffer, a transposed slice, and the 6 filler blocks behind the ten-tile problem write nothing and read
    no band."""
    from omgsr_amd import ops
    xq0, pw0 = _layer(0)
    xq2, pw2 = _layer(2)
    xq3, pw3 = _layer(3, cout=200)
    want0 = ops.linear(xq0, pw0, out_dtype=ops.OUT_F32)
    want2 = _fill((100 + 9, 768 + 128)); ops.linear_into(xq2, pw2, want2, 5, 64)
    want3 = _fill((200, 2344 + 24)); ops.linear_t_into(xq3, pw3, want3, 16)
    e0, e2, e3 = (gb.embed(xq0), gb.embed(pw0)), (gb.embed(xq2), gb.embed(pw2)), (gb.embed(xq3), gb.embed(pw3))
    f2 = gb.Fence((100 + 9, 768 + 128), torch.bfloat16, DEV).window(slice(5, 105), slice(64, 64 + 768))
    f3 = gb.Fence((200, 2344 + 24), torch.bfloat16, DEV).window(slice(None), slice(16, 16 + 2344))
    with gb.fenced_outputs():
        with ops.gemm_group():
            y0 = ops.linear(*e0, out_dtype=ops.OUT_F32)
            ops.linear_into(*e2, f2.out, 5, 64)
            ops.linear_t_into(*e3, f3.out, 16)
        torch.cuda.synchronize()
    f2.check(); f3.check()
    assert torch.isfinite(y0).all() and torch.equal(y0, want0)
    assert torch.equal(f2.out[5:105, 64:64 + 768], want2[5:105, 64:64 + 768]) and torch.isfinite(f2.out[5:105, 64:64 + 768].float()).all()
    assert torch.equal(f3.out[:, 16:16 + 2344], want3[:, 16:16 + 2344]) and torch.isfinite(f3.out[:, 16:16 + 2344].float()).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def _collect(members):
    """The argument blocks ops builds for `members` (a scope that is never launched), the outputs they point at, and the scope."""
    from omgsr_amd import ops
    grp = ops._GemmGroup()
    ops._GEMM_GROUP = grp
    try:
        outs = [fn(sid) for fn, sid in members]
    finally:
        ops._GEMM_GROUP = None
    return grp, outs


def _mutations():
    def not_mxf8(b):
        b[1].mxf8 = 0

    def k192(b):
        b[1].Cin = b[1].K_pad = 192

    def cout_pad_384(b):
        b[0].Cout_pad = 384

    def batch(b):
        b[1].batch = 2

    def out8(b):            # the OMGSR_EL_MXFP8 output form asked for in the block
        b[0].out_mx = 1
    return dict(not_mxf8=not_mxf8, k192=k192, cout_pad_384=cout_pad_384, batch=batch, out8=out8)


@pytest.mark.parametrize("what", sorted(_mutations()))
def test_refused_groups_return_shape_error_and_write_nothing(what):
    """Each block points at real, large enough tensors; the mutated field alone makes the group one the library must refuse."""
    from omgsr_amd import _lib, ops
    lib = _lib.load()
    grp, outs = _collect([(_p_t_slice_c300, 0), (_p_t_slice, 2)])    # (outputs pre-filled by _fill: any store would show)
    before = [o.clone() for o in outs]
    n = len(grp.blocks)
    arr = (_lib.IgemmArgs * n)(*grp.blocks)
    assert lib.omgsr_igemm_mxfp8_multi_ok(arr, n) == 1
    _mutations()[what](arr)
    assert lib.omgsr_igemm_mxfp8_multi_ok(arr, n) == 0
    rc, tr = _traced(lambda: lib.omgsr_igemm_mxfp8_multi(arr, n, ops._stream()))
    torch.cuda.synchronize()
    assert rc == E_SHAPE and tr == []
    assert all(torch.equal(o, b) for o, b in zip(outs, before))


def test_scope_falls_back_to_the_single_calls():
    """Groups ops.gemm_group can be handed that the library refuses or that never reach it: the same launches and bytes as without a scope."""
    from omgsr_amd import ops
    # differing grid.z: refused as a group -> the two single launches, in order
    members = [(_p_into_b2, 2), (_p_bias_gelu, 0)]
    want, _ = _traced(lambda: _separate(members))
    got, tr = _traced(lambda: _grouped(members))
    assert tr == [18, 18] and all(torch.equal(w, y) for w, y in zip(want, got))
    # an OUT8 call and a problem that is not mxf8 launch at once, the plain fp8 member alone is a group of one
    xq, pw = _layer(1)
    g = torch.Generator().manual_seed(9)
    x16, pw16 = _rand(g, 64, 128), ops.pack_linear_weight(_rand(g, 128, 128), None)

    def mixed(scope):
        with (ops.gemm_group() if scope else _null()):
            a = ops.linear(xq, pw, act=ops.ACT_GELU_TANH, out_mxfp8=True)
            b = ops.linear(x16, pw16)
            c = ops.linear(xq, pw)
        return a.codes, a.scales, b, c
    want, tr_w = _traced(lambda: mixed(False))
    got, tr_g = _traced(lambda: mixed(True))
    assert 24 not in tr_g and sorted(tr_g) == sorted(tr_w) and tr_g[-1] == 18
    assert all(torch.equal(w, y) for w, y in zip(want, got))


def _null():
    import contextlib
    return contextlib.nullcontext()


@pytest.mark.parametrize("what", ["k192", "cout_pad_384"])
def test_scope_fallback_of_a_block_no_kernel_takes(what):
    """A member omgsr_igemm refuses too: the scope's fall-back makes the single calls in order - the member before it is written exactly as
    by its own call, the refused one raises as it does without a scope, nothing after it runs."""
    from omgsr_amd import _lib
    grp, outs = _collect([(_p_t_slice, 1), (_p_t_slice_c300, 0), (_p_t_slice, 2)])
    before = [o.clone() for o in outs]
    want0 = _p_t_slice(1)

    class _View:            # the mutations index a block list
        def __getitem__(self, i):
            return grp.blocks[i + 1]
    _mutations()[what](_View())
    bad = 2 if what == "k192" else 1
    with pytest.raises(_lib.OmgsrError):
        _, _ = _traced(grp.launch)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want0)
    assert all(torch.equal(outs[i], before[i]) for i in range(bad, 3))


# ---- the pipeline: test_fp8_gpu.py's small case (2 double + 2 single blocks, dim 256), groups on against off -------------------------------

def _run_small(groups: bool, policy=None, calls=1, batch=1, batch_invariant=False, graphs=False):
    """(outputs, igemm variants of the last call, pipeline) of the small seeded fp8-tier pipeline (built as test_fp8_fused_quant_gpu builds it)."""
    import test_fp8_gpu as base
    from omgsr_amd import ops
    from omgsr_amd.pipelines.omgsr_f import OMGSR_F_Infer
    vae, flux, inp = base._small_case()
    pipe = OMGSR_F_Infer(None, None, DEV, torch.float8_e4m3fn, 244, 1.0, vae=vae, flux_transformer=flux, precision_policy=policy)
    try:
        pipe.enable_gemm_groups(groups)
        ops.set_batch_invariant(batch_invariant)
        outs, trace = [], []
        with torch.no_grad():
            if graphs:
                pipe.enable_graphs(True)
            n = inp["ns"][0] if batch == 1 else torch.cat([inp["ns"][0]] * batch)      # (one tensor object: the graph key holds it by identity)
            for i in range(calls):
                x = inp["xs"][i] if batch == 1 else torch.cat(inp["xs"][:batch])
                if i == calls - 1 and not graphs:
                    y, trace = _traced(lambda: base._call(pipe, inp, x, n))
                else:
                    y = base._call(pipe, inp, x, n)
                outs.append(y.clone())
            if batch_invariant:
                outs.append(base._call(pipe, inp, torch.cat(inp["xs"][:2]), torch.cat([inp["ns"][0]] * 2)).clone())
        return outs, trace, pipe
    finally:
        ops.set_batch_invariant(False)


@pytest.fixture(scope="module")
def off_b1():
    return _run_small(False)


def test_pipeline_groups_on_equals_off_batch_1(off_b1):
    (off,), tr_off, _ = off_b1
    (on,), tr_on, _ = _run_small(True)
    assert torch.isfinite(on.float()).all() and torch.equal(on, off)
    print(f"variant 24 / 18 launches: on {tr_on.count(24)} / {tr_on.count(18)}, off {tr_off.count(24)} / {tr_off.count(18)}")
    assert tr_off.count(24) == 0 and tr_on.count(24) == 2 * 4          # 4 groups per double block
    assert tr_off.count(18) - tr_on.count(18) == 2 * 8
    assert [v for v in tr_on if v not in (18, 24)] == [v for v in tr_off if v not in (18, 24)]


def test_pipeline_groups_on_equals_off_batch_2():
    (off,), tr_off, _ = _run_small(False, batch=2)
    (on,), tr_on, _ = _run_small(True, batch=2)
    assert torch.isfinite(on.float()).all() and torch.equal(on, off)
    assert tr_on.count(24) == 2 * 4 and tr_off.count(18) - tr_on.count(18) == 2 * 8


def test_pipeline_groups_batch_invariant():
    """Under ops.set_batch_invariant a batch of two is the two batch-1 calls, and the groups change none of the three images."""
    a, b, ab = _run_small(True, calls=2, batch_invariant=True)[0]
    a0, b0, ab0 = _run_small(False, calls=2, batch_invariant=True)[0]
    assert torch.equal(ab[0:1], a) and torch.equal(ab[1:2], b)
    assert torch.equal(a, a0) and torch.equal(b, b0) and torch.equal(ab, ab0)


def test_pipeline_groups_graph_replay():
    eager, _, _ = _run_small(False, calls=3)
    got, _, pipe = _run_small(True, calls=3, graphs=True)
    assert pipe.graphs.captures == 1 and pipe.graphs.replays == 2
    assert all(torch.equal(e, g) for e, g in zip(eager, got))


def test_pipeline_narrowed_policy_leaves_that_pair_ungrouped():
    """to_add_out un-marked: to_out / to_add_out run as before (one fp8 launch, one bf16), the other three pairs stay grouped."""
    from omgsr_amd.precision import FP8_ELIGIBLE
    pats = [p.replace("|to_add_out", "") for p in FP8_ELIGIBLE]
    assert pats != list(FP8_ELIGIBLE)
    policy = {"flux": {"fp8": pats}}
    (off,), tr_off, _ = _run_small(False, policy=policy)
    (on,), tr_on, pipe = _run_small(True, policy=policy)
    assert not any(b.attn.to_add_out.fp8 for b in pipe.flux_transformer.transformer_blocks)
    assert torch.equal(on, off)
    assert tr_on.count(24) == 2 * 3 and tr_off.count(18) - tr_on.count(18) == 2 * 6
