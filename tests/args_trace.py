"""Argument traces: what omgsr_amd.ops hands the library, entry point by entry point, without running a GEMM, conv or attention kernel.

`Recorder` replaces the launching entry points on the loaded library object (omgsr_igemm, omgsr_igemm_multi, omgsr_conv_mxfp8,
omgsr_conv_mxfp8_multi, omgsr_attention) with stubs that copy the argument block(s) and return 0, and wraps the host-side queries
(omgsr_igemm_workspace_bytes, ..._gn_slots, ..._gn_entries, ..._gn_fusable, ..._out_mx6_ok, omgsr_conv_mxfp8_ok, ..._multi_ok,
omgsr_igemm_multi_plan) so that they pass through and are recorded with their integer result (the block as the query left it). A trace is
the ordered list of [function name, block or list of blocks, result]. A block holds its non-zero fields only; pointers are normalised:
a pointer inside a tensor the case registered by name is [name, byte offset], the range guard's word is ["ovf", 0], anything else (a tensor
the op allocated: result, workspace, partials, a cast operand) is "alloc".

`CASES` is the table: name -> (mode, batch-invariant, builder). A builder makes and registers the operands and returns the call to trace.
tests/golden/args_trace.json holds the traces of the table as tools/record_args_trace.py recorded them; tests/test_args_trace_gpu.py
compares. Plain helpers (no test in here); imported like tests/guard_bands.py."""
from __future__ import annotations

import ctypes as C
import dataclasses
import hashlib
import json
import math
import os

import torch

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "args_trace.json")

LAUNCHES = ("omgsr_igemm", "omgsr_igemm_multi", "omgsr_conv_mxfp8", "omgsr_conv_mxfp8_multi", "omgsr_attention")
QUERIES = ("omgsr_igemm_workspace_bytes", "omgsr_igemm_gn_slots", "omgsr_igemm_gn_entries", "omgsr_igemm_gn_fusable", "omgsr_igemm_out_mx6_ok",
           "omgsr_conv_mxfp8_ok", "omgsr_conv_mxfp8_multi_ok", "omgsr_igemm_multi_plan")
_ARRAY_FORMS = ("omgsr_igemm_multi", "omgsr_conv_mxfp8_multi", "omgsr_conv_mxfp8_multi_ok", "omgsr_igemm_multi_plan")

# mode -> arguments of ops.set_compute_dtype
MODES = {"bf16": (torch.bfloat16,), "fp16": (torch.float16,), "acc": (torch.float32,), "accbf": (torch.float32, torch.bfloat16)}


def blob_id(path: str) -> str:
    """git's blob id of a file (what `git rev-parse HEAD:<path>` prints for a committed one)."""
    with open(path, "rb") as f:
        data = f.read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


class Tensors:
    """The tensors a case registered by name: the inputs, the members of a packed weight, `out=`, scales, the GroupNorm table."""

    def __init__(self):
        self.named = []                 # (name, first byte, bytes, the tensor: kept alive)

    def reg(self, name: str, obj):
        if obj is None:
            return None
        if isinstance(obj, torch.Tensor):
            self.named.append((name, obj.data_ptr(), obj.numel() * obj.element_size(), obj))
        elif hasattr(obj, "codes") and hasattr(obj, "scales"):              # Mxfp8
            self.reg(name + ".codes", obj.codes)
            self.reg(name + ".scales", obj.scales)
        elif dataclasses.is_dataclass(obj) and hasattr(obj, "w"):           # PackedWeight (w_cm first: the MXFP8 conv weight's `w` is a view of it)
            for member in ("w_cm", "w", "w_ph", "w_scale", "bias"):
                self.reg(f"{name}.{member}", getattr(obj, member, None))
        elif hasattr(obj, "mean") and hasattr(obj, "rstd"):                 # GnSpec
            for member in ("mean", "rstd", "gamma", "beta", "_table"):
                self.reg(f"{name}.{member.lstrip('_')}", getattr(obj, member, None))
        else:
            raise TypeError(f"cannot register a {type(obj).__name__}")
        return obj

    def pointer(self, p: int):
        for name, start, nbytes, _ in self.named:
            if start <= p < start + max(nbytes, 1):
                return [name, p - start]
        from omgsr_amd import ops
        for t in ops._ovf_words.values():
            if t.data_ptr() == p:
                return ["ovf", 0]
        return "alloc"


def _block(s, tensors: Tensors) -> dict:
    out = {}
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if not v:
            continue
        out[name] = tensors.pointer(v) if ctype is C.c_void_p else v
    return out


class Recorder:
    def __init__(self, tensors: Tensors):
        from omgsr_amd import _lib
        self.lib, self.tensors, self.trace, self._real = _lib.load(), tensors, [], {}

    def _blocks(self, name, args):
        if name in _ARRAY_FORMS:
            return [_block(args[0][i], self.tensors) for i in range(args[1])]
        return _block(args[0]._obj, self.tensors)

    def __enter__(self):
        for name in LAUNCHES + QUERIES:
            real = self._real[name] = getattr(self.lib, name)

            def fn(*args, _name=name, _real=real):
                result = 0 if _name in LAUNCHES else int(_real(*args))
                self.trace.append([_name, self._blocks(_name, args), result])
                return result
            setattr(self.lib, name, fn)
        return self

    def __exit__(self, *exc):
        for name, real in self._real.items():
            setattr(self.lib, name, real)


def _describe(r):
    """Shape and dtype of what a call returns (and the GroupNorm statistics handle an output carries: group count, shape of the partials)."""
    if r is None:
        return None
    if isinstance(r, torch.Tensor):
        d = {"shape": list(r.shape), "dtype": str(r.dtype)}
        h = getattr(r, "_omgsr_gn", None)
        if h is not None:
            d["gn"] = {"groups": h[1], "partial": list(h[0].shape), "of_this_tensor": bool(h[2] == r.data_ptr() and h[3] == r._version)}
        return d
    return [_describe(x) for x in r]


def run_case(name: str) -> dict:
    from omgsr_amd import ops
    mode, invariant, build = CASES[name]
    ops.set_compute_dtype(*MODES[mode])
    ops.set_batch_invariant(invariant)
    try:
        tensors = Tensors()
        call = build(ops, tensors)
        with Recorder(tensors) as rec:
            result = call()
        if DEV == "cuda":
            torch.cuda.synchronize()
        return json.loads(json.dumps({"trace": rec.trace, "returns": _describe(result)}))
    finally:
        ops.set_batch_invariant(False)
        ops.set_compute_dtype(torch.bfloat16)
        ops.overflow_seen(); ops.mx_saturation_seen()


def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------

def rnd(*shape, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape))
    return torch.randn(*shape, generator=g).to(device=DEV, dtype=dtype)


def _conv_pw(ops, t, cout, cin, r=3, bias=True, name="pw", **pack):
    g = torch.Generator().manual_seed(cout + 7 * cin)
    w = torch.randn(cout, cin, r, r, generator=g) / math.sqrt(r * r * cin)
    b = torch.randn(cout, generator=g) if bias else None
    return t.reg(name, ops.pack_conv_weight(w, b, device=DEV, **pack))


def _lin_pw(ops, t, cout, cin, bias=True, geglu=False, fp8=False, name="pw", **pack):
    g = torch.Generator().manual_seed(cout + 7 * cin)
    w = torch.randn(2 * cout if geglu else cout, cin, generator=g) / math.sqrt(cin)
    b = torch.randn(w.shape[0], generator=g) if bias else None
    if fp8:
        return t.reg(name, ops.pack_linear_weight_mxfp8(w.to(torch.bfloat16), b, device=DEV))
    return t.reg(name, (ops.pack_geglu_weight if geglu else ops.pack_linear_weight)(w, b, device=DEV, **pack))


def _conv8_pw(ops, t, cout, cin, name="pw8"):
    g = torch.Generator().manual_seed(cout + 11 * cin)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)).to(torch.bfloat16)
    return t.reg(name, ops.pack_conv_weight_mxfp8(w, torch.randn(cout, generator=g), device=DEV))


def _stream(ops, t, name, *shape, seed=1):
    return t.reg(name, rnd(*shape, seed=seed, dtype=ops.stream_dtype()))


def _act(ops, t, name, *shape, seed=2):
    return t.reg(name, rnd(*shape, seed=seed, dtype=ops.act_dtype()))


def _mx(ops, t, name, *shape, seed=3):
    return t.reg(name, ops.quantize_mxfp8(rnd(*shape, seed=seed, dtype=torch.bfloat16)))


def _spec(ops, t, nimg, channels, groups=32, act=None, table=True, name="gn"):
    mean, rstd = 0.25 + 0.1 * rnd(nimg, groups, seed=16), (1.0 + 0.1 * rnd(nimg, groups, seed=17)).abs()
    gamma, beta = 1.0 + 0.2 * rnd(channels, seed=14), 0.3 * rnd(channels, seed=15)
    spec = ops.GnSpec(mean, rstd, gamma, beta, groups, ops.ACT_SILU if act is None else act)
    if table:
        spec.table(channels)                # made up front so that it can be registered; conv2d finds it cached
    return t.reg(name, spec)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------

CASES = {}


def case(name, mode="bf16", invariant=False):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = (mode, invariant, fn)
        return fn
    return deco


def _conv_case(name, N, Cin, Cout, H, W, mode="bf16", r=3, pack=None, x_split=0, res=False, gate=False, out=None, gn=None, fp8=False, **kw):
    """One conv2d case. x_split > 0: x is handed over as that operand form (to_operand) instead of as a stream tensor. out: channels of a
    caller's output tensor. gn: (nimg, act) of a GnSpec. fp8: an fp8_pack callable is handed over."""
    @case(name, mode)
    def _(ops, t):
        pw = _conv_pw(ops, t, Cout, Cin, r=r, **(pack or {}))
        x = _stream(ops, t, "x", N, H, W, Cin)
        if x_split:
            x = t.reg("x", ops.to_operand(x, x_split))
        args = dict(kw)
        stride, pad, ups = args.get("stride", 1), args.get("pad", 1), args.get("upsample", False)
        pt, pb, pl, pr = (pad,) * 4 if isinstance(pad, int) else pad
        Hv, Wv = (2 * H, 2 * W) if ups else (H, W)
        Ho, Wo = (Hv + pt + pb - r) // stride + 1, (Wv + pl + pr - r) // stride + 1
        if res:
            args["residual"] = _stream(ops, t, "residual", N, Ho, Wo, pw.cout, seed=5)
        if gate:
            args["gate"] = t.reg("gate", rnd(pw.cout, seed=6))
        if out:
            args["out"] = t.reg("out", torch.empty((N, Ho, Wo, out), device=DEV, dtype=ops.stream_dtype() if out == pw.cout else ops.act_dtype()))
        if gn:
            args["gn"] = _spec(ops, t, gn[0], Cin, act=gn[1])
        if fp8:
            pw8 = _conv8_pw(ops, t, Cout, Cin)
            args["fp8_pack"] = lambda: pw8
        return lambda: ops.conv2d(x, pw, **args)


_conv_case("conv2d/3x3", 2, 64, 128, 20, 24)
_conv_case("conv2d/3x3-fp16", 2, 64, 128, 20, 24, mode="fp16")
_conv_case("conv2d/stride-2", 2, 128, 128, 32, 32, stride=2, pad=(0, 1, 0, 1))
_conv_case("conv2d/upsample-phases", 2, 64, 128, 43, 150, pack=dict(upsample_phases=True, bias=False), upsample=True)
_conv_case("conv2d/upsample-no-phases", 1, 256, 256, 12, 20, upsample=True)
_conv_case("conv2d/1x1", 2, 64, 96, 16, 16, r=1, pad=0)
_conv_case("conv2d/residual-act", 2, 64, 128, 20, 24, res=True, act=1)
_conv_case("conv2d/gate-alpha", 2, 64, 128, 20, 24, gate=True, alpha=0.5, out_dtype=1)
_conv_case("conv2d/out", 2, 64, 128, 20, 24, out=128)
_conv_case("conv2d/out-wide-split-2", 2, 64, 128, 20, 24, out=2 * 128 + 16, out_dtype=0, out_split=2)
_conv_case("conv2d/gn_groups-slots", 20, 64, 128, 50, 46, gn_groups=32, res=True)
_conv_case("conv2d/gn_groups-split-k-no-slots", 1, 256, 256, 12, 20, upsample=True, gn_groups=32)
_conv_case("conv2d/gn_groups-narrow-cout-no-slots", 2, 128, 3, 128, 192, gn_groups=32)
_conv_case("conv2d/gn_groups-sample_rows", 2, 64, 128, 20, 24, gn_groups=32, sample_rows=240)
_conv_case("conv2d/gn-fusable", 4, 32, 128, 96, 160, gn=(2, None), gn_groups=32)
_conv_case("conv2d/gn-not-fusable", 1, 128, 128, 16, 16, gn=(1, None), gn_groups=32)
_conv_case("conv2d/gn-no-act-not-fusable", 4, 32, 128, 96, 160, gn=(2, 0))
_conv_case("conv2d/gn-non-candidate-1x1", 2, 64, 96, 16, 16, r=1, pad=0, gn=(2, None))
_conv_case("conv2d/gn-non-candidate-fp32", 2, 64, 128, 20, 24, mode="acc", pack=dict(split=2), gn=(2, None))
_conv_case("conv2d/fp8_pack-accepted", 1, 128, 128, 256, 256, gn=(1, None), gn_groups=32, res=True, fp8=True)
_conv_case("conv2d/fp8_pack-refused", 1, 128, 128, 64, 64, gn=(1, None), gn_groups=32, fp8=True)
_conv_case("conv2d/accurate-split-2", 2, 64, 128, 20, 24, mode="acc", pack=dict(split=2), res=True)
_conv_case("conv2d/accurate-split-2-bf16-operands", 2, 64, 128, 20, 24, mode="accbf", pack=dict(split=2), gn_groups=32)
_conv_case("conv2d/accurate-w_split-2", 2, 64, 128, 20, 24, mode="acc", pack=dict(split=2, w_split=2))
_conv_case("conv2d/accurate-w_split-2-plain-operand", 2, 64, 128, 20, 24, mode="acc", pack=dict(w_split=2))
_conv_case("conv2d/accurate-split-3-mx", 8, 128, 128, 43, 86, mode="acc", pack=dict(split=3), res=True, gn_groups=32)
_conv_case("conv2d/accurate-split-3-mx-one-image", 1, 512, 512, 64, 64, mode="acc", pack=dict(split=3), gn_groups=32)
_conv_case("conv2d/accurate-split-4-fp6", 8, 128, 128, 43, 86, mode="acc", pack=dict(split=4))
_conv_case("conv2d/out_split-2", 2, 64, 128, 20, 24, mode="acc", pack=dict(split=2), out_dtype=0, out_split=2)
_conv_case("conv2d/out_split-3", 2, 64, 128, 20, 24, mode="acc", pack=dict(split=2), out_dtype=0, out_split=3)
_conv_case("conv2d/out_split-4-accepted", 8, 128, 128, 43, 86, mode="acc", pack=dict(split=4), x_split=4, res=True, out_dtype=0, out_split=4)
_conv_case("conv2d/out_split-4-refused", 8, 128, 128, 43, 86, mode="acc", pack=dict(split=4), x_split=4, res=True, act=1, out_dtype=0, out_split=4, stride=2,
           alpha=0.5, sample_rows=100)


def _multi_case(name, Cin, Cout, shapes, mode="bf16", pack=None, res=False, gn=None, fp8=False, **kw):
    @case(name, mode)
    def _(ops, t):
        pw = _conv_pw(ops, t, Cout, Cin, **(pack or {}))
        xs = [_stream(ops, t, f"x{i}", n, h, w, Cin, seed=10 + i) for i, (n, h, w) in enumerate(shapes)]
        args = dict(kw)
        s = 2 if args.get("upsample") else 1
        if res:
            args["residuals"] = [_stream(ops, t, f"residual{i}", n, s * h, s * w, pw.cout, seed=20 + i) for i, (n, h, w) in enumerate(shapes)]
        if gn:
            args["gn"] = _spec(ops, t, gn[0], Cin, act=gn[1])
        if fp8:
            pw8 = _conv8_pw(ops, t, Cout, Cin)
            args["fp8_pack"] = lambda: pw8
        return lambda: ops.conv2d_multi(xs, pw, **args)


_multi_case("conv2d_multi/one-group", 64, 128, [(2, 20, 24)], res=True, gn_groups=32)
_multi_case("conv2d_multi/two-groups", 128, 128, [(36, 40, 40), (12, 40, 32)])
_multi_case("conv2d_multi/three-groups-gn_groups", 128, 128, [(36, 40, 40), (12, 40, 32), (4, 32, 32)], res=True, gn_groups=32, act=1)
_multi_case("conv2d_multi/upsample-phases", 256, 256, [(4, 43, 32), (4, 32, 32), (2, 43, 64)], pack=dict(upsample_phases=True), upsample=True)
_multi_case("conv2d_multi/gn-all-fusable", 128, 128, [(8, 86, 86), (4, 86, 64), (4, 64, 86), (2, 64, 64)], res=True, gn=(2, None), gn_groups=32)
_multi_case("conv2d_multi/gn-not-all-fusable", 128, 128, [(8, 86, 86), (1, 16, 16)], gn=(1, None), gn_groups=32)
_multi_case("conv2d_multi/gn-non-candidate", 128, 128, [(8, 86, 86), (4, 86, 64)], mode="acc", pack=dict(split=2), gn=(2, None))
_multi_case("conv2d_multi/fp8_pack-accepted", 128, 128, [(4, 45, 86)] * 3, pack=dict(cout_multiple=8), res=True, gn=(2, None), gn_groups=32, fp8=True)
_multi_case("conv2d_multi/fp8_pack-refused", 128, 128, [(4, 45, 86)] * 3 + [(4, 45, 70)], pack=dict(cout_multiple=8), res=True, gn=(2, None),
            gn_groups=32, fp8=True)
_multi_case("conv2d_multi/member-with-workspace", 256, 256, [(1, 12, 20), (1, 8, 8)], gn_groups=32)
_multi_case("conv2d_multi/accurate-mx", 128, 128, [(8, 43, 86), (1, 64, 64)], mode="acc", pack=dict(split=3), gn_groups=32)
_multi_case("conv2d_multi/out_split-4-accepted", 128, 128, [(8, 43, 86), (8, 86, 43)], mode="acc", pack=dict(split=4), out_dtype=0, out_split=4)
_multi_case("conv2d_multi/out_split-4-refused", 128, 128, [(8, 43, 86), (8, 86, 43)], mode="acc", pack=dict(split=4), out_dtype=0, out_split=4, stride=2)


def _conv8_case(name, shapes, Cin, Cout, multi, res=False, **kw):
    @case(name)
    def _(ops, t):
        pw8 = _conv8_pw(ops, t, Cout, Cin)
        xqs = [_mx(ops, t, f"x{i}", n, h, w, Cin, seed=30 + i) for i, (n, h, w) in enumerate(shapes)]
        rs = [_stream(ops, t, f"residual{i}", n, h, w, pw8.cout, seed=40 + i) for i, (n, h, w) in enumerate(shapes)] if res else None
        if multi:
            return lambda: ops.conv2d_mxfp8_multi(xqs, pw8, residuals=rs, **kw)
        return lambda: ops.conv2d_mxfp8(xqs[0], pw8, residual=None if rs is None else rs[0], **kw)


_conv8_case("conv2d_mxfp8/plain", [(6, 45, 86)], 128, 256, False)
_conv8_case("conv2d_mxfp8/residual-gn_groups", [(6, 45, 86)], 128, 256, False, res=True, gn_groups=32, act=1)
_conv8_case("conv2d_mxfp8/odd-cout-f32-sample_rows", [(6, 45, 86)], 128, 3, False, out_dtype=1, sample_rows=45 * 43)
_conv8_case("conv2d_mxfp8_multi/plain", [(6, 45, 86), (16, 24, 64), (24, 15, 56)], 128, 256, True)
_conv8_case("conv2d_mxfp8_multi/residual-gn_groups", [(6, 45, 86), (16, 24, 64), (24, 15, 56)], 128, 256, True, res=True, gn_groups=32, act=1)
_conv8_case("conv2d_mxfp8_multi/nine-groups", [(6, 45, 86), (12, 32, 64), (24, 15, 56), (6, 41, 86), (12, 30, 64), (16, 23, 56), (6, 47, 86), (12, 28, 64),
                                              (12, 31, 56)], 128, 256, True, gn_groups=32)


@case("conv2d_mxfp8_multi/batch-invariant", invariant=True)
def _(ops, t):
    pw8 = _conv8_pw(ops, t, 256, 128)
    xqs = [_mx(ops, t, f"x{i}", n, h, w, 128, seed=30 + i) for i, (n, h, w) in enumerate([(2, 128, 192), (1, 256, 96)])]
    return lambda: ops.conv2d_mxfp8_multi(xqs, pw8, gn_groups=32)


# ---- linear -------------------------------------------------------------------------------------------------------------------------------------

@case("linear/2-d")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 384, 256), _act(ops, t, "x", 77, 256)
    return lambda: ops.linear(x, pw)


@case("linear/3-d-gn_groups")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 384, 256), _act(ops, t, "x", 2, 64, 256)
    return lambda: ops.linear(x, pw, gn_groups=32)


@case("linear/4-d-gn_groups-residual-gate", mode="acc")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 320, 320, split=2), _stream(ops, t, "x", 2, 16, 16, 320)
    r, gate = _stream(ops, t, "residual", 2, 16, 16, 320, seed=5), t.reg("gate", rnd(320, seed=6))
    return lambda: ops.linear(x, pw, act=ops.ACT_GELU_TANH, residual=r, gate=gate, alpha=0.25, gn_groups=32)


@case("linear/geglu")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 1280, 320, geglu=True), _act(ops, t, "x", 1, 200, 320)
    return lambda: ops.linear(x, pw)


@case("linear/split-k-1x256x2560", mode="acc")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 1280, 2560, bias=False), _stream(ops, t, "x", 1, 256, 2560)
    return lambda: ops.linear(x, pw, out_dtype=ops.OUT_BF16)


@case("linear/split-k-out_split-2", mode="acc")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 1280, 2560, bias=False), _stream(ops, t, "x", 1, 256, 2560)
    return lambda: ops.linear(x, pw, out_dtype=ops.OUT_BF16, out_split=2)


@case("linear/fp8-mxfp8-operand")
def _(ops, t):
    pw, xq = _lin_pw(ops, t, 384, 256, fp8=True), _mx(ops, t, "x", 2, 100, 256)
    r, gate = _stream(ops, t, "residual", 2, 100, 384, seed=5), t.reg("gate", rnd(384, seed=6))
    return lambda: ops.linear(xq, pw, act=ops.ACT_GELU_TANH, residual=r, gate=gate, alpha=0.5)


@case("linear/fp8-bf16-operand")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 384, 256, fp8=True), _act(ops, t, "x", 2, 100, 256)
    return lambda: ops.linear(x, pw, out_dtype=ops.OUT_F32)


def _into_case(name, invariant, mode="bf16", M=300, K=3072, Nout=384, out_shape=(340, 896), x_shape=None, fp8=False, res=False, pack=None, **kw):
    row0, col0, gate = kw.pop("row0", 0), kw.pop("col0", 0), kw.pop("gate", False)

    @case(f"linear_into/{name}/{'batch-invariant' if invariant else 'default'}", mode, invariant)
    def _(ops, t):
        pw = _lin_pw(ops, t, Nout, K, fp8=fp8, **(pack or {}))
        shape = x_shape or (M, K)
        x = _mx(ops, t, "x", *shape) if fp8 else (_stream if pack else _act)(ops, t, "x", *shape)
        out = t.reg("out", torch.empty(out_shape, device=DEV, dtype=ops.act_dtype()))
        args = dict(kw)
        if res:
            args["residual"] = _stream(ops, t, "residual", M, Nout, seed=5)
        if gate:
            args["gate"] = t.reg("gate", rnd(Nout, seed=6))
        return lambda: ops.linear_into(x, pw, out, row0, col0, **args)


for _inv in (False, True):
    _into_case("2-d", _inv)
    _into_case("3-d", _inv, M=50, K=256, x_shape=(3, 50, 256), out_shape=(3, 64, 416), row0=7, col0=16)
    _into_case("row0-col0", _inv, row0=24, col0=392, act=2)
    _into_case("out_split-2", _inv, out_shape=(340, 1216), row0=24, col0=8, out_split=2)
    _into_case("out_split-2-lo_col0", _inv, out_shape=(340, 1216), row0=24, col0=8, out_split=2, lo_col0=2 * 384 + 8)
    _into_case("residual-gate", _inv, res=True, row0=24, col0=8, gate=True)
    _into_case("sample_rows", _inv, row0=24, col0=8, sample_rows=100)
    _into_case("fp8", _inv, M=200, K=256, out_shape=(260, 832), row0=24, col0=392, fp8=True, act=2)
    _into_case("fp8-3-d", _inv, M=50, K=256, x_shape=(3, 50, 256), out_shape=(3, 64, 416), row0=7, col0=16, fp8=True)
    _into_case("accurate-split-operand", _inv, mode="acc", M=300, K=320, Nout=320, out_shape=(340, 704), pack=dict(split=2, w_split=2), row0=8, col0=16,
               out_split=2)


@case("linear_rows/row0")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 384, 256), _act(ops, t, "x", 2, 300, 256)
    return lambda: ops.linear_rows(x, 60, 200, pw)


@case("linear_rows/residual-gate-act")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 384, 256), _act(ops, t, "x", 2, 300, 256)
    r, gate = _stream(ops, t, "residual", 2, 200, 384, seed=5), t.reg("gate", rnd(384, seed=6))
    return lambda: ops.linear_rows(x, 60, 200, pw, act=ops.ACT_GELU_TANH, residual=r, gate=gate)


@case("linear_rows/long-k-no-workspace")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 384, 3072), _act(ops, t, "x", 1, 300, 3072)
    return lambda: ops.linear_rows(x, 44, 256, pw, out_dtype=ops.OUT_F32)


@case("linear_rows/fp8-row0")
def _(ops, t):
    pw, xq = _lin_pw(ops, t, 384, 256, fp8=True), _mx(ops, t, "x", 2, 300, 256)
    r = _stream(ops, t, "residual", 2, 200, 384, seed=5)
    return lambda: ops.linear_rows(xq, 60, 200, pw, residual=r)


@case("linear_rows/accurate-split", mode="acc")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 320, 320, split=2, w_split=2), _act(ops, t, "x", 2, 300, 640)
    return lambda: ops.linear_rows(x, 60, 200, pw)


@case("linear_t_into/2-d")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 200, 320), _act(ops, t, "x", 77, 320)
    out = t.reg("out", torch.empty((200, 144), device=DEV, dtype=ops.act_dtype()))
    return lambda: ops.linear_t_into(x, pw, out, 0)


@case("linear_t_into/3-d-key0")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 200, 320), _act(ops, t, "x", 2, 77, 320)
    out = t.reg("out", torch.empty((2, 200, 144), device=DEV, dtype=ops.act_dtype()))
    return lambda: ops.linear_t_into(x, pw, out, 24)


@case("linear_t_into/fp32-stream-key0", mode="acc")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 320, 320, split=2), _stream(ops, t, "x", 2, 96, 320)
    out = t.reg("out", torch.empty((2, 320, 160), device=DEV, dtype=ops.act_dtype()))
    return lambda: ops.linear_t_into(x, pw, out, 32)


@case("linear_t_into/fp8-key0")
def _(ops, t):
    pw, xq = _lin_pw(ops, t, 256, 256, fp8=True), _mx(ops, t, "x", 2, 77, 256)
    out = t.reg("out", torch.empty((2, 256, 144), device=DEV, dtype=ops.act_dtype()))
    return lambda: ops.linear_t_into(xq, pw, out, 24)


@case("linear_t/ld-equals-L")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 320, 1024, bias=False), _act(ops, t, "x", 2, 80, 1024)
    return lambda: ops.linear_t(x, pw, 80)


@case("linear_t/ld-padded")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 320, 1024), _act(ops, t, "x", 2, 77, 1024)
    return lambda: ops.linear_t(x, pw, 77)


@case("linear_t/ld-given-fp32-stream", mode="acc")
def _(ops, t):
    pw, x = _lin_pw(ops, t, 320, 320, split=2), _stream(ops, t, "x", 2, 77, 320)
    return lambda: ops.linear_t(x, pw, 77, ld=128)


def _bmm_case(name, a_shape, b_shape, mode="bf16", **kw):
    @case(f"bmm_nt/{name}", mode)
    def _(ops, t):
        a, b = _act(ops, t, "a", *a_shape), _act(ops, t, "b", *b_shape, seed=4)
        return lambda: ops.bmm_nt(a, b, **kw)


_bmm_case("plain", (2, 100, 512), (2, 128, 512))
_bmm_case("f32-alpha", (2, 100, 512), (2, 256, 512), out_dtype=1, alpha=0.125)
_bmm_case("out_split-2", (2, 100, 512), (2, 128, 512), mode="accbf", out_split=2)
_bmm_case("both_split", (2, 100, 1024), (2, 128, 1536), mode="accbf", out_dtype=1, both_split=True, alpha=0.5)
_bmm_case("both_split-fp16-guard", (2, 100, 1024), (2, 128, 1536), mode="acc", out_split=2, both_split=True)
_bmm_case("np-not-128", (2, 100, 512), (2, 77, 512))
_bmm_case("np-not-128-out_split-2", (2, 100, 512), (2, 77, 512), mode="accbf", out_split=2)


# ---- attention ----------------------------------------------------------------------------------------------------------------------------------

def _attn_case(name, B, Bk, H, D, Lq, Lk, mode="bf16", qk_split=False, vt_split=False, fused_qk=False, out_ld=0, k_rows=0, **kw):
    @case(f"attention/{name}", mode)
    def _(ops, t):
        inner = H * D
        width = 2 * inner if qk_split else inner
        args = dict(kw)
        if fused_qk:
            q = k = _act(ops, t, "qk", B, Lq, 2 * width)
            args.update(q_col=0, k_col=width)
        else:
            q, k = _act(ops, t, "q", B, Lq, width), _act(ops, t, "k", Bk, k_rows or Lk, width, seed=4)
        if qk_split:
            args.update(q_lo_col=args.get("q_col", 0) + inner, k_lo_col=args.get("k_col", 0) + inner)
        vt = _act(ops, t, "vt", Bk, 2 * inner if vt_split else inner, (Lk + 7) // 8 * 8 + 8, seed=5)
        if out_ld:
            args["out"] = t.reg("out", torch.empty((B, Lq, out_ld), device=DEV, dtype=ops.act_dtype()))
        return lambda: ops.attention(q, k, vt, H, D, D ** -0.5, Lk=Lk, **args)


_attn_case("d64-plain", 2, 2, 5, 64, 100, 77)
_attn_case("d64-columns-into-out", 2, 2, 5, 64, 200, 200, fused_qk=True, out_ld=2 * 320 + 192, o_col=64)
_attn_case("d64-k-rows-past-lk", 1, 1, 5, 64, 100, 77, k_rows=82)
_attn_case("d64-split-qk-p_split", 2, 2, 5, 64, 300, 77, mode="accbf", qk_split=True, vt_split=True, out_split=2)
_attn_case("d64-split-qk-no-p_split", 2, 2, 5, 64, 300, 77, mode="accbf", qk_split=True, out_split=2, p_split=False)
_attn_case("d64-split-qk-fused-buffer", 2, 2, 5, 64, 200, 200, mode="accbf", qk_split=True, vt_split=True, fused_qk=True)
_attn_case("d64-out_split-2-o_lo_col", 2, 2, 5, 64, 100, 77, out_ld=2 * 320 + 192, o_col=64, out_split=2, o_lo_col=64 + 320 + 64)
_attn_case("d64-out_split-2-default-lo", 2, 2, 5, 64, 100, 77, out_split=2)
_attn_case("d64-out_split-3", 2, 2, 5, 64, 100, 77, mode="acc", out_split=3)
_attn_case("d64-broadcast", 2, 1, 5, 64, 256, 128)
_attn_case("d64-bk-1-b-1", 1, 1, 5, 64, 256, 128)
_attn_case("d128", 1, 1, 2, 128, 200, 136)
_attn_case("d512-plain", 2, 2, 1, 512, 100, 77)
_attn_case("d512-out_split-2-into-out", 2, 2, 1, 512, 200, 136, out_ld=2 * 512 + 192, o_col=64, out_split=2, o_lo_col=64 + 512 + 64)
_attn_case("d512-split-qk-single-vt", 2, 2, 1, 512, 300, 77, mode="accbf", qk_split=True, out_split=2, p_split=False)
_attn_case("d512-full-split", 2, 1, 2, 512, 300, 77, mode="accbf", qk_split=True, vt_split=True, out_split=2)


def _attn8_case(name, B, Bk, H, Lq, Lk, fused_qk=False, out_ld=0, **kw):
    @case(f"attention/mxfp8-{name}")
    def _(ops, t):
        inner = H * 128
        args = dict(kw)
        if fused_qk:
            q = k = _mx(ops, t, "qk", B, Lq, 2 * inner)
            args.update(q_col=0, k_col=inner)
        else:
            q, k = _mx(ops, t, "q", B, Lq, inner), _mx(ops, t, "k", Bk, Lk + 4, inner, seed=4)
        vt = _mx(ops, t, "vt", Bk, inner, (Lk + 127) // 128 * 128, seed=5)
        if out_ld:
            args["out"] = t.reg("out", torch.empty((B, Lq, out_ld), device=DEV, dtype=torch.bfloat16))
        return lambda: ops.attention(q, k, vt, H, 128, 128 ** -0.5, Lk=Lk, **args)


_attn8_case("plain", 2, 2, 2, 200, 136)
_attn8_case("columns-into-out", 2, 2, 2, 200, 200, fused_qk=True, out_ld=256 + 256, o_col=128)
_attn8_case("broadcast", 2, 1, 2, 200, 136)
