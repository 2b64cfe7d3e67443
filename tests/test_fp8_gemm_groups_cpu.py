"""The fp8 tier's launch groups without a GPU: ops.gemm_group's hand-over (order, fall-back, exceptions, nesting, what passes straight
through) against monkeypatched launch functions, OMGSR_F_Infer's switches on meta modules, the double block's launch order on recorded ops
calls, the compiler's resource figures of mxfp8_gemm_multi_kernel, and the additive symbols."""
import os
import shutil

import pytest
import torch


class _FakeLib:
    """Records what ops hands the library; `accept`: omgsr_igemm_mxfp8_multi_ok's answer."""

    def __init__(self, accept=1):
        self.accept, self.calls = accept, []

    def omgsr_igemm_workspace_bytes(self, a):
        self.calls.append(("workspace_bytes", a._obj.Cout))
        return 0

    def omgsr_igemm(self, a, stream):
        self.calls.append(("igemm", a._obj.Cout))
        return 0

    def omgsr_igemm_out_mxfp8(self, a, scale, ld, stream):
        self.calls.append(("out8", a._obj.Cout))
        return 0

    def omgsr_igemm_mxfp8_multi_ok(self, arr, n):
        self.calls.append(("multi_ok", [arr[i].Cout for i in range(n)]))
        return self.accept

    def omgsr_igemm_mxfp8_multi(self, arr, n, stream):
        self.calls.append(("multi", [arr[i].Cout for i in range(n)]))
        return 0


@pytest.fixture
def fake(monkeypatch):
    from omgsr_amd import _lib, ops
    lib = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda path=None: lib)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    return lib


def _block(tag, mxf8=1):
    from omgsr_amd._lib import IgemmArgs
    a = IgemmArgs()
    a.mxf8, a.Cout = mxf8, tag          # (Cout carries the tag the fake library reports)
    return a


def test_scope_hands_the_blocks_over_in_order(fake):
    from omgsr_amd import ops
    keep = object()
    with ops.gemm_group() as grp:
        for tag in (3, 1, 2):
            ops._igemm(_block(tag), None, f"p{tag}", workspace=False, keep=(keep, None))
        assert fake.calls == [] and grp.keep[0] == (keep, None)            # nothing launches inside; the scope holds the tensors
    assert fake.calls == [("multi_ok", [3, 1, 2]), ("multi", [3, 1, 2])]
    assert grp.keep == [] and ops._GEMM_GROUP is None


def test_refused_group_makes_the_single_calls_in_order(fake):
    from omgsr_amd import ops
    fake.accept = 0
    with ops.gemm_group():
        for tag in (3, 1, 2):
            ops._igemm(_block(tag), None, f"p{tag}", z_batched_api=True)
    assert fake.calls == [("multi_ok", [3, 1, 2]), ("igemm", 3), ("igemm", 1), ("igemm", 2)]


def test_empty_scope_calls_nothing(fake):
    from omgsr_amd import ops
    with ops.gemm_group():
        pass
    assert fake.calls == []


def test_exception_inside_the_scope_launches_nothing(fake):
    from omgsr_amd import ops
    with pytest.raises(KeyError):
        with ops.gemm_group():
            ops._igemm(_block(1), None, "p1", workspace=False)
            raise KeyError("x")
    assert fake.calls == [] and ops._GEMM_GROUP is None
    ops._igemm(_block(5), None, "p5", workspace=False)                     # the scope is closed: a launch of its own again
    assert fake.calls == [("igemm", 5)]


def test_nested_scopes_raise(fake):
    from omgsr_amd import ops
    with pytest.raises(RuntimeError):
        with ops.gemm_group():
            ops._igemm(_block(1), None, "p1", workspace=False)
            with ops.gemm_group():
                pass
    assert fake.calls == [] and ops._GEMM_GROUP is None


def test_out8_and_non_fp8_calls_pass_straight_through(fake):
    from omgsr_amd import ops
    with ops.gemm_group():
        ops._igemm(_block(1), None, "p1", workspace=False)
        ops._igemm_out_mxfp8(_block(7), (None, 0), "out8")
        ops._igemm(_block(8, mxf8=0), None, "bf16")
        assert fake.calls == [("out8", 7), ("workspace_bytes", 8), ("igemm", 8)]
        ops._igemm(_block(2), None, "p2", workspace=False)
    assert fake.calls[3:] == [("multi_ok", [1, 2]), ("multi", [1, 2])]


# ---- the pipeline's switches (meta modules) --------------------------------------------------------------------------------------------

def _meta_flux():
    from omgsr_amd.diffusers_api import FluxTransformer2DModel
    with torch.device("meta"):
        return FluxTransformer2DModel(num_layers=2, num_single_layers=1)


def _mk(monkeypatch, wd, flux):
    from omgsr_amd import ops
    from omgsr_amd.pipelines import omgsr_f

    class _Vae(torch.nn.Module):
        config = type("cfg", (), {"block_out_channels": [1, 2, 3, 4]})()
    monkeypatch.setattr(ops, "set_compute_dtype", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_PRECISE", False)
    monkeypatch.setattr(ops, "_ACT", torch.bfloat16)
    return omgsr_f.OMGSR_F_Infer(None, None, "meta", wd, vae=_Vae(), flux_transformer=flux)


def test_enable_gemm_groups_is_fp8_tier_only_and_clears_graphs(monkeypatch):
    monkeypatch.delenv("OMGSR_FP8_GEMM_GROUPS", raising=False)
    flux = _meta_flux()
    pipe = _mk(monkeypatch, torch.float8_e4m3fn, flux)
    assert pipe.gemm_groups is False and not any(b.gemm_groups for b in flux.transformer_blocks)       # off by default
    cleared = []
    monkeypatch.setattr(pipe.graphs, "clear", lambda: cleared.append(1))
    pipe.enable_gemm_groups()
    assert pipe.gemm_groups is True and all(b.gemm_groups for b in flux.transformer_blocks) and len(cleared) == 1
    pipe.enable_gemm_groups(False)
    assert pipe.gemm_groups is False and not any(b.gemm_groups for b in flux.transformer_blocks) and len(cleared) == 2
    pipe.enable_gemm_groups(True)
    other = _mk(monkeypatch, torch.bfloat16, flux)                         # the same transformer in another tier: the setting does not travel
    assert not any(b.gemm_groups for b in flux.transformer_blocks)
    with pytest.raises(ValueError):
        other.enable_gemm_groups()
    assert other.gemm_groups is False


def test_environment_switch_is_read(monkeypatch):
    flux = _meta_flux()
    monkeypatch.setenv("OMGSR_FP8_GEMM_GROUPS", "1")
    assert _mk(monkeypatch, torch.float8_e4m3fn, flux).gemm_groups is True and all(b.gemm_groups for b in flux.transformer_blocks)
    assert _mk(monkeypatch, torch.bfloat16, flux).gemm_groups is False          # names the fp8 tier only
    monkeypatch.setenv("OMGSR_FP8_GEMM_GROUPS", "0")
    assert _mk(monkeypatch, torch.float8_e4m3fn, flux).gemm_groups is False


def test_graph_key_carries_the_flag():
    import inspect
    from omgsr_amd.pipelines import omgsr_f
    src = inspect.getsource(omgsr_f.OMGSR_F_Infer.forward)
    assert "self.gemm_groups" in src.split("key = ")[1].split("\n")[0]


# ---- the double block's launch order on recorded ops calls ----------------------------------------------------------------------------------

class _Rec:
    """Stands in for omgsr_amd.ops inside transformer_flux: records (call, layer tag, open scope?) and returns placeholders."""
    ACT_GELU_TANH, OUT_BF16, ACT_NONE, OUT_STREAM = 2, 0, 0, -1
    FP8_FUSED_QUANT = {"layernorm": True, "gemm": True}

    def __init__(self):
        self.log, self.scope, self.scopes = [], False, 0

    def gemm_group(self):
        import contextlib

        @contextlib.contextmanager
        def cm():
            assert not self.scope
            self.scope = True
            self.scopes += 1
            self.log.append("open")
            yield
            self.scope = False
            self.log.append("close")
        return cm()

    def __getattr__(self, name):
        def call(*a, **k):
            tag = next((x for x in a if isinstance(x, str)), None)
            self.log.append((name, tag) if tag else name)
            return torch.empty(1, 4, 8, device="meta")
        return call


def _block_log(monkeypatch, groups, unmark=()):
    from omgsr_amd.diffusers_api import transformer_flux as tf
    from omgsr_amd.nn import Linear
    rec = _Rec()
    monkeypatch.setattr(tf, "ops", rec)
    with torch.device("meta"):
        blk = tf.FluxTransformerBlock(256, 2, 128)
    names = {}
    for name, m in blk.named_modules():
        if isinstance(m, Linear):
            m.fp8 = name not in unmark
            names[id(m)] = name
    monkeypatch.setattr(Linear, "packed", lambda self: names[id(self)])
    monkeypatch.setattr(Linear, "nhwc", lambda self, x, **k: rec.log.append(("nhwc", names[id(self)])) or torch.empty(1, 4, 8, device="meta"))
    monkeypatch.setattr(tf.FluxAttention, "qk_packed", lambda self, ctx=False: "qk_ctx" if ctx else "qk")
    monkeypatch.setattr(tf.FluxAttention, "norm_table", lambda self, ctx=False: None)
    blk.gemm_groups = groups
    six = dict(a1=None, b1=None, g1=None, a2=None, b2=None, g2=None)
    t = torch.empty(1, 4, 8, device="meta")
    blk.run(t, t, dict(img=six, ctx=dict(six)), (None, None), dict(qk=t, vt=t, o=t, o2=t))
    return [e for e in rec.log if e == "open" or e == "close" or (isinstance(e, tuple) and e[0] in ("linear_into", "linear_t_into", "linear_rows", "nhwc"))], rec


def test_double_block_groups_image_first_and_off_changes_nothing(monkeypatch):
    off, rec_off = _block_log(monkeypatch, False)
    assert rec_off.scopes == 0
    assert off == [("linear_into", "qk_ctx"), ("linear_into", "qk"), ("linear_t_into", "attn.add_v_proj"), ("linear_t_into", "attn.to_v"),
                   ("linear_rows", "attn.to_out.0"), ("linear_rows", "attn.to_add_out"), ("nhwc", "ff.net.0.proj"), ("nhwc", "ff.net.2"),
                   ("nhwc", "ff_context.net.0.proj"), ("nhwc", "ff_context.net.2")]
    on, rec_on = _block_log(monkeypatch, True)
    assert rec_on.scopes == 4
    assert on == ["open", ("linear_into", "qk"), ("linear_into", "qk_ctx"), "close",
                  "open", ("linear_t_into", "attn.to_v"), ("linear_t_into", "attn.add_v_proj"), "close",
                  "open", ("linear_rows", "attn.to_out.0"), ("linear_rows", "attn.to_add_out"), "close",
                  ("nhwc", "ff.net.0.proj"), ("nhwc", "ff_context.net.0.proj"), "open", ("nhwc", "ff.net.2"), ("nhwc", "ff_context.net.2"), "close"]


def test_double_block_groups_only_pairs_that_are_both_fp8(monkeypatch):
    on, rec = _block_log(monkeypatch, True, unmark=("attn.to_add_out", "ff_context.net.2"))
    assert rec.scopes == 2
    assert on[8:] == [("linear_rows", "attn.to_out.0"), ("linear_rows", "attn.to_add_out"), ("nhwc", "ff.net.0.proj"), ("nhwc", "ff.net.2"),
                      ("nhwc", "ff_context.net.0.proj"), ("nhwc", "ff_context.net.2")]


# ---- the library ---------------------------------------------------------------------------------------------------------------------------

def test_multi_kernel_resources_match_the_single_kernel():
    """The compiler's figures of mxfp8_gemm_multi_kernel are held here (the committed table pins the igemm_* / attention kernels only): no
    spills, no scratch, and the occupancy of the single-problem kernel whose body it inlines."""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    from omgsr_amd.build import kernel_resources
    t = kernel_resources()
    multi, single = t["mxfp8_gemm_multi_kernel"], t["mxfp8_gemm_kernel"]
    assert multi["spill_vgpr"] == 0 and multi["spill_sgpr"] == 0 and multi["scratch"] == 0
    assert multi["occupancy"] == single["occupancy"] and multi["vgpr"] <= 256


def test_symbols_are_declared_bound_and_additive():
    from omgsr_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "omgsr_hip.h")).read()
    for name in ("omgsr_igemm_mxfp8_multi_ok", "omgsr_igemm_mxfp8_multi"):
        assert name in _lib.SIGNATURES and f"{name}(const omgsr_igemm_args* args, int32_t count" in hdr
    assert _lib.ABI_VERSION == 22 and "24 mxfp8_gemm_multi_kernel" in hdr
