"""The guard-band instrument (tests/guard_bands.py) proves itself on the CPU: embed keeps values / shape / contiguity / alignment and its bands
decode as NaN in every format the library reads; a Fence passes untouched and raises for a single changed byte wherever it is not allowed."""
import dataclasses
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as gb  # noqa: E402


def _storage_bytes(view):
    """The whole uint8 allocation a view lives in, and the view's byte offset in it."""
    n = view.untyped_storage().nbytes()
    whole = torch.empty(0, dtype=torch.uint8).set_(view.untyped_storage(), 0, (n,), (1,))
    return whole, view.storage_offset() * view.element_size()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.float8_e4m3fn])
@pytest.mark.parametrize("shape", [(3, 5, 7, 24), (77, 1024), (1,), (2, 33, 2000)])
def test_embed_preserves_the_tensor_and_poisons_both_bands(dtype, shape):
    g = torch.Generator().manual_seed(1)
    t = (torch.randn(*shape, generator=g) * 3).to(dtype) if dtype != torch.uint8 else torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    e = gb.embed(t)
    assert e.shape == t.shape and e.dtype == t.dtype and e.is_contiguous()
    assert torch.equal(e.view(torch.uint8), t.view(torch.uint8))
    assert e.data_ptr() % 256 == 0
    whole, off = _storage_bytes(e)
    band = gb.band_bytes(shape, t.element_size())
    nbytes = t.numel() * t.element_size()
    assert band <= off < band + 256 and whole.numel() == 2 * band + nbytes + 256
    assert band % 256 == 0 and band >= 4096 and band >= 4 * shape[-1] * t.element_size()
    assert bool((whole[off - band:off] == 0xFF).all()) and bool((whole[off + nbytes:off + nbytes + band] == 0xFF).all())
    assert e.untyped_storage().data_ptr() != t.untyped_storage().data_ptr()          # a copy: the original stays dense


def test_embed_guard_bytes_override_and_plane_rule():
    assert gb.band_bytes((8, 8), 2) == 4096
    assert gb.band_bytes((8, 8), 2, guard_bytes=5000) == 5120
    assert gb.band_bytes((100, 3072), 4) == 4 * 3072 * 4                              # four leading-dimension rows
    assert gb.band_bytes((2, 86, 43, 64), 2) == (4 * 43 * 64 * 2 + 255) // 256 * 256   # four image rows of an NHWC map
    assert gb.band_bytes((1, 36900, 1536), 2) == 1 << 20                              # ... capped


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn])
def test_the_bands_decode_as_nan(dtype):
    e = gb.embed(torch.zeros(4, 8, dtype=dtype))
    whole, off = _storage_bytes(e)
    for band in (whole[off - 4096:off], whole[off + e.numel() * e.element_size():][:4096]):
        assert band.numel() == 4096
        assert bool(torch.isnan(band.view(dtype).float()).all())
    assert int(whole[off - 1]) == 0xFF                                               # E8M0 0xFF: the NaN scale


def test_poison_tail_fills_only_the_tail():
    for dtype in (torch.bfloat16, torch.float16, torch.float32, torch.uint8):
        t = torch.ones(2, 6, 16, dtype=dtype)
        assert gb.poison_tail(t, 1, 4) is t
        assert bool((t[:, :4] == 1).all()) and bool((t[:, 4:].contiguous().view(torch.uint8) == 0xFF).all())
        gb.poison_tail(t, 2, 13)
        assert bool((t[:, :4, :13] == 1).all()) and bool((t[:, :, 13:].contiguous().view(torch.uint8) == 0xFF).all())
        gb.poison_tail(t, 1, 6)                                                      # nothing past the end: a no-op
    assert bool(torch.isnan(gb.poison_tail(torch.zeros(3, 8, dtype=torch.bfloat16), 0, 2)[2].float()).all())


@dataclasses.dataclass
class _Packed:
    w: torch.Tensor
    bias: object
    cout: int
    w_cm: object = None
    w_ph: object = None
    w_scale: object = None


class _Mx:
    def __init__(self, codes, scales):
        self.codes, self.scales = codes, scales


def test_embed_of_the_operand_containers():
    assert gb.embed(None) is None
    m = gb.embed(_Mx(torch.arange(256, dtype=torch.uint8).reshape(2, 128), torch.full((2, 4), 127, dtype=torch.uint8)))
    assert isinstance(m, _Mx) and torch.equal(m.codes, torch.arange(256, dtype=torch.uint8).reshape(2, 128)) and bool((m.scales == 127).all())
    assert m.codes.untyped_storage().data_ptr() != m.scales.untyped_storage().data_ptr()
    p = _Packed(torch.ones(128, 32, dtype=torch.bfloat16), torch.ones(5), 5, w_cm=torch.ones(1, 9, 128, 32, dtype=torch.bfloat16))
    q = gb.embed(p)
    assert q.cout == 5 and q.w_ph is None and q.w_scale is None
    for name in ("w", "bias", "w_cm"):
        a, b = getattr(p, name), getattr(q, name)
        assert torch.equal(a, b) and b.data_ptr() % 256 == 0 and _storage_bytes(b)[1] >= 4096
    with pytest.raises(TypeError):
        gb.embed(3.0)


def test_embed_packed_weight_of_the_library():
    from omgsr_amd.ops import Mxfp8, PackedWeight
    w = torch.ones(128, 288, dtype=torch.bfloat16)
    pw = PackedWeight(w, torch.zeros(8), 8, 32, 3, 3, w_cm=w.view(128, 9, 1, 32).permute(2, 1, 0, 3).contiguous(), w_ph=torch.ones(4, 1, 4, 128, 32),
                      w_scale=torch.ones(4, dtype=torch.uint8))
    e = gb.embed(pw)
    assert isinstance(e, PackedWeight) and (e.cout, e.cin, e.R, e.S) == (8, 32, 3, 3)
    for name in ("w", "bias", "w_cm", "w_ph", "w_scale"):
        assert torch.equal(getattr(e, name), getattr(pw, name)) and _storage_bytes(getattr(e, name))[1] >= 4096
    m = gb.embed(Mxfp8(torch.zeros(3, 128, dtype=torch.uint8), torch.zeros(3, 4, dtype=torch.uint8)))
    assert isinstance(m, Mxfp8) and m.shape == (3, 128)


def test_pattern_is_not_constant():
    p = gb.pattern(1024, "cpu")
    assert p.dtype == torch.uint8 and [int(v) for v in p[:3]] == [7, 138, 13]
    assert bool((p[1:] != p[:-1]).all()) and torch.equal(p[:256], p[256:512]) and p.unique().numel() == 256


def test_fence_passes_untouched_and_after_writes_inside_the_window():
    f = gb.Fence((6, 10), torch.bfloat16)
    assert f.out.shape == (6, 10) and f.out.dtype == torch.bfloat16 and f.out.is_contiguous() and f.out.data_ptr() % 256 == 0
    assert torch.equal(f.out.view(torch.uint8).reshape(-1), gb.pattern(f.buf.numel(), "cpu")[f.band:f.band + 120])     # the output is pre-filled too
    f.check()
    f.out.fill_(1.0)                   # no window declared: the whole output may be written
    f.check()
    f = gb.Fence((6, 10), torch.bfloat16).window(slice(2, 4), slice(3, 8))
    f.check()
    f.out[2:4, 3:8] = 0.0
    f.check()
    f = gb.Fence((3, 6, 10), torch.bfloat16).window(Ellipsis, slice(3, 8))             # the last dimension of `out`, not the bytes of an element
    f.out[..., 3:8] = 1.0
    f.check()
    f.out[1, 2, 8] = 1.0
    with pytest.raises(AssertionError, match="outside the window"):
        f.check()
    f = gb.Fence((4, 8), torch.float32).window(0).window(slice(None), slice(6, 8))     # windows add up
    f.out[0] = 1.0
    f.out[:, 6:] = 2.0
    f.check()


def _flip(f, byte):
    f.buf[byte] = (int(f.buf[byte]) + 1) & 0xFF


@pytest.mark.parametrize("where", ["front", "behind", "gap", "first-front", "last-behind"])
def test_fence_raises_for_one_changed_byte(where):
    f = gb.Fence((6, 10), torch.bfloat16).window(slice(2, 4), slice(3, 8))
    total = f.buf.numel()
    byte = {"front": f.band - 1, "behind": f.band + f.nbytes, "gap": f.band + 2 * (2 * 10 + 8), "first-front": 0, "last-behind": total - 1}[where]
    _flip(f, byte)
    with pytest.raises(AssertionError) as e:
        f.check()
    assert f"byte offset {byte - f.band} " in str(e.value) and "1 bytes changed" in str(e.value)
    assert {"front": "in front of", "first-front": "in front of", "behind": "behind", "last-behind": "behind", "gap": "outside the window"}[where] in str(e.value)


def test_fence_raises_for_a_stray_zero_nan_or_plausible_value():
    for value in (0.0, float("nan"), 1.0):
        f = gb.Fence((6, 10), torch.bfloat16).window(slice(2, 4), slice(3, 8))
        f.out[2:4, 3:8] = value
        f.check()
        f.out[4, 3] = value            # the row under the window
        with pytest.raises(AssertionError, match="outside the window"):
            f.check()
    f = gb.Fence((16,), torch.uint8)   # a whole-output fence: the byte behind it, written with the value zero
    f.buf[f.band + 16] = 0
    with pytest.raises(AssertionError, match="behind"):
        f.check()
    # one byte in 256 of the pattern IS zero: a one-byte zero store there is the only one a check cannot see; a store of two or more bytes
    # always shows (neighbouring pattern bytes differ)
    z = int((gb.pattern(256, "cpu") == 0).nonzero()[0])
    f = gb.Fence((16,), torch.uint8)
    f.buf[z:z + 2] = 0
    assert z < f.band
    with pytest.raises(AssertionError, match="1 bytes changed"):
        f.check()


def test_fenced_outputs_fences_what_is_allocated_inside():
    real = (torch.empty, torch.empty_like, torch.zeros)
    with gb.fenced_outputs(host=True) as fences:
        a = torch.empty((3, 5), device="cpu", dtype=torch.float32)
        b = torch.zeros(7, device="cpu", dtype=torch.int32)
        c = torch.empty_like(a)
        d = torch.empty(torch.Size([2, 2]), dtype=torch.uint8, device="cpu")
        plain = torch.empty(4)                                    # no device named: not an op's allocation, passes through
        a.fill_(1.0); c.fill_(2.0); d.fill_(3)
    assert len(fences) == 4 and plain.shape == (4,)
    assert a.shape == (3, 5) and c.shape == (3, 5) and c.dtype == torch.float32 and d.shape == (2, 2) and bool((b == 0).all()) and b.dtype == torch.int32
    assert (torch.empty, torch.empty_like, torch.zeros) == real
    with gb.fenced_outputs() as fences:                            # device tensors only by default
        torch.empty((3,), device="cpu")
    assert not fences
    with pytest.raises(AssertionError, match="behind"):
        with gb.fenced_outputs(host=True) as fences:
            a = torch.empty((3, 5), device="cpu", dtype=torch.float32)
            a.view(-1).as_strided((16,), (1,))[15] = 0.0           # one element past the end
    assert (torch.empty, torch.empty_like, torch.zeros) == real
    with pytest.raises(RuntimeError, match="boom"):                # an exception inside restores torch and is not masked
        with gb.fenced_outputs(host=True):
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like, torch.zeros) == real
