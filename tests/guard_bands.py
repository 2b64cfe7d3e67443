"""Guard bands: the instrument that shows a kernel staying inside the tensors it is handed, where no sanitizer can run.

Two kinds of error pass every parity test that feeds a kernel freshly allocated dense tensors and reads back only the tensor it returns:

  a READ past an operand   the bytes behind a fresh allocation are zero or finite left-overs - exactly what a conv border or a K tail is meant to
                           contribute. `embed` puts an operand between two bands of 0xFF bytes, NaN in every format the library reads (bf16 / fp16
                           0xFFFF, fp32 0xFFFFFFFF, e4m3fn 0xFF, E8M0 0xFF): one element fetched from a band makes the result NaN, or at least
                           different from the dense call's (the kernels are bit-repeatable and dispatch does not look at addresses).
  a WRITE outside a window a `Fence` pre-fills an allocation - bands AND the output - with the non-constant byte pattern (131 i + 7) & 0xFF, so a stray
                           store of zeros, of NaN or of a plausible value changes it; `check` compares every byte outside the declared window.

`fenced_outputs` covers the tensors an op allocates itself (results, split-K workspaces, GroupNorm partials): for its duration torch.empty /
torch.empty_like / torch.zeros hand out device tensors that live inside a Fence.

Plain helpers (no test in here); imported like tests/dyadic_probe.py. Everything runs on any device: tests/test_guard_bands_cpu.py proves it on the CPU.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math

import torch

POISON = 0xFF
ALIGN = 256                 # a band is a multiple of this, so the view starts aligned like a fresh allocation
MIN_BAND = 4096
MAX_PLANE_BAND = 1 << 20    # the band also covers four [-2] x [-1] planes (image rows of an NHWC map) up to this size


def band_bytes(shape, itemsize: int, guard_bytes=None) -> int:
    """Size of one band around a tensor of `shape`: a multiple of 256 bytes, at least four leading-dimension rows (shape[-1] elements), at
    least 4 KiB; and four rows of the next dimension too (an image row of an NHWC map: where a halo fetch one row out lands) up to 1 MiB."""
    shape = tuple(shape)
    row = (shape[-1] if shape else 1) * itemsize
    plane = row * (shape[-2] if len(shape) >= 3 else 1)
    need = max(MIN_BAND, 4 * row, min(4 * plane, MAX_PLANE_BAND), int(guard_bytes or 0))
    return (need + ALIGN - 1) // ALIGN * ALIGN


def pattern(n: int, device) -> torch.Tensor:
    """uint8 [n]: byte i = (131 i + 7) & 0xFF (131 is odd: the period is 256 and neighbouring bytes always differ)."""
    i = torch.arange(n, device=device, dtype=torch.int32)       # (wraps past 2^31 / 131 bytes: the low 8 bits are unaffected)
    return ((i * 131 + 7) & 0xFF).to(torch.uint8)


def _raw(n: int, device) -> torch.Tensor:
    """uint8 [n] starting at a 256-byte boundary (a device allocation does anyway; a host one is only 64-byte aligned)."""
    buf = torch.ones(n + ALIGN, dtype=torch.uint8, device=device)      # (torch.ones is never patched by fenced_outputs)
    shift = -buf.data_ptr() % ALIGN
    return buf[shift:shift + n]


def _embed_tensor(t: torch.Tensor, guard_bytes=None) -> torch.Tensor:
    band = band_bytes(t.shape, t.element_size(), guard_bytes)
    nbytes = t.numel() * t.element_size()
    buf = _raw(band + nbytes + band, t.device).fill_(POISON)
    view = buf[band:band + nbytes].view(t.dtype).view(t.shape)
    view.copy_(t)
    return view


def embed(t, guard_bytes=None):
    """A contiguous tensor of t's shape, dtype and values inside one larger uint8 allocation whose bytes in front of and behind it are 0xFF.
    None passes through; an Mxfp8 (codes, scales) and a PackedWeight (w, w_cm, w_ph, w_scale, bias) come back with every tensor embedded on its own."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return _embed_tensor(t, guard_bytes)
    if hasattr(t, "codes") and hasattr(t, "scales"):
        return type(t)(_embed_tensor(t.codes, guard_bytes), _embed_tensor(t.scales, guard_bytes))
    if dataclasses.is_dataclass(t) and hasattr(t, "w"):
        fields = {n: _embed_tensor(getattr(t, n), guard_bytes) for n in ("w", "w_cm", "w_ph", "w_scale", "bias") if getattr(t, n, None) is not None}
        return dataclasses.replace(t, **fields)
    raise TypeError(f"embed: cannot embed a {type(t).__name__}")


def poison_tail(t: torch.Tensor, dim: int, start: int) -> torch.Tensor:
    """Fill t.narrow(dim, start, rest) with 0xFF bytes in place (padding INSIDE a tensor: K rows >= Lk, V^T columns >= Lk). Returns t."""
    n = t.shape[dim] - start
    if n > 0:
        tail = t.narrow(dim, start, n)
        ones = torch.full((), -1, dtype={1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()], device=t.device)
        tail.copy_(ones.view(t.dtype).expand(tail.shape))
    return t


class Fence:
    """An output tensor `out` of a given shape and dtype inside a larger allocation pre-filled, output included, with `pattern`.
    window(index) declares elements of `out` the call may write (several calls add up; none declared = all of `out`); check() compares every
    other byte of the allocation with the pattern and raises AssertionError naming the first changed offset (relative to out's first byte)."""

    def __init__(self, shape, dtype, device="cpu", guard_bytes=None):
        if isinstance(shape, int):
            shape = (shape,)
        self.shape = tuple(int(s) for s in shape)
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.band = band_bytes(self.shape, self.itemsize, guard_bytes)
        self.nbytes = math.prod(self.shape) * self.itemsize
        self.buf = _raw(self.band + self.nbytes + self.band, device)
        self.buf.copy_(pattern(self.buf.numel(), device))
        self.out = self.buf[self.band:self.band + self.nbytes].view(dtype).view(self.shape)
        self._mask = None

    def window(self, *index) -> "Fence":
        if self._mask is None:
            self._mask = torch.full((self.nbytes,), False, dtype=torch.bool, device=self.buf.device)
        if any(i is Ellipsis for i in index):
            index = index + (slice(None),)          # (the mask has one more dimension than `out`: the bytes of an element)
        self._mask.view(*self.shape, self.itemsize)[index] = True
        return self

    def check(self) -> None:
        changed = self.buf != pattern(self.buf.numel(), self.buf.device)
        inside = changed[self.band:self.band + self.nbytes]
        if self._mask is None:
            inside.zero_()
        else:
            inside &= ~self._mask
        if bool(changed.any()):
            first = int(changed.nonzero()[0])
            where = "in the band in front of" if first < self.band else "in the band behind" if first >= self.band + self.nbytes else "outside the window of"
            raise AssertionError(f"stray write {where} a {self.shape} output: {int(changed.sum())} bytes changed, the first at byte offset "
                                 f"{first - self.band} from the output's start (element {(first - self.band) // self.itemsize}), "
                                 f"value 0x{int(self.buf[first]):02x}")


@contextlib.contextmanager
def fenced_outputs(host: bool = False):
    """For its duration torch.empty, torch.empty_like and torch.zeros return DEVICE tensors that live inside a Fence (whole tensor writable): every
    result, workspace and partials buffer an op allocates. Host tensors and calls with options this does not model pass through. All fences are checked
    on a clean exit; the list of fences is what the block yields. host=True fences host tensors as well (the CPU proof of this instrument)."""
    real_empty, real_like, real_zeros = torch.empty, torch.empty_like, torch.zeros
    fences = []

    def _shape(size):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        return tuple(int(s) for s in size)

    def _wants(kw):
        dev = kw.get("device")
        return dev is not None and (host or torch.device(dev).type != "cpu") and set(kw) <= {"device", "dtype"}

    def _fenced(shape, dtype, device):
        f = Fence(shape, dtype or torch.get_default_dtype(), device)
        fences.append(f)
        return f.out

    def empty(*size, **kw):
        return _fenced(_shape(size), kw.get("dtype"), kw["device"]) if _wants(kw) else real_empty(*size, **kw)

    def zeros(*size, **kw):
        return _fenced(_shape(size), kw.get("dtype"), kw["device"]).zero_() if _wants(kw) else real_zeros(*size, **kw)

    def empty_like(t, **kw):
        return _fenced(t.shape, t.dtype, t.device) if ((host or t.device.type != "cpu") and not kw and t.is_contiguous()) else real_like(t, **kw)

    torch.empty, torch.empty_like, torch.zeros = empty, empty_like, zeros
    try:
        yield fences
    finally:
        torch.empty, torch.empty_like, torch.zeros = real_empty, real_like, real_zeros
    for f in fences:
        f.check()
