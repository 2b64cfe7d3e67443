"""Tensor-level wrappers over the C ABI (include/omgsr_hip.h).

torch is used for device memory and streams only: every function here validates shapes, allocates
the output with torch.empty and launches a hand-written gfx950 kernel on torch's current stream.
Activations are channels-last ([N, H, W, C]; token matrices are [B, L, C]).

Two tensor classes (include/omgsr_hip.h, OMGSR_EL_*):
  operand tensors  feed an MFMA: the 16-bit compute type `act_dtype()`; optionally the two-term split
                   x = hi + lo stored as [hi (C) | lo (C)] per row (`split=2`), consumed by a weight packed with
                   duplicated input channels, so the fp32 accumulator receives hi*W + lo*W
  stream tensors   everything between two GEMMs: `stream_dtype()` = the compute type in the fast tiers
                   (--weight_dtype bf16 | fp16), fp32 in the accurate tier (--weight_dtype fp32)
Every function dispatches on the dtype of the tensors it is handed.
"""
from __future__ import annotations

import ctypes as C
import os
from contextlib import contextmanager
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import AttnArgs, IgemmArgs, check

ACT_NONE, ACT_SILU, ACT_GELU_TANH, ACT_GEGLU = 0, 1, 2, 3
OUT_STREAM, OUT_BF16, OUT_F32 = -1, 0, 1      # conv / linear outputs: stream tensor (default) | 16-bit operand | fp32
LAYOUT_NHWC, LAYOUT_T = 0, 1
EL_16, EL_F32, EL_SPLIT, EL_MX, EL_MX6, EL_MXFP8 = 0, 1, 2, 3, 4, 5
MX_LO_SHIFT = 11          # OMGSR_MX_LO_SHIFT (csrc/common.hip.h): a_lo' = (a - a_hi) * 2^11 as fp8


def _el_of_split(split: int) -> int:
    """Operand form of a `split` code: 1 plain, 2 two-term split [hi | lo] (both fp16), 3 the mixed-precision form
    [hi fp16 | lo' fp8 | hi' fp8] (OMGSR_EL_MX: same row width as 2, its correction segments run as block-scaled fp8 MFMAs)."""
    return {1: EL_16, 2: EL_SPLIT, 3: EL_MX, 4: EL_MX6}[split]


_ACT = torch.bfloat16
_PRECISE = False


def act_dtype() -> torch.dtype:
    """The 16-bit element type of every MFMA operand / packed weight (bf16 default, fp16 optional)."""
    return _ACT


def stream_dtype() -> torch.dtype:
    """Element type of the tensors between GEMMs: the compute type, or fp32 in the accurate tier."""
    return torch.float32 if _PRECISE else _ACT


def precise() -> bool:
    return _PRECISE


def attn_split() -> bool:
    """The UNet's attention takes q, k (from their projections' epilogues) and P (in registers) as two-term splits: in the range-fallback tier
    (fp32 stream, bf16 operands: 8-bit mantissas), where single q / k / P cost the north-star tolerance on OMGSR-S 256->1024 (1.15e-3).
    OMGSR_ATTN_SPLIT=0 | 1 forces it off / on in the accurate tiers (A/B runs)."""
    env = os.environ.get("OMGSR_ATTN_SPLIT")
    if env is not None and _PRECISE:
        return env != "0"
    return bool(_PRECISE and _ACT == torch.bfloat16)


def mode_key() -> tuple:
    """Cache key of anything derived from weights under the current tier."""
    return (_ACT, _PRECISE)


def set_compute_dtype(dtype: torch.dtype, operand_dtype: Optional[torch.dtype] = None) -> None:
    """Process-wide tier switch; packed-weight caches are keyed on it and rebuild lazily. Mirrors the reference's
    --weight_dtype (infer/infer_omgsr_s.py:134-149):
      bf16 / fp16  fast tiers: operands AND stream tensors in that 16-bit type (omgsr_set_compute_dtype)
      fp32         accurate tier: fp32 stream tensors, fp16 MFMA operands with fp32 accumulation, two-term split
                   operands / weights on the layers a precision policy names (omgsr_amd.precision)
    operand_dtype (accurate tier only): torch.bfloat16 runs the same tier with bf16 operands - fp32's exponent range, 8-bit
    mantissas (16 with the two-term split): the range-safe fallback the fp16 range guard (overflow_seen) switches to."""
    global _ACT, _PRECISE
    if dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"compute dtype must be bfloat16, float16 or float32, got {dtype}")
    if operand_dtype is not None and (dtype != torch.float32 or operand_dtype not in (torch.float16, torch.bfloat16)):
        raise TypeError("operand_dtype applies to the accurate tier (dtype float32) and must be float16 or bfloat16")
    act = torch.bfloat16 if dtype == torch.bfloat16 else (operand_dtype or torch.float16)
    check(_lib.load().omgsr_set_compute_dtype(0 if act == torch.bfloat16 else 1), "set_compute_dtype")
    # fast tiers: deferred softmax maximum (+5 % attention); accurate tier: exact running maximum
    # (OMGSR_ATTN_DEFER_ACCURATE=<log2 threshold>: A/B runs of a deferred maximum in the accurate tier)
    acc_defer = float(os.environ.get("OMGSR_ATTN_DEFER_ACCURATE", "0"))
    check(_lib.load().omgsr_set_attention_defer_max(acc_defer if dtype == torch.float32 else 8.0), "set_attention_defer_max")
    _ACT, _PRECISE = act, dtype == torch.float32


# ---- fp16 range guard (accurate tier) -----------------------------------------------------------------------------------------
# fp16 operands saturate at +-65504 (pack2 clips instead of producing inf). Every kernel that writes a 16-bit operand from values
# that are not normalised - GEMM / conv epilogues (q, k, v, FF hidden, operand-only outputs), stream -> operand casts - ORs 1 into a
# device word when it clips one. The pipelines read the word once per call, at the synchronisation the reference's forward() already
# has, and fall back to bf16 operands for that call instead of returning a silently clipped image.
_GUARD = True
_ovf_words: dict = {}


def set_range_guard(on: bool) -> None:
    global _GUARD
    _GUARD = bool(on)


def _ovf(device) -> Optional[int]:
    """Device pointer of the overflow word when the guard applies (accurate tier with fp16 operands), else None."""
    if not (_GUARD and _PRECISE and _ACT == torch.float16):
        return None
    key = str(device)
    t = _ovf_words.get(key)
    if t is None:
        t = _ovf_words[key] = torch.zeros(1, device=device, dtype=torch.int32)
    return t.data_ptr()


_weight_overflow = False        # a WEIGHT beyond the fp16 range was packed for fp16 operands (pack_conv_weight saturates it at +-65504)


def _note_weight_range(w: torch.Tensor) -> torch.Tensor:
    """Accurate tier, fp16 operands: a weight beyond +-65504 cannot be carried by an fp16 operand (the reason the reference defaults
    FLUX to bf16). Saturate it like the kernels saturate activations and raise the same guard the activations raise, so the pipelines
    fall back to bf16 operands instead of multiplying by inf."""
    global _weight_overflow
    if _PRECISE and _ACT == torch.float16 and w.numel() and float(w.abs().max()) > 65504.0:
        if _GUARD:
            _weight_overflow = True
        return w.clamp(-65504.0, 65504.0)
    return w


def overflow_seen(reset: bool = True) -> bool:
    """True when a kernel clipped an fp16 operand (or a weight beyond the fp16 range was packed) since the last reset (synchronises:
    one 4-byte read per device in use)."""
    global _weight_overflow
    seen = _weight_overflow
    if reset:
        _weight_overflow = False
    global _mx_saturated
    for t in _ovf_words.values():
        v = int(t.item())
        if v & 2:
            _mx_saturated = True
        if v & 1:
            seen = True
        if v and reset:
            t.zero_()
    return seen


_mx_saturated = False


def mx_saturation_seen(reset: bool = True) -> bool:
    """Diagnostic: True when, since the last reset, a kernel wrote a value beyond +-448 into a mixed-precision (OMGSR_EL_MX)
    operand. Its fp8 correction fields use fixed scales and clamp there, so that element carried single-rounding fp16 accuracy (nothing
    becomes NaN, the fp16 main term is exact). The word is read with the range guard's (overflow_seen, at the pipelines' own sync)."""
    global _mx_saturated
    for t in _ovf_words.values():
        if int(t.item()) & 2:
            _mx_saturated = True
            if reset:
                t.bitwise_and_(1)
    seen = _mx_saturated
    if reset:
        _mx_saturated = False
    return seen


_BATCH_INVARIANT = False


def set_batch_invariant(on: bool) -> None:
    """Process-wide: make kernel-family / split-K choices depend on one sample's size instead of the batch's (omgsr_set_batch_invariant):
    a batch of B then equals B batch-1 calls bit for bit, at some cost in speed for small batches."""
    global _BATCH_INVARIANT
    check(_lib.load().omgsr_set_batch_invariant(int(bool(on))), "omgsr_set_batch_invariant")
    _BATCH_INVARIANT = bool(on)


STAGE_NONE, STAGE_ENCODE, STAGE_DENOISE, STAGE_DECODE = 0, 1, 2, 3


def timing_stage(stage: int) -> None:
    """Tag the launches that follow for the per-launch timing leg (omgsr_timing_stage): the pipelines mark VAE encode / denoiser /
    VAE decode so bench.py can report per-stage time and the denoiser-only MFMA fraction. One host-side store; free when timing is off."""
    _lib.load().omgsr_timing_stage(stage)


def compute_dtype_name() -> str:
    return "fp32" if _PRECISE else ("bf16" if _ACT == torch.bfloat16 else "fp16")


def io_dtype(x: torch.Tensor) -> torch.dtype:
    """Boundary dtype the kernels can write directly for a caller holding `x`: f32 stays f32, else the compute dtype."""
    return torch.float32 if x.dtype == torch.float32 else _ACT


def _el(t: torch.Tensor, name: str) -> int:
    """Element kind of a stream-or-operand tensor argument."""
    if not t.is_cuda:
        raise _lib.OmgsrError(f"{name}: tensor is on {t.device}; the OMGSR HIP path runs on an MI355X only")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if t.dtype == torch.float32:
        return EL_F32
    if t.dtype != _ACT:
        raise TypeError(f"{name}: expected {_ACT} or float32, got {t.dtype}")
    return EL_16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise _lib.OmgsrError(f"{name}: tensor is on {t.device}; the OMGSR HIP path runs on an MI355X only")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class _GemmGroup:
    """What an ops.gemm_group scope collects: the argument blocks in call order, their labels, and the tensors they point into."""

    def __init__(self):
        self.blocks, self.whats, self.keep = [], [], []

    def add(self, a: "IgemmArgs", what: str, keep=()) -> None:
        self.blocks.append(a)
        self.whats.append(what)
        self.keep.append(tuple(keep))

    def launch(self) -> None:
        n = len(self.blocks)
        if n == 0:
            return
        lib = _lib.load()
        arr = (IgemmArgs * n)(*self.blocks)
        if lib.omgsr_igemm_mxfp8_multi_ok(arr, n):
            check(lib.omgsr_igemm_mxfp8_multi(arr, n, _stream()), "omgsr_igemm_mxfp8_multi(" + ", ".join(self.whats) + ")")
        else:                                       # refused as a group: exactly the single calls, in order
            for a, what in zip(self.blocks, self.whats):
                check(lib.omgsr_igemm(C.byref(a), _stream()), what)
        self.keep.clear()


_GEMM_GROUP: Optional[_GemmGroup] = None


@contextmanager
def gemm_group():
    """Deferred-launch scope of the fp8 tier's MXFP8 token GEMMs: inside it the plain MXFP8 forms of linear, linear_into, linear_rows and
    linear_t_into (everything that reaches omgsr_igemm with mxf8 = 1) append their finished argument block instead of launching, and a clean
    exit runs them as ONE omgsr_igemm_mxfp8_multi call in the order given (mxfp8_gemm_multi_kernel: up to 4 problems per launch, each
    problem's bits those of its own launch). A group the library refuses (omgsr_igemm_mxfp8_multi_ok: differing grid.z, ...) runs as the
    single calls it would have been. The outputs are allocated and returned at once but NOT written before the scope ends: only
    independent work belongs inside. OUT8 calls (out_mxfp8=) and problems that are not mxf8 launch immediately, as outside a scope. An
    exception inside the scope launches nothing; scopes do not nest."""
    global _GEMM_GROUP
    if _GEMM_GROUP is not None:
        raise RuntimeError("ops.gemm_group: scopes do not nest")
    grp = _GEMM_GROUP = _GemmGroup()
    try:
        yield grp
    except BaseException:
        _GEMM_GROUP = None
        raise
    _GEMM_GROUP = None
    grp.launch()


def _igemm(a: "IgemmArgs", device, what: str, z_batched_api: bool = False, workspace: bool = True, keep=()) -> None:
    """Launch omgsr_igemm; when the library wants to split K (small-M / long-K problems) hand it an fp32 scratch.
    z_batched_api: the caller puts the images of a call on grid.z and offers a workspace (linear_into is the one that does). The library
    cannot split K there when there is more than one image, so in batch-invariant mode it must not split the one-image call either
    (round 4: OMGSR-F batch 1 == batch N bit for bit under ops.set_batch_invariant).
    workspace=False: no query and a NULL workspace, so the library never splits K (linear_rows, linear_t_into, linear_t, bmm_nt and the
    fp8 form of linear).
    keep: the tensors the block points into, held by an open ops.gemm_group scope until it launches."""
    if _GEMM_GROUP is not None and a.mxf8 == 1:     # ops.gemm_group: the finished block joins the scope (an mxf8 problem never splits K)
        _GEMM_GROUP.add(a, what, keep)
        return
    lib = _lib.load()
    need = 0 if (not workspace or (z_batched_api and _BATCH_INVARIANT)) else lib.omgsr_igemm_workspace_bytes(C.byref(a))
    ws = None
    if need > 0:
        ws = torch.empty(need // 4, device=device, dtype=torch.float32)
        a.workspace = ws.data_ptr()
    check(lib.omgsr_igemm(C.byref(a), _stream()), what)


# --------------------------------------------------------------------------------------------
# weight packing (load time)

@dataclass
class PackedWeight:
    """KRSC bf16 weight [Cout_pad, K_pad] for omgsr_igemm (+ optional f32 bias)."""
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    cout: int          # logical output channels (GEGLU: halved)
    cin: int           # padded input channels (multiple of 8)
    R: int
    S: int
    geglu: bool = False
    w_cm: Optional[torch.Tensor] = None   # chunk-major second packing (3x3, Cin % 32 == 0): halo-tile kernel
    split: int = 1     # 2: the input is a two-term split operand [hi | lo]: every input channel packed twice ([w | w]);
                       # 3: the mixed-precision form (OMGSR_EL_MX operand; fp16 [w_hi] + fp8 [w_hi' | w_lo'] per tap, `mx`)
    mx: Optional[tuple] = None      # split 3: (fp16 chunks per tap, E8M0 scale of w_hi', of a_lo', of w_lo', of a_hi')
    mx_fmt: int = 0                 # 6: split 4, the fp6 form (OMGSR_EL_MX6: e2m3 codes + per-block scale bytes in the data; `mx` scales unused)
    w_split: int = 1   # 2: the weight itself is carried as w_hi + w_lo: one more K segment [w_lo] that re-reads the operand's
                       # first (hi) half - the contraction WRAPS (omgsr_igemm_args.in_ld); `cin` counts every segment
    in_ld: int = 0     # physical channels of the operand row this weight expects (split * padded Cin); 0 = cin
    w_ph: Optional[torch.Tensor] = None   # 3x3 convs applied to a nearest-2x upsampled map: the four phase-summed 2 x 2 kernels,
                                          # [4][Kc/32][4 taps][Cout_pad][32] (omgsr_igemm_args.weight_ph): 4 / 9 of the MFMA work
    w_scale: Optional[torch.Tensor] = None  # the fp8 tier's form (OMGSR_EL_MXFP8, pack_linear_weight_mxfp8): `w` holds the e4m3 codes
                                            # uint8 [Cout_pad][K], this the E8M0 scales uint8 [Cout_pad][K / 32]

    @property
    def fp8(self) -> bool:
        return self.w_scale is not None

    @property
    def cout_pad(self) -> int:
        return self.w.shape[0]

    @property
    def k_pad(self) -> int:
        return self.w.shape[1]

    @property
    def row_channels(self) -> int:
        """Channels of one operand row ([a] or [a_hi | a_lo]); < cin when the weight carries its own low half (w_split 2)."""
        return self.in_ld or self.cin


def _segments(w: torch.Tensor, split: int, w_split: int) -> torch.Tensor:
    """[..., Cin8] fp32 -> [..., Kc]: the K-concatenation of pack_conv_weight ([w_hi] * split, then [w_lo] when w_split 2), every value
    already rounded to the compute type."""
    w_hi = w.to(act_dtype()).float()
    segs = [w_hi] * split           # [hi (cin8) | lo (cin8)] operand rows: both halves meet the same (rounded) weights
    if w_split == 2:
        segs.append((w - w_hi).to(act_dtype()).float())      # ... and the operand's hi half meets the weights' low halves
    return torch.cat(segs, dim=-1) if len(segs) > 1 else w_hi


def _mx_rows(w: torch.Tensor, s1: int, s2: int) -> torch.Tensor:
    """[..., C] fp32 -> [..., 4C] uint8: [w_hi fp16 | fp8(w_hi 2^s1) | fp8((w - w_hi) 2^s2)]."""
    w_hi = w.to(torch.float16)
    hi8 = (w_hi.float() * 2.0 ** s1).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    lo8 = ((w - w_hi.float()) * 2.0 ** s2).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return torch.cat([w_hi.contiguous().view(torch.uint8).reshape(*w.shape[:-1], 2 * w.shape[-1]), hi8, lo8], dim=-1)


def _e2m3_blocks(v: torch.Tensor) -> torch.Tensor:
    """[..., C] fp32 (C % 64 == 0) -> [..., C] uint8: one correction third of an OMGSR_EL_MX6 row (include/omgsr_hip.h). Every 64-byte group covers
    64 channels = two 32-channel blocks; block h owns bytes [16h, 16h + 16) and [32 + 16h, 40 + 16h) (its 192-bit string of e2m3 codes, channel i
    at bits [6i, 6i + 6)), byte 40 + 16h (E8M0 scale = max(0, biased exponent of the block's largest magnitude - 2)) and 7 zero bytes. Codes round
    to nearest even and saturate at +-7.5. The SAME integer arithmetic as the device producers (csrc/common.hip.h store8_mx6): tests compare bytes."""
    lead, Cc = v.shape[:-1], v.shape[-1]
    b = v.reshape(-1, Cc // 32, 32).float()
    m = b.abs().amax(-1)
    sb = ((m.view(torch.int32) >> 23) - 2).clamp(min=0)                                    # [R, nb] scale bytes
    inv = ((254 - sb) << 23).to(torch.int32).view(torch.float32).unsqueeze(-1)
    s_ = b * inv
    a = s_.abs().clamp(max=7.5)
    eb = (a.view(torch.int32) >> 23).clamp(min=127)
    q = torch.round(a * ((257 - eb) << 23).to(torch.int32).view(torch.float32)).to(torch.int64)      # torch.round: half to even, like v_rndne
    code = (q + ((eb.to(torch.int64) - 127) << 3)) | (((s_.view(torch.int32).to(torch.int64) >> 26) & 32))
    # four codes = 24 bits = three bytes: code i sits at bits [6i, 6i + 6) of the block's little-endian 192-bit string
    c4 = code.reshape(*code.shape[:-1], 8, 4)
    v24 = c4[..., 0] | (c4[..., 1] << 6) | (c4[..., 2] << 12) | (c4[..., 3] << 18)
    string = torch.stack([v24 & 0xFF, (v24 >> 8) & 0xFF, (v24 >> 16) & 0xFF], dim=-1).to(torch.uint8).reshape(*code.shape[:-1], 24)
    R, nb = string.shape[0], string.shape[1]
    out = torch.zeros((R, nb // 2, 64), dtype=torch.uint8, device=v.device)
    st = string.reshape(R, nb // 2, 2, 24)
    sbv = sb.reshape(R, nb // 2, 2).to(torch.uint8)
    for h in (0, 1):
        out[..., 16 * h:16 * h + 16] = st[..., h, :16]
        out[..., 32 + 16 * h:40 + 16 * h] = st[..., h, 16:]
        out[..., 40 + 16 * h] = sbv[..., h]
    return out.reshape(*lead, Cc)


def _mx6_rows(w: torch.Tensor) -> torch.Tensor:
    """[..., C] fp32 -> [..., 4C] uint8: [w_hi fp16 | e2m3 blocks of w_hi | e2m3 blocks of w - w_hi] (meets an OMGSR_EL_MX6 operand's [a_hi | a_lo' | a_hi'])."""
    w_hi = w.to(torch.float16)
    return torch.cat([w_hi.contiguous().view(torch.uint8).reshape(*w.shape[:-1], 2 * w.shape[-1]), _e2m3_blocks(w_hi.float()), _e2m3_blocks(w - w_hi.float())], dim=-1)


def _mx_shift(t: torch.Tensor) -> int:
    """s with max |t| 2^s in [128, 256): e4m3 tops out at 448, its 17 binades below cover values 5 orders of magnitude under the largest."""
    import math
    m = float(t.abs().max())
    return max(-100, min(100, 7 - math.floor(math.log2(m)))) if m > 0 else 0


def _pack_mx(w: torch.Tensor, bias, cout: int, cin: int, R: int, S: int, dev, upsample_phases: bool = False, fmt: int = 8) -> "PackedWeight":
    """[Cout, R, S, C] fp32 -> the mixed-precision weight of an OMGSR_EL_MX operand: per tap 4C bytes = 2C 16-bit slots,
    [w_hi fp16 (2C B) | w_hi' fp8 (C B) | w_lo' fp8 (C B)] with w_hi = fp16(w), w_hi' = fp8(w_hi 2^s1), w_lo' = fp8((w - w_hi) 2^s2): the
    first C / 32 chunks meet a_hi in fp16 MFMAs, then C / 64 fp8 chunks meet a_lo' (w_hi') and C / 64 meet a_hi' (w_lo') in block-scaled
    fp8 MFMAs whose E8M0 scale operands undo s1 / s2 and the operand's 2^11.
    fmt 6 (split 4, OMGSR_EL_MX6; 3x3 convs of the halo-tile kernel only): the two correction thirds hold fp6 (e2m3) codes with a scale byte per
    32-channel block inside the data (_e2m3_blocks) - the MFMA runs them in half the passes of fp8."""
    if fmt == 6 and (R, S) != (3, 3):
        raise ValueError("the fp6 form (split 4) serves the 3x3 stride-1 convolutions of the halo-tile kernel")
    rows = (lambda t: _mx6_rows(t)) if fmt == 6 else (lambda t: _mx_rows(t, s1, s2))
    if (R, S) not in ((3, 3), (1, 1)) or cin % 64 or act_dtype() != torch.float16:
        raise ValueError("the mixed-precision (MX) form serves 3x3 and 1x1 convolutions (linears) with Cin % 64 == 0 in the fp16 compute type")
    ph = _phase_kernels(w) if upsample_phases else None       # [4, Cout, 2, 2, C]: one set of scales for the taps AND the phase sums
    both = w if ph is None else torch.cat([w.reshape(-1), ph.reshape(-1)])
    both_hi = both.to(torch.float16).float()
    s1, s2 = _mx_shift(both_hi), _mx_shift(both - both_hi)
    kslots = 2 * cin                                           # 16-bit slots per tap
    cout_pad = _round_up(cout, 256 if cout >= 256 else 128)
    out = torch.zeros((cout_pad, R * S * kslots), device=dev, dtype=torch.float16)
    out[:cout] = rows(w).reshape(cout, R * S * 4 * cin).contiguous().view(torch.float16)
    # 3x3: slice-major copy for the halo-tile kernel; 1x1 (a Linear): `out` itself is what igemm_gmx_kernel streams, row by row
    w_cm = out.view(cout_pad, 9, kslots // 32, 32).permute(2, 1, 0, 3).contiguous() if R == 3 else None
    w_ph = None
    if ph is not None:
        full = torch.zeros((4, cout_pad, 4 * kslots), device=dev, dtype=torch.float16)
        full[:, :cout] = rows(ph).reshape(4, cout, 4 * 4 * cin).contiguous().view(torch.float16)
        w_ph = full.view(4, cout_pad, 4, kslots // 32, 32).permute(0, 3, 2, 1, 4).contiguous()         # [phase][chunk][tap][Cout_pad][32]
    b = None if bias is None else bias.detach().to(device=dev, dtype=torch.float32).contiguous()
    if fmt == 6:
        return PackedWeight(out, b, cout, kslots, R, S, w_cm=w_cm, split=4, w_split=1, in_ld=kslots, w_ph=w_ph, mx=(cin // 32, 127, 127, 127, 127), mx_fmt=6)
    return PackedWeight(out, b, cout, kslots, R, S, w_cm=w_cm, split=3, w_split=1, in_ld=kslots, w_ph=w_ph,
                        mx=(cin // 32, 127 - s1, 127 - MX_LO_SHIFT, 127 - s2, 127))


def _phase_kernels(w: torch.Tensor) -> torch.Tensor:
    """[Cout, 3, 3, C] -> [4, Cout, 2, 2, C]: conv3x3(nearest_up2(x)) at output pixel (2y + a, 2x + b) only sees input rows
    y - 1 + a, y + a (columns likewise): the taps that land on one input pixel are summed (in fp64), phase index 2a + b."""
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    w64 = w.double()
    out = []
    for a in (0, 1):
        for b in (0, 1):
            k = torch.zeros((w.shape[0], 2, 2, w.shape[3]), dtype=torch.float64, device=w.device)
            for dy, rs in enumerate(rows[a]):
                for dx, ss in enumerate(rows[b]):
                    for r in rs:
                        for s_ in ss:
                            k[:, dy, dx] += w64[:, r, s_]
            out.append(k.float())
    return torch.stack(out, 0)


def pack_conv_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None, cout_multiple: int = 1,
                     split: int = 1, w_split: int = 1, upsample_phases: bool = False) -> PackedWeight:
    """[Cout, Cin, R, S] (torch conv layout) -> [Cout_pad, roundup(R*S*Kc, 32)] in the compute type, k = (r*S+s)*Kc + c.
    cout_multiple=8 widens the LOGICAL output to a multiple of 8 channels (zero weights, zero bias) so a
    3/4-channel conv writes 16-byte rows that the next kernel can consume directly.
    Per tap the contraction is a K-concatenation of segments of Cin8 channels, Kc = Cin8 * (split + w_split - 1):
      split 1, w_split 1   [w_hi]                 x [a]            one rounding of a, one of w
      split 2, w_split 1   [w_hi | w_hi]          x [a_hi | a_lo]  a to 2^-22
      split 1, w_split 2   [w_hi | w_lo]          x [a] (wraps)    w to 2^-22
      split 2, w_split 2   [w_hi | w_hi | w_lo]   x [a_hi | a_lo] (the third segment wraps to a_hi): both to 2^-22
    with w_hi = round(w), w_lo = round(w - w_hi) in the compute type; everything accumulates in ONE fp32 accumulator."""
    cout, cin, R, S = weight.shape
    dev = device or weight.device
    if cout % cout_multiple:
        extra = _round_up(cout, cout_multiple) - cout
        weight = torch.cat([weight.detach().to(dev), torch.zeros((extra, cin, R, S), device=dev, dtype=weight.dtype)], dim=0)
        if bias is not None:
            bias = torch.cat([bias.detach().to(dev), torch.zeros(extra, device=dev, dtype=bias.dtype)], dim=0)
        cout += extra
    cin8 = _round_up(cin, 8)
    w = _note_weight_range(weight.detach().to(device=dev, dtype=torch.float32)).permute(0, 2, 3, 1)  # [Cout,R,S,Cin]
    if cin8 != cin:
        w = torch.nn.functional.pad(w, (0, cin8 - cin))
    if split in (3, 4):
        if cin8 != cin:
            raise ValueError("the mixed-precision (MX) form needs Cin % 64 == 0")
        return _pack_mx(w, bias if bias is None else bias.detach().to(dev), cout, cin, R, S, dev, upsample_phases, fmt=6 if split == 4 else 8)
    if split not in (1, 2) or w_split not in (1, 2):
        raise ValueError("split / w_split must be 1 or 2")
    if w_split == 2 and bool(torch.equal(w.to(act_dtype()).float(), w)):
        # every value is exact in the compute type (an fp16 / bf16 checkpoint's layers that no LoRA merge touched): w_lo == 0, and a
        # segment of zeros adds exactly 0 to the accumulator - drop it (same bits, one K segment less). The phase form of an up-sampling conv
        # carries SUMS of 2 - 4 taps (_phase_kernels), which are not representable just because the taps are (round 6: with bf16-representable
        # weights the range-fallback tier rounded those sums to 8 bits and measured 3.4e-3 where full-mantissa weights measure 1.1e-3): the
        # segment goes only if the summed kernels are exact too - one w_split serves both packings, their K layouts must agree
        ph_exact = True
        if upsample_phases and R == 3 and S == 3:
            ph0 = _phase_kernels(w)
            ph_exact = bool(torch.equal(ph0.to(act_dtype()).float(), ph0))
        if ph_exact:
            w_split = 1
    in_ld = cin8 * split
    w_raw = w
    w = _segments(w, split, w_split)
    cin8 = w.shape[-1]
    w = w.reshape(cout, R * S * cin8)
    k_pad = _round_up(w.shape[1], 32)
    cout_pad = _round_up(cout, 256 if cout >= 256 else 128)   # 256-row padding lets the 256x256 GEMM tile run
    out = torch.zeros(cout_pad, k_pad, device=dev, dtype=act_dtype())
    out[:cout, : w.shape[1]] = w.to(act_dtype())
    b = None if bias is None else bias.detach().to(device=dev, dtype=torch.float32).contiguous()
    w_cm = None
    if R == 3 and S == 3 and cin8 % 32 == 0:
        # slice-major: [Cin/32][9 taps][Cout_pad][32] - the 128 x 32 weight slice of one (chunk, tap) K-step is one
        # contiguous 8 KB run, so every LDS-DMA wave instruction reads 8 full 128-B lines
        w_cm = out.view(cout_pad, 9, cin8 // 32, 32).permute(2, 1, 0, 3).contiguous()
    w_ph = None
    if upsample_phases and w_cm is not None and in_ld % 32 == 0:
        ph = _segments(_phase_kernels(w_raw), split, w_split).reshape(4, cout, 4 * cin8)          # k = (2 dy + dx) * Kc + c
        full = torch.zeros((4, cout_pad, 4 * cin8), device=dev, dtype=act_dtype())
        full[:, :cout] = ph.to(act_dtype())
        w_ph = full.view(4, cout_pad, 4, cin8 // 32, 32).permute(0, 3, 2, 1, 4).contiguous()         # [phase][chunk][tap][Cout_pad][32]
    return PackedWeight(out, b, cout, cin8, R, S, w_cm=w_cm, split=split, w_split=w_split, in_ld=in_ld, w_ph=w_ph)


def pack_linear_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None, split: int = 1, w_split: int = 1) -> PackedWeight:
    """[out, in] -> 1x1 'conv' weight."""
    return pack_conv_weight(weight[:, :, None, None], bias, device, split=split, w_split=w_split)


def pack_geglu_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None, split: int = 1, w_split: int = 1) -> PackedWeight:
    """GEGLU projection [2*inner, in] (rows [a | gate], diffusers `chunk(2, -1)`) -> rows interleaved in
    blocks of 32: [a_0..31, g_0..31, a_32..63, g_32..63, ...] so one 64-wide wave tile holds both halves."""
    two_inner, cin = weight.shape
    inner = two_inner // 2
    if inner % 32:
        raise ValueError("GEGLU inner dim must be a multiple of 32")
    a, g = weight[:inner], weight[inner:]
    w = torch.stack([a.reshape(inner // 32, 32, cin), g.reshape(inner // 32, 32, cin)], dim=1).reshape(two_inner, cin)
    pw = pack_linear_weight(w, None, device, split=split, w_split=w_split)
    if bias is not None:
        ba, bg = bias[:inner], bias[inner:]
        b = torch.stack([ba.reshape(-1, 32), bg.reshape(-1, 32)], dim=1).reshape(two_inner)
        pw.bias = b.detach().to(device=pw.w.device, dtype=torch.float32).contiguous()
    pw.cout = inner
    pw.geglu = True
    return pw


# --------------------------------------------------------------------------------------------
# MXFP8 (the fp8 tier: include/omgsr_hip.h OMGSR_EL_MXFP8)

@dataclass
class Mxfp8:
    """An OMGSR_EL_MXFP8 operand: e4m3fn codes uint8 [..., K] and E8M0 scales uint8 [..., K / 32] (one per 32 consecutive K values)."""
    codes: torch.Tensor
    scales: torch.Tensor

    @property
    def shape(self):
        return self.codes.shape

    def reshape(self, *lead) -> "Mxfp8":
        """Reshape the leading dims (the K / K-block dim stays last)."""
        lead = lead[:-1] if lead and lead[-1] == -1 else lead
        return Mxfp8(self.codes.reshape(*lead, self.codes.shape[-1]), self.scales.reshape(*lead, self.scales.shape[-1]))


def _mxfp8_like(x: torch.Tensor) -> Mxfp8:
    """An uninitialised Mxfp8 of x's shape."""
    return Mxfp8(torch.empty(x.shape, device=x.device, dtype=torch.uint8),
                 torch.empty((*x.shape[:-1], x.shape[-1] // 32), device=x.device, dtype=torch.uint8))


def parse_fp8_fused_quant(value: Optional[str]) -> dict:
    """OMGSR_FP8_FUSED_QUANT -> which producers of the fp8 tier write their MXFP8 output themselves: unset = the measured defaults
    below, "0" = none (the pass form everywhere: producer writes bf16, quantize_mxfp8 reads it), "1" = every fused producer. The fused forms
    write the pass form's bytes, so the switch changes launches, never results."""
    if value is None or value.strip() == "":
        return dict(FP8_FUSED_QUANT_DEFAULT)
    if value.strip() not in ("0", "1"):
        raise ValueError(f"OMGSR_FP8_FUSED_QUANT must be 0 or 1, got {value!r}")
    on = value.strip() == "1"
    return {"layernorm": on, "gemm": on}


# per fused producer kind. profiles/fp8_fused_quant.json: each kernel beats the launches it replaces; in the F-1024 batch-8 step the pair is the one
# setting whose every step is faster than every pass-form step (each kind alone gains ~3 ms at the median, inside the spread) - so both are on
FP8_FUSED_QUANT_DEFAULT = {"layernorm": True, "gemm": True}
FP8_FUSED_QUANT = parse_fp8_fused_quant(os.environ.get("OMGSR_FP8_FUSED_QUANT"))         # A/B switch, parsed once at import


def _row_pitch(x: torch.Tensor, name: str) -> int:
    """Pitch (elements) of the rows of x [..., K]: x is dense, or the column window t[..., c0:c0 + K] of a dense tensor."""
    K = x.shape[-1]
    if x.dim() < 2 or x.is_contiguous():
        return K
    ld = x.stride(-2)
    ok = x.stride(-1) == 1 and ld >= K and all(x.stride(i) == x.stride(i + 1) * x.shape[i + 1] for i in range(x.dim() - 2))
    if not ok:
        raise ValueError(f"{name}: expected a dense tensor or a column window of one")
    return ld


def quantize_mxfp8(x: torch.Tensor, out: Optional[Mxfp8] = None, out_col: Optional[int] = None) -> Mxfp8:
    """x bf16 or fp32 [..., K] (K % 128 == 0) -> its OMGSR_EL_MXFP8 form, on the device (omgsr_quantize_mxfp8): scale = max(0, biased
    exponent of the block's largest |v| - 8), code = (v / 2^(scale - 127)).clamp(-448, 448) in e4m3fn, round to nearest even.
    out: a dense Mxfp8 of x's shape to write into (a workspace).
    out_col (with `out` a dense Mxfp8 [..., Kw], Kw >= K): x - dense, or a column window of a dense tensor - goes into columns
    [out_col, out_col + K) of `out` (out_col % 128 == 0; omgsr_quantize_mxfp8_ld); the other columns are not touched. Returns `out`."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"quantize_mxfp8: expected bfloat16 or float32, got {x.dtype}")
    K = x.shape[-1]
    if K % 128:
        raise ValueError(f"quantize_mxfp8: K = {K} is not a multiple of 128")
    rows = x.numel() // K
    el = EL_F32 if x.dtype == torch.float32 else EL_16
    if out_col is not None:
        if out is None:
            raise ValueError("quantize_mxfp8: out_col needs `out`")
        Kw = out.codes.shape[-1]
        if (out.codes.shape[:-1] != x.shape[:-1] or out.scales.shape != (*x.shape[:-1], Kw // 32) or Kw % 128 or out_col % 128 or out_col < 0
                or out_col + K > Kw or not (out.codes.is_contiguous() and out.scales.is_contiguous())):
            raise ValueError("quantize_mxfp8: x does not fit `out` at out_col")
        check(_lib.load().omgsr_quantize_mxfp8_ld(x.data_ptr(), el, rows, K, _row_pitch(x, "quantize_mxfp8"), out.codes.data_ptr() + out_col,
                                                  out.scales.data_ptr() + out_col // 32, Kw, Kw // 32, _stream()), "omgsr_quantize_mxfp8_ld")
        return out
    _req(x, x.dtype, "x")
    if out is not None:
        if out.codes.shape != x.shape or out.scales.shape != (*x.shape[:-1], K // 32) or not (out.codes.is_contiguous() and out.scales.is_contiguous()):
            raise ValueError("quantize_mxfp8: `out` does not match x")
        out = Mxfp8(out.codes, out.scales)
    else:
        out = _mxfp8_like(x)
    check(_lib.load().omgsr_quantize_mxfp8(x.data_ptr(), el, rows, K, K, out.codes.data_ptr(), out.scales.data_ptr(), _stream()),
          "omgsr_quantize_mxfp8")
    return out


def pack_linear_weight_mxfp8(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None) -> PackedWeight:
    """[out, in] bf16 -> the fp8 tier's weight: rows padded with zeros to a multiple of 256 and quantised on the device (quantize_mxfp8)."""
    if _PRECISE or _ACT != torch.bfloat16:
        raise ValueError("an fp8 (MXFP8) layer needs the bf16 compute type (the fp8 tier); the accurate tier and fp16 have none")
    dev = device or weight.device
    cout, cin = weight.shape
    if cin % 128:
        raise ValueError(f"an fp8 (MXFP8) layer needs in_features % 128 == 0, got {cin}")
    w = torch.zeros((_round_up(cout, 256), cin), device=dev, dtype=torch.bfloat16)
    w[:cout] = weight.detach().to(device=dev, dtype=torch.bfloat16)
    q = quantize_mxfp8(w)
    b = None if bias is None else bias.detach().to(device=dev, dtype=torch.float32).contiguous()
    return PackedWeight(q.codes, b, cout, cin, 1, 1, w_scale=q.scales)


def pack_geglu_weight_mxfp8(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None) -> PackedWeight:
    """GEGLU projection [2 * inner, in] bf16 -> the weight of omgsr_igemm_geglu_mxfp8: rows interleaved as pack_geglu_weight does
    ([32 a | 32 gate] per 64 packed rows), K zero-padded to a multiple of 128 (the UNet's C = 320 -> 384: the operand carries the same pad,
    layer_norm_mxfp8(pad128=True)) and the packed rows to a multiple of 256, quantised on the device (quantize_mxfp8: a zero block is codes
    0x00 under scale byte 0x00). `cout` = inner, `cin` = the padded K; the bias is interleaved the same way, fp32, zero-padded to the rows."""
    if _PRECISE or _ACT != torch.bfloat16:
        raise ValueError("an fp8 (MXFP8) layer needs the bf16 compute type; the accurate tier and fp16 have none")
    dev = device or weight.device
    two_inner, cin = weight.shape
    inner = two_inner // 2
    if two_inner % 2 or inner % 32:
        raise ValueError("GEGLU inner dim must be a multiple of 32")
    kp, rows = _round_up(cin, 128), _round_up(two_inner, 256)
    wd = weight.detach().to(device=dev, dtype=torch.bfloat16)
    w = torch.zeros((rows, kp), device=dev, dtype=torch.bfloat16)
    w[:two_inner, :cin] = torch.stack([wd[:inner].reshape(inner // 32, 32, cin), wd[inner:].reshape(inner // 32, 32, cin)], dim=1).reshape(two_inner, cin)
    q = quantize_mxfp8(w)
    b = None
    if bias is not None:
        bd = bias.detach().to(device=dev, dtype=torch.float32)
        b = torch.zeros(rows, device=dev, dtype=torch.float32)
        b[:two_inner] = torch.stack([bd[:inner].reshape(-1, 32), bd[inner:].reshape(-1, 32)], dim=1).reshape(two_inner)
    return PackedWeight(q.codes, b, inner, kp, 1, 1, geglu=True, w_scale=q.scales)


def _fp8_operand(x, pw: PackedWeight, what: str) -> Optional[Mxfp8]:
    """The MXFP8 operand of an fp8 weight (a bf16 tensor is quantised here); None for the other weight forms, which take no MXFP8 operand."""
    if not pw.fp8:
        if isinstance(x, Mxfp8):
            raise ValueError(f"{what}: an MXFP8 operand needs an fp8-packed weight")
        return None
    xq = x if isinstance(x, Mxfp8) else quantize_mxfp8(x)
    if xq.codes.shape[-1] != pw.cin:
        raise ValueError(f"{what}: operand K {xq.codes.shape[-1]} != weight K {pw.cin}")
    return xq


def _fill_mxfp8(a: IgemmArgs, codes_ptr: int, scales_ptr: int, pw: PackedWeight) -> None:
    """Operand and weight side of a GEMM over an MXFP8 operand and an fp8-packed linear weight (pack_linear_weight_mxfp8)."""
    a.in_, a.in_scale = codes_ptr, scales_ptr
    a.weight, a.w_scale, a.bias = pw.w.data_ptr(), pw.w_scale.data_ptr(), _ptr(pw.bias)
    a.mxf8 = 1
    a.Cin, a.Cout, a.Cout_pad, a.K_pad = pw.cin, pw.cout, pw.cout_pad, pw.k_pad
    _fill_taps_1x1(a)


def pack_conv_weight_mxfp8(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None, cin_multiple: int = 128) -> PackedWeight:
    """[Cout, Cin, 3, 3] bf16 -> the weight of omgsr_conv_mxfp8 (include/omgsr_hip.h): one MXFP8 block per 32 consecutive input channels of
    one (cout, ky, kx), quantised on the device by quantize_mxfp8 (rows = (cout, tap), K = Cin), then laid out slice-major:
    `w_cm` codes uint8 [Cin/64][9][Cout_pad][64], `w_scale` uint8 [Cin/64][Cout_pad][2][16] (byte t < 9 = tap t). Rows are padded with zeros
    to a multiple of 128; `w` is the codes tensor too (the row-major packing does not exist in this form).
    cin_multiple=64: the same layout for omgsr_conv_mxfp8_deep (whole 64-channel chunks; nothing in the layout needs more). quantize_mxfp8
    wants K % 128 == 0, so the rows are quantised with Cin padded by zero channels - blocks are independent, the padding's are dropped."""
    if _PRECISE or _ACT != torch.bfloat16:
        raise ValueError("an fp8 (MXFP8) layer needs the bf16 compute type (the fp8 tier); the accurate tier and fp16 have none")
    dev = device or weight.device
    cout, cin, R, S = weight.shape
    if cin_multiple not in (64, 128):
        raise ValueError(f"pack_conv_weight_mxfp8: cin_multiple is 128 (omgsr_conv_mxfp8) or 64 (omgsr_conv_mxfp8_deep), got {cin_multiple}")
    if (R, S) != (3, 3) or cin % cin_multiple:
        raise ValueError(f"an fp8 (MXFP8) conv needs a 3x3 kernel and in_channels % {cin_multiple} == 0, got {tuple(weight.shape)}")
    cout8 = _round_up(cout, 8)
    cout_pad = _round_up(cout8, 128)
    cin_q = _round_up(cin, 128)
    w = torch.zeros((cout_pad, 9, cin_q), device=dev, dtype=torch.bfloat16)
    w[:cout, :, :cin] = weight.detach().to(device=dev, dtype=torch.bfloat16).permute(0, 2, 3, 1).reshape(cout, 9, cin)
    q = quantize_mxfp8(w)
    if cin_q != cin:
        q = Mxfp8(q.codes[..., :cin].contiguous(), q.scales[..., :cin // 32].contiguous())
    codes = q.codes.view(cout_pad, 9, cin // 64, 64).permute(2, 1, 0, 3).contiguous()                 # [chunk][tap][cout][64]
    sc = torch.zeros((cin // 64, cout_pad, 2, 16), device=dev, dtype=torch.uint8)
    sc[..., :9] = q.scales.view(cout_pad, 9, cin // 64, 2).permute(2, 0, 3, 1)                          # [chunk][cout][block][tap]
    b = None
    if bias is not None:
        b = torch.zeros(cout8, device=dev, dtype=torch.float32)
        b[:cout] = bias.detach().to(device=dev, dtype=torch.float32)
    return PackedWeight(codes.view(cin // 64 * 9 * cout_pad, 64), b, cout8, cin, 3, 3, w_cm=codes, w_scale=sc)


def pack_conv_weight_mxfp8_up(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None) -> PackedWeight:
    """[Cout, Cin, 3, 3] bf16 -> the weight of omgsr_conv_mxfp8_up (include/omgsr_hip.h): the four phase-summed 2 x 2 kernels of a 3x3 conv
    applied to a nearest-2x up-sampled map (_phase_kernels: fp64 sums, phase 2a + b, tap 2 dy + dx), one MXFP8 block per 32 consecutive input
    channels of one (phase, cout, tap), quantised on the device by quantize_mxfp8 (rows = (phase, cout, tap), K = Cin, from the fp32 sums), then
    laid out slice-major: `w_ph` codes uint8 [4][Cin/64][4][Cout_pad][64], `w_scale` uint8 [4][Cin/64][Cout_pad][2][4] (byte t = tap t of that
    (phase, chunk, cout, block)). Rows are padded with zeros to a multiple of 128; `w` is the codes tensor too."""
    if _PRECISE or _ACT != torch.bfloat16:
        raise ValueError("an fp8 (MXFP8) layer needs the bf16 compute type (the fp8 tier); the accurate tier and fp16 have none")
    dev = device or weight.device
    cout, cin, R, S = weight.shape
    if (R, S) != (3, 3) or cin % 128:
        raise ValueError(f"an fp8 (MXFP8) up-sampling conv needs a 3x3 kernel and in_channels % 128 == 0, got {tuple(weight.shape)}")
    cout8 = _round_up(cout, 8)
    cout_pad = _round_up(cout8, 128)
    ph = _phase_kernels(weight.detach().to(device=dev, dtype=torch.bfloat16).permute(0, 2, 3, 1).float())      # [4, Cout, 2, 2, Cin]
    w = torch.zeros((4, cout_pad, 4, cin), device=dev, dtype=torch.float32)
    w[:, :cout] = ph.reshape(4, cout, 4, cin)
    q = quantize_mxfp8(w)
    codes = q.codes.view(4, cout_pad, 4, cin // 64, 64).permute(0, 3, 2, 1, 4).contiguous()           # [phase][chunk][tap][cout][64]
    sc = q.scales.view(4, cout_pad, 4, cin // 64, 2).permute(0, 3, 1, 4, 2).contiguous()                # [phase][chunk][cout][block][tap]
    b = None
    if bias is not None:
        b = torch.zeros(cout8, device=dev, dtype=torch.float32)
        b[:cout] = bias.detach().to(device=dev, dtype=torch.float32)
    return PackedWeight(codes.view(-1, 64), b, cout8, cin, 3, 3, w_ph=codes, w_scale=sc)


# --------------------------------------------------------------------------------------------
# K1-K3, K5, K6: implicit-GEMM conv / linear / bmm

def to_operand(x: torch.Tensor, split: int = 1) -> torch.Tensor:
    """Stream tensor -> MFMA operand [..., split*C]: a no-op for a tensor already in the compute type (fast tiers),
    one rounding (split 1) or the two-term split [hi | lo] (split 2) of an fp32 stream tensor."""
    if x.dtype == _ACT:
        if split != 1:
            raise ValueError("to_operand: a 16-bit tensor cannot be split (split operands exist in the accurate tier only)")
        return x
    _req(x, torch.float32, "x")
    Cc = x.shape[-1]
    y = torch.empty((*x.shape[:-1], min(split, 2) * Cc), device=x.device, dtype=_ACT)
    check(_lib.load().omgsr_to_operand(x.data_ptr(), y.data_ptr(), x.numel() // Cc, Cc, _el_of_split(split), _ovf(x.device),
                                       _stream()), "omgsr_to_operand")
    return y


def _out_tensor(shape, cout: int, out_dtype: int, out_split: int, device) -> torch.Tensor:
    if out_dtype == OUT_STREAM:
        out_dtype = OUT_F32 if _PRECISE else OUT_BF16
        if out_split != 1:
            raise ValueError("out_split applies to operand outputs (out_dtype=OUT_BF16)")
    if out_dtype == OUT_F32:
        return torch.empty((*shape, cout), device=device, dtype=torch.float32)
    return torch.empty((*shape, cout * min(out_split, 2)), device=device, dtype=_ACT)       # split 3 (MX): 4 bytes per channel, like split 2


# The fillers below write one concern each into a ZEROED omgsr_igemm_args (a fresh IgemmArgs()): what they do not mention stays 0 / NULL.

def _fill_weight(a: IgemmArgs, pw: PackedWeight, x_ptr: int, scales_ptr: Optional[int] = None) -> None:
    """Operand pointer and weight side of a packed weight: pointers, padded extents and the contraction geometry (Cin = every K segment
    of a tap, in_ld = the operand row it wraps over).
    scales_ptr: the operand is MXFP8 (x_ptr its codes) and `pw` an fp8-packed linear weight - _fill_mxfp8 on top."""
    a.in_, a.weight, a.bias, a.weight_cm = x_ptr, pw.w.data_ptr(), _ptr(pw.bias), _ptr(pw.w_cm)
    a.Cin, a.Cout, a.Cout_pad, a.K_pad = pw.cin, pw.cout, pw.cout_pad, pw.k_pad
    a.overflow_flag = _ovf(pw.w.device)
    a.in_ld = pw.row_channels if pw.row_channels != pw.cin else 0
    a.in_split = int(pw.split >= 2)            # split 3 (MX): 2C slots per tap for C logical channels, like the two-term split
    a.w_split = int(pw.w_split == 2)
    if pw.mx is not None:
        a.mx_chunks16, a.mx_scale_w1, a.mx_scale_a1, a.mx_scale_w2, a.mx_scale_a2 = pw.mx
        a.mx_fmt = pw.mx_fmt
    if scales_ptr is not None:
        _fill_mxfp8(a, x_ptr, scales_ptr, pw)


def _fill_taps_1x1(a: IgemmArgs) -> None:
    a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample = 1, 1, 1, 0, 0, 0


def _fill_gemm(a: IgemmArgs, M: int, batch: int = 1, in_bstride: int = 0, w_bstride: int = 0, out_bstride: int = 0) -> None:
    """GEMM-shaped geometry: M rows as a 1 x M map under a 1x1 kernel; `batch` problems on grid.z, the three strides in elements."""
    a.N, a.H, a.W, a.Ho, a.Wo = 1, 1, M, 1, M
    _fill_taps_1x1(a)
    a.batch, a.in_bstride, a.w_bstride, a.out_bstride = batch, in_bstride, w_bstride, out_bstride


def _fill_out(a: IgemmArgs, out: torch.Tensor, out_split: int, residual: Optional[torch.Tensor], cout: int) -> None:
    """A dense output (out_split 2: [hi | lo] at the front of rows that may be wider) and the residual."""
    a.out = out.data_ptr()
    a.out_dtype = OUT_F32 if out.dtype == torch.float32 else OUT_BF16
    a.out_lo_off = cout if out_split == 2 else 0
    a.out_ld = out.shape[-1] if out_split == 2 else 0
    a.out_mx = {3: 1, 4: 6}.get(out_split, 0)
    if residual is not None:
        a.residual, a.res_el = residual.data_ptr(), _el(residual, "residual")


def _fill_out_slice(a: IgemmArgs, buf: torch.Tensor, first: int, *, ld: int = 0, lo_off: int = 0, t_rows: Optional[int] = None) -> None:
    """A 16-bit output inside a caller's buffer, `first` elements in. Row-major window (linear_into): rows of pitch `ld`, the low halves of
    a two-term split `lo_off` columns behind the high ones. t_rows given: the transposed layout (LAYOUT_T), t_rows rows per image, pitch
    buf.shape[-1]."""
    a.out, a.out_dtype = buf.data_ptr() + 2 * first, OUT_BF16
    a.out_ld, a.out_lo_off = ld, lo_off
    if t_rows is not None:
        a.out_layout, a.t_rows, a.t_ld = LAYOUT_T, t_rows, buf.shape[-1]


def _fill_out_mxfp8(a: IgemmArgs, dst: Mxfp8, row0: int, col0: int) -> tuple:
    """The output written as OMGSR_EL_MXFP8 (omgsr_igemm_out_mxfp8: the fp8 tier's MXFP8 GEMM only): rows row0 ..., columns col0 ... of the dense
    planes of `dst` [rows, Kw] - the column offset goes into both pointers, the pitches are the planes' own. The code plane goes into the block;
    returns what travels next to it: (scale pointer, scale pitch)."""
    Kw = dst.codes.shape[-1]
    a.out, a.out_dtype, a.out_ld = dst.codes.data_ptr() + row0 * Kw + col0, OUT_BF16, Kw
    return dst.scales.data_ptr() + row0 * (Kw // 32) + col0 // 32, Kw // 32


def _igemm_out_mxfp8(a: IgemmArgs, scale: tuple, what: str) -> None:
    """Launch omgsr_igemm_out_mxfp8 (never splits K: no workspace)."""
    check(_lib.load().omgsr_igemm_out_mxfp8(C.byref(a), scale[0], scale[1], _stream()), what)


def _fill_geglu_mxfp8(a: IgemmArgs, xq: Mxfp8, pw: PackedWeight, M: int) -> None:
    """The argument block of omgsr_igemm_geglu_mxfp8 but for its output: an MXFP8 operand [M, K] against pack_geglu_weight_mxfp8's weight (the
    operand's K is the pack's padded K); `Cout` counts the logical columns, `Cout_pad` the packed rows."""
    _fill_mxfp8(a, xq.codes.data_ptr(), xq.scales.data_ptr(), pw)
    _fill_gemm(a, M)
    a.act, a.alpha, a.sample_rows = ACT_GEGLU, 1.0, M


def _igemm_geglu_mxfp8(a: IgemmArgs, scale: Optional[tuple], what: str) -> None:
    """Launch omgsr_igemm_geglu_mxfp8: scale = (scale pointer, scale pitch) of the OMGSR_EL_MXFP8 output (_fill_out_mxfp8), None = the plain output."""
    check(_lib.load().omgsr_igemm_geglu_mxfp8(C.byref(a), scale[0] if scale else None, scale[1] if scale else 0, _stream()), what)


def _linear_geglu_mxfp8(xq: Mxfp8, pw: PackedWeight, out_dtype: int, dst8: Optional[Mxfp8]):
    """linear() of an MXFP8 operand against an fp8 GEGLU pack: mxfp8_gemm_geglu_kernel. dst8: the hidden tensor as an Mxfp8 - from the GEMM's
    epilogue, or (FP8_FUSED_QUANT["gemm"] off: the pass form) from quantize_mxfp8 over the bf16 output; the same bytes."""
    lead = xq.codes.shape[:-1]
    M = xq.codes.numel() // pw.cin
    a = IgemmArgs()
    _fill_geglu_mxfp8(a, xq, pw, M)
    if dst8 is not None and FP8_FUSED_QUANT["gemm"]:
        scale = _fill_out_mxfp8(a, dst8.reshape(M, -1), 0, 0)
        _igemm_geglu_mxfp8(a, scale, "omgsr_igemm_geglu_mxfp8(linear, out_mxfp8)")
        return dst8
    out = _out_tensor(lead, pw.cout, OUT_BF16 if dst8 is not None else out_dtype, 1, xq.codes.device)
    _fill_out(a, out, 1, None, pw.cout)
    _igemm_geglu_mxfp8(a, None, "omgsr_igemm_geglu_mxfp8(linear)")
    if dst8 is None:
        return out
    if dst8.codes.shape[-1] == pw.cout:
        return quantize_mxfp8(out, out=dst8)
    return quantize_mxfp8(out, out=dst8, out_col=0)


def _out_mxfp8_dst(what: str, out_mxfp8, pw: PackedWeight, lead, device, col0: int = 0, *, residual=None, gate=None, plain: bool = True) -> Optional[Mxfp8]:
    """Validates an `out_mxfp8=` request (True: a fresh dense Mxfp8 [*lead, Cout]; an Mxfp8: the destination, dense, [*lead, Kw] with the
    result at columns col0 ...) before anything is launched; None when not requested."""
    if out_mxfp8 is None or out_mxfp8 is False:
        return None
    if not pw.fp8:
        raise ValueError(f"{what}: out_mxfp8 needs an fp8-packed weight (the MXFP8 GEMM's epilogue writes the form)")
    if residual is not None or gate is not None or not plain:
        raise ValueError(f"{what}: out_mxfp8 goes with bias and act only (no residual, gate, GroupNorm statistics, split or fp32 output)")
    if pw.cout % 32:
        raise ValueError(f"{what}: out_mxfp8 needs Cout % 32 == 0, got {pw.cout}")
    if out_mxfp8 is True:
        if col0:
            raise ValueError(f"{what}: out_mxfp8=True writes a dense result")
        if pw.cout % 128:
            raise ValueError(f"{what}: a dense Mxfp8 result needs Cout % 128 == 0, got {pw.cout}")
        return Mxfp8(torch.empty((*lead, pw.cout), device=device, dtype=torch.uint8), torch.empty((*lead, pw.cout // 32), device=device, dtype=torch.uint8))
    if not isinstance(out_mxfp8, Mxfp8):
        raise TypeError(f"{what}: out_mxfp8 is True or an Mxfp8")
    Kw = out_mxfp8.codes.shape[-1]
    if (tuple(out_mxfp8.codes.shape[:-1]) != tuple(lead) or tuple(out_mxfp8.scales.shape) != (*lead, Kw // 32) or Kw % 128 or col0 % 128 or col0 < 0
            or col0 + pw.cout > Kw or not (out_mxfp8.codes.is_contiguous() and out_mxfp8.scales.is_contiguous())):
        raise ValueError(f"{what}: the result does not fit the Mxfp8 destination at column {col0}")
    return out_mxfp8


def _conv_args(a: IgemmArgs, x: torch.Tensor, pw: PackedWeight, stride, pad, upsample, act, residual, gate, out_dtype, alpha, out, out_split,
               sample_rows):
    """Fill `a` for one conv problem; returns (x as operand, out). Keep both alive until the launch."""
    if x.dtype == torch.float32:
        x = to_operand(x, pw.split)
    _req(x, act_dtype(), "x")
    N, H, W, Cin = x.shape
    if Cin != pw.row_channels:
        raise ValueError(f"conv2d: input has {Cin} channels, packed weight expects {pw.row_channels}")
    if isinstance(pad, int):
        pad = (pad, pad, pad, pad)
    pt, pb, pl, pr = pad
    Hv, Wv = (H * 2, W * 2) if upsample else (H, W)
    Ho = (Hv + pt + pb - pw.R) // stride + 1
    Wo = (Wv + pl + pr - pw.S) // stride + 1
    if pw.geglu:
        act = ACT_GEGLU
    if out is None:
        out = _out_tensor((N, Ho, Wo), pw.cout, out_dtype, out_split, x.device)
    if residual is not None and tuple(residual.shape) != (N, Ho, Wo, pw.cout):
        raise ValueError(f"residual shape {tuple(residual.shape)} != output {(N, Ho, Wo, pw.cout)}")
    _fill_weight(a, pw, x.data_ptr())
    a.weight_ph = _ptr(pw.w_ph) if upsample else None
    a.N, a.H, a.W, a.Ho, a.Wo = N, H, W, Ho, Wo
    a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample = pw.R, pw.S, stride, pt, pl, int(upsample)
    _fill_out(a, out, out_split, residual, pw.cout)
    a.gate, a.act, a.alpha, a.batch = _ptr(gate), act, alpha, 1
    a.sample_rows = sample_rows or Ho * Wo
    return x, out


class GnHandle(NamedTuple):
    """The GroupNorm statistics a producer's epilogue left, carried by its output as `_omgsr_gn` (read by index: a plain tuple serves too)."""
    partial: torch.Tensor      # [N, nslot, entries, 2] (sum, sum of squares); entries = groups, or channels for odd group sizes
    groups: int                # the group count the producer was told
    ptr: int                   # the output's data_ptr() and _version when the statistics were left: stale once either moves
    version: int


def _leave_gn(out: torch.Tensor, partial: torch.Tensor, groups: int) -> None:
    """Attach the handle group_norm_stats(out) / group_norm_pair consume."""
    out._omgsr_gn = GnHandle(partial, groups, out.data_ptr(), out._version)


def _gn_handle(x: torch.Tensor, N: int):
    """x's handle when it still describes x (same storage, not written since) for N images, else None."""
    h = getattr(x, "_omgsr_gn", None)
    if h is not None and h[2] == x.data_ptr() and h[3] == x._version and h[0].shape[0] == N:
        return h
    return None


def _conv_gn(a: IgemmArgs, gn_groups: int, out_split: int, device):
    """Ask the library whether this problem's epilogue can leave the GroupNorm statistics; allocates the partials if so."""
    if gn_groups <= 0 or out_split != 1:
        return None
    a.gn_groups = gn_groups
    lib = _lib.load()
    # a problem that will be split over K (it is handed the workspace) finishes in the reduce pass: no statistics there
    nslot = 0 if lib.omgsr_igemm_workspace_bytes(C.byref(a)) > 0 else lib.omgsr_igemm_gn_slots(C.byref(a))
    if nslot <= 0:
        return None
    a.gn_entries = lib.omgsr_igemm_gn_entries(C.byref(a))       # per group, or per channel for odd group sizes
    partial = torch.empty((a.N, nslot, a.gn_entries, 2), device=device, dtype=torch.float32)
    a.gn_partial = partial.data_ptr()
    return partial


class GnSpec:
    """A GroupNorm waiting for its consumer: statistics (mean / rstd [nimg, G]; rows n of the tensor use image n % nimg), affine, activation.
    conv2d(..., gn=spec) runs it as the conv's patch producer when the library says the problem qualifies (omgsr_igemm_gn_fusable: the
    halo-tile kernel's spatial 3x3 form over a 16-bit stream tensor, plain operand and weight) - the apply pass and the conv's read of its
    output disappear - and as the separate apply pass in front of the conv otherwise. Same values either way up to the 16-bit rounding the
    apply pass performs too (the fused form evaluates x * scale + shift from the same fp32 (scale, shift) table)."""

    def __init__(self, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int, act: int = ACT_NONE):
        self.mean, self.rstd, self.gamma, self.beta, self.groups, self.act = mean, rstd, gamma, beta, groups, act
        self._table = None

    def table(self, channels: int) -> torch.Tensor:
        """f32 [nimg, C, 2] = (rstd gamma, beta - mean rstd gamma): one tiny launch per GroupNorm, shared by every tile-shape group."""
        if self._table is None:
            nimg = self.mean.shape[0]
            t = torch.empty((nimg, channels, 2), device=self.mean.device, dtype=torch.float32)
            check(_lib.load().omgsr_groupnorm_scale_shift(self.mean.data_ptr(), self.rstd.data_ptr(), _ptr(self.gamma), _ptr(self.beta),
                                                          t.data_ptr(), nimg, channels, self.groups, _stream()), "omgsr_groupnorm_scale_shift")
            self._table = t
        return self._table

    def apply(self, x: torch.Tensor, split: int = 1) -> torch.Tensor:
        """The separate pass: stream tensor -> normalised operand in the form the consumer reads (split 5: an Mxfp8)."""
        if split == 5:
            return group_norm_apply_mxfp8(x, self.mean, self.rstd, self.gamma, self.beta, self.groups, self.act)
        if self.mean.shape[0] != x.shape[0]:
            return group_norm_apply_shared(x, self.mean, self.rstd, self.gamma, self.beta, self.groups, self.act, split=split)
        return group_norm_apply(x, self.mean, self.rstd, self.gamma, self.beta, self.groups, self.act, split=split)


def _gn_candidate(x: torch.Tensor, pw: PackedWeight) -> bool:
    """Host-side part of the fusable test (the library decides the rest from the geometry): a 16-bit stream tensor, plain operand / weight."""
    return x.dtype == _ACT and pw.split == 1 and pw.w_split == 1 and pw.mx is None and pw.R == 3 and pw.S == 3


def _gn_fusable(a: IgemmArgs, gn: "GnSpec") -> bool:
    return gn.act == ACT_SILU and bool(_lib.load().omgsr_igemm_gn_fusable(C.byref(a)))


def _attach_gn(a: IgemmArgs, gn: "GnSpec", channels: int) -> torch.Tensor:
    t = gn.table(channels)
    a.gn_scale_shift, a.gn_nimg, a.gn_act, a.in_el = t.data_ptr(), t.shape[0], gn.act, EL_16
    return t


def conv2d(x: torch.Tensor, pw: PackedWeight, *, stride: int = 1, pad: tuple[int, int, int, int] | int = 1,
           upsample: bool = False, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None,
           gate: Optional[torch.Tensor] = None, out_dtype: int = OUT_STREAM, alpha: float = 1.0,
           out: Optional[torch.Tensor] = None, gn_groups: int = 0, out_split: int = 1, sample_rows: int = 0,
           gn: Optional["GnSpec"] = None, fp8_pack=None, fp8_up_pack=None, fp8_deep_pack=None) -> torch.Tensor:
    """x [N,H,W,Cin] operand (or a stream tensor: cast / split here) -> [N,Ho,Wo,Cout]. pad = (top, bottom, left, right) on
    the (virtual) input. out_dtype: OUT_STREAM (a stream tensor: default), OUT_BF16 (a 16-bit operand for the next GEMM,
    `out_split` 2 = written as the two-term split) or OUT_F32. residual: a stream tensor of the output's shape.
    gn_groups > 0: the caller will GroupNorm the result with that many groups; when the kernel can, it emits the
    (sum, sum of squares) partials from its epilogue and group_norm_stats() skips its read pass over the tensor.
    gn: x is the stream tensor a GroupNorm (+ SiLU) reads and the conv consumes the normalised tensor (GnSpec): fused into the conv's
    patch producer where the library can, the apply pass in front of the conv otherwise.
    fp8_pack (a layer marked by precision.set_fp8_conv; needs gn): a callable returning the layer's pack_conv_weight_mxfp8 form. Where
    omgsr_conv_mxfp8_ok accepts the problem (a per-problem decision from one sample's geometry), the GroupNorm runs as the apply pass that
    writes MXFP8 and mxfp8_conv_kernel runs the conv; otherwise the call takes the 16-bit path below exactly as without it.
    fp8_up_pack (upsample=True on a layer marked by precision.set_fp8_upsample; no gn, no residual): a callable returning the layer's
    pack_conv_weight_mxfp8_up form. Where omgsr_conv_mxfp8_up_ok accepts the problem, x goes through quantize_mxfp8 (one pass over the
    low-resolution map) and mxfp8_conv_up_kernel runs the conv; otherwise the call takes the 16-bit path below exactly as without it.
    fp8_deep_pack (a layer marked by precision.set_fp8_unet_conv; needs gn): a callable returning the layer's
    pack_conv_weight_mxfp8(cin_multiple=64) form. Where omgsr_conv_mxfp8_deep_ok accepts the problem, the GroupNorm runs as the apply pass that
    writes MXFP8 (group_norm_apply_mxfp8 with c64) and mxfp8_conv_deep_kernel runs the conv; otherwise the call takes the 16-bit path below
    exactly as without it. The deep kernel serves everything omgsr_conv_mxfp8_ok accepts too, so a layer with this mark never needs the other
    pack. (Every shape of the UNet's served levels is faster this way in every timed step, DESIGN.md 3.5: none is held back by shape.)"""
    a = IgemmArgs()
    if gn is not None and not _gn_candidate(x, pw):
        x, gn = gn.apply(x, pw.split), None
    x, out = _conv_args(a, x, pw, stride, pad, upsample, act, residual, gate, out_dtype, alpha, out, out_split, sample_rows)
    if fp8_pack is not None and gn is not None and out_split == 1 and _lib.load().omgsr_conv_mxfp8_ok(C.byref(a)):
        return _conv2d_mxfp8(a, gn.apply(x, 5), fp8_pack(), out, gn_groups)
    if fp8_deep_pack is not None and gn is not None and out_split == 1 and _lib.load().omgsr_conv_mxfp8_deep_ok(C.byref(a)):
        xq = group_norm_apply_mxfp8(x, gn.mean, gn.rstd, gn.gamma, gn.beta, gn.groups, gn.act, c64=True)
        return _conv2d_mxfp8(a, xq, fp8_deep_pack(), out, gn_groups, deep=True)
    if (fp8_up_pack is not None and upsample and gn is None and residual is None and out_split == 1
            and _lib.load().omgsr_conv_mxfp8_up_ok(C.byref(a))):
        return _conv2d_mxfp8_up(a, quantize_mxfp8(x), fp8_up_pack(), out, gn_groups)
    if out_split == 4 and not _lib.load().omgsr_igemm_out_mx6_ok(C.byref(a)):
        # the fp6 operand form comes out of the halo-tile kernel's dedicated instantiations only: anything else writes a stream tensor and the
        # cast kernel makes the operand (one more pass over the tensor; small maps and GEMM-shaped problems)
        return to_operand(conv2d(x, pw, stride=stride, pad=pad, upsample=upsample, act=act, residual=residual, gate=gate, out_dtype=OUT_STREAM,
                                 alpha=alpha, sample_rows=sample_rows, gn=gn), 4)
    keep = None
    if gn is not None:
        a.in_el = EL_16
        if _gn_fusable(a, gn):
            keep = _attach_gn(a, gn, x.shape[-1])
        else:
            x = gn.apply(x, pw.split)
            a.in_ = x.data_ptr()
    partial = _conv_gn(a, gn_groups, out_split, x.device)
    _igemm(a, x.device, "omgsr_igemm(conv2d)")
    del keep
    if partial is not None:
        _leave_gn(out, partial, gn_groups)
    return out


def _conv2d_mxfp8(a: IgemmArgs, xq: "Mxfp8", pw8: PackedWeight, out: torch.Tensor, gn_groups: int, deep: bool = False) -> torch.Tensor:
    """Launch omgsr_conv_mxfp8 (deep: omgsr_conv_mxfp8_deep) on an argument block filled for the 16-bit form of the same problem (geometry,
    epilogue, output)."""
    if xq.codes.shape[-1] != pw8.cin or a.Cout != pw8.cout:
        raise ValueError(f"conv2d_mxfp8: operand K {xq.codes.shape[-1]} / Cout {a.Cout} do not match the packed weight ({pw8.cin}, {pw8.cout})")
    a.in_, a.in_scale = xq.codes.data_ptr(), xq.scales.data_ptr()
    _fill_conv_mxfp8(a, pw8)
    partial = _conv_gn(a, gn_groups, 1, out.device)
    if deep:
        check(_lib.load().omgsr_conv_mxfp8_deep(C.byref(a), _stream()), "omgsr_conv_mxfp8_deep")
    else:
        check(_lib.load().omgsr_conv_mxfp8(C.byref(a), _stream()), "omgsr_conv_mxfp8")
    if partial is not None:
        _leave_gn(out, partial, gn_groups)
    return out


def _conv_mxfp8_args(a: IgemmArgs, xq: "Mxfp8", pw8: PackedWeight, act: int, residual, out_dtype: int, sample_rows: int) -> torch.Tensor:
    """Geometry, epilogue and output of one 3x3 stride-1 pad-1 MXFP8 conv problem (the operand and weight side: _conv2d_mxfp8(_multi));
    returns the output it allocated."""
    N, H, W, Cin = xq.codes.shape
    out = _out_tensor((N, H, W), pw8.cout, out_dtype, 1, xq.codes.device)
    if residual is not None and tuple(residual.shape) != (N, H, W, pw8.cout):
        raise ValueError(f"residual shape {tuple(residual.shape)} != output {(N, H, W, pw8.cout)}")
    _fill_out(a, out, 1, residual, pw8.cout)
    a.N, a.H, a.W, a.Ho, a.Wo, a.Cin, a.Cout = N, H, W, H, W, Cin, pw8.cout
    a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample = 3, 3, 1, 1, 1, 0
    a.act, a.batch, a.alpha, a.sample_rows = act, 1, 1.0, sample_rows or H * W
    return out


def conv2d_mxfp8(xq: "Mxfp8", pw8: PackedWeight, *, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None,
                 gate: Optional[torch.Tensor] = None, out_dtype: int = OUT_STREAM, gn_groups: int = 0, sample_rows: int = 0,
                 deep: bool = False) -> torch.Tensor:
    """3x3 stride-1 pad-1 conv of an MXFP8 operand xq [N,H,W,Cin] (quantize_mxfp8 / group_norm_apply split 5) with a pack_conv_weight_mxfp8
    weight -> [N,H,W,Cout8]. No other kernel stands behind it: a problem omgsr_conv_mxfp8_ok does not accept raises (OMGSR_E_SHAPE).
    deep: through omgsr_conv_mxfp8_deep (mxfp8_conv_deep_kernel: Cin % 64 == 0 up to 2048, a cin_multiple=64 pack) under the same rule."""
    if not isinstance(xq, Mxfp8) or not pw8.fp8 or pw8.w_cm is None:
        raise ValueError("conv2d_mxfp8: an Mxfp8 operand and a pack_conv_weight_mxfp8 weight")
    a = IgemmArgs()
    out = _conv_mxfp8_args(a, xq, pw8, act, residual, out_dtype, sample_rows)
    a.gate = _ptr(gate)
    return _conv2d_mxfp8(a, xq, pw8, out, gn_groups, deep=deep)


def _mxfp8_group_tiles(arr, n: int) -> int:
    """The group's total of spatial-form workgroup tiles (include/omgsr_hip.h, omgsr_conv_mxfp8_multi): what `group_tiles` holds when the
    library plans a member's GroupNorm partials; 0 in batch-invariant mode (every member on its own)."""
    if _BATCH_INVARIANT:
        return 0
    return sum(arr[i].N * ((arr[i].Wo + 31) // 32) * ((arr[i].Ho + 7) // 8) * ((arr[i].Cout + 127) // 128) for i in range(n))


def _fill_conv_mxfp8(a: IgemmArgs, pw8: PackedWeight) -> None:
    """The weight side of an argument block filled for the 16-bit form of the same problem -> the MXFP8 form's (the pointers do not enter
    omgsr_conv_mxfp8_multi_ok's per-problem rules, but the problems of a launch must agree in them)."""
    a.weight, a.weight_cm, a.w_scale, a.weight_ph = pw8.w_cm.data_ptr(), pw8.w_cm.data_ptr(), pw8.w_scale.data_ptr(), None
    a.Cout_pad, a.K_pad = pw8.w_cm.shape[2], 9 * pw8.cin
    a.bias = _ptr(pw8.bias) if a.bias is None else a.bias


def _conv2d_mxfp8_multi(arr, n: int, xqs, pw8: PackedWeight, outs, gn_groups: int):
    """Launch omgsr_conv_mxfp8_multi on argument blocks filled for the 16-bit form of the same problems (omgsr_conv_mxfp8_multi_ok said 1)."""
    total = _mxfp8_group_tiles(arr, n)
    partials = []
    for i in range(n):
        a, xq = arr[i], xqs[i]
        if xq.codes.shape[-1] != pw8.cin or a.Cout != pw8.cout:
            raise ValueError(f"conv2d_mxfp8_multi: operand K {xq.codes.shape[-1]} / Cout {a.Cout} do not match the packed weight ({pw8.cin}, {pw8.cout})")
        a.in_, a.in_scale = xq.codes.data_ptr(), xq.scales.data_ptr()
        _fill_conv_mxfp8(a, pw8)
        a.workspace, a.group_tiles = None, total
        partials.append(_conv_gn(a, gn_groups, 1, outs[i].device))
    check(_lib.load().omgsr_conv_mxfp8_multi(arr, n, _stream()), "omgsr_conv_mxfp8_multi")
    for out, partial in zip(outs, partials):
        if partial is not None:
            _leave_gn(out, partial, gn_groups)
    return outs


def conv2d_mxfp8_multi(xqs, pw8: PackedWeight, *, act: int = ACT_NONE, residuals=None, out_dtype: int = OUT_STREAM, gn_groups: int = 0):
    """conv2d_mxfp8 of several MXFP8 operands xqs[k] [N_k, H_k, W_k, Cin] with ONE pack_conv_weight_mxfp8 weight (the tile-shape groups of a
    tiled-VAE layer) through omgsr_conv_mxfp8_multi: one launch of mxfp8_conv_multi_kernel per 8 problems, served as a GROUP (the sum of the
    problems' tiles fills the chip where no problem alone does). No other kernel stands behind it: a group omgsr_conv_mxfp8_multi_ok does not
    accept raises (OMGSR_E_SHAPE). Same bytes as one conv2d_mxfp8 call per operand where those are served. Returns the list of outputs."""
    xqs = list(xqs)
    if not xqs or not all(isinstance(xq, Mxfp8) for xq in xqs) or not pw8.fp8 or pw8.w_cm is None:
        raise ValueError("conv2d_mxfp8_multi: Mxfp8 operands and a pack_conv_weight_mxfp8 weight")
    n = len(xqs)
    arr = (IgemmArgs * n)()
    outs = []
    for i, xq in enumerate(xqs):
        outs.append(_conv_mxfp8_args(arr[i], xq, pw8, act, None if residuals is None else residuals[i], out_dtype, 0))
    return _conv2d_mxfp8_multi(arr, n, xqs, pw8, outs, gn_groups)


def _fill_conv_mxfp8_up(a: IgemmArgs, xq: "Mxfp8", pw8: PackedWeight) -> None:
    """Operand and weight side of an argument block filled for the 16-bit form of the same up-sampling problem -> the MXFP8 form's."""
    if pw8.w_ph is None or not pw8.fp8 or xq.codes.shape[-1] != pw8.cin or a.Cout != pw8.cout:
        raise ValueError(f"conv2d_mxfp8_up: operand K {xq.codes.shape[-1]} / Cout {a.Cout} do not match a pack_conv_weight_mxfp8_up weight "
                         f"({pw8.cin}, {pw8.cout})")
    a.in_, a.in_scale = xq.codes.data_ptr(), xq.scales.data_ptr()
    a.weight, a.weight_ph, a.w_scale, a.weight_cm = pw8.w_ph.data_ptr(), pw8.w_ph.data_ptr(), pw8.w_scale.data_ptr(), None
    a.Cout_pad, a.K_pad = pw8.w_ph.shape[3], 9 * pw8.cin
    a.bias = _ptr(pw8.bias) if a.bias is None else a.bias


def _conv2d_mxfp8_up(a: IgemmArgs, xq: "Mxfp8", pw8: PackedWeight, out: torch.Tensor, gn_groups: int) -> torch.Tensor:
    """Launch omgsr_conv_mxfp8_up on an argument block filled for the 16-bit form of the same problem (geometry, epilogue, output)."""
    _fill_conv_mxfp8_up(a, xq, pw8)
    a.workspace, a.group_tiles = None, 0
    partial = _conv_gn(a, gn_groups, 1, out.device)
    check(_lib.load().omgsr_conv_mxfp8_up(C.byref(a), _stream()), "omgsr_conv_mxfp8_up")
    if partial is not None:
        _leave_gn(out, partial, gn_groups)
    return out


def _conv_mxfp8_up_args(a: IgemmArgs, xq: "Mxfp8", pw8: PackedWeight, act: int, out_dtype: int, sample_rows: int) -> torch.Tensor:
    """Geometry, epilogue and output of one nearest-2x + 3x3 stride-1 pad-1 MXFP8 conv problem; returns the output it allocated."""
    N, H, W, Cin = xq.codes.shape
    out = _out_tensor((N, 2 * H, 2 * W), pw8.cout, out_dtype, 1, xq.codes.device)
    _fill_out(a, out, 1, None, pw8.cout)
    a.N, a.H, a.W, a.Ho, a.Wo, a.Cin, a.Cout = N, H, W, 2 * H, 2 * W, Cin, pw8.cout
    a.R, a.S, a.stride, a.pad_top, a.pad_left, a.upsample = 3, 3, 1, 1, 1, 1
    a.act, a.batch, a.alpha, a.sample_rows = act, 1, 1.0, sample_rows or 4 * H * W
    a.overflow_flag = _ovf(xq.codes.device)
    return out


def conv2d_mxfp8_up(xq: "Mxfp8", pw8: PackedWeight, *, act: int = ACT_NONE, gate: Optional[torch.Tensor] = None, out_dtype: int = OUT_STREAM,
                    gn_groups: int = 0, sample_rows: int = 0) -> torch.Tensor:
    """conv3x3(nearest_up2(x)), stride 1, pad 1, of an MXFP8 operand xq [N,H,W,Cin] (quantize_mxfp8 of the low-resolution map) with a
    pack_conv_weight_mxfp8_up weight -> [N,2H,2W,Cout8]. No other kernel stands behind it: a problem omgsr_conv_mxfp8_up_ok does not accept
    raises (OMGSR_E_SHAPE)."""
    if not isinstance(xq, Mxfp8) or not pw8.fp8 or pw8.w_ph is None:
        raise ValueError("conv2d_mxfp8_up: an Mxfp8 operand and a pack_conv_weight_mxfp8_up weight")
    a = IgemmArgs()
    out = _conv_mxfp8_up_args(a, xq, pw8, act, out_dtype, sample_rows)
    a.gate = _ptr(gate)
    return _conv2d_mxfp8_up(a, xq, pw8, out, gn_groups)


def _conv2d_mxfp8_up_multi(arr, n: int, xqs, pw8: PackedWeight, outs, gn_groups: int):
    """Launch omgsr_conv_mxfp8_up_multi on argument blocks filled for the 16-bit form of the same problems (omgsr_conv_mxfp8_up_multi_ok said 1)."""
    # the group's total of phase-form workgroup tiles: what `group_tiles` holds when the library plans a member's GroupNorm partials
    total = 0 if _BATCH_INVARIANT else sum(4 * arr[i].N * ((arr[i].W + 31) // 32) * ((arr[i].H + 7) // 8) * ((arr[i].Cout + 127) // 128) for i in range(n))
    partials = []
    for i in range(n):
        _fill_conv_mxfp8_up(arr[i], xqs[i], pw8)
        arr[i].workspace, arr[i].group_tiles = None, total
        partials.append(_conv_gn(arr[i], gn_groups, 1, outs[i].device))
    check(_lib.load().omgsr_conv_mxfp8_up_multi(arr, n, _stream()), "omgsr_conv_mxfp8_up_multi")
    for out, partial in zip(outs, partials):
        if partial is not None:
            _leave_gn(out, partial, gn_groups)
    return outs


def conv2d_mxfp8_up_multi(xqs, pw8: PackedWeight, *, act: int = ACT_NONE, out_dtype: int = OUT_STREAM, gn_groups: int = 0):
    """conv2d_mxfp8_up of several MXFP8 operands xqs[k] [N_k, H_k, W_k, Cin] with ONE pack_conv_weight_mxfp8_up weight (the tile-shape groups of
    a tiled-VAE layer) through omgsr_conv_mxfp8_up_multi: one launch of mxfp8_conv_up_multi_kernel per 8 problems, served as a GROUP. No other
    kernel stands behind it: a group omgsr_conv_mxfp8_up_multi_ok does not accept raises (OMGSR_E_SHAPE). Same bytes as one conv2d_mxfp8_up call
    per operand where those are served. Returns the list of outputs."""
    xqs = list(xqs)
    if not xqs or not all(isinstance(xq, Mxfp8) for xq in xqs) or not pw8.fp8 or pw8.w_ph is None:
        raise ValueError("conv2d_mxfp8_up_multi: Mxfp8 operands and a pack_conv_weight_mxfp8_up weight")
    n = len(xqs)
    arr = (IgemmArgs * n)()
    outs = [_conv_mxfp8_up_args(arr[i], xq, pw8, act, out_dtype, 0) for i, xq in enumerate(xqs)]
    return _conv2d_mxfp8_up_multi(arr, n, xqs, pw8, outs, gn_groups)


def conv2d_multi(xs, pw: PackedWeight, *, stride: int = 1, pad: tuple[int, int, int, int] | int = 1, upsample: bool = False,
                 act: int = ACT_NONE, residuals=None, out_dtype: int = OUT_STREAM, gn_groups: int = 0, out_split: int = 1,
                 gn: Optional["GnSpec"] = None, fp8_pack=None, fp8_up_pack=None):
    """conv2d of several inputs with ONE weight (the tile-shape groups of a tiled-VAE layer: each x is its own dense [T*N, h, w, C]
    tensor) through omgsr_igemm_multi: the problems that take the halo-tile kernel run as one launch, with the kernel choice and the
    fused GroupNorm statistics planned for the group. Same results as a conv2d call per input. Returns the list of outputs.
    fp8_pack (see conv2d; needs gn and out_split 1): where omgsr_conv_mxfp8_multi_ok accepts the GROUP, the layer is one apply-to-MXFP8
    launch (group_norm_apply_mxfp8_multi) and one mxfp8_conv_multi_kernel launch; otherwise the WHOLE layer takes the 16-bit path below
    exactly as without it - one form per layer, tiles of one image never see different arithmetic.
    fp8_up_pack (see conv2d; upsample=True, no gn, no residuals): where omgsr_conv_mxfp8_up_multi_ok accepts the GROUP, the layer is one
    quantize_mxfp8 pass per tile-shape group and one mxfp8_conv_up_multi_kernel launch; otherwise the WHOLE layer takes the 16-bit path."""
    n = len(xs)
    if n == 1:
        return [conv2d(xs[0], pw, stride=stride, pad=pad, upsample=upsample, act=act, residual=None if residuals is None else residuals[0],
                       out_dtype=out_dtype, gn_groups=gn_groups, out_split=out_split, gn=gn, fp8_pack=fp8_pack, fp8_up_pack=fp8_up_pack)]
    lib = _lib.load()
    if gn is not None and not all(_gn_candidate(x, pw) for x in xs):
        xs, gn = [gn.apply(x, pw.split) for x in xs], None
    arr = (IgemmArgs * n)()
    keep, outs = [], []
    for i in range(n):
        x, out = _conv_args(arr[i], xs[i], pw, stride, pad, upsample, act, None if residuals is None else residuals[i], None, out_dtype, 1.0,
                            None, out_split, 0)
        keep.append(x)
        outs.append(out)
        if gn is not None:
            arr[i].in_el = EL_16
    if fp8_pack is not None and gn is not None and out_split == 1 and lib.omgsr_conv_mxfp8_multi_ok(arr, n):
        xqs = []
        for k in range(0, n, _lib.GN_MAX_GROUPS):
            xqs += group_norm_apply_mxfp8_multi(keep[k:k + _lib.GN_MAX_GROUPS], gn.mean, gn.rstd, gn.gamma, gn.beta, gn.groups, gn.act)
        return _conv2d_mxfp8_multi(arr, n, xqs, fp8_pack(), outs, gn_groups)
    if (fp8_up_pack is not None and upsample and gn is None and residuals is None and out_split == 1
            and lib.omgsr_conv_mxfp8_up_multi_ok(arr, n)):
        return _conv2d_mxfp8_up_multi(arr, n, [quantize_mxfp8(x) for x in keep], fp8_up_pack(), outs, gn_groups)
    check(lib.omgsr_igemm_multi_plan(arr, n), "omgsr_igemm_multi_plan")
    if out_split == 4 and not all(lib.omgsr_igemm_out_mx6_ok(C.byref(arr[i])) for i in range(n)):
        ys = conv2d_multi(keep, pw, stride=stride, pad=pad, upsample=upsample, act=act, residuals=residuals, out_dtype=OUT_STREAM, gn=gn)
        return [to_operand(y, 4) for y in ys]
    if gn is not None:
        # one form per layer: every tile-shape group runs the normalising patch producer, or the apply pass runs for all of them
        if all(_gn_fusable(arr[i], gn) for i in range(n)):
            for i in range(n):
                keep.append(_attach_gn(arr[i], gn, keep[i].shape[-1]))
        else:
            for i in range(n):
                y = gn.apply(keep[i], pw.split)
                keep.append(y)
                arr[i].in_ = y.data_ptr()
    partials = []
    for i in range(n):
        partials.append(_conv_gn(arr[i], gn_groups, out_split, outs[i].device))
        need = lib.omgsr_igemm_workspace_bytes(C.byref(arr[i]))
        if need > 0:
            ws = torch.empty(need // 4, device=outs[i].device, dtype=torch.float32)
            keep.append(ws)
            arr[i].workspace = ws.data_ptr()
    check(lib.omgsr_igemm_multi(arr, n, _stream()), "omgsr_igemm_multi(conv2d_multi)")
    for out, partial in zip(outs, partials):
        if partial is not None:
            _leave_gn(out, partial, gn_groups)
    return outs


def linear(x: torch.Tensor, pw: PackedWeight, *, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None,
           gate: Optional[torch.Tensor] = None, out_dtype: int = OUT_STREAM, alpha: float = 1.0, gn_groups: int = 0,
           out_split: int = 1, out_mxfp8=None):
    """x [..., K] -> [..., Cout]. gn_groups > 0 (x [B, ..., K]): the result feeds a GroupNorm over each x[b]; the GEMM
    then runs as B images of prod(...) rows so its epilogue can leave the per-image statistics (see conv2d).
    An fp8-packed weight (pack_linear_weight_mxfp8) takes an Mxfp8 operand, or quantises a bf16 `x` first. An fp8 GEGLU pack
    (pack_geglu_weight_mxfp8; the operand carries the pack's padded K) runs mxfp8_gemm_geglu_kernel: bias only, plain or out_mxfp8 output.
    out_mxfp8 (fp8-packed weight only; True or a dense Mxfp8 [..., Cout] to write into): the result act(x W^T + bias) as an Mxfp8 - the bytes
    of quantize_mxfp8(linear(..., out_dtype=OUT_BF16)), written by the GEMM's epilogue. No residual, gate, statistics or split."""
    if out_mxfp8 is not None and out_mxfp8 is not False:
        lead8 = (x.codes if isinstance(x, Mxfp8) else x).shape[:-1]
        dst8 = _out_mxfp8_dst("linear", out_mxfp8, pw, lead8, (x.codes if isinstance(x, Mxfp8) else x).device, residual=residual, gate=gate,
                              plain=not gn_groups and out_split == 1 and out_dtype in (OUT_STREAM, OUT_BF16) and alpha == 1.0)
    else:
        dst8 = None
    xq = _fp8_operand(x, pw, "linear")
    if xq is not None:
        if gn_groups or out_split != 1:
            raise ValueError("linear: an fp8 layer writes a plain output (no GroupNorm statistics, no split)")
        if pw.geglu:                                # pack_geglu_weight_mxfp8: the GEGLU form of the kernel, its own entry point
            if act != ACT_NONE or residual is not None or gate is not None or alpha != 1.0:
                raise ValueError("linear: an fp8 GEGLU projection goes with its bias only (no act, residual, gate or alpha)")
            return _linear_geglu_mxfp8(xq, pw, out_dtype, dst8)
        lead = xq.codes.shape[:-1]
        M = xq.codes.numel() // pw.cin
        a = IgemmArgs()
        _fill_mxfp8(a, xq.codes.data_ptr(), xq.scales.data_ptr(), pw)       # (not _fill_weight: this form never took the contraction-geometry fields)
        _fill_gemm(a, M)
        if dst8 is not None:
            scale = _fill_out_mxfp8(a, dst8.reshape(M, -1), 0, 0)
            a.act, a.alpha, a.sample_rows = act, 1.0, M
            _igemm_out_mxfp8(a, scale, "omgsr_igemm_out_mxfp8(linear)")
            return dst8
        out = _out_tensor(lead, pw.cout, out_dtype, 1, xq.codes.device)
        if residual is not None and residual.numel() != M * pw.cout:
            raise ValueError("linear: residual must be [..., Cout]")
        _fill_out(a, out, 1, residual, pw.cout)
        a.gate, a.act, a.alpha, a.sample_rows = _ptr(gate), act, alpha, M
        _igemm(a, out.device, "omgsr_igemm(linear, mxfp8)", workspace=False, keep=(xq, pw, out, residual, gate))
        return out
    lead = x.shape[:-1]
    M = 1
    for d in lead:
        M *= d
    B = lead[0] if (gn_groups > 0 and len(lead) >= 2) else 1
    x2 = x.reshape(B, 1, M // B, x.shape[-1])
    r2 = None if residual is None else residual.reshape(B, 1, M // B, pw.cout)
    y = conv2d(x2, pw, stride=1, pad=0, act=act, residual=r2, gate=gate, out_dtype=out_dtype, alpha=alpha, gn_groups=gn_groups,
               out_split=out_split, sample_rows=(M // lead[0]) if len(lead) >= 2 else M)
    out = y.reshape(*lead, y.shape[-1])
    carry_gn(y, out)
    return out


def carry_gn(src: torch.Tensor, view: torch.Tensor) -> torch.Tensor:
    """Views are new Python objects: hand the fused-statistics handle of `src` on to a view of the same storage."""
    h = getattr(src, "_omgsr_gn", None)
    if h is not None and view.data_ptr() == src.data_ptr() and view.shape[0] == src.shape[0]:
        view._omgsr_gn = h
    return view


def linear_into(x: torch.Tensor, pw: PackedWeight, out: torch.Tensor, row0: int, col0: int, *, act: int = ACT_NONE,
                residual: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None, out_split: int = 1,
                lo_col0: Optional[int] = None, sample_rows: int = 0, out_mxfp8: Optional[Mxfp8] = None) -> None:
    """out[row0:row0+M, col0:col0+Cout] = epilogue(x @ W^T): writes a projection straight into a slice of a
    larger 2-D operand buffer `out` [rows, ld] (joint text+image sequences, [attn | mlp] concat). out_split 2: the low
    halves of the two-term split go to columns lo_col0 ... lo_col0+Cout of the same rows (default col0 + Cout).
    An fp8-packed weight takes an Mxfp8 operand (or quantises `x`).
    out_mxfp8 (fp8-packed weight only; `out` is then None): a dense Mxfp8 [rows, Kw] - the result goes into its rows row0 ..., columns col0 ...
    (col0 % 128 == 0) with the bytes quantize_mxfp8 makes of the bf16 slice; bias and act only."""
    if out_mxfp8 is not None:
        if out is not None:
            raise ValueError("linear_into: either `out` or out_mxfp8")
        if not isinstance(out_mxfp8, Mxfp8) or out_mxfp8.codes.dim() != 2:
            raise TypeError("linear_into: out_mxfp8 is a dense Mxfp8 [rows, Kw]")
        _out_mxfp8_dst("linear_into", out_mxfp8, pw, out_mxfp8.codes.shape[:-1], None, col0, residual=residual, gate=gate, plain=out_split == 1)
        xq = _fp8_operand(x, pw, "linear_into")
        M = xq.codes.numel() // pw.cin
        if row0 < 0 or row0 + M > out_mxfp8.codes.shape[0]:
            raise ValueError("linear_into: slice does not fit")
        a = IgemmArgs()
        _fill_weight(a, pw, xq.codes.data_ptr(), xq.scales.data_ptr())
        _fill_gemm(a, M)
        scale = _fill_out_mxfp8(a, out_mxfp8, row0, col0)
        a.act, a.alpha, a.sample_rows = act, 1.0, sample_rows or M
        _igemm_out_mxfp8(a, scale, "omgsr_igemm_out_mxfp8(linear_into)")
        return
    xq = _fp8_operand(x, pw, "linear_into")
    if xq is not None:
        if out_split != 1:
            raise ValueError("linear_into: an fp8 layer writes a plain output")
        x = xq.codes
    elif x.dtype == torch.float32:
        x = to_operand(x, pw.split)
    if xq is None:
        _req(x, act_dtype(), "x")
    _req(out, act_dtype(), "out")
    # out [rows, ld], or [B, rows, ld] with x [B, M, K]: image b's M rows land at rows row0 .. row0+M of out[b] (grid.z = B)
    Bz = out.shape[0] if out.dim() == 3 else 1
    M, K = x.numel() // x.shape[-1] // Bz, x.shape[-1]
    ld, nrows = out.shape[-1], out.shape[-2]
    if K != pw.row_channels or out.dim() not in (2, 3) or row0 + M > nrows or col0 + pw.cout > ld or (col0 & 7):
        raise ValueError("linear_into: slice does not fit")
    if residual is not None and (Bz != 1 or residual.numel() != M * pw.cout):
        raise ValueError("linear_into: residual must be a dense [M, Cout] (unbatched call)")
    lo_off = 0
    if out_split == 2:
        lo_off = (lo_col0 - col0) if lo_col0 is not None else pw.cout
        if lo_off < pw.cout or col0 + lo_off + pw.cout > ld:
            raise ValueError("linear_into: the low halves do not fit the row")
    a = IgemmArgs()
    _fill_weight(a, pw, x.data_ptr(), None if xq is None else xq.scales.data_ptr())
    _fill_gemm(a, M, Bz, M * K, 0, nrows * ld)
    _fill_out_slice(a, out, row0 * ld + col0, ld=ld, lo_off=lo_off)
    if residual is not None:
        a.residual, a.res_el = residual.data_ptr(), _el(residual, "residual")
    a.gate, a.act, a.alpha = _ptr(gate), act, 1.0
    a.sample_rows = sample_rows or M              # rows of ONE image when the caller flattened a batch into M (batch-invariant dispatch)
    _igemm(a, x.device, "omgsr_igemm(linear_into)", z_batched_api=True, keep=(x, xq, pw, out, residual, gate))


def linear_rows(x_buf: torch.Tensor, row0: int, rows: int, pw: PackedWeight, *, act: int = ACT_NONE, residual: Optional[torch.Tensor] = None,
                gate: Optional[torch.Tensor] = None, out_dtype: int = OUT_STREAM) -> torch.Tensor:
    """out[b] = epilogue(x_buf[b, row0:row0+rows] @ W^T) for an operand buffer x_buf [B, L, K]: a projection of a row range of
    every image's joint sequence (to_out / to_add_out after joint attention) without gathering the rows first. Returns a dense
    [B, rows, Cout] stream tensor; residual: dense [B, rows, Cout]. An fp8-packed weight takes an Mxfp8 x_buf (or quantises it)."""
    xq = _fp8_operand(x_buf, pw, "linear_rows")
    if xq is not None:
        x_buf = xq.codes
    else:
        _req(x_buf, act_dtype(), "x_buf")
    B, L, K = x_buf.shape
    if K != pw.row_channels or row0 < 0 or row0 + rows > L:
        raise ValueError("linear_rows: row range / channels do not fit")
    out = _out_tensor((B, rows), pw.cout, out_dtype, 1, x_buf.device)
    if residual is not None and tuple(residual.shape) != (B, rows, pw.cout):
        raise ValueError("linear_rows: residual must be [B, rows, Cout]")
    a = IgemmArgs()
    if xq is None:
        _fill_weight(a, pw, x_buf.data_ptr() + 2 * row0 * K)
    else:                                         # one byte per code, one scale per 32 of them
        _fill_weight(a, pw, x_buf.data_ptr() + row0 * K, xq.scales.data_ptr() + row0 * (K // 32))
    _fill_gemm(a, rows, B, L * K, 0, rows * pw.cout)
    _fill_out(a, out, 1, residual, pw.cout)
    a.gate, a.act, a.alpha, a.sample_rows = _ptr(gate), act, 1.0, rows
    _igemm(a, x_buf.device, "omgsr_igemm(linear_rows)", workspace=False, keep=(x_buf, xq, pw, out, residual, gate))
    return out


def linear_t_into(x: torch.Tensor, pw: PackedWeight, out_t: torch.Tensor, key0: int) -> None:
    """out_t[n, key0 + l] = (x W^T + b)[l, n] for x [L, K]: transposed projection into a slice of a joint
    V^T buffer [Cout, ld]. An fp8-packed weight takes an Mxfp8 operand (or quantises `x`)."""
    xq = _fp8_operand(x, pw, "linear_t_into")
    if xq is not None:
        x = xq.codes
    elif x.dtype == torch.float32:
        x = to_operand(x, pw.split)
    if xq is None:
        _req(x, act_dtype(), "x")
    _req(out_t, act_dtype(), "out_t")
    # out_t [Cout, ld], or [B, Cout, ld] with x [B, L, K] (grid.z = B)
    Bz = out_t.shape[0] if out_t.dim() == 3 else 1
    L, K = x.numel() // x.shape[-1] // Bz, x.shape[-1]
    if out_t.dim() not in (2, 3) or out_t.shape[-2] != pw.cout or key0 + L > out_t.shape[-1] or K != pw.row_channels:
        raise ValueError("linear_t_into: slice does not fit")
    a = IgemmArgs()
    _fill_weight(a, pw, x.data_ptr(), None if xq is None else xq.scales.data_ptr())
    _fill_gemm(a, L, Bz, L * K, 0, pw.cout * out_t.shape[-1])
    _fill_out_slice(a, out_t, key0, t_rows=L)
    a.alpha, a.sample_rows = 1.0, L
    _igemm(a, x.device, "omgsr_igemm(linear_t_into)", workspace=False, keep=(x, xq, pw, out_t))


def linear_t(x: torch.Tensor, pw: PackedWeight, rows_per_batch: int, ld: Optional[int] = None) -> torch.Tensor:
    """Transposed-output projection: x [B, L, K] -> out [B, Cout, ld] with out[b, n, l] = (x W^T + bias)[b, l, n].
    This is how V reaches omgsr_attention (key index contiguous). Columns l >= L are zero."""
    if x.dtype == torch.float32:
        x = to_operand(x, pw.split)
    _req(x, act_dtype(), "x")
    B, L, K = x.shape
    if L != rows_per_batch or K != pw.row_channels:
        raise ValueError("linear_t: shape mismatch")
    ld = ld or _round_up(L, 8)
    out = torch.zeros((B, pw.cout, ld), device=x.device, dtype=act_dtype()) if ld != L else \
        torch.empty((B, pw.cout, ld), device=x.device, dtype=act_dtype())
    a = IgemmArgs()
    _fill_weight(a, pw, x.data_ptr())
    _fill_gemm(a, B * L)                          # one problem of B * L rows: the transposed epilogue finds the image from t_rows
    _fill_out_slice(a, out, 0, t_rows=L)
    a.alpha, a.sample_rows = 1.0, L
    _igemm(a, x.device, "omgsr_igemm(linear_t)", workspace=False)
    return out


def transpose_split(x: torch.Tensor, ld: Optional[int] = None) -> torch.Tensor:
    """x fp32 [B, L, C] (a projection's stream output) -> [B, 2C, ld] in the operand type: rows [0, C) = round(x)^T, rows [C, 2C) = the low halves.
    The attention's V^T operand as a two-term split (range-fallback tier, ops.attn_split). Columns >= L are zero."""
    _req(x, torch.float32, "x")
    B, L, Cc = x.shape
    ld = ld or _round_up(L, 8)
    out = (torch.zeros if ld != L else torch.empty)((B, 2 * Cc, ld), device=x.device, dtype=act_dtype())
    check(_lib.load().omgsr_transpose_split(x.data_ptr(), out.data_ptr(), B, L, Cc, ld, _stream()), "omgsr_transpose_split")
    return out


def bmm_nt(a_mat: torch.Tensor, b_mat: torch.Tensor, *, alpha: float = 1.0, out_dtype: int = OUT_BF16, out_split: int = 1,
           both_split: bool = False) -> torch.Tensor:
    """out[b] = alpha * a[b] @ b[b]^T ; a [B, M, K], b [B, Npad, K] operands with Npad % 128 == 0, K % 32 == 0.
    Returns [B, M, Npad] (OUT_F32: fp32; OUT_BF16: a 16-bit operand, [B, M, 2*Npad] as a two-term split when out_split 2).
    (d=512 VAE attention scores / PV product.)
    both_split: BOTH factors carry two-term splits - a = [a_hi | a_lo] ([B, M, 2C], what a GEMM epilogue writes with out_split 2) and
    b = [b_hi | b_hi | b_lo] ([B, Npad, 3C], split_rows_hhl): the contraction runs the three segments a_hi b_hi + a_lo b_hi + a_hi b_lo,
    the third one wrapping back to a_hi (omgsr_igemm_args.in_ld) exactly like a Linear with operand and weight splits."""
    _req(a_mat, act_dtype(), "a")
    _req(b_mat, act_dtype(), "b")
    B, M, K = a_mat.shape
    Bb, Np, Kb = b_mat.shape
    if both_split:
        if Bb != B or K % 64 or Kb * 2 != K * 3:
            raise ValueError(f"bmm_nt(both_split): incompatible shapes {tuple(a_mat.shape)} x {tuple(b_mat.shape)}")
    elif Bb != B or Kb != K or K % 32:
        raise ValueError(f"bmm_nt: incompatible shapes {tuple(a_mat.shape)} x {tuple(b_mat.shape)}")
    if Np % 128:    # reduced test configs only (the real VAE has 512 channels / 128-padded key counts)
        bp = torch.zeros((B, _round_up(Np, 128), Kb), device=b_mat.device, dtype=act_dtype())
        bp[:, :Np] = b_mat
        full = bmm_nt(a_mat, bp, alpha=alpha, out_dtype=out_dtype, out_split=out_split, both_split=both_split)
        Npp = bp.shape[1]
        if out_split == 2 and out_dtype == OUT_BF16:
            return torch.cat([full[:, :, :Np], full[:, :, Npp:Npp + Np]], dim=-1).contiguous()
        return full[:, :, :Np].contiguous()
    split = out_split if out_dtype == OUT_BF16 else 1
    out = torch.empty((B, M, Np * split), device=a_mat.device, dtype=act_dtype() if out_dtype == OUT_BF16 else torch.float32)
    a = IgemmArgs()
    a.in_, a.weight = a_mat.data_ptr(), b_mat.data_ptr()          # the second factor stands where a packed weight would: no padding, no bias
    a.Cin, a.Cout, a.Cout_pad, a.K_pad = Kb, Np, Np, Kb
    if both_split:
        a.in_ld, a.in_split, a.w_split = K, 1, 1
        a.overflow_flag = _ovf(a_mat.device)
    _fill_gemm(a, M, B, M * K, Np * Kb, M * Np * split)
    _fill_out(a, out, 2 if split == 2 else 1, None, Np)
    a.out_dtype, a.alpha = out_dtype, alpha                       # (out_dtype as the caller gave it, not as _fill_out reads it off the tensor)
    _igemm(a, a_mat.device, "omgsr_igemm(bmm_nt)", workspace=False)
    return out


def split_rows_hhl(x: torch.Tensor, pad_rows: int = 0) -> torch.Tensor:
    """[B, L, 2C] two-term split rows [hi | lo] -> [B, max(L, pad_rows), 3C] rows [hi | hi | lo] (zero rows past L): the second factor of
    bmm_nt(both_split=True). Plain device copies (a few MB: the keys of the VAE's one-head attention)."""
    B, L, C2 = x.shape
    Cc = C2 // 2
    out = (torch.zeros if pad_rows > L else torch.empty)((B, max(L, pad_rows), 3 * Cc), device=x.device, dtype=x.dtype)
    out[:, :L, :Cc] = x[:, :, :Cc]
    out[:, :L, Cc:2 * Cc] = x[:, :, :Cc]
    out[:, :L, 2 * Cc:] = x[:, :, Cc:]
    return out


# --------------------------------------------------------------------------------------------
# K4: GroupNorm

def _fused_gn(x: torch.Tensor, groups: int, N: int):
    h = _gn_handle(x, N)
    return h[0] if h is not None and h[1] == groups else None


def _gn_stats_out(N: int, groups: int, device):
    """Uninitialised (mean, rstd, var) [N, G] f32."""
    mean = torch.empty((N, groups), device=device, dtype=torch.float32)
    return mean, torch.empty_like(mean), torch.empty_like(mean)


def group_norm_stats(x: torch.Tensor, groups: int, eps: float):
    """x [N, ..., C] stream tensor -> (mean [N,G], rstd [N,G], var [N,G]) f32 (biased variance)."""
    xel = _el(x, "x")
    N, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (N * Cc)
    lib = _lib.load()
    mean, rstd, var = _gn_stats_out(N, groups, x.device)
    fused = _fused_gn(x, groups, N)
    if fused is not None:
        # the producing conv already reduced this tensor (omgsr_igemm gn_partial): fold its partials only
        check(lib.omgsr_groupnorm_finalize(fused.data_ptr(), mean.data_ptr(), rstd.data_ptr(), var.data_ptr(), N,
                                           fused.shape[1], groups, fused.shape[2], float(HW) * (Cc // groups), eps, _stream()),
              "omgsr_groupnorm_finalize")
        return mean, rstd, var
    nchunk = lib.omgsr_groupnorm_nchunk(HW)
    partial = torch.empty((N, nchunk, groups, 2), device=x.device, dtype=torch.float32)
    check(lib.omgsr_groupnorm_stats(x.data_ptr(), partial.data_ptr(), mean.data_ptr(), rstd.data_ptr(), var.data_ptr(),
                                    N, HW, Cc, groups, eps, xel, _stream()), "omgsr_groupnorm_stats")
    return mean, rstd, var


def group_norm_partial(x: torch.Tensor, groups: int) -> torch.Tensor:
    """(sum, sum of squares) partials [N, nslot, G, 2] of x: the producing conv's fused ones when it left them
    (conv2d gn_groups), else one read pass over x."""
    xel = _el(x, "x")
    N, Cc = x.shape[0], x.shape[-1]
    fused = _fused_gn(x, groups, N)
    if fused is not None:
        return fused
    HW = x.numel() // (N * Cc)
    lib = _lib.load()
    partial = torch.empty((N, lib.omgsr_groupnorm_nchunk(HW), groups, 2), device=x.device, dtype=torch.float32)
    check(lib.omgsr_groupnorm_partial(x.data_ptr(), partial.data_ptr(), N, HW, Cc, groups, xel, _stream()), "omgsr_groupnorm_partial")
    return partial


def group_norm_stats_merged(tensors, tiles, N: int, groups: int, eps: float):
    """Tiled-VAE GroupNorm statistics in ONE launch: tensors[k] is [tiles[k]*N, h_k, w_k, C] (tile-major); returns
    per-image (mean, rstd, var) [N, G] merged with pixel-count weights (the reference's GroupNormParam.summary)."""
    if len(tensors) > _lib.GN_MAX_GROUPS:
        raise ValueError(f"at most {_lib.GN_MAX_GROUPS} tile shape groups")
    a = _lib.GnMergeArgs()
    keep = []
    tot = float(sum(t.shape[1] * t.shape[2] * tiles[k] for k, t in enumerate(tensors)))
    for k, t in enumerate(tensors):
        part = group_norm_partial(t, groups)
        keep.append(part)
        a.partial[k] = part.data_ptr()
        a.nslot[k] = part.shape[1]
        a.entries[k] = part.shape[2]
        a.tiles[k] = tiles[k]
        a.count[k] = float(t.shape[1] * t.shape[2] * (t.shape[3] // groups))
        a.weight[k] = t.shape[1] * t.shape[2] / tot
    a.ngroups = len(tensors)
    mean, rstd, var = _gn_stats_out(N, groups, tensors[0].device)
    check(_lib.load().omgsr_groupnorm_finalize_merged(C.byref(a), mean.data_ptr(), rstd.data_ptr(), var.data_ptr(), N, groups,
                                                      eps, _stream()), "omgsr_groupnorm_finalize_merged")
    return mean, rstd, var


def _operand_like(x: torch.Tensor, split: int) -> torch.Tensor:
    if split not in (1, 2, 3, 4):
        raise ValueError("split must be 1, 2, 3 (MX) or 4 (MX6)")
    return torch.empty((*x.shape[:-1], x.shape[-1] * min(split, 2)), device=x.device, dtype=_ACT)


def _cast_twin(x: torch.Tensor, xel: int, also_cast: int):
    """The optional second output of the GroupNorm apply kernels: x itself as an operand (a fp32 stream tensor only; a 16-bit
    stream tensor IS its own operand)."""
    if not also_cast:
        return None
    if xel != EL_F32:
        if also_cast != 1:
            raise ValueError("a 16-bit tensor cannot be split")
        return x
    return _operand_like(x, also_cast)


def group_norm_apply_shared(x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int,
                            act: int = ACT_NONE, split: int = 1, also_cast: int = 0):
    """x [T*N, ..., C] tile-major; mean / rstd [N, G]: row r is normalised with the statistics of image r % N.
    also_cast 1 | 2 | 3: returns (y, x as a plain / split / mixed-precision operand) - see group_norm_apply."""
    return _group_norm_apply(x, mean, rstd, gamma, beta, groups, act, False, split, also_cast, shared=True)


def _gn_apply_table(xs, ys, y2s, Cc: int):
    """The omgsr_gn_apply_group table of a multi launch: tensor k reads xs[k] and writes ys[k] (and y2s[k] unless None)."""
    desc = (_lib.GnApplyGroup * len(xs))()
    for k, x in enumerate(xs):
        desc[k].x, desc[k].y, desc[k].y2 = x.data_ptr(), ys[k].data_ptr(), _ptr(y2s[k])
        desc[k].rows, desc[k].HW = x.shape[0], x.numel() // (x.shape[0] * Cc)
    return desc


def group_norm_apply_multi(xs, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int, act: int = ACT_NONE, split: int = 1,
                           also_cast: int = 0):
    """group_norm_apply_shared over the tile-shape groups of one tiled-VAE layer in ONE launch: xs[k] is [T_k*N, h_k, w_k, C]
    (tile-major), all of one channel count and element kind. Returns the list of y (of (y, y2) pairs with also_cast); the bytes are
    those of one group_norm_apply_shared call per tensor."""
    if not 0 < len(xs) <= _lib.GN_MAX_GROUPS:
        raise ValueError(f"1 ... {_lib.GN_MAX_GROUPS} tile shape groups")
    xel = _el(xs[0], "x")
    Cc = xs[0].shape[-1]
    if any(_el(x, "x") != xel or x.shape[-1] != Cc for x in xs):
        raise ValueError("group_norm_apply_multi: one channel count and element kind per launch")
    ys = [_operand_like(x, split) for x in xs]
    y2s = [_cast_twin(x, xel, also_cast) for x in xs]
    fused = bool(also_cast) and xel == EL_F32
    desc = _gn_apply_table(xs, ys, y2s if fused else [None] * len(xs), Cc)
    check(_lib.load().omgsr_groupnorm_apply_multi(desc, len(xs), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta), Cc, groups, act,
                                                  mean.shape[0], xel, _el_of_split(split), _el_of_split(also_cast) if also_cast else EL_16,
                                                  _ovf(xs[0].device) if fused else None, _stream()),
          "omgsr_groupnorm_apply_multi")
    return list(zip(ys, y2s)) if also_cast else ys


def group_norm_apply(x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma: Optional[torch.Tensor],
                     beta: Optional[torch.Tensor], groups: int, act: int = ACT_NONE, inplace: bool = False, split: int = 1,
                     also_cast: int = 0):
    """Stream tensor -> normalised (+SiLU) MFMA operand [..., split*C]. also_cast 1 | 2 | 3: additionally returns x itself as a
    plain / two-term split / mixed-precision operand (the input of a ResnetBlock's 1x1 shortcut conv), written by the same pass.
    split 5: the result as an Mxfp8 (group_norm_apply_mxfp8; no also_cast / inplace)."""
    if split == 5:
        if also_cast or inplace:
            raise ValueError("group_norm_apply: split 5 (MXFP8) has no second output and cannot run in place")
        return group_norm_apply_mxfp8(x, mean, rstd, gamma, beta, groups, act)
    return _group_norm_apply(x, mean, rstd, gamma, beta, groups, act, inplace, split, also_cast, shared=False)


def _group_norm_apply(x, mean, rstd, gamma, beta, groups: int, act: int, inplace: bool, split: int, also_cast: int, shared: bool):
    """The body of group_norm_apply (row r uses statistics row r: omgsr_groupnorm_apply) and group_norm_apply_shared (row r uses statistics
    row r % mean.shape[0]: omgsr_groupnorm_apply_shared, which takes that count behind `act`)."""
    xel = _el(x, "x")
    rows, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (rows * Cc)
    y = x if (inplace and xel == EL_16 and split == 1 and not also_cast) else _operand_like(x, split)
    y2 = _cast_twin(x, xel, also_cast)
    fused = y2 is not None and y2 is not x
    lib = _lib.load()
    fn, what, nimg = (lib.omgsr_groupnorm_apply_shared, "omgsr_groupnorm_apply_shared", (mean.shape[0],)) if shared else \
        (lib.omgsr_groupnorm_apply, "omgsr_groupnorm_apply", ())
    check(fn(x.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta), rows, HW, Cc, groups, act, *nimg, xel,
             _el_of_split(split), y2.data_ptr() if fused else None, _el_of_split(also_cast) if also_cast else EL_16,
             _ovf(x.device) if fused else None, _stream()), what)
    return (y, y2) if also_cast else y


def group_norm_apply_mxfp8(x: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int, act: int = ACT_NONE,
                           c64: bool = False) -> "Mxfp8":
    """Stream tensor x [rows, ..., C] (bf16 or fp32, read only) -> act(GroupNorm(x)) as an Mxfp8 [rows, ..., C]: the fp32 result of the apply
    arithmetic quantised by quantize_mxfp8's rule in the same pass (omgsr_groupnorm_apply_mxfp8). mean / rstd [N, G]: row r uses the
    statistics of image r % N. C % 128 == 0, bf16 compute type. c64: C % 64 == 0 through omgsr_groupnorm_apply_mxfp8_c64 (the same kernel; the
    operand of the deep conv form)."""
    xel = _el(x, "x")
    rows, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (rows * Cc)
    if Cc % (64 if c64 else 128):
        raise ValueError(f"group_norm_apply_mxfp8: C = {Cc} is not a multiple of {64 if c64 else 128}")
    out = _mxfp8_like(x)
    lib = _lib.load()
    fn, what = (lib.omgsr_groupnorm_apply_mxfp8_c64, "omgsr_groupnorm_apply_mxfp8_c64") if c64 else (lib.omgsr_groupnorm_apply_mxfp8, "omgsr_groupnorm_apply_mxfp8")
    check(fn(x.data_ptr(), out.codes.data_ptr(), out.scales.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta), rows, HW, Cc, groups,
             act, mean.shape[0], xel, _stream()), what)
    return out


def group_norm_apply_mxfp8_multi(xs, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int, act: int = ACT_NONE):
    """group_norm_apply_mxfp8 over the tile-shape groups of one tiled-VAE layer in ONE launch (omgsr_groupnorm_apply_mxfp8_multi): xs[k] is
    [T_k*N, h_k, w_k, C] (tile-major), all of one channel count and element kind. Returns the list of Mxfp8; the bytes are those of one
    group_norm_apply_mxfp8 call per tensor."""
    if not 0 < len(xs) <= _lib.GN_MAX_GROUPS:
        raise ValueError(f"1 ... {_lib.GN_MAX_GROUPS} tile shape groups")
    xel = _el(xs[0], "x")
    Cc = xs[0].shape[-1]
    if any(_el(x, "x") != xel or x.shape[-1] != Cc for x in xs):
        raise ValueError("group_norm_apply_mxfp8_multi: one channel count and element kind per launch")
    if Cc % 128:
        raise ValueError(f"group_norm_apply_mxfp8_multi: C = {Cc} is not a multiple of 128")
    outs = [_mxfp8_like(x) for x in xs]
    desc = _gn_apply_table(xs, [o.codes for o in outs], [o.scales for o in outs], Cc)
    check(_lib.load().omgsr_groupnorm_apply_mxfp8_multi(desc, len(xs), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta), Cc, groups, act,
                                                        mean.shape[0], xel, _stream()), "omgsr_groupnorm_apply_mxfp8_multi")
    return outs


def group_norm(x: torch.Tensor, gamma, beta, groups: int, eps: float, act: int = ACT_NONE, split: int = 1, also_cast: int = 0):
    mean, rstd, _ = group_norm_stats(x, groups, eps)
    return group_norm_apply(x, mean, rstd, gamma, beta, groups, act, split=split, also_cast=also_cast)


def _fused_gn_channels(x: torch.Tensor, N: int):
    """The producer's partials when it left them PER CHANNEL ([N, nslot, C, 2]: they fold into any group boundary, whatever group count
    the producer was told), else None. _fused_gn's validity rules otherwise."""
    h = _gn_handle(x, N)
    return h[0] if h is not None and h[0].shape[2] == x.shape[-1] else None


def group_norm_pair_stats(a: torch.Tensor, b: torch.Tensor, groups: int, eps: float):
    """(mean, rstd, var) [N, G] of the channel concatenation [a | b] from the per-channel partials both producers left, or None when
    the pair does not qualify (see group_norm_pair)."""
    N, Ca, Cb = a.shape[0], a.shape[-1], b.shape[-1]
    if not (a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape[:-1] == b.shape[:-1] and Ca % 8 == 0 and Cb % 8 == 0
            and (Ca + Cb) % groups == 0 and a.is_contiguous() and b.is_contiguous()):
        return None
    pa, pb = _fused_gn_channels(a, N), _fused_gn_channels(b, N)
    if pa is None or pb is None:
        return None
    HW = a.numel() // (N * Ca)
    mean, rstd, var = _gn_stats_out(N, groups, a.device)
    check(_lib.load().omgsr_groupnorm_finalize2(pa.data_ptr(), pa.shape[1], Ca, pb.data_ptr(), pb.shape[1], Cb, mean.data_ptr(), rstd.data_ptr(),
                                                var.data_ptr(), N, groups, float(HW) * ((Ca + Cb) // groups), eps, _stream()),
          "omgsr_groupnorm_finalize2")
    return mean, rstd, var


def group_norm_apply_pair(a: torch.Tensor, b: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int, act: int = ACT_NONE,
                          split: int = 1, also_cast: int = 0):
    """group_norm_apply of the channel concatenation [a | b] of two fp32 stream tensors, read from the two tensors: the same bytes."""
    _req(a, torch.float32, "a"); _req(b, torch.float32, "b")
    N, Ca, Cb = a.shape[0], a.shape[-1], b.shape[-1]
    if a.shape[:-1] != b.shape[:-1]:
        raise ValueError("group_norm_apply_pair: a and b differ in more than the channel count")
    HW = a.numel() // (N * Ca)
    y = torch.empty((*a.shape[:-1], (Ca + Cb) * min(split, 2)), device=a.device, dtype=_ACT)
    y2 = torch.empty((*a.shape[:-1], (Ca + Cb) * min(also_cast, 2)), device=a.device, dtype=_ACT) if also_cast else None
    check(_lib.load().omgsr_groupnorm_apply2(a.data_ptr(), b.data_ptr(), Ca, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _ptr(gamma), _ptr(beta),
                                             N, HW, Ca + Cb, groups, act, _el_of_split(split), _ptr(y2),
                                             _el_of_split(also_cast) if also_cast else EL_16, _ovf(a.device) if also_cast else None, _stream()),
          "omgsr_groupnorm_apply2")
    return (y, y2) if also_cast else y


def group_norm_pair(a: torch.Tensor, b: torch.Tensor, gamma, beta, groups: int, eps: float, act: int = ACT_NONE, split: int = 1, also_cast: int = 0):
    """group_norm(concat_channels(a, b), ...) - the first GroupNorm of a UNet up-path resnet (decoder tensor | skip tensor). When both are
    fp32 stream tensors whose producers left per-channel statistics, neither the concatenated tensor nor a statistics read pass over it
    exists: the statistics fold from the two sets of partials and the apply pass reads the two tensors. Anything else - a 16-bit tier, a
    producer that left nothing (a split-K conv, as on the 8x8 maps) or per-GROUP partials (reduced-size models with group sizes 2 / 4 / 8:
    a group of the concatenation cannot be regrouped from those) - runs concat_channels + group_norm as before."""
    st = group_norm_pair_stats(a, b, groups, eps)
    if st is None:
        return group_norm(concat_channels(a, b), gamma, beta, groups, eps, act, split=split, also_cast=also_cast)
    return group_norm_apply_pair(a, b, st[0], st[1], gamma, beta, groups, act, split=split, also_cast=also_cast)


# --------------------------------------------------------------------------------------------
# The thin 3x3 convolutions at the edges of the networks as fp32 streaming kernels (csrc/conv_edge.hip): the accurate tiers only
# (fp32 stream tensors); the 16-bit tiers never come here. New wrappers the model code calls - conv2d / conv2d_multi are unchanged.

@dataclass
class EdgeWeight:
    """A conv_out's fp32 weight as omgsr_conv_out_gn reads it: w [Cin / 4][3][3][4][CP] (CP = 4 | 8 columns), bias [CP]."""
    w: torch.Tensor
    bias: torch.Tensor
    cin: int
    cout: int


def edge_conv_out_ok(stream: torch.dtype, weight_shape, stride: int, padding: int, groups: int) -> bool:
    """The routing predicate of the call sites (VAEHook._run, Encoder / Decoder.nhwc, the UNet): a GroupNorm + SiLU + 3x3 stride-1 pad-1 conv
    with at most 8 output channels on an fp32 stream tensor runs as omgsr_conv_out_gn; everything else (every 16-bit tier) as before."""
    cout, cin, kh, kw = (int(v) for v in weight_shape)
    return (stream == torch.float32 and (kh, kw) == (3, 3) and stride == 1 and padding == 1 and cout <= 8
            and cin % 32 == 0 and cin <= 1024 and groups > 0 and cin % groups == 0)


def pack_edge_out_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None) -> EdgeWeight:
    """[Cout, Cin, 3, 3] (any float dtype; used as fp32, unsplit and unrounded) -> EdgeWeight."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if tuple(weight.shape[2:]) != (3, 3) or cout > 8 or cin % 4:
        raise ValueError("pack_edge_out_weight: a 3x3 kernel, Cout <= 8, Cin % 4 == 0")
    cp = 4 if cout <= 4 else 8
    dev = device or weight.device
    w = torch.zeros((cin // 4, 3, 3, 4, cp), device=dev, dtype=torch.float32)
    w[..., :cout] = weight.detach().to(device=dev, dtype=torch.float32).reshape(cout, cin // 4, 4, 3, 3).permute(1, 3, 4, 2, 0)
    b = torch.zeros((cp,), device=dev, dtype=torch.float32)
    if bias is not None:
        b[:cout] = bias.detach().to(device=dev, dtype=torch.float32)
    return EdgeWeight(w.contiguous(), b, cin, cout)


def conv_out_gn_multi(xs, ew: EdgeWeight, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                      one_launch: bool = True):
    """conv3x3(silu(GroupNorm(x))) + bias of every xs[k] ([rows_k, h_k, w_k, Cin] fp32 stream tensors: the tile-shape groups of a tiled-VAE
    layer) with the statistics mean / rstd [nimg, G] (row r of a tensor uses image r % nimg) -> list of [rows_k, h_k, w_k, 8] fp32, channels
    beyond Cout exact zeros. One launch over a prefix table of the groups, or (one_launch False) one launch per tensor: the same bytes."""
    if not 0 < len(xs) <= _lib.GN_MAX_GROUPS:
        raise ValueError(f"1 ... {_lib.GN_MAX_GROUPS} tile shape groups")
    for x in xs:
        if _req(x, torch.float32, "x").dim() != 4 or x.shape[-1] != ew.cin:
            raise ValueError(f"conv_out_gn: x must be [rows, H, W, {ew.cin}]")
    outs = [torch.empty((*x.shape[:-1], 8), device=x.device, dtype=torch.float32) for x in xs]
    desc = (_lib.EdgeGroup * len(xs))()
    for k, x in enumerate(xs):
        desc[k].x, desc[k].y = x.data_ptr(), outs[k].data_ptr()
        desc[k].rows, desc[k].H, desc[k].W = x.shape[0], x.shape[1], x.shape[2]
    fn = _lib.load().omgsr_conv_out_gn
    for first, count in ([(0, len(xs))] if one_launch else [(k, 1) for k in range(len(xs))]):
        check(fn(C.byref(desc[first]), count, _req(mean, torch.float32, "mean").data_ptr(), _req(rstd, torch.float32, "rstd").data_ptr(),
                 _req(gamma, torch.float32, "gamma").data_ptr(), _req(beta, torch.float32, "beta").data_ptr(), ew.w.data_ptr(),
                 ew.bias.data_ptr(), ew.cin, ew.cout, groups, mean.shape[0], _stream()), "omgsr_conv_out_gn")
    return outs


def conv_out_gn(x: torch.Tensor, ew: EdgeWeight, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                groups: int) -> torch.Tensor:
    return conv_out_gn_multi([x], ew, mean, rstd, gamma, beta, groups)[0]


# --------------------------------------------------------------------------------------------
# norm1's apply pass with the block's 1x1 conv_shortcut computed in it (csrc/norm_shortcut.hip): the accurate tier with fp16 operands only.
# New wrappers the model code calls - group_norm* with also_cast, to_operand and conv2d are unchanged and serve everything else.

GN_SHORTCUT_CHANNELS = (128, 256, 512)
GN_SHORTCUT_SPLITS = (1, 4)          # y forms: plain fp16, OMGSR_EL_MX6


@dataclass
class ShortcutWeight:
    """A 1x1 conv_shortcut's weight as omgsr_groupnorm_shortcut streams it: w fp16 [Cin / 64][4][Cout / 32][hi | lo][64 lanes][8]
    (include/omgsr_hip.h), bias fp32 [Cout]."""
    w: torch.Tensor
    bias: torch.Tensor
    cin: int
    cout: int


def gn_shortcut_enabled() -> bool:
    """OMGSR_GN_SHORTCUT_FUSED=0 restores the apply-with-twin + shortcut GEMM path (A/B runs)."""
    return os.environ.get("OMGSR_GN_SHORTCUT_FUSED", "1") != "0"


def gn_shortcut_ok(stream: torch.dtype, weight_shape, stride: int, padding: int, groups: int, split: int) -> bool:
    """The routing predicate of the call sites (ResnetBlock2D.nhwc, VAEHook._run): a GroupNorm apply whose result is a plain fp16 or MX6
    operand (split 1 | 4), on an fp32 stream tensor under fp16 operands, next to a 1x1 stride-1 unpadded shortcut with Cin and Cout in
    {128, 256, 512} runs as omgsr_groupnorm_shortcut; everything else (every 16-bit tier, the bf16-operand range-fallback tier, other operand
    forms and channel counts, the switch off) as before."""
    if len(weight_shape) != 4:
        return False
    cout, cin, kh, kw = (int(v) for v in weight_shape)
    return (gn_shortcut_enabled() and _PRECISE and _ACT == torch.float16 and stream == torch.float32 and (kh, kw) == (1, 1) and stride == 1
            and padding == 0 and cin in GN_SHORTCUT_CHANNELS and cout in GN_SHORTCUT_CHANNELS and groups > 0 and cin % groups == 0
            and split in GN_SHORTCUT_SPLITS)


def pack_gn_shortcut_weight(weight: torch.Tensor, bias: Optional[torch.Tensor], device=None) -> ShortcutWeight:
    """[Cout, Cin, 1, 1] (any float dtype; taken as fp32) -> ShortcutWeight: hi = fp16(w), lo = fp16(w - hi), both in the kernel's
    B-fragment order (lane l of a 16-channel step holds column l & 31, channels 8 (l >> 5) ... + 7)."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if tuple(weight.shape[2:]) != (1, 1) or cin % 64 or cout % 32:
        raise ValueError("pack_gn_shortcut_weight: a 1x1 kernel, Cin % 64 == 0, Cout % 32 == 0")
    dev = device or weight.device
    w = _note_weight_range(weight.detach().to(device=dev, dtype=torch.float32).reshape(cout, cin))
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)

    def frag(m):        # [Cout, Cin] -> [chunk][step][column tile][lane half][column][8]
        return m.reshape(cout // 32, 32, cin // 64, 4, 2, 8).permute(2, 3, 0, 4, 1, 5)

    pk = torch.stack((frag(hi), frag(lo)), dim=3).contiguous().reshape(cin // 64, 4, cout // 32, 2, 64, 8)
    b = torch.zeros((cout,), device=dev, dtype=torch.float32)
    if bias is not None:
        b.copy_(bias.detach().to(device=dev, dtype=torch.float32))
    return ShortcutWeight(pk, b, cin, cout)


def group_norm_shortcut_multi(xs, sw: ShortcutWeight, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int, act: int = ACT_NONE,
                              split: int = 1, one_launch: bool = True):
    """For every xs[k] ([rows_k, ..., Cin] fp32 stream tensors: the tile-shape groups of a tiled-VAE layer, or one tensor) the pair
    (y, sc): y = act(GroupNorm(x)) as the operand `split` names (the bytes of group_norm_apply_shared), sc = the 1x1 shortcut of the
    un-normalised x, fp32 [rows_k, ..., Cout]. mean / rstd [nimg, G]: row r uses image r % nimg. One launch over a prefix table of the
    groups, or (one_launch False) one launch per tensor: the same bytes."""
    if not 0 < len(xs) <= _lib.GN_MAX_GROUPS:
        raise ValueError(f"1 ... {_lib.GN_MAX_GROUPS} tile shape groups")
    if split not in GN_SHORTCUT_SPLITS:
        raise ValueError("group_norm_shortcut: y is a plain (split 1) or MX6 (split 4) operand")
    for x in xs:
        if _req(x, torch.float32, "x").shape[-1] != sw.cin:
            raise ValueError(f"group_norm_shortcut: x must be [rows, ..., {sw.cin}]")
    ys = [_operand_like(x, split) for x in xs]
    scs = [torch.empty((*x.shape[:-1], sw.cout), device=x.device, dtype=torch.float32) for x in xs]
    desc = (_lib.GnShortcutGroup * len(xs))()
    for k, x in enumerate(xs):
        desc[k].x, desc[k].y, desc[k].sc = x.data_ptr(), ys[k].data_ptr(), scs[k].data_ptr()
        desc[k].rows, desc[k].HW = x.shape[0], x.numel() // (x.shape[0] * sw.cin)
    fn = _lib.load().omgsr_groupnorm_shortcut
    for first, count in ([(0, len(xs))] if one_launch else [(k, 1) for k in range(len(xs))]):
        check(fn(C.byref(desc[first]), count, _req(mean, torch.float32, "mean").data_ptr(), _req(rstd, torch.float32, "rstd").data_ptr(),
                 _ptr(gamma), _ptr(beta), sw.w.data_ptr(), sw.bias.data_ptr(), sw.cin, sw.cout, groups, act, mean.shape[0],
                 _el_of_split(split), _ovf(xs[0].device), _stream()), "omgsr_groupnorm_shortcut")
    return list(zip(ys, scs))


def group_norm_shortcut(x: torch.Tensor, sw: ShortcutWeight, mean: torch.Tensor, rstd: torch.Tensor, gamma, beta, groups: int,
                        act: int = ACT_NONE, split: int = 1):
    return group_norm_shortcut_multi([x], sw, mean, rstd, gamma, beta, groups, act, split)[0]


# --------------------------------------------------------------------------------------------
# K9/K10: LayerNorm (affine or AdaLN-modulated)

def layer_norm(x: torch.Tensor, a: Optional[torch.Tensor], b: Optional[torch.Tensor], eps: float, split: int = 1) -> torch.Tensor:
    """Stream tensor rows -> normalised MFMA operand [..., split*C]."""
    xel = _el(x, "x")
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = _operand_like(x, split)
    check(_lib.load().omgsr_layernorm(x.data_ptr(), y.data_ptr(), _ptr(a), _ptr(b), rows, Cc, eps, xel, _el_of_split(split), _stream()),
          "omgsr_layernorm")
    return y


def layer_norm_mxfp8(x: torch.Tensor, a: Optional[torch.Tensor], b: Optional[torch.Tensor], eps: float, out: Optional[Mxfp8] = None,
                     pad128: bool = False) -> Mxfp8:
    """bf16 stream tensor rows [..., C] (the fp8 tier; C % 128 == 0, C <= 4096) -> the normalised rows as an Mxfp8, written by the LayerNorm
    kernel itself (omgsr_layernorm_mxfp8): the bytes of quantize_mxfp8(layer_norm(x, a, b, eps)). out: a dense Mxfp8 of x's shape.
    pad128 (C % 32 == 0; no `out`): the Mxfp8's last dim is C rounded up to 128, the pad holding zero codes under zero scale bytes - the operand
    of a GEMM whose weight carries the same K pad (pack_geglu_weight_mxfp8). omgsr_layernorm_mxfp8_pad, or with FP8_FUSED_QUANT["layernorm"] off
    the pass form (bf16 layer_norm, zero-pad, quantize_mxfp8): the same bytes."""
    if x.dtype != torch.bfloat16 or _ACT != torch.bfloat16 or _PRECISE:
        raise ValueError("layer_norm_mxfp8: a bf16 stream tensor under the bf16 compute type (the fp8 tier)")
    _req(x, torch.bfloat16, "x")
    Cc = x.shape[-1]
    if pad128:
        if out is not None:
            raise ValueError("layer_norm_mxfp8: pad128 allocates its result")
        if Cc % 32 or Cc > 4096:
            raise ValueError(f"layer_norm_mxfp8: C = {Cc} must be a multiple of 32, at most 4096")
        Kp = _round_up(Cc, 128)
        if not FP8_FUSED_QUANT["layernorm"]:
            y = layer_norm(x, a, b, eps)
            if Kp != Cc:
                yp = torch.zeros((*x.shape[:-1], Kp), device=x.device, dtype=torch.bfloat16)
                yp[..., :Cc] = y
                y = yp
            return quantize_mxfp8(y)
        out = Mxfp8(torch.empty((*x.shape[:-1], Kp), device=x.device, dtype=torch.uint8),
                    torch.empty((*x.shape[:-1], Kp // 32), device=x.device, dtype=torch.uint8))
        check(_lib.load().omgsr_layernorm_mxfp8_pad(x.data_ptr(), _ptr(a), _ptr(b), x.numel() // Cc, Cc, eps, EL_16, out.codes.data_ptr(),
                                                    out.scales.data_ptr(), Kp, Kp // 32, _stream()), "omgsr_layernorm_mxfp8_pad")
        return out
    if Cc % 128 or Cc > 4096:
        raise ValueError(f"layer_norm_mxfp8: C = {Cc} must be a multiple of 128, at most 4096")
    if out is None:
        out = _mxfp8_like(x)
    elif out.codes.shape != x.shape or out.scales.shape != (*x.shape[:-1], Cc // 32) or not (out.codes.is_contiguous() and out.scales.is_contiguous()):
        raise ValueError("layer_norm_mxfp8: `out` does not match x")
    check(_lib.load().omgsr_layernorm_mxfp8(x.data_ptr(), _ptr(a), _ptr(b), x.numel() // Cc, Cc, eps, EL_16, out.codes.data_ptr(), out.scales.data_ptr(),
                                            Cc, Cc // 32, _stream()), "omgsr_layernorm_mxfp8")
    return out


# --------------------------------------------------------------------------------------------
# K7/K8: attention

def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, head_dim: int, scale: float,
              *, q_col: int = 0, k_col: int = 0, Lk: Optional[int] = None, out: Optional[torch.Tensor] = None,
              o_col: int = 0, out_split: int = 1, o_lo_col: Optional[int] = None, q_lo_col: Optional[int] = None,
              k_lo_col: Optional[int] = None, p_split: bool = True) -> torch.Tensor:
    """q [B, Lq, *] (heads at columns q_col + h*D), k [Bk, Lk, *], vt [Bk, heads*D, ld] -> o [B, Lq, heads*D]
    head_dim 512 (the VAE mid block, any Lk): out_split 1 or 2; q_lo_col / k_lo_col with p_split=False and a single V^T, or (the
    range-fallback tier: every operand a two-term split) with p_split=True and the split V^T of transpose_split.
    q_lo_col / k_lo_col (both or neither, head_dim 64 or 512): q and k are two-term splits whose low halves start at those columns of the same rows
    (a projection written with out_split = 2); the scores then run three MFMA passes and, with p_split, the probabilities two (attn_split()).
    (an operand for the output projection; out_split 2: [B, Lq, 2*heads*D] as the two-term split; 3: the same bytes per row in the
    mixed-precision form OMGSR_EL_MX, for an output projection that runs as an MX GEMM).
    Bk == 1 broadcasts one K/V over the batch (constant cross-attention context).
    q, k and vt may instead all be Mxfp8 (the fp8 tier's `fp8_attention`, head_dim 128, bf16 compute type): codes with the layouts above
    (columns in bytes), vt [Bk, heads*D, ld] with ld % 128 == 0 quantised along the key index; the output is bf16 (out_split 1)."""
    mx = [isinstance(x, Mxfp8) for x in (q, k, vt)]
    if any(mx):
        if not all(mx):
            raise ValueError("attention: q, k and vt are all MXFP8 or none is")
        if out_split != 1 or q_lo_col is not None or k_lo_col is not None:
            raise ValueError("attention: MXFP8 operands take a plain bf16 output and no two-term splits")
        return _attention_mxfp8(q, k, vt, heads, head_dim, scale, q_col, k_col, Lk, out, o_col)
    if head_dim == 512:             # vae_attn_kernel / vae_attn_full_kernel: checked here, before the library is called
        if out_split == 3:
            raise ValueError("attention: head_dim 512 writes a plain or two-term-split output (out_split 1 or 2), not the MX form")
        qk2 = q_lo_col is not None and k_lo_col is not None
        if vt.shape[1] == 2 * heads * head_dim:
            if not qk2:
                raise ValueError("attention: a split V^T comes with split q / k")
            if not p_split:
                raise ValueError("attention: head_dim 512 with p_split=False takes a single V^T; the two-term-split V^T comes with p_split=True")
        elif qk2 and p_split:
            raise ValueError("attention: head_dim 512 takes split q / k and a single V^T with p_split=False; split probabilities come with "
                             "the two-term-split V^T")
    _req(q, act_dtype(), "q"); _req(k, act_dtype(), "k"); _req(vt, act_dtype(), "vt")
    B, Lq = q.shape[0], q.shape[1]
    Lk = Lk if Lk is not None else k.shape[1]
    inner = heads * head_dim
    if out is None:
        out = torch.empty((B, Lq, inner * min(out_split, 2)), device=q.device, dtype=act_dtype())      # split 3 (MX): 4 bytes per channel
    a = AttnArgs()
    _fill_attn(a, q, k, vt, out, o_col, heads, head_dim, Lk, scale)
    a.q, a.k, a.vt = q.data_ptr() + q_col * 2, k.data_ptr() + k_col * 2, vt.data_ptr()
    a.o_lo_off = 0 if out_split != 2 else ((o_lo_col - o_col) if o_lo_col is not None else inner)
    a.o_mx = int(out_split == 3)
    if (q_lo_col is None) != (k_lo_col is None):
        raise ValueError("attention: q_lo_col and k_lo_col come together")
    a.q_lo_off = 0 if q_lo_col is None else q_lo_col - q_col
    a.k_lo_off = 0 if k_lo_col is None else k_lo_col - k_col
    a.p_split = int(q_lo_col is not None and p_split)
    if vt.shape[1] == 2 * inner:                      # [Bk, 2 * inner, ld]: V^T as the transposed two-term split (transpose_split)
        if q_lo_col is None:
            raise ValueError("attention: a split V^T comes with split q / k")
        a.vt_lo_off = inner * vt.shape[-1]
    elif vt.shape[1] != inner:
        raise ValueError(f"attention: vt has {vt.shape[1]} rows, expected {inner} (or {2 * inner} as a two-term split)")
    if out_split == 3 and o_col != 0:
        raise ValueError("attention: an MX output owns its whole row (o_col must be 0)")
    check(_lib.load().omgsr_attention(C.byref(a), _stream()), "omgsr_attention")
    return out


def _fill_attn(a: AttnArgs, q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, o_col: int, heads: int, head_dim: int,
               Lk: int, scale: float) -> bool:
    """What the 16-bit and the MXFP8 form share (q, k, vt: the element tensors - the codes of an Mxfp8): extents, leading dimensions, batch
    strides (one K / V for the whole batch when k has one image and q more: stride 0) and the 16-bit output. Returns that broadcast flag."""
    B, Lq = q.shape[0], q.shape[1]
    bcast = k.shape[0] == 1 and B > 1
    a.B, a.H, a.D, a.Lq, a.Lk = B, heads, head_dim, Lq, Lk
    a.q_ld, a.k_ld, a.vt_ld, a.o_ld = q.shape[-1], k.shape[-1], vt.shape[-1], out.shape[-1]
    a.q_bstride, a.o_bstride = Lq * q.shape[-1], Lq * out.shape[-1]
    a.k_bstride, a.vt_bstride = (0, 0) if bcast else (k.shape[1] * k.shape[-1], vt.shape[1] * vt.shape[-1])
    a.o = out.data_ptr() + o_col * 2
    a.scale = scale
    return bcast


def _attention_mxfp8(q: Mxfp8, k: Mxfp8, vt: Mxfp8, heads: int, head_dim: int, scale: float, q_col: int, k_col: int, Lk: Optional[int],
                     out: Optional[torch.Tensor], o_col: int) -> torch.Tensor:
    """attention() on OMGSR_EL_MXFP8 q / k / V^T (mxfp8_attn_kernel, ABI v19)."""
    if _PRECISE or _ACT != torch.bfloat16:
        raise ValueError("MXFP8 attention needs the bf16 compute type (the fp8 tier)")
    if head_dim != 128:
        raise ValueError(f"MXFP8 attention needs head_dim 128, got {head_dim}")
    for name, t in (("q", q), ("k", k), ("vt", vt)):
        _req(t.codes, torch.uint8, name); _req(t.scales, torch.uint8, name + " scales")
        if t.codes.dim() != 3 or t.scales.shape != (*t.codes.shape[:-1], t.codes.shape[-1] // 32):
            raise ValueError(f"attention: {name} is not an [B, rows, ld] MXFP8 operand")
    if q_col % 128 or k_col % 128:
        raise ValueError("attention: MXFP8 q / k columns must be multiples of 128")
    B, Lq = q.codes.shape[0], q.codes.shape[1]
    Lk = Lk if Lk is not None else k.codes.shape[1]
    inner = heads * head_dim
    ld = vt.codes.shape[-1]
    if vt.codes.shape[1] != inner:
        raise ValueError(f"attention: vt has {vt.codes.shape[1]} rows, expected {inner}")
    if ld % 128 or ld < Lk:
        raise ValueError(f"attention: an MXFP8 V^T needs ld % 128 == 0 and ld >= Lk, got ld {ld} for Lk {Lk}")
    if out is None:
        out = torch.empty((B, Lq, inner), device=q.codes.device, dtype=torch.bfloat16)
    _req(out, torch.bfloat16, "out")
    a = AttnArgs()
    bcast = _fill_attn(a, q.codes, k.codes, vt.codes, out, o_col, heads, head_dim, Lk, scale)
    a.qkv_el = EL_MXFP8
    a.q, a.k, a.vt = q.codes.data_ptr() + q_col, k.codes.data_ptr() + k_col, vt.codes.data_ptr()
    a.q_scale, a.k_scale, a.vt_scale = q.scales.data_ptr() + q_col // 32, k.scales.data_ptr() + k_col // 32, vt.scales.data_ptr()
    a.q_sld, a.k_sld, a.vt_sld = q.scales.shape[-1], k.scales.shape[-1], vt.scales.shape[-1]
    a.q_sbstride = Lq * a.q_sld
    a.k_sbstride, a.vt_sbstride = (0, 0) if bcast else (k.codes.shape[1] * a.k_sld, inner * a.vt_sld)
    check(_lib.load().omgsr_attention(C.byref(a), _stream()), "omgsr_attention")
    return out


def softmax_rows(s: torch.Tensor, valid: Optional[int] = None, split: bool = False) -> torch.Tensor:
    """softmax over the first `valid` columns of each row (the rest come out 0). split: [..., 2 L] rows [p_hi | p_lo] (the first factor of
    bmm_nt(both_split=True): the range-fallback tier's PV product)."""
    _req(s, torch.float32, "s")
    L = s.shape[-1]
    rows = s.numel() // L
    p = torch.empty(s.shape[:-1] + ((2 * L) if split else L,), device=s.device, dtype=act_dtype())
    fn = _lib.load().omgsr_softmax_rows_split if split else _lib.load().omgsr_softmax_rows
    check(fn(s.data_ptr(), p.data_ptr(), rows, L, valid or L, _stream()), "omgsr_softmax_rows")
    return p


def rmsnorm_rope_(x: torch.Tensor, w: torch.Tensor, cos: Optional[torch.Tensor], sin: Optional[torch.Tensor],
                  heads: int, head_dim: int, col0: int = 0, pos0: int = 0, eps: float = 1e-6,
                  w_after: Optional[torch.Tensor] = None, split_at: int = 0) -> torch.Tensor:
    """In place on x [B, L, ld]: per head RMSNorm(head_dim) * w[h] then RoPE with cos/sin [>= pos0+L, D] (f32).
    w is [heads, D]: one call can cover the q heads and the k heads of a fused [q|k] buffer. w_after / split_at: rows at
    sequence positions >= split_at use w_after instead (joint [text ; image] sequences)."""
    _req(x, act_dtype(), "x"); _req(w, torch.float32, "w")
    B, L, ld = x.shape
    if tuple(w.shape) != (heads, head_dim) or (w_after is not None and tuple(w_after.shape) != (heads, head_dim)):
        raise ValueError(f"rmsnorm_rope_: w must be [{heads}, {head_dim}], got {tuple(w.shape)}")
    if cos is not None and (cos.shape[0] < pos0 + L or sin.shape[0] < pos0 + L or cos.shape[-1] != head_dim):
        raise ValueError(f"rmsnorm_rope_: rope tables {tuple(cos.shape)} do not cover positions {pos0}..{pos0 + L - 1} x {head_dim}")
    check(_lib.load().omgsr_rmsnorm_rope(x.data_ptr(), w.data_ptr(), _ptr(w_after), split_at, _ptr(cos), _ptr(sin), B, L, heads, head_dim, ld,
                                         col0, pos0, eps, _stream()), "omgsr_rmsnorm_rope")
    return x


def rmsnorm_rope_mxfp8(x: torch.Tensor, w: torch.Tensor, cos: Optional[torch.Tensor], sin: Optional[torch.Tensor], heads: int, head_dim: int,
                       pos0: int = 0, eps: float = 1e-6, w_after: Optional[torch.Tensor] = None, split_at: int = 0,
                       out: Optional[Mxfp8] = None) -> Mxfp8:
    """rmsnorm_rope_ of the first heads * head_dim columns of x [B, L, ld] (bf16) with the fp32 result written as OMGSR_EL_MXFP8 (codes
    [B, L, ld] bytes, scales [B, L, ld / 32]) instead of in place: quantize_mxfp8's rule on the fp32 values, no separate pass. x is unchanged.
    out: a workspace of that shape."""
    _req(x, torch.bfloat16, "x"); _req(w, torch.float32, "w")
    if _PRECISE or _ACT != torch.bfloat16:
        raise ValueError("rmsnorm_rope_mxfp8 needs the bf16 compute type (the fp8 tier)")
    B, L, ld = x.shape
    if ld % 128:
        raise ValueError(f"rmsnorm_rope_mxfp8: row length {ld} is not a multiple of 128")
    if tuple(w.shape) != (heads, head_dim) or (w_after is not None and tuple(w_after.shape) != (heads, head_dim)):
        raise ValueError(f"rmsnorm_rope_mxfp8: w must be [{heads}, {head_dim}], got {tuple(w.shape)}")
    if cos is not None and (cos.shape[0] < pos0 + L or sin.shape[0] < pos0 + L or cos.shape[-1] != head_dim):
        raise ValueError(f"rmsnorm_rope_mxfp8: rope tables {tuple(cos.shape)} do not cover positions {pos0}..{pos0 + L - 1} x {head_dim}")
    if out is None:
        out = _mxfp8_like(x)
    elif out.codes.shape != (B, L, ld) or out.scales.shape != (B, L, ld // 32) or not (out.codes.is_contiguous() and out.scales.is_contiguous()):
        raise ValueError("rmsnorm_rope_mxfp8: `out` does not match x")
    check(_lib.load().omgsr_rmsnorm_rope_mxfp8(x.data_ptr(), w.data_ptr(), _ptr(w_after), split_at, _ptr(cos), _ptr(sin), B, L, heads, head_dim,
                                               ld, 0, pos0, eps, out.codes.data_ptr(), out.scales.data_ptr(), ld, ld // 32, _stream()),
          "omgsr_rmsnorm_rope_mxfp8")
    return out


# --------------------------------------------------------------------------------------------
# K14: layout + latent algebra

def nchw_to_nhwc(x: torch.Tensor, cpad: Optional[int] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """NCHW (f32 or the compute type) -> NHWC stream tensor (channels zero-padded to cpad); dtype overrides stream_dtype()."""
    if x.dtype not in (torch.float32, act_dtype()):
        x = x.to(act_dtype() if not _PRECISE else torch.float32)          # the other 16-bit type / f64: one conversion at the boundary
    _req(x, x.dtype, "x")
    N, Cc, H, W = x.shape
    cpad = cpad or _round_up(Cc, 8)
    dtype = dtype or stream_dtype()
    y = torch.empty((N, H, W, cpad), device=x.device, dtype=dtype)
    check(_lib.load().omgsr_nchw_to_nhwc(x.data_ptr(), y.data_ptr(), N, Cc, H, W, cpad, int(x.dtype == torch.float32),
                                         EL_F32 if dtype == torch.float32 else EL_16, _stream()), "omgsr_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor, channels: Optional[int] = None, dtype=None,
                 clamp: Optional[tuple[float, float]] = None) -> torch.Tensor:
    xel = _el(x, "x")
    dtype = dtype or (torch.float32 if xel == EL_F32 else act_dtype())
    if dtype not in (torch.float32, act_dtype()):
        raise TypeError(f"nhwc_to_nchw: output dtype must be float32 or {act_dtype()}, got {dtype}")
    N, H, W, ld = x.shape
    Cc = channels or ld
    y = torch.empty((N, Cc, H, W), device=x.device, dtype=dtype)
    lo, hi = clamp if clamp else (0.0, 0.0)
    check(_lib.load().omgsr_nhwc_to_nchw(x.data_ptr(), y.data_ptr(), N, Cc, H, W, ld, int(dtype == torch.float32),
                                         int(clamp is not None), lo, hi, xel, _stream()), "omgsr_nhwc_to_nchw")
    return y


def concat_channels(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """torch.cat([a, b], dim=channel) for two NHWC stream tensors of one element kind."""
    el = _el(a, "a")
    if _el(b, "b") != el:
        raise TypeError("concat_channels: element kinds differ")
    Ca, Cb = a.shape[-1], b.shape[-1]
    rows = a.numel() // Ca
    out = torch.empty((*a.shape[:-1], Ca + Cb), device=a.device, dtype=a.dtype)
    lib = _lib.load()
    check(lib.omgsr_copy_channels(a.data_ptr(), out.data_ptr(), rows, Ca, Ca, Ca + Cb, 0, el, _stream()), "omgsr_copy_channels")
    check(lib.omgsr_copy_channels(b.data_ptr(), out.data_ptr(), rows, Cb, Cb, Ca + Cb, Ca, el, _stream()), "omgsr_copy_channels")
    return out


def vae_sample(moments: torch.Tensor, eps: torch.Tensor, latent_channels: int, shift: float, scale: float,
               ld_out: Optional[int] = None) -> torch.Tensor:
    """moments [N,h,w,2C] stream, eps [N,h,w,C] f32 -> z [N,h,w,ld_out] stream of the same kind (zero padded channels)."""
    el = _el(moments, "moments"); _req(eps, torch.float32, "eps")
    N, h, w, _ = moments.shape
    ld_out = ld_out or _round_up(latent_channels, 8)
    z = torch.empty((N, h, w, ld_out), device=moments.device, dtype=moments.dtype)
    check(_lib.load().omgsr_vae_sample(moments.data_ptr(), eps.data_ptr(), z.data_ptr(), N * h * w, latent_channels, ld_out,
                                       shift, scale, el, _stream()), "omgsr_vae_sample")
    return z


def axpby(x: torch.Tensor, y: Optional[torch.Tensor], a: float, b: float, c: float = 0.0, d: float = 1.0,
          bf16_steps: bool = False) -> torch.Tensor:
    el = _el(x, "x")
    if y is not None and _el(y, "y") != el:
        raise TypeError("axpby: element kinds differ")
    out = torch.empty_like(x)
    check(_lib.load().omgsr_axpby(x.data_ptr(), _ptr(y), out.data_ptr(), x.numel(), a, b, c, d, int(bf16_steps), el, _stream()),
          "omgsr_axpby")
    return out


def linear_f32(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, silu_in: bool = False) -> torch.Tensor:
    """fp32 constant folding: y = act(x) @ weight.T + bias with x [..., K], weight [N, K] (any float dtype; widened to fp32 first), in the
    library's own fixed-order kernel (omgsr_linear_f32) - the time / guidance / pooled-text embeddings and the modulation vectors a model
    derives once per (t*, guidance, prompt), so no vendor BLAS runs in the product process. Device tensors only: weights still on the host
    (CPU-side tooling and the `not gpu` tests, where no kernel of this library can run either) take torch's fp32 math instead."""
    w32 = weight.detach().float().contiguous()
    b32 = None if bias is None else bias.detach().float().contiguous()
    x32 = x.detach().float().contiguous()
    if not w32.is_cuda:
        xin = torch.nn.functional.silu(x32) if silu_in else x32
        return torch.nn.functional.linear(xin, w32, b32)
    N, K = w32.shape
    if x32.shape[-1] != K:
        raise ValueError(f"linear_f32: x[..., {x32.shape[-1]}] against weight [{N}, {K}]")
    rows = x32.numel() // K
    y = torch.empty(x32.shape[:-1] + (N,), dtype=torch.float32, device=w32.device)
    check(_lib.load().omgsr_linear_f32(x32.data_ptr(), w32.data_ptr(), _ptr(b32), y.data_ptr(), rows, K, N, int(silu_in), _stream()),
          "omgsr_linear_f32")
    return y


def tile_accumulate(tile: Optional[torch.Tensor], w: torch.Tensor, acc: torch.Tensor, y0: int, x0: int,
                    channels: Optional[int] = None) -> None:
    """acc [N,H,W,C] f32 += tile[..., :C] * w[th,tw]; tile None accumulates the weights alone (acc [1,H,W,1])."""
    _req(w, torch.float32, "w"); _req(acc, torch.float32, "acc")
    N, H, W, Cc = acc.shape
    th, tw = w.shape
    tile_ld, el = 0, EL_16
    if tile is not None:
        el = _el(tile, "tile")
        tile_ld = tile.shape[-1]
    check(_lib.load().omgsr_tile_accumulate(_ptr(tile), w.data_ptr(), acc.data_ptr(), N, Cc, th, tw, tile_ld, H, W, y0, x0,
                                            el, _stream()), "omgsr_tile_accumulate")


def tile_normalise(acc: torch.Tensor, wsum: torch.Tensor, ld: Optional[int] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    N, H, W, Cc = acc.shape
    ld = ld or _round_up(Cc, 8)
    dtype = dtype or stream_dtype()
    out = torch.empty((N, H, W, ld), device=acc.device, dtype=dtype)
    check(_lib.load().omgsr_tile_normalise(acc.data_ptr(), wsum.data_ptr(), out.data_ptr(), N, H * W, Cc, ld,
                                           EL_F32 if dtype == torch.float32 else EL_16, _stream()), "omgsr_tile_normalise")
    return out


def crop_nhwc(x: torch.Tensor, y0: int, x0: int, th: int, tw: int) -> torch.Tensor:
    el = _el(x, "x")
    N, H, W, Cc = x.shape
    out = torch.empty((N, th, tw, Cc), device=x.device, dtype=x.dtype)
    check(_lib.load().omgsr_crop_nhwc(x.data_ptr(), out.data_ptr(), N, H, W, Cc, y0, x0, th, tw, el, _stream()), "omgsr_crop_nhwc")
    return out


def resize_nearest_exact(x: torch.Tensor, scale_factor: float) -> torch.Tensor:
    """F.interpolate(x_nchw, scale_factor=s, mode="nearest-exact") on an NHWC tensor [N, H, W, C] (any element kind): output
    [N, floor(H s), floor(W s), C], source index min(floorf((dst + .5) * (float)(1 / s)), in - 1) - ATen's formula (omgsr_resize_nearest_exact_nhwc)."""
    import math
    el = _el(x, "x")
    N, H, W, Cc = x.shape
    Ho, Wo = int(math.floor(float(H) * scale_factor)), int(math.floor(float(W) * scale_factor))
    out = torch.empty((N, Ho, Wo, Cc), device=x.device, dtype=x.dtype)
    inv = float(torch.tensor(1.0 / scale_factor, dtype=torch.float32))            # (float)(1 / s), as compute_scales_value<float> makes it
    check(_lib.load().omgsr_resize_nearest_exact_nhwc(x.data_ptr(), out.data_ptr(), N, H, W, Cc, Ho, Wo, inv, inv, el, _stream()),
          "omgsr_resize_nearest_exact_nhwc")
    return out


def paste_nhwc(src: torch.Tensor, dst: torch.Tensor, sy0: int, sx0: int, dy0: int, dx0: int, th: int, tw: int) -> None:
    """dst[:, dy0:dy0+th, dx0:dx0+tw, :] = src[:, sy0:sy0+th, sx0:sx0+tw, :] (NHWC, same N, C and element kind)."""
    el = _el(src, "src")
    if _el(dst, "dst") != el:
        raise TypeError("paste_nhwc: element kinds differ")
    N, sH, sW, Cc = src.shape
    if dst.shape[0] != N or dst.shape[3] != Cc:
        raise ValueError("paste_nhwc: batch/channel mismatch")
    check(_lib.load().omgsr_paste_nhwc(src.data_ptr(), dst.data_ptr(), N, Cc, sH, sW, sy0, sx0, dst.shape[1], dst.shape[2],
                                       dy0, dx0, th, tw, el, _stream()), "omgsr_paste_nhwc")


def flux_pack(x: torch.Tensor, channels: int) -> torch.Tensor:
    """NHWC [N,H,W,ld] (first `channels`) -> tokens [N, (H/2)(W/2), 4*channels]."""
    el = _el(x, "x")
    N, H, W, ld = x.shape
    out = torch.empty((N, (H // 2) * (W // 2), 4 * channels), device=x.device, dtype=x.dtype)
    check(_lib.load().omgsr_flux_pack(x.data_ptr(), out.data_ptr(), N, H, W, channels, ld, 0, el, _stream()), "omgsr_flux_pack")
    return out


def flux_unpack(tok: torch.Tensor, H: int, W: int, ld: Optional[int] = None) -> torch.Tensor:
    el = _el(tok, "tok")
    N, _, c4 = tok.shape
    Cc = c4 // 4
    ld = ld or _round_up(Cc, 8)
    out = torch.zeros((N, H, W, ld), device=tok.device, dtype=tok.dtype) if ld != Cc else \
        torch.empty((N, H, W, ld), device=tok.device, dtype=tok.dtype)
    check(_lib.load().omgsr_flux_pack(tok.data_ptr(), out.data_ptr(), N, H, W, Cc, ld, 1, el, _stream()), "omgsr_flux_pack")
    return out
