"""Leaf modules of the MI355X path: torch.nn parameter containers (so diffusers state dicts, `.to()`
and PEFT-style weight merging work unchanged) whose compute runs through the HIP kernels.

Two ways in:
  * `.nhwc(x, ...)`  — fast path used by the model executors: channels-last; stream tensors in and out by default
                       (ops.py: the compute type in the fast tiers, fp32 in the accurate tier), MFMA operands in between
  * `.forward(x)`    — diffusers/torch calling convention (NCHW for convs/GroupNorm) so code that
                       duck-types the modules op by op (the reference's infer/vaehook.py:248-276)
                       still works; it converts layout around the same kernels.
Packed (KRSC bf16) weights are built lazily and rebuilt if the parameter changes (LoRA merge, .to()).
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch
import torch.nn as nn

from . import ops


def _key(*tensors) -> tuple:
    """Identity of PARAMETER tensors (held alive by their module, so an address names one tensor) under the current tier.
    Not for per-call inputs: see input_key()."""
    return ops.mode_key() + tuple((t.data_ptr(), t._version, str(t.device), t.dtype, tuple(t.shape)) if torch.is_tensor(t) else t for t in tensors)


# Every rebuild of a cached device value (packed weights, folded constants, cross-attention K / V^T, modulation / rope tables) bumps this
# counter. A captured hipGraph bakes the ADDRESSES of those values into its launches, and the one-slot caches free the old value when they
# rebuild: pipelines/graphed.py stamps each graph with the epoch it was captured under and drops it when any cache has rebuilt since
# (prompt A -> prompt B -> prompt A would otherwise replay graph A against freed or re-used K / V^T memory).
_CACHE_EPOCH = 0


def cache_epoch() -> int:
    return _CACHE_EPOCH


def bump_cache_epoch() -> None:
    global _CACHE_EPOCH
    _CACHE_EPOCH += 1


# Rebuild log (pipelines/graphed.py): while a hipGraph capture is open, every cache that rebuilds registers how to INVALIDATE itself. A value built
# under capture was never computed (its kernels were recorded, not run); if the capture is then discarded, the slots are emptied so that the eager
# re-run rebuilds them for real instead of reading uninitialised memory.
_REBUILD_LOG = None


def begin_rebuild_log() -> None:
    global _REBUILD_LOG
    _REBUILD_LOG = []


def end_rebuild_log() -> list:
    global _REBUILD_LOG
    log, _REBUILD_LOG = _REBUILD_LOG or [], None
    return log


def _log_rebuild(invalidate) -> None:
    if _REBUILD_LOG is not None:
        _REBUILD_LOG.append(invalidate)


class InputCache:
    """One-slot cache keyed on per-call INPUT tensors (prompt embeddings, ids, pooled projections). The caching allocator
    reuses addresses, so an address is not an identity: the slot keeps a strong reference to every keyed tensor and
    compares with `is` + `_version` (+ the weights' parameter key)."""

    def __init__(self):
        self._inputs, self._versions, self._wkey, self._value = None, None, None, None

    def prime(self, inputs: tuple, wkey: tuple, value) -> None:
        """Install a value computed elsewhere (omgsr_amd.constants: the serialised constant cache)."""
        self._value, self._inputs, self._wkey = value, tuple(inputs), wkey
        self._versions = tuple(None if t is None else t._version for t in inputs)
        bump_cache_epoch()

    def invalidate(self) -> None:
        self._inputs, self._versions, self._wkey, self._value = None, None, None, None
        bump_cache_epoch()

    def get(self, inputs: tuple, wkey: tuple, builder):
        same = (self._inputs is not None and len(self._inputs) == len(inputs) and self._wkey == wkey and
                all(a is b for a, b in zip(self._inputs, inputs)) and
                self._versions == tuple(None if t is None else t._version for t in inputs))
        if not same:
            bump_cache_epoch()
            _log_rebuild(self.invalidate)
            self._value = builder()
            self._inputs, self._wkey = tuple(inputs), wkey
            self._versions = tuple(None if t is None else t._version for t in inputs)
        return self._value


class _Packed:
    """Mixin: lazily packed weights keyed on the parameters' identity/version."""

    def _drop_packed(self) -> None:
        self._pk, self._pk_key = None, None
        bump_cache_epoch()

    def _packed(self, builder, *tensors):
        k = _key(*tensors)
        if getattr(self, "_pk_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed)
            self._pk = builder()
            self._pk_key = k
        return self._pk


class _Operand:
    """`op_split`: 1, or 2 when this layer's INPUT arrives as a two-term split operand (accurate tier, set per layer by a
    precision policy: omgsr_amd.precision). The producer of the input (norm / cast / GEMM epilogue) asks the consumer."""
    op_split = 1
    # `w_split`: 1, or 2 when this layer's WEIGHT is carried as the two-term split w_hi + w_lo (accurate tier, fp32 checkpoints whose
    # values are not 16-bit representable; precision.set_weight_split). Invisible to producers: the operand row is unchanged, the
    # packed weight gains a [w_lo] K segment that wraps over the operand's (hi) half (ops.pack_conv_weight).
    w_split = 1
    # accurate tier: this layer's OUTPUT is only ever normalised and fed to the next GEMM (a ResnetBlock's conv1): keep it in the
    # 16-bit compute type instead of the fp32 stream type where the policy says the rounding is affordable (precision.py)
    out_inner16 = False

    def in_split(self) -> int:
        return self.op_split if ops.precise() else 1

    def in_wsplit(self) -> int:
        return self.w_split if ops.precise() else 1


class Conv2d(nn.Conv2d, _Packed, _Operand):
    # set by Upsample2D: this 3x3 conv is applied to a nearest-2x upsampled map, so its packed weight also carries the four
    # phase-summed 2 x 2 kernels (ops.pack_conv_weight upsample_phases) and runs with 4 / 9 of the MFMA work
    phase_upsample = False
    # the fp8 tier (precision.set_fp8_conv): where the library serves the problem (ops.conv2d fp8_pack) this 3x3 conv runs as an MXFP8 x MXFP8
    # convolution behind a GroupNorm apply pass that writes MXFP8. The bf16 pack stays (problems the kernel does not serve take it, exactly as
    # without the mark); the MXFP8 form is packed lazily next to it, under a key of its own that names the form, so a weight edit re-packs both
    fp8 = False

    def packed_mxfp8(self) -> ops.PackedWeight:
        k = _key(self.weight, self.bias, "mxfp8-conv")
        if getattr(self, "_pk8_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed_mxfp8)
            self._pk8 = ops.pack_conv_weight_mxfp8(self.weight, self.bias)
            self._pk8_key = k
        return self._pk8

    def _drop_packed_mxfp8(self) -> None:
        self._pk8, self._pk8_key = None, None
        bump_cache_epoch()

    # the fp8 tier (precision.set_fp8_upsample): an up-sampling conv (Upsample2D) whose problems the library serves (ops.conv2d fp8_up_pack) run
    # as mxfp8_conv_up_kernel behind one quantize pass over the low-resolution map; packed lazily like the nine-tap MXFP8 form, under its own key
    fp8_up = False

    def packed_mxfp8_up(self) -> ops.PackedWeight:
        k = _key(self.weight, self.bias, "mxfp8-conv-up")
        if getattr(self, "_pk8u_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed_mxfp8_up)
            self._pk8u = ops.pack_conv_weight_mxfp8_up(self.weight, self.bias)
            self._pk8u_key = k
        return self._pk8u

    def _drop_packed_mxfp8_up(self) -> None:
        self._pk8u, self._pk8u_key = None, None
        bump_cache_epoch()

    # OMGSR-S's bf16 tier (precision.set_fp8_unet_conv): a UNet resnet conv whose problems the library serves (ops.conv2d fp8_deep_pack) runs as
    # mxfp8_conv_deep_kernel behind the GroupNorm apply pass that writes MXFP8; the same layout as packed_mxfp8 with whole 64-channel chunks
    # (Cin = 320 ... 1920), packed lazily under its own key
    fp8_deep = False

    def packed_mxfp8_deep(self) -> ops.PackedWeight:
        k = _key(self.weight, self.bias, "mxfp8-conv-deep")
        if getattr(self, "_pk8d_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed_mxfp8_deep)
            self._pk8d = ops.pack_conv_weight_mxfp8(self.weight, self.bias, cin_multiple=64)
            self._pk8d_key = k
        return self._pk8d

    def _drop_packed_mxfp8_deep(self) -> None:
        self._pk8d, self._pk8d_key = None, None
        bump_cache_epoch()

    # the accurate tiers' edge layers (csrc/conv_edge.hip): a conv_out behind its GroupNorm + SiLU on an fp32 stream tensor runs as ONE fp32
    # kernel on the un-normalised map (ops.conv_out_gn_multi) instead of the apply pass + the MFMA conv. The call sites ask edge_out() and
    # route; nhwc() / nhwc_multi() and the packs above do not change. The fp32 pack is lazy, under a key of its own like the MXFP8 forms
    def edge_out(self, x: torch.Tensor, norm: "GroupNorm") -> bool:
        return (self.groups == 1 and self.dilation == (1, 1) and self.stride[0] == self.stride[1] and self.padding[0] == self.padding[1]
                and x.shape[-1] == self.in_channels
                and ops.edge_conv_out_ok(x.dtype, self.weight.shape, self.stride[0], self.padding[0], norm.num_groups))

    def packed_edge_out(self) -> "ops.EdgeWeight":
        k = _key(self.weight, self.bias, "edge-out")
        if getattr(self, "_pke_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed_edge_out)
            self._pke = ops.pack_edge_out_weight(self.weight, self.bias)
            self._pke_key = k
        return self._pke

    def _drop_packed_edge_out(self) -> None:
        self._pke, self._pke_key = None, None
        bump_cache_epoch()

    def nhwc_edge_out_multi(self, xs, norm: "GroupNorm", mean: torch.Tensor, rstd: torch.Tensor):
        """conv(silu(norm(x))) of every xs[k] with the statistics mean / rstd [nimg, G] (edge_out() said yes): [rows, H, W, Cout8] fp32."""
        g, b = norm._affine()
        return ops.conv_out_gn_multi(list(xs), self.packed_edge_out(), mean, rstd, g, b, norm.num_groups)

    # the accurate tier's channel-changing ResnetBlocks (csrc/norm_shortcut.hip): this 1x1 conv_shortcut is computed inside norm1's apply pass
    # over the fp32 stream tensor (ops.group_norm_shortcut*) instead of as a GEMM on a cast twin of it. The call sites ask gn_shortcut() and
    # route; nhwc() and the packs above do not change. The hi / lo fp16 pack is lazy, under a key of its own like the other forms
    def gn_shortcut(self, x: torch.Tensor, norm: "GroupNorm", split: int) -> bool:
        """split: the operand form norm1's consumer (conv1) asked for."""
        return (self.groups == 1 and self.dilation == (1, 1) and self.stride[0] == self.stride[1] and self.padding[0] == self.padding[1]
                and x.shape[-1] == self.in_channels == norm.num_channels and not self.out_inner16
                and ops.gn_shortcut_ok(x.dtype, self.weight.shape, self.stride[0], self.padding[0], norm.num_groups, split))

    def packed_gn_shortcut(self) -> "ops.ShortcutWeight":
        k = _key(self.weight, self.bias, "gn-shortcut")
        if getattr(self, "_pks_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed_gn_shortcut)
            self._pks = ops.pack_gn_shortcut_weight(self.weight, self.bias)
            self._pks_key = k
        return self._pks

    def _drop_packed_gn_shortcut(self) -> None:
        self._pks, self._pks_key = None, None
        bump_cache_epoch()

    def packed(self) -> ops.PackedWeight:
        # logical Cout widened to a multiple of 8 (zero rows): 3/4-channel heads write 16-byte NHWC rows
        sp, wsp, ph = self.in_split(), self.in_wsplit(), self.phase_upsample
        return self._packed(lambda: ops.pack_conv_weight(self.weight, self.bias, cout_multiple=8, split=sp, w_split=wsp, upsample_phases=ph),
                            self.weight, self.bias, sp, wsp, ph)

    def nhwc(self, x, *, pad=None, upsample=False, act=ops.ACT_NONE, residual=None, bias_override=None, stride=None, gn_groups=0,
             out_dtype=ops.OUT_STREAM, out_split=1, gn=None):
        """x [N,H,W,Cin8] (operand, or a stream tensor that is cast / split here) -> [N,Ho,Wo,Cout8]; channels beyond
        out_channels are exact zeros. gn (ops.GnSpec): x is the stream tensor a GroupNorm reads; the norm runs as this conv's patch
        producer where the kernel can, as the separate apply pass otherwise (ops.conv2d)."""
        pw = self.packed()
        if bias_override is not None:
            pw = dataclasses.replace(pw, bias=bias_override)
        p = self.padding[0] if pad is None else pad
        if out_dtype == ops.OUT_STREAM and self.out_inner16 and ops.precise():
            out_dtype = ops.OUT_BF16
        fp8_pack = self.packed_mxfp8 if (self.fp8 and gn is not None and bias_override is None) else None
        fp8_up_pack = self.packed_mxfp8_up if (self.fp8_up and upsample and gn is None and bias_override is None) else None
        fp8_deep_pack = None
        if self.fp8_deep and gn is not None and self.in_channels % 64 == 0:
            # (the UNet's conv1 carries the folded time embedding as bias_override: it rides the MXFP8 pack as it rides the bf16 one)
            fp8_deep_pack = self.packed_mxfp8_deep if bias_override is None else \
                (lambda: dataclasses.replace(self.packed_mxfp8_deep(), bias=bias_override))
        return ops.conv2d(x, pw, stride=stride or self.stride[0], pad=p, upsample=upsample, act=act, residual=residual,
                          gn_groups=gn_groups, out_dtype=out_dtype, out_split=out_split, gn=gn, fp8_pack=fp8_pack, fp8_up_pack=fp8_up_pack,
                          fp8_deep_pack=fp8_deep_pack)

    def nhwc_multi(self, xs, *, pad=None, upsample=False, act=ops.ACT_NONE, residuals=None, stride=None, gn_groups=0,
                   out_dtype=ops.OUT_STREAM, out_split=1, gn=None, fp8=False):
        """nhwc() of several inputs (the tile-shape groups of a tiled-VAE layer) in one launch where the kernel allows (ops.conv2d_multi).
        fp8: the caller serves marked layers (VAEHook.fp8_convs) - a marked conv then hands its MXFP8 form on under nhwc()'s condition."""
        pw = self.packed()
        p = self.padding[0] if pad is None else pad
        if out_dtype == ops.OUT_STREAM and self.out_inner16 and ops.precise():
            out_dtype = ops.OUT_BF16
        fp8_pack = self.packed_mxfp8 if (fp8 and self.fp8 and gn is not None) else None
        fp8_up_pack = self.packed_mxfp8_up if (fp8 and self.fp8_up and upsample and gn is None) else None
        return ops.conv2d_multi(list(xs), pw, stride=stride or self.stride[0], pad=p, upsample=upsample, act=act, residuals=residuals,
                                gn_groups=gn_groups, out_dtype=out_dtype, out_split=out_split, gn=gn, fp8_pack=fp8_pack, fp8_up_pack=fp8_up_pack)

    def forward(self, x):  # NCHW compat
        y = self.nhwc(ops.nchw_to_nhwc(x.contiguous(), ops._round_up(self.in_channels, 8)))
        return ops.nhwc_to_nchw(y, channels=self.out_channels,
                                dtype=ops.io_dtype(x))


class Linear(nn.Linear, _Packed, _Operand):
    # the fp8 tier (precision.set_fp8_linear): this layer runs as an MXFP8 x MXFP8 GEMM. The module keeps its bf16 weight (LoRA merges and
    # in-place edits work as before); the packed form is quantised from it and joins the pack key, so an edit re-packs
    fp8 = False

    def packed(self) -> ops.PackedWeight:
        if self.fp8:
            return self._packed(lambda: ops.pack_linear_weight_mxfp8(self.weight, self.bias), self.weight, self.bias, "fp8")
        sp, wsp = self.in_split(), self.in_wsplit()
        return self._packed(lambda: ops.pack_linear_weight(self.weight, self.bias, split=sp, w_split=wsp), self.weight, self.bias, sp, wsp)

    def packed_plain(self) -> ops.PackedWeight:
        """The 16-bit pack of an fp8-marked layer, for the problems its caller keeps off the MXFP8 path (the UNet's routed feed-forwards,
        precision.fp8_unet_ff_routed): packed() without the mark, in a slot of its own so that the two forms do not evict each other."""
        sp, wsp = self.in_split(), self.in_wsplit()
        k = _key(self.weight, self.bias, sp, wsp, "plain")
        if getattr(self, "_pkp_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed_plain)
            self._pkp = ops.pack_linear_weight(self.weight, self.bias, split=sp, w_split=wsp)
            self._pkp_key = k
        return self._pkp

    def _drop_packed_plain(self) -> None:
        self._pkp, self._pkp_key = None, None
        bump_cache_epoch()

    def nhwc(self, x, *, act=ops.ACT_NONE, residual=None, gate=None, out_dtype=ops.OUT_STREAM, gn_groups=0, out_split=1, out_mxfp8=None):
        """out_mxfp8 (an fp8 layer only; True or an Mxfp8 to write into): the result as an Mxfp8, from the GEMM's epilogue (ops.linear)."""
        return ops.linear(x, self.packed(), act=act, residual=residual, gate=gate, out_dtype=out_dtype, gn_groups=gn_groups,
                          out_split=out_split, out_mxfp8=out_mxfp8)

    def forward(self, x):
        y = self.nhwc(x.to(ops.stream_dtype()).contiguous())
        return y.to(x.dtype)


class GroupNorm(nn.GroupNorm, _Packed):
    def _affine(self):
        return self._packed(lambda: (self.weight.detach().float().contiguous(), self.bias.detach().float().contiguous()),
                            self.weight, self.bias)

    def nhwc(self, x, act=ops.ACT_NONE, split=1, also_cast=0):
        """Stream tensor -> normalised (+SiLU) MFMA operand; split 2: as the two-term split its consumer asked for.
        also_cast 1 | 2: returns (operand, x itself as a plain / split operand) from the same pass over x."""
        g, b = self._affine()
        return ops.group_norm(x, g, b, self.num_groups, self.eps, act, split=split, also_cast=also_cast)

    def nhwc_pair(self, a, b, act=ops.ACT_NONE, split=1, also_cast=0):
        """nhwc of the channel concatenation [a | b] without building it where ops.group_norm_pair can."""
        g, bt = self._affine()
        return ops.group_norm_pair(a, b, g, bt, self.num_groups, self.eps, act, split=split, also_cast=also_cast)

    def stats(self, x):
        return ops.group_norm_stats(x, self.num_groups, self.eps)

    def spec(self, x, act=ops.ACT_NONE) -> "ops.GnSpec":
        """This norm (statistics of x included) as something a conv can run as its patch producer: conv.nhwc(x, gn=norm.spec(x, SILU))."""
        mean, rstd, _ = self.stats(x)
        return self.spec_stats(mean, rstd, act)

    def spec_stats(self, mean, rstd, act=ops.ACT_NONE) -> "ops.GnSpec":
        """The same with externally supplied per-(image, group) statistics (tiled VAE)."""
        g, b = self._affine()
        return ops.GnSpec(mean, rstd, g, b, self.num_groups, act)

    def apply_stats(self, x, mean, rstd, act=ops.ACT_NONE, split=1, also_cast=0):
        """Normalise with externally supplied per-(n, group) statistics (tiled VAE)."""
        g, b = self._affine()
        if mean.shape[0] != x.shape[0]:       # tile-major rows sharing their image's statistics
            return ops.group_norm_apply_shared(x, mean, rstd, g, b, self.num_groups, act, split=split, also_cast=also_cast)
        return ops.group_norm_apply(x, mean, rstd, g, b, self.num_groups, act, split=split, also_cast=also_cast)

    def apply_stats_multi(self, xs, mean, rstd, act=ops.ACT_NONE, split=1, also_cast=0):
        """apply_stats over the tile-shape groups of a tiled-VAE layer in one launch (the same bytes as one call per group)."""
        g, b = self._affine()
        return ops.group_norm_apply_multi(xs, mean, rstd, g, b, self.num_groups, act, split=split, also_cast=also_cast)

    def nhwc_shortcut(self, x, shortcut: "Conv2d", act=ops.ACT_NONE, split=1):
        """nhwc(x, act, split) and the 1x1 `shortcut` of the un-normalised x from ONE pass over x (shortcut.gn_shortcut() said yes):
        (operand, fp32 shortcut result)."""
        g, b = self._affine()
        mean, rstd, _ = ops.group_norm_stats(x, self.num_groups, self.eps)
        return ops.group_norm_shortcut(x, shortcut.packed_gn_shortcut(), mean, rstd, g, b, self.num_groups, act, split)

    def apply_stats_shortcut_multi(self, xs, mean, rstd, shortcut: "Conv2d", act=ops.ACT_NONE, split=1):
        """The same over the tile-shape groups of a tiled-VAE layer with supplied statistics, in one launch: [(operand, shortcut result)]."""
        g, b = self._affine()
        return ops.group_norm_shortcut_multi(list(xs), shortcut.packed_gn_shortcut(), mean, rstd, g, b, self.num_groups, act, split)

    def forward(self, x):  # NCHW (or [B, C, L]) compat
        shp = x.shape
        x4 = x.reshape(shp[0], shp[1], -1, 1) if x.dim() == 3 else x
        y = self.nhwc(ops.nchw_to_nhwc(x4.contiguous()))
        return ops.nhwc_to_nchw(y, dtype=ops.io_dtype(x)).to(x.dtype).reshape(shp)


def norm_silu_conv(norm: GroupNorm, conv: Conv2d, h: torch.Tensor) -> torch.Tensor:
    """conv(silu(norm(h))): the tail of the UNet and of the untiled VAE encoder / decoder (conv_norm_out, conv_out). Accurate tiers: the fp32
    edge kernel; 16-bit tiers: the conv takes the norm as before."""
    if conv.edge_out(h, norm):
        mean, rstd, _ = norm.stats(h)
        return conv.nhwc_edge_out_multi([h], norm, mean, rstd)[0]
    return conv.nhwc(h, gn=norm.spec(h, ops.ACT_SILU))


class LayerNorm(nn.LayerNorm, _Packed):
    def _affine(self):
        if not self.elementwise_affine:
            return None, None
        return self._packed(lambda: (self.weight.detach().float().contiguous(), self.bias.detach().float().contiguous()),
                            self.weight, self.bias)

    def nhwc(self, x, a=None, b=None, split=1):
        if a is None and b is None:
            a, b = self._affine()
        return ops.layer_norm(x, a, b, self.eps, split=split)

    def forward(self, x):
        return self.nhwc(x.to(ops.stream_dtype()).contiguous()).to(x.dtype)


class RMSNormWeight(nn.Module):
    """Parameter holder for diffusers' RMSNorm (`weight` [dim]); applied inside omgsr_rmsnorm_rope."""

    def __init__(self, dim: int, eps: float):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def w32(self):
        return self.weight.detach().float().contiguous()
