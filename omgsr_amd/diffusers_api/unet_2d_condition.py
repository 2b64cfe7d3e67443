"""UNet2DConditionModel (SD2.1-base architecture) with diffusers' API surface on the gfx950 kernels.

Stands in for `diffusers.UNet2DConditionModel` at infer/omgsr_s_infer_model.py:15,75-79,132:
`unet(sample[B,4,h,w], timestep:int, encoder_hidden_states=[1|B,77,1024]).sample`, `.config.in_channels`,
`.dtype`. State-dict keys follow SURVEY A.5.

MI355X-first execution (not a module-by-module port):
  * bf16 NHWC throughout: a [B,H,W,C] map IS the [B,HW,C] token matrix, so Transformer2DModel's
    permute/reshape pair disappears
  * OMGSR runs the UNet at ONE fixed timestep t*: the sinusoid, the time-embedding MLP and every
    resnet's time_emb_proj are constants -> folded (fp32) into each conv1's bias, cached per timestep
  * the prompt is fixed too: cross-attention K and V^T of every layer are computed once per
    encoder_hidden_states tensor and cached
  * self-attention reads q|k straight out of one fused projection GEMM; V is produced transposed by
    the GEMM epilogue, which is the layout the fused attention kernel wants
  * GEGLU is a GEMM epilogue (weight rows interleaved at pack time); residual adds are conv/GEMM
    epilogues; nearest-2x upsampling is folded into the conv gather; skip concat is a 16-B/lane copy
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..nn import Conv2d, GroupNorm, InputCache, LayerNorm, Linear, _key, _log_rebuild, bump_cache_epoch, norm_silu_conv
from .autoencoder_kl import Downsample2D, ResnetBlock2D, Upsample2D
from .modeling_utils import ConfigDict, ModelMixin

SD21_UNET_CONFIG = dict(
    in_channels=4, out_channels=4, sample_size=64, block_out_channels=[320, 640, 1280, 1280],
    down_block_types=["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
    up_block_types=["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"],
    layers_per_block=2, attention_head_dim=[5, 10, 20, 20], cross_attention_dim=1024,
    use_linear_projection=True, norm_num_groups=32, norm_eps=1e-5, flip_sin_to_cos=True, freq_shift=0,
    downsample_padding=1, act_fn="silu", mid_block_scale_factor=1, upcast_attention=False)


def timestep_sinusoid(t: torch.Tensor, dim: int, flip_sin_to_cos: bool, freq_shift: float) -> torch.Tensor:
    half = dim // 2
    exponent = -math.log(10000) * torch.arange(half, dtype=torch.float32, device=t.device) / (half - freq_shift)
    emb = t[:, None].float() * torch.exp(exponent)[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
    if flip_sin_to_cos:
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)
    return emb


class TimestepEmbedding(nn.Module):
    def __init__(self, in_dim: int, dim: int):
        super().__init__()
        self.linear_1 = Linear(in_dim, dim)
        self.linear_2 = Linear(dim, dim)

    def fp32(self, x: torch.Tensor) -> torch.Tensor:
        """Constant-folding path (fp32, the library's fixed-order kernel; once per timestep - not on the per-image path)."""
        h = ops.linear_f32(x, self.linear_1.weight, self.linear_1.bias)
        return ops.linear_f32(h, self.linear_2.weight, self.linear_2.bias, silu_in=True)


class Attention(nn.Module):
    """UNet attention: q/k/v without bias, out-proj with bias; head_dim 64."""

    def __init__(self, query_dim: int, heads: int, dim_head: int, cross_attention_dim: Optional[int] = None):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.dim_head, self.scale, self.inner = heads, dim_head, dim_head ** -0.5, inner
        self.is_cross = cross_attention_dim is not None
        kv = cross_attention_dim or query_dim
        self.to_q = Linear(query_dim, inner, bias=False)
        self.to_k = Linear(kv, inner, bias=False)
        self.to_v = Linear(kv, inner, bias=False)
        self.to_out = nn.ModuleList([Linear(inner, query_dim), nn.Dropout(0.0)])
        self._ctx_cache = InputCache()

    def in_split(self) -> int:
        """Split of the LayerNorm'd operand that to_q (| to_k, to_v) consume."""
        return self.to_q.in_split()

    def _qk_packed(self):
        sp, wsp = self.in_split(), self.to_q.in_wsplit()

        def build():
            return ops.pack_linear_weight(torch.cat([self.to_q.weight, self.to_k.weight], dim=0), None, split=sp, w_split=wsp)
        k = _key(self.to_q.weight, self.to_k.weight, sp, wsp)
        if getattr(self, "_qk_key", None) != k:
            bump_cache_epoch()
            self._qk, self._qk_key = build(), k
        return self._qk

    def self_nhwc(self, xn: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        """xn: LayerNorm'd operand tokens [B, L, C*split]; returns residual + to_out(attn) on the stream."""
        B, L, _ = xn.shape
        sp = ops.attn_split() and self.dim_head == 64
        # [B, L, 2*inner]; range-fallback tier: [q_hi | k_hi | q_lo | k_lo] (two-term split from the projection's epilogue, ops.attn_split)
        qk = ops.linear(xn, self._qk_packed(), out_dtype=ops.OUT_BF16, out_split=2 if sp else 1)
        # [B, inner, L8]; split: [B, 2 * inner, L8] = V^T hi rows, then lo rows (fp32 projection output transposed by transpose_split)
        vt = ops.transpose_split(ops.linear(xn, self.to_v.packed(), out_dtype=ops.OUT_F32)) if sp else ops.linear_t(xn, self.to_v.packed(), L)
        o = ops.attention(qk, qk, vt, self.heads, self.dim_head, self.scale, q_col=0, k_col=self.inner, Lk=L,
                          out_split=self.to_out[0].in_split(), q_lo_col=2 * self.inner if sp else None, k_lo_col=3 * self.inner if sp else None)
        return self.to_out[0].nhwc(o, residual=residual)

    def context(self, ehs: torch.Tensor):
        """K and V^T of a fixed prompt: computed once per prompt TENSOR (the cache holds a reference to it and compares
        identity + version; an address is not an identity, the allocator reuses addresses)."""
        sp = ops.attn_split() and self.dim_head == 64

        def build():
            e = ehs.float().contiguous() if ops.precise() else ehs.to(ops.act_dtype()).contiguous()
            kk = ops.linear(e, self.to_k.packed(), out_dtype=ops.OUT_BF16, out_split=2 if sp else 1)      # [Bc, 77, inner] ([k_hi | k_lo] when split)
            vt = (ops.transpose_split(ops.linear(e, self.to_v.packed(), out_dtype=ops.OUT_F32)) if sp else
                  ops.linear_t(e, self.to_v.packed(), e.shape[1]))              # [Bc, inner, 80] ([Bc, 2 * inner, 80] when split)
            return kk, vt, e.shape[1]
        return self._ctx_cache.get((ehs,), self._ctx_key(), build)

    def _ctx_key(self) -> tuple:
        return _key(self.to_k.weight, self.to_v.weight, self.to_k.in_split(), self.to_k.in_wsplit(), self.to_v.in_wsplit(),
                    bool(ops.attn_split() and self.dim_head == 64))

    def cross_nhwc(self, xn: torch.Tensor, ehs: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        kk, vt, Lk = self.context(ehs)
        sp = kk.shape[-1] == 2 * self.inner
        q = self.to_q.nhwc(xn, out_dtype=ops.OUT_BF16, out_split=2 if sp else 1)
        o = ops.attention(q, kk, vt, self.heads, self.dim_head, self.scale, Lk=Lk, out_split=self.to_out[0].in_split(),
                          q_lo_col=self.inner if sp else None, k_lo_col=self.inner if sp else None)
        return self.to_out[0].nhwc(o, residual=residual)


class GEGLU(nn.Module):
    def __init__(self, dim_in: int, dim_out: int):
        super().__init__()
        self.proj = Linear(dim_in, dim_out * 2)

    def packed(self):
        sp, wsp = self.proj.in_split(), self.proj.in_wsplit()
        k = _key(self.proj.weight, self.proj.bias, sp, wsp)
        if getattr(self, "_pk_key", None) != k:
            bump_cache_epoch()
            self._pk, self._pk_key = ops.pack_geglu_weight(self.proj.weight, self.proj.bias, split=sp, w_split=wsp), k
        return self._pk

    # OMGSR-S's bf16 tier (precision.set_fp8_unet_ff): this projection runs as mxfp8_gemm_geglu_kernel on the MXFP8 LayerNorm output where the
    # routing rule admits the problem (FeedForward.fp8_routed). The bf16 pack above stays; the MXFP8 form is packed lazily next to it, under a
    # key of its own that names the form, and a rebuild under graph capture is logged
    fp8 = False

    def packed_mxfp8(self) -> ops.PackedWeight:
        k = _key(self.proj.weight, self.proj.bias, "mxfp8-geglu")
        if getattr(self, "_pk8_key", None) != k:
            bump_cache_epoch()
            _log_rebuild(self._drop_packed_mxfp8)
            self._pk8 = ops.pack_geglu_weight_mxfp8(self.proj.weight, self.proj.bias)
            self._pk8_key = k
        return self._pk8

    def _drop_packed_mxfp8(self) -> None:
        self._pk8, self._pk8_key = None, None
        bump_cache_epoch()


class FeedForward(nn.Module):
    def __init__(self, dim: int, mult: int = 4):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * mult), nn.Dropout(0.0), Linear(dim * mult, dim)])

    def fp8_routed(self, rows: int) -> bool:
        """Whether this feed-forward takes the MXFP8 chain for a problem of `rows` tokens: marked (precision.set_fp8_unet_ff), under the bf16
        tier, and admitted by the one routing rule (precision.fp8_unet_ff_routed)."""
        if not (self.net[0].fp8 and self.net[2].fp8) or ops.precise() or ops.act_dtype() != torch.bfloat16:
            return False
        from ..precision import fp8_unet_ff_routed
        return fp8_unet_ff_routed(rows, self.net[0].proj.in_features)

    def nhwc(self, xn, residual, out_for=None):
        if isinstance(xn, ops.Mxfp8):  # (BasicTransformerBlock asked fp8_routed): GEGLU GEMM -> MXFP8 hidden -> net.2 + the bf16 residual
            h = ops.linear(xn, self.net[0].packed_mxfp8(), out_mxfp8=True)
            if out_for is not None:
                return self.net[2].nhwc(h, residual=residual, out_dtype=ops.OUT_BF16, out_split=out_for.in_split())
            return self.net[2].nhwc(h, residual=residual)
        net2 = self.net[2].packed_plain() if self.net[2].fp8 else self.net[2].packed()    # a marked block on a problem the rule refuses: today's path
        # a * gelu(gate) in the GEMM epilogue; the hidden tensor is the operand of net[2]
        h = ops.linear(xn, self.net[0].packed(), out_dtype=ops.OUT_BF16, out_split=self.net[2].in_split())
        if out_for is not None:       # the sum's only consumer is that linear (Transformer2DModel.proj_out): write its operand directly
            return ops.linear(h, net2, residual=residual, out_dtype=ops.OUT_BF16, out_split=out_for.in_split())
        return ops.linear(h, net2, residual=residual)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim: int, heads: int, dim_head: int, cross_attention_dim: int):
        super().__init__()
        self.norm1 = LayerNorm(dim, eps=1e-5)
        self.attn1 = Attention(dim, heads, dim_head)
        self.norm2 = LayerNorm(dim, eps=1e-5)
        self.attn2 = Attention(dim, heads, dim_head, cross_attention_dim=cross_attention_dim)
        self.norm3 = LayerNorm(dim, eps=1e-5)
        self.ff = FeedForward(dim)

    def nhwc(self, y, ehs, out_for=None):
        y = self.attn1.self_nhwc(self.norm1.nhwc(y, split=self.attn1.in_split()), y)
        y = self.attn2.cross_nhwc(self.norm2.nhwc(y, split=self.attn2.in_split()), ehs, y)
        if self.ff.fp8_routed(y.numel() // y.shape[-1]):       # norm3 writes the GEGLU GEMM's MXFP8 operand, K padded to 128 (C = 320 -> 384)
            a, b = self.norm3._affine()
            return self.ff.nhwc(ops.layer_norm_mxfp8(y, a, b, self.norm3.eps, pad128=True), y, out_for=out_for)
        return self.ff.nhwc(self.norm3.nhwc(y, split=self.ff.net[0].proj.in_split()), y, out_for=out_for)


class Transformer2DModel(nn.Module):
    def __init__(self, channels: int, heads: int, dim_head: int, cross_attention_dim: int, groups: int):
        super().__init__()
        self.norm = GroupNorm(groups, channels, eps=1e-6)
        self.proj_in = Linear(channels, channels)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(channels, heads, dim_head, cross_attention_dim)])
        self.proj_out = Linear(channels, channels)

    def nhwc(self, x, ehs, out_for=None):
        """out_for: the result's only consumer is that conv (the up block's upsampler): written directly as its operand."""
        N, H, W, Cc = x.shape
        res = x.reshape(N, H * W, Cc)
        y = self.proj_in.nhwc(self.norm.nhwc(x, split=self.proj_in.in_split()).reshape(N, H * W, -1))
        nb = len(self.transformer_blocks)
        for i, blk in enumerate(self.transformer_blocks):
            y = blk.nhwc(y, ehs, out_for=self.proj_out if i == nb - 1 else None)
        if out_for is not None:
            out = self.proj_out.nhwc(y, residual=res, out_dtype=ops.OUT_BF16, out_split=out_for.in_split())
            return out.reshape(N, H, W, -1)
        out = self.proj_out.nhwc(y, residual=res, gn_groups=self.norm.num_groups)     # a resnet's GroupNorm usually consumes it
        return ops.carry_gn(out, out.reshape(N, H, W, Cc))


class _DownBlock(nn.Module):
    def __init__(self, cin, cout, temb, layers, heads, cross_dim, groups, eps, add_down, down_pad, with_attn):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(cin if j == 0 else cout, cout, temb, groups, eps) for j in range(layers)])
        self.attentions = nn.ModuleList([Transformer2DModel(cout, heads, cout // heads, cross_dim, groups) for _ in range(layers)]) if with_attn else None
        self.downsamplers = nn.ModuleList([Downsample2D(cout, down_pad)]) if add_down else None


class _UpBlock(nn.Module):
    def __init__(self, in_channels, prev_out, cout, temb, layers, heads, cross_dim, groups, eps, add_up, with_attn):
        super().__init__()
        rs = []
        for j in range(layers):
            skip = in_channels if j == layers - 1 else cout
            rin = prev_out if j == 0 else cout
            rs.append(ResnetBlock2D(rin + skip, cout, temb, groups, eps))
        self.resnets = nn.ModuleList(rs)
        self.attentions = nn.ModuleList([Transformer2DModel(cout, heads, cout // heads, cross_dim, groups) for _ in range(layers)]) if with_attn else None
        self.upsamplers = nn.ModuleList([Upsample2D(cout)]) if add_up else None


class _MidBlock(nn.Module):
    def __init__(self, ch, temb, heads, cross_dim, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(ch, ch, temb, groups, eps), ResnetBlock2D(ch, ch, temb, groups, eps)])
        self.attentions = nn.ModuleList([Transformer2DModel(ch, heads, ch // heads, cross_dim, groups)])


class UNet2DConditionModel(ModelMixin):
    default_config = SD21_UNET_CONFIG

    def __init__(self, **cfg):
        super().__init__()
        c = ConfigDict({**SD21_UNET_CONFIG, **cfg})
        self.config = c
        boc = c.block_out_channels
        temb = boc[0] * 4
        heads = c.attention_head_dim if isinstance(c.attention_head_dim, (list, tuple)) else [c.attention_head_dim] * len(boc)
        g, eps = c.norm_num_groups, c.norm_eps
        self.conv_in = Conv2d(c.in_channels, boc[0], 3, padding=1)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        downs, out_ch = [], boc[0]
        for i, t in enumerate(c.down_block_types):
            in_ch, out_ch = out_ch, boc[i]
            downs.append(_DownBlock(in_ch, out_ch, temb, c.layers_per_block, heads[i], c.cross_attention_dim, g, eps,
                                    add_down=i < len(boc) - 1, down_pad=c.downsample_padding,
                                    with_attn=t == "CrossAttnDownBlock2D"))
        self.down_blocks = nn.ModuleList(downs)
        self.mid_block = _MidBlock(boc[-1], temb, heads[-1], c.cross_attention_dim, g, eps)
        rev, rheads = list(reversed(boc)), list(reversed(heads))
        ups, out_ch = [], rev[0]
        for i, t in enumerate(c.up_block_types):
            prev, out_ch = out_ch, rev[i]
            in_ch = rev[min(i + 1, len(boc) - 1)]
            ups.append(_UpBlock(in_ch, prev, out_ch, temb, c.layers_per_block + 1, rheads[i], c.cross_attention_dim, g, eps,
                                add_up=i < len(boc) - 1, with_attn=t == "CrossAttnUpBlock2D"))
        self.up_blocks = nn.ModuleList(ups)
        self.conv_norm_out = GroupNorm(g, boc[0], eps=eps)
        self.conv_act = nn.SiLU()
        self.conv_out = Conv2d(boc[0], c.out_channels, 3, padding=1)
        self._temb_cache: dict = {}

    # ---- constant folding at fixed t* ------------------------------------------------------
    def _resnets(self):
        for b in self.down_blocks:
            yield from b.resnets
        yield from self.mid_block.resnets
        for b in self.up_blocks:
            yield from b.resnets

    def _fold_key(self, timestep) -> tuple:
        t = int(timestep) if not torch.is_tensor(timestep) else int(timestep.reshape(-1)[0].item())
        # every parameter the folded biases depend on is in the key (a LoRA merge into one resnet's time_emb_proj must refold)
        deps = [self.time_embedding.linear_1.weight, self.time_embedding.linear_1.bias, self.time_embedding.linear_2.weight,
                self.time_embedding.linear_2.bias]
        for r in self._resnets():
            deps += [r.time_emb_proj.weight, r.time_emb_proj.bias, r.conv1.bias]
        return (t, _key(*deps))

    def _folded_biases(self, timestep) -> dict:
        """{id(resnet): conv1.bias + time_emb_proj(silu(time_embedding(sinusoid(t))))} in fp32."""
        key = self._fold_key(timestep)
        t = key[0]
        if key not in self._temb_cache:
            bump_cache_epoch()
            dev = self.conv_in.weight.device
            with torch.no_grad():
                tt = torch.tensor([t], dtype=torch.int64, device=dev)
                emb = self.time_embedding.fp32(timestep_sinusoid(tt, self.config.block_out_channels[0],
                                                                 self.config.flip_sin_to_cos, self.config.freq_shift))
                out = {}
                for r in self._resnets():
                    v = ops.linear_f32(emb, r.time_emb_proj.weight, r.time_emb_proj.bias, silu_in=True)[0]
                    out[id(r)] = (r.conv1.bias.float() + v).contiguous()
            self._temb_cache = {key: out}
        return self._temb_cache[key]

    # ---- NHWC executor ---------------------------------------------------------------------
    def nhwc(self, x: torch.Tensor, timestep, ehs: torch.Tensor) -> torch.Tensor:
        """x [B,h,w,8] stream (4 latent channels + zero pad) -> eps [B,h,w,8] stream (4 channels + zero pad)."""
        fb = self._folded_biases(timestep)
        g = self.config.norm_num_groups       # producers leave the statistics of the GroupNorm that reads them next
        h = self.conv_in.nhwc(x, gn_groups=g)
        skips = [h]
        for blk in self.down_blocks:
            for j, r in enumerate(blk.resnets):
                h = r.nhwc(h, fb[id(r)])
                if blk.attentions is not None:
                    h = blk.attentions[j].nhwc(h, ehs)
                skips.append(h)
            if blk.downsamplers is not None:
                h = blk.downsamplers[0].nhwc(h, gn_groups=g)
                skips.append(h)
        m = self.mid_block
        h = m.resnets[0].nhwc(h, fb[id(m.resnets[0])])
        h = m.attentions[0].nhwc(h, ehs)
        h = m.resnets[1].nhwc(h, fb[id(m.resnets[1])])
        for blk in self.up_blocks:
            up = blk.upsamplers[0].conv if blk.upsamplers is not None else None
            for j, r in enumerate(blk.resnets):
                last = up if j == len(blk.resnets) - 1 else None       # the block's last tensor feeds only the upsampling conv
                skip = skips.pop()
                if h.dtype == torch.float32 and r.conv_shortcut is not None:
                    h = (h, skip)       # accurate tier: only norm1 reads the concatenation (ResnetBlock2D.nhwc, ops.group_norm_pair)
                else:                   # 16-bit tiers: the concatenated tensor is itself the shortcut's operand
                    h = ops.concat_channels(h, skip)
                h = r.nhwc(h, fb[id(r)], out_for=last if blk.attentions is None else None)
                if blk.attentions is not None:
                    h = blk.attentions[j].nhwc(h, ehs, out_for=last)
            if blk.upsamplers is not None:
                h = blk.upsamplers[0].nhwc(h, gn_groups=g if ops.precise() else 0)        # accurate tier: the next norm1 folds these with its skip's
        return norm_silu_conv(self.conv_norm_out, self.conv_out, h)

    # ---- diffusers API ---------------------------------------------------------------------
    def forward(self, sample: torch.Tensor, timestep, encoder_hidden_states: torch.Tensor, return_dict: bool = True):
        x = ops.nchw_to_nhwc(sample.contiguous(), 8)
        y = self.nhwc(x, timestep, encoder_hidden_states)
        out_dtype = ops.io_dtype(sample)
        out = ops.nhwc_to_nchw(y, channels=self.config.out_channels, dtype=out_dtype)
        return SimpleNamespace(sample=out) if return_dict else (out,)
