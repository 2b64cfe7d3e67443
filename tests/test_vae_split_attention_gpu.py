"""The range-fallback tier's fused head_dim-512 attention (vae_attn_full_kernel, omgsr_attention with D = 512, p_split and vt_lo_off, timing
variant 23: split q, k, P and V^T) and its opt-in route in VaeAttention (fused_range_fallback): the kernel against float64, against the
split-q/k kernel and against the materialised chain; bit-exact probes of the V_lo and P_lo lane maps; masking; writes; the rescale branch;
module parity, peak memory, 20480 tokens, a small VAE decode against the fp32 oracle and batch invariance."""
import copy
import math
import time

import pytest
import torch
import torch.nn.functional as F

from test_vae_fused_attention_gpu import _Timing, _g, _module_ref64, _rel, _sdpa_ref, _vae_attention

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 512
DTYPES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _ops():
    from omgsr_amd import ops
    return ops


class _Tier:
    """The range-fallback tier (fp32 stream, 16-bit operands of type dt, every operand a two-term split) inside the block."""

    def __init__(self, dt=torch.bfloat16):
        self.dt = dt

    def __enter__(self):
        _ops().set_compute_dtype(torch.float32, operand_dtype=self.dt)
        return _ops()

    def __exit__(self, *exc):
        _ops().set_batch_invariant(False)
        _ops().set_compute_dtype(torch.bfloat16)
        return False


def _sp(t, dt):
    """[hi | lo] along the last dimension, as a projection writes with out_split=2."""
    hi = t.to(dt)
    return torch.cat([hi, (t - hi.float()).to(dt)], -1)


def _both(o):
    inner = o.shape[-1] // 2
    return o[..., :inner].double() + o[..., inner:].double()


def _kinds(tm):
    return [(kind, var if kind == 2 else 0) for kind, var, _, _ in tm.entries if kind in (2, 6)]           # attention / softmax launches


def _full(ops, qq, kk, vts, H, scale, Lk, **kw):
    return ops.attention(qq, kk, vts, H, D, scale, Lk=Lk, out_split=2, q_lo_col=H * D, k_lo_col=H * D, p_split=True, **kw)


def _qk_only(ops, qq, kk, vts, H, scale, Lk):
    """The existing split-q/k kernel (variant 20) on V_hi: single P, single V^T."""
    return ops.attention(qq, kk, vts[:, :H * D].contiguous(), H, D, scale, Lk=Lk, out_split=2, q_lo_col=H * D, k_lo_col=H * D, p_split=False)


def _materialised(ops, qq, kk, v32, H, scale, Lk):
    """The chain VaeAttention runs in this tier, head by head: bmm_nt(both_split) -> softmax_rows(split) -> bmm_nt(p, [v_hi | v_hi | v_lo])."""
    B, inner, Lp = qq.shape[0], H * D, (Lk + 127) // 128 * 128
    outs = []
    for h in range(H):
        cols = slice(h * D, (h + 1) * D)
        qh = torch.cat([qq[..., :inner][..., cols], qq[..., inner:][..., cols]], -1).contiguous()
        kh = torch.cat([kk[..., :inner][..., cols], kk[..., inner:][..., cols]], -1).expand(B, -1, -1).contiguous()
        s = ops.bmm_nt(qh, ops.split_rows_hhl(kh, Lp), alpha=scale, out_dtype=ops.OUT_F32, both_split=True)
        vts = ops.transpose_split(v32[..., cols].expand(B, -1, -1).contiguous(), Lp)
        vt = torch.cat([vts[:, :D], vts[:, :D], vts[:, D:]], dim=-1)
        outs.append(ops.bmm_nt(ops.softmax_rows(s, valid=Lk, split=True), vt, out_split=2, both_split=True))
    return torch.cat([o[..., :D] for o in outs] + [o[..., D:] for o in outs], -1)


# ---- 1. the kernel against float64 ---------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("B,H,Lq,Lk,bcast", [
    (2, 1, 1000, 1000, False),          # ragged queries and keys
    (1, 2, 200, 136, False),            # two heads
    (2, 1, 300, 77, True),              # 77 keys, one K / V broadcast over the batch
    (1, 1, 256, 256, False)])           # a multiple of every tile size
def test_full_split_against_float64(dt, B, H, Lq, Lk, bcast):
    """Against float64 attention on the UNsplit values: e_full (the new call) is at least 10x below e_qk (split q / k only, single P and V^T: a
    dropped or mis-mapped low half of P or V lands at that order; a CPU emulation of the two arithmetics gives a factor of about 200) and no
    more than 25 % above e_mat, the materialised chain on the same operands (the margin of test_attention_d512_two_term_split_q_k)."""
    with _Tier(dt) as ops:
        inner, Bk, scale = H * D, 1 if bcast else B, D ** -0.5
        q = torch.randn(B, Lq, inner, generator=_g(90)) * 1.5
        k = torch.randn(Bk, Lk, inner, generator=_g(91)) * 1.5
        v = torch.randn(Bk, Lk, inner, generator=_g(92))                  # full-mantissa fp32
        ref = _sdpa_ref(q.double(), k.double(), v.double(), H, scale)
        qq, kk, v32 = _sp(q, dt).to(DEV), _sp(k, dt).to(DEV), v.to(DEV)
        vts = ops.transpose_split(v32)
        assert vts.shape == (Bk, 2 * inner, (Lk + 7) // 8 * 8)
        with _Timing() as tm:
            full = _full(ops, qq, kk, vts, H, scale, Lk)
        assert [(kind, var) for kind, var, _, _ in tm.entries] == [(2, 23)]
        assert tm.entries[0][2] == 4.0 * B * H * Lq * Lk * D and tm.entries[0][3] == 2.0 * B * H * D * (3 * Lq + 4 * Lk)
        e_full = _rel(_both(full), ref)
        e_qk = _rel(_both(_qk_only(ops, qq, kk, vts, H, scale, Lk)), ref)
        e_mat = _rel(_both(_materialised(ops, qq, kk, v32, H, scale, Lk)), ref)
        print(f"attention d512 full split {(B, H, Lq, Lk)} {dt}: full split {e_full:.3e}  split q / k only {e_qk:.3e}  materialised chain {e_mat:.3e}")
        assert torch.isfinite(full.float()).all()
        assert e_full <= e_qk / 10
        assert e_full <= 1.25 * e_mat
        assert torch.equal(_full(ops, qq, kk, vts, H, scale, Lk), full)


# ---- 2. / 3. lane maps of the two new operands ---------------------------------------------------------------------------------------------------

def test_lane_map_v_lo_one_hot():
    """q = 0 makes every probability exactly 1 (p_hi = 1, p_lo = 0). Channel d of V^T_hi holds ONE dyadic value val_d at key 37 d mod Lk, V^T_lo
    holds val_d 2^-9 at key (37 d + 5) mod Lk: o_hi + o_lo must be exactly val_d (1 + 2^-9) / Lk."""
    with _Tier() as ops:
        Lq, Lk = 160, 1024
        vts = torch.zeros(1, 2 * D, Lk)
        want = torch.empty(D, dtype=torch.float64)
        for d in range(D):
            val = (-1) ** d * (1.0 + (d % 8) / 8) * 2.0 ** (d % 5 - 2)
            vts[0, d, (37 * d) % Lk] = val
            vts[0, D + d, (37 * d + 5) % Lk] = val * 2.0 ** -9
            want[d] = val * (1 + 2.0 ** -9) / Lk
        kk = _sp(torch.randn(1, Lk, D, generator=_g(3)), torch.bfloat16).to(DEV)
        o = _full(ops, torch.zeros(1, Lq, 2 * D, dtype=torch.bfloat16, device=DEV), kk, vts.to(torch.bfloat16).to(DEV), 1, D ** -0.5, Lk)
        assert torch.equal(_both(o)[0].cpu(), want.expand(Lq, D))


def test_lane_map_p_lo_identity_v():
    """V^T_hi = identity over 512 keys, V^T_lo = 0: o_hi + o_lo is the probability row itself, p_hi + p_lo. Within 2^-13 relative of float64
    softmax on the hi + lo operands on EVERY element (a CPU emulation of the arithmetic: 2.1e-5 at most; with P_lo dropped 95 % of the
    elements exceed 2^-13, up to 3.9e-3)."""
    with _Tier() as ops:
        Lq, Lk, dt = 160, 512, torch.bfloat16
        qq, kk = _sp(torch.randn(1, Lq, D, generator=_g(11)), dt), _sp(torch.randn(1, Lk, D, generator=_g(12)), dt)
        vts = torch.zeros(1, 2 * D, Lk, dtype=dt)
        vts[0, :D] = torch.eye(D)
        o = _both(_full(ops, qq.to(DEV), kk.to(DEV), vts.to(DEV), 1, D ** -0.5, Lk))[0].cpu()
        ref = torch.softmax(_both(qq)[0] @ _both(kk)[0].T * D ** -0.5, -1)
        worst = float(((o - ref).abs() / ref).max())
        print(f"P_lo lane map: worst relative error of a probability {worst:.3e} (bound 2^-13 = {2.0 ** -13:.3e})")
        assert worst <= 2.0 ** -13


# ---- 4. masking ----------------------------------------------------------------------------------------------------------------------------------

def test_masked_keys_never_reach_the_result():
    """k rows (both halves) and the columns of both V^T halves past Lk hold NaN: the result does not move a bit."""
    with _Tier() as ops:
        B, H, Lq, Lk, rows, ld, dt = 2, 2, 300, 1000, 1100, 1104, torch.bfloat16
        qq = _sp(torch.randn(B, Lq, H * D, generator=_g(1)), dt).to(DEV)
        kk = _sp(torch.randn(B, Lk, H * D, generator=_g(2)), dt)
        vts = _sp(torch.randn(B, Lk, H * D, generator=_g(3)), dt).transpose(1, 2).contiguous()        # [B, 2 inner, Lk]: hi rows, then lo rows
        clean = _full(ops, qq, kk.to(DEV), vts.to(DEV), H, D ** -0.5, Lk)
        k2 = torch.full((B, rows, 2 * H * D), float("nan"), dtype=dt)
        k2[:, :Lk] = kk
        vt2 = torch.full((B, 2 * H * D, ld), float("nan"), dtype=dt)
        vt2[:, :, :Lk] = vts
        got = _full(ops, qq, k2.to(DEV), vt2.to(DEV), H, D ** -0.5, Lk)
        assert torch.isfinite(got.float()).all() and torch.equal(got, clean)


# ---- 5. writes stay inside -----------------------------------------------------------------------------------------------------------------------

def test_writes_stay_inside_their_columns():
    """out= a wider, taller tensor prefilled with a sentinel, o_col > 0 and the low halves a gap further: only [o_col, o_col + inner) and
    [o_lo_col, o_lo_col + inner) of the first Lq rows change, and they hold the plain call's bits."""
    with _Tier() as ops:
        H, Lq, Lk, dt = 2, 200, 136, torch.bfloat16
        inner, o_col, o_lo_col, extra = H * D, 8, H * D + 24, 40
        qq = _sp(torch.randn(1, Lq, inner, generator=_g(21)), dt).to(DEV)
        kk = _sp(torch.randn(1, Lk, inner, generator=_g(22)), dt).to(DEV)
        vts = ops.transpose_split(torch.randn(1, Lk, inner, generator=_g(23)).to(DEV))
        plain = _full(ops, qq, kk, vts, H, D ** -0.5, Lk)
        out = torch.full((1, Lq + extra, 2 * inner + 40), -7.0, dtype=dt, device=DEV)
        got = _full(ops, qq, kk, vts, H, D ** -0.5, Lk, out=out, o_col=o_col, o_lo_col=o_lo_col)
        assert got.data_ptr() == out.data_ptr()
        # (the batch stride is Lq rows of `out`: with B = 1 the rows past Lq belong to nobody)
        assert torch.equal(out[:, :Lq, o_col:o_col + inner], plain[..., :inner]) and torch.equal(out[:, :Lq, o_lo_col:o_lo_col + inner], plain[..., inner:])
        keep = torch.ones(out.shape, dtype=torch.bool, device=DEV)
        keep[:, :Lq, o_col:o_col + inner] = False
        keep[:, :Lq, o_lo_col:o_lo_col + inner] = False
        assert bool((out[keep] == -7.0).all())


# ---- 6. the rescale branch -----------------------------------------------------------------------------------------------------------------------

@DTYPES
def test_full_split_spiked_max(dt):
    """test_attention_d512_spiked_max's construction on full-mantissa draws: keys that dominate late in the sweep, far above and below 2^8 in
    the base-2 domain, in tiles 9 and 12 and in the partial last tile (Lk = 500). Same bound as test 1."""
    with _Tier(dt) as ops:
        L, Lk, scale = 512, 500, D ** -0.5
        q, k, v = (torch.randn(1, n, D, generator=_g(s)) for n, s in ((L, 29), (Lk, 30), (Lk, 31)))
        c = math.sqrt(64 / D)
        k[0, 300] = q[0, 5] * 4.0 * c
        k[0, 495] = q[0, 70] * 6.0 * c
        k[0, 400] = q[0, 9] * 0.6 * c
        k[0, 490] = q[0, 200] * 0.6 * c
        s = (q[0] @ k[0].T) * scale * math.log2(math.e)
        for row, key, above in ((5, 300, True), (70, 495, True), (9, 400, False), (200, 490, False)):
            jump = float(s[row, key] - s[row, :key].max())
            assert (jump > 8.0) if above else (0.0 < jump < 8.0), (row, key, jump)
        ref = _sdpa_ref(q.double(), k.double(), v.double(), 1, scale)
        qq, kk, vts = _sp(q, dt).to(DEV), _sp(k, dt).to(DEV), ops.transpose_split(v.to(DEV))
        full = _full(ops, qq, kk, vts, 1, scale, Lk)
        e_full, e_qk = _rel(_both(full), ref), _rel(_both(_qk_only(ops, qq, kk, vts, 1, scale, Lk)), ref)
        print(f"attention d512 full split, spiked maximum {dt}: full split {e_full:.3e}  split q / k only {e_qk:.3e}")
        assert torch.isfinite(full.float()).all() and e_full <= e_qk / 10


# ---- 7. / 8. / 11. the module ----------------------------------------------------------------------------------------------------------------------

def _rf_module(a0):
    """The module on the device with the range fallback's policy (every operand and weight a two-term split); call inside _Tier."""
    from omgsr_amd.precision import apply_policy
    a = copy.deepcopy(a0).to(DEV, torch.float32)
    apply_policy(a, [r"."], [r"."])
    assert _ops().attn_split() and a.fused_range_fallback is False and a.to_out[0].in_split() == 2
    return a


def test_module_parity_and_route():
    """VaeAttention.nhwc, N = 2, 36 x 37 (ragged queries and keys): each route against the float64 host restatement. The switch decides the
    route and nothing else: on, ONE launch of variant 23 and no softmax launch; off again, the bits of the first call."""
    with _Tier() as ops, torch.no_grad():
        a0 = _vae_attention()
        x = (torch.randn(2, 36, 37, D, generator=_g(83)) * 2).to(torch.bfloat16).float()
        want = _module_ref64(a0, x)
        a, xd = _rf_module(a0), x.to(DEV)
        with _Timing() as t_before:
            before = a.nhwc(xd)
        a.fused_range_fallback = True
        with _Timing() as t_fused:
            fused = a.nhwc(xd)
        a.fused_range_fallback = False
        with _Timing() as t_after:
            after = a.nhwc(xd)
        assert _kinds(t_fused) == [(2, 23)]
        assert _kinds(t_before) == _kinds(t_after) == [(6, 0)] and torch.equal(before, after)
        e_f, e_m = _rel(fused, want), _rel(before, want)
        b_f, b_m = _rel(fused.double().cpu() - x.double(), want - x.double()), _rel(before.double().cpu() - x.double(), want - x.double())
        print(f"VaeAttention 36 x 37 N=2 range-fallback: output rel-L2 fused_split {e_f:.3e} materialised {e_m:.3e}; "
              f"attention branch alone fused_split {b_f:.3e} materialised {b_m:.3e}")
        assert torch.isfinite(fused).all() and e_f <= 1.25 * e_m


def test_module_peak_memory():
    """N = 2, 64 x 64: the fused route's peak is below the materialised route's by at least the fp32 score tensor [N, L, Lp] it never builds."""
    with _Tier(), torch.no_grad():
        a = _rf_module(_vae_attention())
        N, L = 2, 64 * 64
        x = (torch.randn(N, 64, 64, D, generator=_g(84)) * 2).to(DEV)
        peaks = {}
        for on in (False, True):
            a.fused_range_fallback = on
            a.nhwc(x)                               # packed weights and workspaces exist before the measured call
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            y = a.nhwc(x)
            torch.cuda.synchronize()
            peaks[on] = torch.cuda.max_memory_allocated()
            del y
        print(f"VaeAttention 64 x 64 N=2 range-fallback: peak memory materialised {peaks[False] / 2 ** 20:.0f} MiB, fused_split {peaks[True] / 2 ** 20:.0f} MiB")
        assert peaks[False] - peaks[True] >= N * L * L * 4


def test_module_batch_invariant():
    with _Tier() as ops, torch.no_grad():
        a = _rf_module(_vae_attention())
        a.fused_range_fallback = True
        x = (torch.randn(2, 36, 37, D, generator=_g(61)) * 2).to(DEV)
        ops.set_batch_invariant(True)
        with _Timing() as tm:
            both = a.nhwc(x)
        one, two = a.nhwc(x[0:1].contiguous()), a.nhwc(x[1:2].contiguous())
        assert _kinds(tm) == [(2, 23)]
        assert torch.equal(both[0:1], one) and torch.equal(both[1:2], two)


# ---- 9. past the old limit -----------------------------------------------------------------------------------------------------------------------

def test_module_20480_tokens():
    """L = 20480 > 16384 with the switch on: finite, and on 256 sampled query rows (the first and the last query tile included) the attention
    branch is no further from float64 than the accurate tier's (fp16 operands, split q / k, vae_attn_kernel) on the same input and rows.
    With the switch off the tier still names its limit."""
    from test_vae_fused_attention_gpu import _tiered
    ops = _ops()
    a0 = _vae_attention()
    x = torch.randn(1, 128, 160, D, generator=_g(71))
    N, H, W, C = x.shape
    L = H * W
    rows = torch.cat([torch.arange(0, 64), torch.arange(L - 64, L), torch.randperm(L - 128, generator=_g(72))[:128] + 64])
    t0 = time.perf_counter()
    with torch.no_grad():
        g = F.group_norm(x.double().permute(0, 3, 1, 2), 32, a0.group_norm.weight.double(), a0.group_norm.bias.double(), 1e-6).reshape(C, L).T
        q, k, v = (F.linear(g, m.weight.double(), m.bias.double()) for m in (a0.to_q, a0.to_k, a0.to_v))
        want = F.linear(torch.softmax(q[rows] @ k.T * C ** -0.5, -1) @ v, a0.to_out[0].weight.double(), a0.to_out[0].bias.double())
    print(f"float64 host restatement, 256 rows of 20480 tokens: {time.perf_counter() - t0:.1f} s")
    branch = lambda y: (y.double().cpu() - x.double()).reshape(L, C)[rows]        # noqa: E731
    with _Tier() as ops, torch.no_grad():
        a = _rf_module(a0)
        with pytest.raises(ValueError, match="range-fallback VAE attention is limited to 16384 keys"):
            a.nhwc(x.to(DEV))
        a.fused_range_fallback = True
        with _Timing() as tm:
            got = a.nhwc(x.to(DEV))
        assert _kinds(tm) == [(2, 23)] and torch.isfinite(got).all()
        e_rf = _rel(branch(got), want)
    try:
        with torch.no_grad():
            acc, _ = _tiered(copy.deepcopy(a0), "accurate")
            acc.fused = True
            with _Timing() as tm:
                got = acc.nhwc(x.to(DEV))
            assert _kinds(tm) == [(2, 20)]
            e_acc = _rel(branch(got), want)
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    print(f"VaeAttention 128 x 160 (20480 tokens), attention branch on 256 rows: range-fallback fused_split {e_rf:.3e}  accurate tier fused {e_acc:.3e}")
    assert e_rf <= e_acc


# ---- 10. a small VAE against the fp32 oracle -----------------------------------------------------------------------------------------------------

def test_tiny_vae_decode_vs_oracle():
    """A 512-wide mid block in a small VAE, latent 24 x 24, batch 2, range-fallback tier with the full policy: both routes meet the accurate
    bound against the fp32 oracle (rel-L2 <= 1e-3, PSNR >= 60 dB), the fused route within 25 % of the materialised one."""
    from omgsr_amd.diffusers_api import AutoencoderKL
    from omgsr_amd.precision import apply_policy
    from omgsr_amd.testing import psnr, rel_l2, seeded_init_
    from oracle import diffusers_ref as R
    cfg = dict(block_out_channels=[32, 64, 128, 512], layers_per_block=1)
    ov = seeded_init_(R.AutoencoderKL(**cfg), 303, rounded=False).eval()
    z = torch.randn(2, 4, 24, 24, generator=_g(77))
    with torch.no_grad():
        ref = ov.decode(z).sample
    with _Tier(), torch.no_grad():
        p = AutoencoderKL(**cfg)
        p.load_state_dict(ov.state_dict())
        p = p.to(DEV, torch.float32).eval()
        apply_policy(p, [r"."], [r"."])
        res = {}
        for on in (False, True):
            p.set_range_fallback_fused_attention(on)
            with _Timing() as tm:
                got = p.decode(z.to(DEV)).sample.float().cpu()
            assert _kinds(tm) == ([(2, 23)] if on else [(6, 0)])
            assert got.shape == ref.shape and torch.isfinite(got).all()
            res[on] = (rel_l2(got, ref), psnr(got, ref))
    print(f"tiny VAE decode 192 x 192 N=2, range-fallback: materialised rel-L2 {res[False][0]:.3e} PSNR {res[False][1]:.1f} dB; "
          f"fused_split rel-L2 {res[True][0]:.3e} PSNR {res[True][1]:.1f} dB")
    for e, ps in res.values():
        assert e <= 1e-3 and ps >= 60.0
    assert res[True][0] <= 1.25 * res[False][0]
