"""The fused head_dim-512 attention (vae_attn_kernel, omgsr_attention with D = 512, timing variant 20) and its routing in VaeAttention:
kernel parity against host references, the rescale branch, bit-exact lane-map probes, the two-term-split q / k of the accurate tier,
module parity with the materialised path at sizes both run, an untiled FLUX-VAE decode past the materialised path's 16384-key limit
against the fp32 oracle, a 65536-key launch, repeatability / batch invariance / graph replay, and the range-fallback tier's error."""
import math
import time

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 512


def _ops():
    from omgsr_amd import ops
    return ops


@pytest.fixture(params=["bf16", "fp16"])
def compute_dtype(request):
    ops = _ops()
    ops.set_compute_dtype(torch.bfloat16 if request.param == "bf16" else torch.float16)
    yield request.param
    ops.set_compute_dtype(torch.bfloat16)


def bf(x):
    return x.to(_ops().act_dtype())


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).float()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / ref.norm())


def assert_close(got, ref, name, rel_l2=6e-3, max_ulps=6.0):
    """tests/test_kernels_gpu.py::assert_close with test_attention's bounds (P is rounded to 16 bits before the PV product)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).norm() / ref.norm().clamp_min(1e-12)
    scale = ref.abs().clamp_min(ref.abs().mean())
    worst = ((got - ref).abs() / scale).max().item()
    print(f"{name}: rel-L2 {err.item():.3e}, worst element {worst:.3e}")
    assert err.item() < rel_l2, f"{name}: rel-L2 {err.item():.3e} (worst elt {worst:.3e})"
    assert worst < max_ulps * 2 ** -8, f"{name}: worst element error {worst:.3e} (rel-L2 {err.item():.3e})"


def _sdpa_ref(q, k, v, heads, scale):
    B, Lq, inner = q.shape
    d = inner // heads
    qh = q.reshape(B, Lq, heads, d).transpose(1, 2)
    kh = k.reshape(k.shape[0], -1, heads, d).transpose(1, 2)
    vh = v.reshape(v.shape[0], -1, heads, d).transpose(1, 2)
    s = torch.einsum("bhqd,bhkd->bhqk", qh, kh.expand(B, -1, -1, -1)) * scale
    o = torch.einsum("bhqk,bhkd->bhqd", s.softmax(-1), vh.expand(B, -1, -1, -1))
    return o.transpose(1, 2).reshape(B, Lq, inner)


def _vt(v, ld=None):
    Bk, Lk, inner = v.shape
    ld = ld or (Lk + 7) // 8 * 8
    vt = torch.zeros(Bk, inner, ld)
    vt[:, :, :Lk] = v.transpose(1, 2)
    return vt


class _Timing:
    """The library's per-launch timing records of the launches inside the block."""

    def __enter__(self):
        from omgsr_amd import _lib
        self.lib = _lib.load()
        self.lib.omgsr_timing_enable(1); self.lib.omgsr_timing_reset()
        self.entries = []
        return self

    def __exit__(self, *exc):
        from omgsr_amd import _lib
        torch.cuda.synchronize()
        buf = (_lib.TimingEntry * 8192)()
        n = self.lib.omgsr_timing_collect(buf, 8192)
        self.lib.omgsr_timing_enable(0)
        self.entries = [(e.kind, e.variant, e.flops, e.bytes) for e in buf[:n]]
        return False


# ---- 1. kernel vs the fp32 host reference --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,Lq,Lk,bcast", [
    (1, 1, 256, 256, False),            # a multiple of every tile size
    (2, 1, 1000, 1000, False),          # ragged queries and keys
    (1, 1, 4096, 4090, False),
    (2, 1, 300, 77, True),              # 77 keys, one K / V broadcast over the batch
    (1, 2, 200, 136, False),            # two heads
    (1, 1, 2048, 20480, False)])        # past the materialised path's 16384 keys
def test_attention_d512(compute_dtype, B, H, Lq, Lk, bcast):
    ops = _ops()
    inner = H * D
    q = rnd(B, Lq, inner, seed=26)
    Bk = 1 if bcast else B
    k = rnd(Bk, Lk, inner, seed=27)
    v = rnd(Bk, Lk, inner, seed=28)
    scale = D ** -0.5
    ref = _sdpa_ref(q, k, v, H, scale)
    with _Timing() as tm:
        o = ops.attention(bf(q).to(DEV), bf(k).to(DEV), bf(_vt(v)).to(DEV), H, D, scale, Lk=Lk)
    assert_close(o, ref, f"attention d512 {compute_dtype} {(B, H, Lq, Lk)}")
    assert [(kind, var) for kind, var, _, _ in tm.entries] == [(2, 20)]
    assert tm.entries[0][2] == 4.0 * B * H * Lq * Lk * D and tm.entries[0][3] == 2.0 * B * H * D * (2 * Lq + 2 * Lk)


def test_masked_keys_never_reach_the_result(compute_dtype):
    """k rows and V^T columns past Lk hold NaN: the result does not move a bit."""
    ops = _ops()
    B, H, Lq, Lk, rows = 2, 2, 300, 1000, 1100
    q, k, v = rnd(B, Lq, H * D, seed=1), rnd(B, Lk, H * D, seed=2), rnd(B, Lk, H * D, seed=3)
    clean = ops.attention(bf(q).to(DEV), bf(k).to(DEV), bf(_vt(v)).to(DEV), H, D, D ** -0.5, Lk=Lk)
    k2 = torch.full((B, rows, H * D), float("nan"))
    k2[:, :Lk] = k
    vt2 = torch.full((B, H * D, 1104), float("nan"))
    vt2[:, :, :Lk] = v.transpose(1, 2)
    got = ops.attention(bf(q).to(DEV), bf(k2).to(DEV), bf(vt2).to(DEV), H, D, D ** -0.5, Lk=Lk)
    assert torch.isfinite(got.float()).all() and torch.equal(got, clean)


# ---- 2. the rescale branch -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tier", ["bf16", "fp16", "accurate"])
def test_attention_d512_spiked_max(tier):
    """Force the online-softmax rescale: keys that dominate late in the sweep - once far above the deferred-maximum threshold (2^8 in the scaled
    base-2 domain) and once below it (p > 1, no rescale in the fast tiers; the accurate tier runs the exact running maximum) - in a tile other
    than the first (32-key tiles: keys 300 and 400 are in tiles 9 and 12) and in the partial last tile (Lk = 500: keys 480 .. 499)."""
    ops = _ops()
    try:
        ops.set_compute_dtype({"bf16": torch.bfloat16, "fp16": torch.float16, "accurate": torch.float32}[tier])
        B, H, L, Lk = 1, 1, 512, 500
        q, k, v = rnd(B, L, D, seed=29), rnd(B, Lk, D, seed=30), rnd(B, Lk, D, seed=31)
        c = math.sqrt(64 / D)               # q . q ~ D: the factors of the D = 64 test scaled to the same logits
        k[0, 300] = q[0, 5] * 4.0 * c
        k[0, 495] = q[0, 70] * 6.0 * c
        k[0, 400] = q[0, 9] * 0.6 * c
        k[0, 490] = q[0, 200] * 0.6 * c
        k = k.to(torch.bfloat16).float()
        scale = D ** -0.5
        ref = _sdpa_ref(q, k, v, H, scale)
        s = (q[0] @ k[0].T) * scale * math.log2(math.e)
        for row, key, above in ((5, 300, True), (70, 495, True), (9, 400, False), (200, 490, False)):
            jump = float(s[row, key] - s[row, :key].max())
            assert (jump > 8.0) if above else (0.0 < jump < 8.0), (row, key, jump)
        o = ops.attention(bf(q).to(DEV), bf(k).to(DEV), bf(_vt(v)).to(DEV), H, D, scale, Lk=Lk)
        assert_close(o, ref, f"attention d512 spiked {tier}")
    finally:
        ops.set_compute_dtype(torch.bfloat16)


# ---- 3. lane-map probes, bit-exact ---------------------------------------------------------------------------------------------------------------

def test_lane_map_one_hot_pv(compute_dtype):
    """q = 0 makes every probability exactly 1; channel d of V^T holds ONE dyadic value, at key 37 d mod Lk (every key slot of the 32-key tile,
    every channel block of both workgroups of a query tile). O[., d] must be exactly value / Lk."""
    ops = _ops()
    Lq, Lk = 160, 1024
    vt = torch.zeros(1, D, Lk)
    want = torch.empty(D)
    for d in range(D):
        val = (-1) ** d * (1.0 + (d % 8) / 8) * 2.0 ** (d % 5 - 2)
        vt[0, d, (37 * d) % Lk] = val
        want[d] = val / Lk
    o = ops.attention(bf(torch.zeros(1, Lq, D)).to(DEV), bf(rnd(1, Lk, D, seed=3)).to(DEV), bf(vt).to(DEV), 1, D, D ** -0.5)
    assert torch.equal(o[0].float().cpu(), want.expand(Lq, D))


def test_lane_map_one_hot_qk(compute_dtype):
    """V^T = identity over 512 keys (O[., j] = P_j), k row j one-hot at head-dim position 53 j mod 512 (a bijection: every 16-byte chunk of every
    swizzled K row) with magnitude 2^(j mod 3), q small integers, scale = ln 2: key j's probability is 2^(q[53 j mod 512] 2^(j mod 3)) / sum, powers
    of two that the 16-bit P holds exactly. The output equals the float64 restatement up to its one rounding; an operand taken from the wrong
    lane, chunk or row moves a score by at least a factor of two."""
    ops = _ops()
    Lq, Lk = 96, 512
    i, d = torch.arange(Lq)[:, None], torch.arange(D)[None, :]
    q = ((i + d) % 4).float()[None]
    k = torch.zeros(1, Lk, D)
    pos = (53 * torch.arange(Lk)) % D
    k[0, torch.arange(Lk), pos] = 2.0 ** (torch.arange(Lk) % 3).float()
    vt = torch.eye(D)[None]
    o = ops.attention(bf(q).to(DEV), bf(k).to(DEV), bf(vt).to(DEV), 1, D, math.log(2.0))[0].double().cpu()
    s = q[0].double() @ k[0].double().T
    ref = torch.exp2(s - s.amax(-1, keepdim=True))
    ref = ref / ref.sum(-1, keepdim=True)
    assert float(ref.max() / ref.min()) > 30
    # one output rounding: a relative ulp, or - for the fp16 results below 2^-14 - half a step of fp16's subnormal grid (2^-24)
    ulp, floor = (2.0 ** -8, 0.0) if compute_dtype == "bf16" else (2.0 ** -11, 2.0 ** -25)
    assert bool(((o - ref).abs() <= ulp * ref + floor).all()), float(((o - ref).abs() / ref).max())


def test_constant_v_comes_out_unchanged(compute_dtype):
    ops = _ops()
    B, H, Lq, Lk = 2, 2, 130, 1000
    c = torch.tensor([(-1) ** d * (1.0 + (d % 7) / 8) * 2.0 ** (d % 5 - 2) for d in range(H * D)])
    vt = torch.zeros(B, H * D, 1000)
    vt[:] = c[None, :, None]
    o = ops.attention(bf(torch.zeros(B, Lq, H * D)).to(DEV), bf(rnd(B, Lk, H * D, seed=4)).to(DEV), bf(vt).to(DEV), H, D, D ** -0.5)
    assert torch.equal(o.float().cpu(), c.expand(B, Lq, -1))


# ---- 4. two-term-split q / k (accurate tier) -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_attention_d512_two_term_split_q_k(dt):
    """q_lo_off / k_lo_off at D = 512 (p_split = 0): S^T = K_hi Q_hi^T + K_lo Q_hi^T + K_hi Q_lo^T. Against float64 attention on the UNsplit q / k
    the split call (e3) beats the single-term call (e1) and is no more than 25 % above the materialised chain VaeAttention runs on the same split
    operands (bmm_nt(both_split) -> softmax_rows -> bmm_nt): both round P once to 16 bits and accumulate in fp32.
    Measured on MI355X: see the printed line (DESIGN 3.3 quotes it)."""
    ops = _ops()
    try:
        ops.set_compute_dtype(torch.float32, operand_dtype=dt)
        B, H, Lq, Lk = 2, 1, 1000, 1000
        Lp = 1024
        q = torch.randn(B, Lq, D, generator=_g(90)) * 1.5
        k = torch.randn(B, Lk, D, generator=_g(91)) * 1.5
        v = torch.randn(B, Lk, D, generator=_g(92)).to(dt)
        vt = torch.zeros(B, D, Lp, dtype=dt)
        vt[:, :, :Lk] = v.transpose(1, 2)
        sp = lambda t: torch.cat([t.to(dt), (t - t.to(dt).float()).to(dt)], -1)        # noqa: E731  [hi | lo], as a projection writes with out_split=2
        qq, kk, vtd = sp(q).to(DEV), sp(k).to(DEV), vt.to(DEV)
        ref = torch.softmax(q.double() @ k.double().transpose(1, 2) * D ** -0.5, -1) @ v.double()
        both = lambda o: o[..., :D].float() + o[..., D:].float()                        # noqa: E731
        single = ops.attention(qq[..., :D].contiguous(), kk[..., :D].contiguous(), vtd, H, D, D ** -0.5, Lk=Lk, out_split=2)
        with _Timing() as tm:
            split = ops.attention(qq, kk, vtd, H, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=D, k_lo_col=D, p_split=False)
        assert [(kind, var) for kind, var, _, _ in tm.entries] == [(2, 20)]
        s = ops.bmm_nt(qq, ops.split_rows_hhl(kk, Lp), alpha=D ** -0.5, out_dtype=ops.OUT_F32, both_split=True)
        mat = ops.bmm_nt(ops.softmax_rows(s, valid=Lk), vtd, out_split=2)
        e1, e3, em = _rel(both(single), ref), _rel(both(split), ref), _rel(both(mat), ref)
        print(f"attention d512 {Lq} x {Lk} {dt}: single q / k {e1:.3e}  split q / k {e3:.3e}  materialised chain on the split operands {em:.3e}")
        assert e3 < e1 and e3 <= 1.25 * em
        assert torch.equal(ops.attention(qq, kk, vtd, H, D, D ** -0.5, Lk=Lk, out_split=2, q_lo_col=D, k_lo_col=D, p_split=False), split)
        with pytest.raises(Exception):
            ops.attention(qq, kk, vtd, H, D, D ** -0.5, Lk=Lk, q_lo_col=D, p_split=False)            # one low half without the other
        with pytest.raises(ValueError):
            ops.attention(qq, kk, vtd, H, D, D ** -0.5, Lk=Lk, q_lo_col=D, k_lo_col=D)                # split P is a head_dim-64 form
    finally:
        ops.set_compute_dtype(torch.bfloat16)


# ---- 5. module parity at sizes both paths run ----------------------------------------------------------------------------------------------------

def _vae_attention(seed=80):
    from omgsr_amd.diffusers_api.autoencoder_kl import VaeAttention
    a = VaeAttention(D, 32)
    with torch.no_grad():
        for n, p_ in a.named_parameters():
            p_.copy_(torch.randn(p_.shape, generator=_g(seed + len(n))) * (1.7 * D ** -0.5 if ("to_q.weight" in n or "to_k.weight" in n) else D ** -0.5 if p_.dim() == 2 else 0.1))
        a.group_norm.weight.add_(1.0)
    return a


_REF64 = {}


def _module_ref64(a, x):
    """The block in float64 on the host: x [N, H, W, C] -> x + to_out(softmax(q k^T / sqrt C) v)."""
    N, H, W, C = x.shape
    xd = x.double().permute(0, 3, 1, 2)
    g = F.group_norm(xd, 32, a.group_norm.weight.double(), a.group_norm.bias.double(), 1e-6).reshape(N, C, H * W).transpose(1, 2)
    q, k, v = (F.linear(g, m.weight.double(), m.bias.double()) for m in (a.to_q, a.to_k, a.to_v))
    out = torch.empty_like(q)
    for n in range(N):
        for r0 in range(0, H * W, 2048):
            out[n, r0:r0 + 2048] = torch.softmax(q[n, r0:r0 + 2048] @ k[n].T * C ** -0.5, -1) @ v[n]
    o = F.linear(out, a.to_out[0].weight.double(), a.to_out[0].bias.double())
    return x.double() + o.reshape(N, H, W, C)


def _tiered(a, tier):
    """The module on the device in a tier; the accurate tier with the default policy's marks of decoder.mid_block.attentions.0."""
    from omgsr_amd.precision import apply_default_policy
    ops = _ops()
    wd = {"bf16": torch.bfloat16, "fp16": torch.float16, "accurate": torch.float32}[tier]
    ops.set_compute_dtype(wd)
    a = a.to(DEV, wd)
    if tier == "accurate":
        root = nn.Module()
        root.decoder = nn.Module()
        root.decoder.mid_block = nn.Module()
        root.decoder.mid_block.attentions = nn.ModuleList([a])
        apply_default_policy(vae=root)
        assert a.qk_split and a.to_q.in_split() == 2
    return a, wd


@pytest.mark.parametrize("tier", ["bf16", "fp16", "accurate"])
@pytest.mark.parametrize("hw", [64, 128])
def test_module_parity_fused_vs_materialised(tier, hw):
    """VaeAttention.nhwc, N = 2, C = 512: the fused and the materialised path each against the float64 host restatement on the same inputs; the
    fused rel-L2 may not exceed the materialised one by more than 25 % (both round P once to 16 bits and accumulate in fp32: two draws of the
    same size). With the switch unset the module takes the materialised path at these sizes, bit for bit."""
    import copy
    ops = _ops()
    try:
        a0 = _vae_attention()
        x = rnd(2, hw, hw, D, seed=81 + hw, scale=2.0)              # 16-bit representable: every tier's stream type holds it exactly
        if hw not in _REF64:
            t0 = time.perf_counter()
            with torch.no_grad():
                _REF64[hw] = _module_ref64(a0, x)
            print(f"float64 host restatement {hw} x {hw}: {time.perf_counter() - t0:.1f} s")
        want = _REF64[hw]
        a, wd = _tiered(copy.deepcopy(a0), tier)
        xd = x.to(DEV, wd)
        with torch.no_grad():
            assert a.fused is None
            with _Timing() as t_auto:
                auto = a.nhwc(xd)
            a.fused = False
            with _Timing() as t_mat:
                mat = a.nhwc(xd)
            a.fused = True
            with _Timing() as t_fused:
                fused = a.nhwc(xd)
        kinds = lambda tm: [(kind, var if kind == 2 else 0) for kind, var, _, _ in tm.entries if kind in (2, 6)]       # noqa: E731  attention / softmax
        assert kinds(t_auto) == kinds(t_mat) == [(6, 0)] and torch.equal(auto, mat)
        assert kinds(t_fused) == [(2, 20)]
        e_f, e_m = _rel(fused, want), _rel(mat, want)
        b_f, b_m = _rel(fused.double().cpu() - x.double(), want - x.double()), _rel(mat.double().cpu() - x.double(), want - x.double())
        print(f"VaeAttention {hw} x {hw} N=2 {tier}: output rel-L2 fused {e_f:.3e} materialised {e_m:.3e}; attention branch alone fused {b_f:.3e} materialised {b_m:.3e}")
        assert torch.isfinite(fused.float()).all() and e_f <= 1.25 * e_m
    finally:
        ops.set_compute_dtype(torch.bfloat16)


# ---- 6. past the old limit, end to end -----------------------------------------------------------------------------------------------------------

BOUNDS = {"fp32": (1e-3, 60.0), "bf16": (3e-2, 40.0)}         # tests/test_flux_fullsize_gpu.py BOUNDS (pipeline rel-L2, PSNR dB)


@pytest.fixture(scope="module")
def flux_vae_case():
    from omgsr_amd.diffusers_api import FLUX_VAE_CONFIG
    from omgsr_amd.testing import seeded_init_
    from oracle import diffusers_ref as R
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ov = seeded_init_(R.AutoencoderKL(**FLUX_VAE_CONFIG), 303, rounded=False).eval()        # full-mantissa weights
    z = torch.randn(1, 16, 128, 160, generator=_g(77))
    t0 = time.perf_counter()
    with torch.no_grad():
        ref = ov.decode(z).sample
    print(f"fp32 oracle, FLUX VAE decode of a 160 x 128 latent (1280 x 1024 pixels, 20480 tokens): {time.perf_counter() - t0:.1f} s")
    return dict(sd=ov.state_dict(), z=z, ref=ref)


@pytest.mark.parametrize("tier", ["fp32", "bf16"])
def test_untiled_flux_vae_decode_1280x1024_vs_oracle(flux_vae_case, tier):
    """L = 20480 > 16384: the mid-block attention runs as ONE launch of variant 20 and no softmax-kind launch; the image meets the tier's bound
    against the fp32 oracle."""
    from omgsr_amd.diffusers_api import AutoencoderKL, FLUX_VAE_CONFIG
    from omgsr_amd.precision import apply_default_policy
    from omgsr_amd.testing import psnr, rel_l2
    ops = _ops()
    c = flux_vae_case
    tol, min_psnr = BOUNDS[tier]
    wd = torch.float32 if tier == "fp32" else torch.bfloat16
    try:
        ops.set_compute_dtype(wd)
        p = AutoencoderKL(**FLUX_VAE_CONFIG)
        p.load_state_dict(c["sd"])
        p = p.to(DEV, wd).eval()
        if tier == "fp32":
            apply_default_policy(vae=p)
        with torch.no_grad(), _Timing() as tm:
            got = p.decode(c["z"].to(DEV, wd)).sample
        got = got.float().cpu()
    finally:
        ops.set_compute_dtype(torch.bfloat16)
    attn = [(kind, var) for kind, var, _, _ in tm.entries if kind in (2, 6)]
    e, ps = rel_l2(got, c["ref"]), psnr(got, c["ref"])
    print(f"untiled FLUX VAE decode 1280 x 1024, {tier}: rel-L2 {e:.3e} PSNR {ps:.1f} dB (bounds {tol:g} / {min_psnr} dB)")
    assert attn == [(2, 20)]
    assert got.shape == c["ref"].shape and torch.isfinite(got).all()
    assert e <= tol and ps >= min_psnr


# ---- 7. 2048^2 at kernel level -------------------------------------------------------------------------------------------------------------------

def test_attention_d512_65536_keys():
    """Lq = Lk = 65536 (a 2048^2 image's latent tokens), B = 1, bf16: 64-bit indexing and a grid of 512 query tiles x 2. Reference on the host for
    512 sampled query rows (the first and the last query tile included)."""
    ops = _ops()
    ops.set_compute_dtype(torch.bfloat16)
    L = 65536
    q, k, v = rnd(1, L, D, seed=41), rnd(1, L, D, seed=42), rnd(1, L, D, seed=43)
    rows = torch.cat([torch.arange(0, 128), torch.arange(L - 128, L), torch.randperm(L - 256, generator=_g(44))[:256] + 128])
    ref = torch.softmax(q[0, rows] @ k[0].T * D ** -0.5, -1) @ v[0]
    o = ops.attention(bf(q).to(DEV), bf(k).to(DEV), bf(v.transpose(1, 2).contiguous()).to(DEV), 1, D, D ** -0.5)
    assert torch.isfinite(o.float()).all()
    assert_close(o[0, rows.to(DEV)], ref, "attention d512 65536 x 65536 (512 sampled rows)")


# ---- 8. repeatability, batch invariance, graph replay --------------------------------------------------------------------------------------------

def test_repeatable(compute_dtype):
    ops = _ops()
    B, H, Lq, Lk = 2, 1, 4096, 4090
    q, k, vt = bf(rnd(B, Lq, D, seed=51)).to(DEV), bf(rnd(B, Lk, D, seed=52)).to(DEV), bf(_vt(rnd(B, Lk, D, seed=53))).to(DEV)
    first = ops.attention(q, k, vt, H, D, D ** -0.5, Lk=Lk)
    for _ in range(49):
        assert torch.equal(ops.attention(q, k, vt, H, D, D ** -0.5, Lk=Lk), first)


@pytest.mark.parametrize("tier", ["bf16", "accurate"])
def test_module_batch_invariant(tier):
    ops = _ops()
    try:
        a, wd = _tiered(_vae_attention(), tier)
        a.fused = True
        x = (torch.randn(2, 40, 36, D, generator=_g(61)) * 2).to(DEV, wd)
        ops.set_batch_invariant(True)
        with torch.no_grad():
            both, one, two = a.nhwc(x), a.nhwc(x[0:1].contiguous()), a.nhwc(x[1:2].contiguous())
        assert torch.equal(both[0:1], one) and torch.equal(both[1:2], two)
    finally:
        ops.set_batch_invariant(False)
        ops.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("wd", [torch.float32, torch.bfloat16], ids=["accurate", "bf16"])
def test_omgsr_s_fused_vae_attention_graph_replay_equals_eager(wd):
    from omgsr_amd.diffusers_api import AutoencoderKL, UNet2DConditionModel
    from omgsr_amd.pipelines.omgsr_s import OMGSR_S_Infer
    from omgsr_amd.testing import seeded_init_, synthetic_lq
    ops = _ops()
    try:
        vcfg = dict(block_out_channels=[32, 64, 128, 512], layers_per_block=1)            # a 512-wide mid block: the fused kernel's head size
        ucfg = dict(block_out_channels=[64, 128, 256, 256], attention_head_dim=[1, 2, 4, 4], cross_attention_dim=128)
        v, u = seeded_init_(AutoencoderKL(**vcfg), 1, rounded=False), seeded_init_(UNet2DConditionModel(**ucfg), 2, rounded=False)
        pipe = OMGSR_S_Infer(None, None, 273, DEV, wd, vae=v, unet=u)
        g = _g(5)
        prompt = torch.randn(1, 77, 128, generator=g).to(device=DEV, dtype=wd)
        pipe.vae.posterior_noise = torch.randn(2, 4, 24, 24, generator=g).to(DEV)
        xs = [synthetic_lq(2, 192, 192, seed=s).to(device=DEV, dtype=wd) for s in (1, 2, 3)]
        with torch.no_grad():
            default = pipe(xs[0], prompt, 32, 8)[0]
            pipe.vae.set_fused_attention(True)
            with _Timing() as tm:
                eager = [pipe(x, prompt, 32, 8)[0] for x in xs]
            attn = [var for kind, var, _, _ in tm.entries if kind == 2 and var == 20]
            assert len(attn) == 2 * len(xs) and not any(kind == 6 for kind, _, _, _ in tm.entries)       # encoder + decoder mid block per call
            assert not torch.equal(eager[0], default) and float((eager[0].float() - default.float()).norm() / default.float().norm()) < 0.05
            pipe.enable_graphs(True)
            got = [pipe(x, prompt, 32, 8)[0] for x in xs]
            assert pipe.graphs.captures == 1 and pipe.graphs.replays == 2
            for e, r in zip(eager, got):
                assert torch.equal(e, r)
            pipe.enable_graphs(False)
            pipe.vae.set_fused_attention(None)
            assert torch.equal(pipe(xs[0], prompt, 32, 8)[0], default)
    finally:
        ops.set_compute_dtype(torch.bfloat16)


# ---- 9. the range-fallback tier's message --------------------------------------------------------------------------------------------------------

def test_range_fallback_tier_names_its_limit():
    ops = _ops()
    try:
        ops.set_compute_dtype(torch.float32, operand_dtype=torch.bfloat16)
        assert ops.attn_split()
        a = _vae_attention().to(DEV, torch.float32)
        x = torch.randn(1, 128, 160, D, generator=_g(71)).to(DEV)
        for mode in (None, True):
            a.fused = mode
            with pytest.raises(ValueError, match="range-fallback VAE attention is limited to 16384 keys"):
                with torch.no_grad():
                    a.nhwc(x)
    finally:
        ops.set_compute_dtype(torch.bfloat16)
