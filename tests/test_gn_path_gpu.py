"""The tiled VAE's GroupNorm launches: omgsr_groupnorm_apply_multi (every tile-shape group of a layer in one apply launch) must write
the bytes of one omgsr_groupnorm_apply_shared call per group, and the 16-wave omgsr_groupnorm_finalize_merged fold must give the bits of
the four-wave kernel it replaces (same summation tree) - at the encoder's and the decoder's real group shapes of the 256 -> 1024
workload (encoder tile 256 on a 1024^2 image, decoder tile 64 on a 128^2 latent)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 32


def _ops():
    from omgsr_amd import ops
    return ops


@pytest.fixture
def accurate():
    ops = _ops()
    ops.set_compute_dtype(torch.float32)          # fp32 stream tensors, fp16 operands: every operand form exists
    yield ops
    ops.set_compute_dtype(torch.bfloat16)


def _group_shapes(net):
    """{(h, w): tiles} of the tiles' input boxes, the way VAEHook.vae_tile_forward stacks them."""
    from omgsr_amd.pipelines.vaehook import split_tiles
    ins, _ = split_tiles(128, 128, 64, 11, True) if net == "decoder" else split_tiles(1024, 1024, 256, 32, False)
    shapes = {}
    for b in ins:
        k = (b[3] - b[2], b[1] - b[0])
        shapes[k] = shapes.get(k, 0) + 1
    return shapes


def _levels(net):
    """(scale numerator, denominator, channels) of the net's GroupNorm inputs (SD2.1 VAE widths)."""
    if net == "decoder":
        return [(1, 1, 512), (2, 1, 512), (4, 1, 256), (8, 1, 256), (8, 1, 128)]
    return [(1, 1, 128), (1, 2, 128), (1, 2, 256), (1, 4, 256), (1, 4, 512), (1, 8, 512)]


def test_real_group_shapes():
    assert _group_shapes("decoder") == {(86, 86): 1, (86, 64): 1, (64, 86): 1, (64, 64): 1}
    assert _group_shapes("encoder") == {(320, 320): 9, (320, 256): 3, (256, 320): 3, (256, 256): 1}


# (split of the normalised operand, form of the shortcut twin or 0): plain / two-term split / MX / MX6 operands, each twin form
FORMS = [(1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (2, 2), (3, 3), (4, 3), (4, 2), (4, 1), (3, 1), (2, 1)]


@pytest.mark.parametrize("net", ["encoder", "decoder"])
def test_multi_group_apply_writes_the_bytes_of_the_per_group_calls(accurate, net):
    ops = accurate
    N = 2
    gen = torch.Generator(device=DEV).manual_seed(11)
    shapes = _group_shapes(net)
    checked = 0
    for li, (num, den, Cc) in enumerate(_levels(net)):
        xs = [torch.randn((t * N, h * num // den, w * num // den, Cc), device=DEV, generator=gen) * 3.0 + 0.5 for (h, w), t in shapes.items()]
        mean = torch.randn((N, G), device=DEV, generator=gen) * 0.3
        rstd = torch.rand((N, G), device=DEV, generator=gen) + 0.2
        gamma = torch.randn(Cc, device=DEV, generator=gen) + 1.0
        beta = torch.randn(Cc, device=DEV, generator=gen)
        for split, twin in (FORMS if li % 2 == 0 else FORMS[3::4]):      # every form on every other level, the fp6 ones on all
            act = ops.ACT_SILU if (split + twin) % 2 == 0 else ops.ACT_NONE
            ref = [ops.group_norm_apply_shared(x, mean, rstd, gamma, beta, G, act, split=split, also_cast=twin) for x in xs]
            got = ops.group_norm_apply_multi(xs, mean, rstd, gamma, beta, G, act, split=split, also_cast=twin)
            again = ops.group_norm_apply_multi(xs, mean, rstd, gamma, beta, G, act, split=split, also_cast=twin)
            for k, (r, g2, g3) in enumerate(zip(ref, got, again)):
                for name, a, b, c in zip(("y", "y2"), r if twin else (r,), g2 if twin else (g2,), g3 if twin else (g3,)):
                    assert a.shape == b.shape and a.dtype == b.dtype
                    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{net} level {li} C {Cc} split {split} twin {twin} group {k} {name}"
                    assert torch.equal(b.view(torch.int16), c.view(torch.int16)), f"repeat: {net} level {li} split {split} twin {twin} group {k} {name}"
            checked += 1
    print(f"{net}: {checked} (level, form) cases byte-equal over {len(shapes)} shape groups")
    assert not ops.overflow_seen()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_multi_group_apply_16bit_stream(dt):
    """The fast tiers' stream tensors (a GroupNorm in front of a 1x1 projection: the VAE attention's) take the multi launch too."""
    ops = _ops()
    ops.set_compute_dtype(dt)
    try:
        gen = torch.Generator(device=DEV).manual_seed(12)
        N, Cc = 2, 512
        xs = [(torch.randn((t * N, h, w, Cc), device=DEV, generator=gen) * 2.0).to(dt) for (h, w), t in _group_shapes("decoder").items()]
        mean = torch.randn((N, G), device=DEV, generator=gen) * 0.3
        rstd = torch.rand((N, G), device=DEV, generator=gen) + 0.2
        gamma, beta = torch.randn(Cc, device=DEV, generator=gen) + 1.0, torch.randn(Cc, device=DEV, generator=gen)
        for split, twin in [(1, 0), (1, 1)] + ([(2, 0)] if dt == torch.float16 else []):
            ref = [ops.group_norm_apply_shared(x, mean, rstd, gamma, beta, G, ops.ACT_NONE, split=split, also_cast=twin) for x in xs]
            got = ops.group_norm_apply_multi(xs, mean, rstd, gamma, beta, G, ops.ACT_NONE, split=split, also_cast=twin)
            for r, g2 in zip(ref, got):
                for a, b in zip(r if twin else (r,), g2 if twin else (g2,)):
                    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (dt, split, twin)
    finally:
        ops.set_compute_dtype(torch.bfloat16)


def test_multi_group_apply_rejects_bad_arguments(accurate):
    ops = accurate
    x = torch.zeros((2, 8, 8, 64), device=DEV)
    st = torch.zeros((2, G), device=DEV)
    with pytest.raises(ValueError):
        ops.group_norm_apply_multi([x] * 9, st, st, None, None, G)
    with pytest.raises(ValueError):
        ops.group_norm_apply_multi([x, torch.zeros((2, 8, 8, 128), device=DEV)], st, st, None, None, G)
    from omgsr_amd._lib import OmgsrError
    with pytest.raises(OmgsrError):          # rows not a multiple of the statistics rows
        ops.group_norm_apply_multi([torch.zeros((3, 8, 8, 64), device=DEV)], st, st, None, None, G)


# ---- omgsr_groupnorm_finalize_merged -------------------------------------------------------------------------------------------

def _merge_case(net, Cc, entries, N, seed):
    """Partials [rows][nslot][entries][2] of every shape group as a producing conv leaves them (slot counts differ per group)."""
    gen = torch.Generator().manual_seed(seed)
    shapes = _group_shapes(net)
    tot = float(sum(h * w * t for (h, w), t in shapes.items()))
    parts, meta = [], []
    for i, ((h, w), t) in enumerate(shapes.items()):
        nslot = (h * w + 255) // 256 + i                  # a halo tile per 256 pixels, and a count no other group has
        px = h * w / nslot
        s = torch.randn(t * N, nslot, entries, generator=gen) * px * 0.4
        q = (torch.rand(t * N, nslot, entries, generator=gen) + 0.5) * px * 2.0
        parts.append(torch.stack([s, q], -1).contiguous())
        meta.append((t, nslot, float(h * w * (Cc // G)), h * w / tot))
    return parts, meta


def _run_merge(parts, meta, N, entries):
    from omgsr_amd import _lib
    dev = [p.to(DEV) for p in parts]
    a = _lib.GnMergeArgs()
    for k, (p, (t, nslot, count, wgt)) in enumerate(zip(dev, meta)):
        a.partial[k], a.nslot[k], a.entries[k], a.tiles[k], a.count[k], a.weight[k] = p.data_ptr(), nslot, entries, t, count, wgt
    a.ngroups = len(dev)
    out = torch.empty((3, N, G), device=DEV)
    _lib.check(_lib.load().omgsr_groupnorm_finalize_merged(C.byref(a), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), N, G, 1e-6, None),
               "omgsr_groupnorm_finalize_merged")
    torch.cuda.synchronize()
    return out.cpu()


MERGE_CASES = [("encoder", 128, 128), ("encoder", 512, 512), ("encoder", 256, G), ("decoder", 512, 512), ("decoder", 128, G)]


def _merge_all(N=4):
    outs = []
    for i, (net, Cc, entries) in enumerate(MERGE_CASES):
        parts, meta = _merge_case(net, Cc, entries, N, 500 + i)
        outs.append(_run_merge(parts, meta, N, entries))
    return outs


def test_merged_finalize_matches_the_weighted_merge_and_the_four_wave_kernel(tmp_path):
    N = 4
    outs, again = _merge_all(N), _merge_all(N)
    for i, (net, Cc, entries) in enumerate(MERGE_CASES):
        parts, meta = _merge_case(net, Cc, entries, N, 500 + i)
        mean = torch.zeros(N, G, dtype=torch.float64); var = torch.zeros(N, G, dtype=torch.float64)
        for p, (t, nslot, count, wgt) in zip(parts, meta):
            sq = p.double().view(t, N, nslot, G, entries // G, 2).sum((2, 4))           # [t, N, G, 2]
            m = sq[..., 0] / count
            v = (sq[..., 1] / count - m * m).clamp_min(0.0)
            mean += float(torch.tensor(wgt, dtype=torch.float32)) * m.sum(0)
            var += float(torch.tensor(wgt, dtype=torch.float32)) * v.sum(0)
        got = outs[i].double()
        assert torch.allclose(got[0], mean, rtol=1e-6, atol=1e-6), (net, Cc, entries)
        assert torch.allclose(got[2], var, rtol=1e-6, atol=1e-6), (net, Cc, entries)
        assert torch.allclose(got[1], torch.rsqrt(var + 1e-6), rtol=1e-6), (net, Cc, entries)
        assert torch.equal(outs[i], again[i]), "repeated launches differ"
    # the four-wave kernel (OMGSR_GN_MERGE_NARROW=1 is read once per process: a fresh child) must give the same BITS
    script = ("import sys, torch; sys.path[:0] = [%r, %r]; import test_gn_path_gpu as t; torch.save(t._merge_all(), %r)"
              % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path / "narrow.pt")))
    subprocess.run([sys.executable, "-c", script], check=True, timeout=300, env=dict(os.environ, OMGSR_GN_MERGE_NARROW="1"))
    narrow = torch.load(tmp_path / "narrow.pt")
    for i, case in enumerate(MERGE_CASES):
        assert torch.equal(outs[i].view(torch.int32), narrow[i].view(torch.int32)), f"{case}: the 16-wave fold moved bits against the four-wave fold"
