"""The tiled mode-3 compose kernel (ofl_compose3_dev -> compose3_xpose_kernel) on every path it takes, bit-exact against
the C oracle: waves wholly outside, wholly inside and on the border of the sampled field, the transposed (rotated) form,
whole and ragged tiles, batches whose tile rows straddle field boundaries, clamping flows, and one 8K field."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _flows(kind, B, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    if kind == "random":                     # border and interior waves mixed
        return (rng.standard_normal((B, H, W, 2)) * 6).astype('f')
    if kind == "shift":                      # every tap inside: interior path, shared mask loads
        f = np.zeros((B, H, W, 2), 'f')
        f[..., 0], f[..., 1] = 1.3, 0.6
        return f
    if kind == "outside":                    # every tap outside: nothing gathered
        return np.full((B, H, W, 2), 3.0e4, 'f')
    if kind == "rotate":                     # rotated sampling grid: the transposed form (far beyond 6 rows per 128 px)
        a = np.deg2rad(35.0)
        cx, cy = W / 2.0, H / 2.0
        u = (np.cos(a) - 1) * (xx - cx) - np.sin(a) * (yy - cy)
        v = np.sin(a) * (xx - cx) + (np.cos(a) - 1) * (yy - cy)
        return np.broadcast_to(np.stack([u, v], -1), (B, H, W, 2)).astype('f').copy()
    if kind == "clamp":                      # huge flows of both signs on both axes
        f = (rng.standard_normal((B, H, W, 2)) * 1.0e5).astype('f')
        f[:, ::3, ::2] *= 1e-4
        return f
    raise ValueError(kind)


def _run(of, oracle, fa, ma, fb, mb, sign, quant, stats_on, all_gathered=False):
    """ofl_compose3_dev on device-resident stacks: with a flag-word buffer the launch is compose3_xpose_kernel<Q, true>,
    whose words are checked against the oracle (fb: words 4..7 exact; fa: words 0/1 are certificates -- a set word means
    the oracle finds the masked fa non-zero; words 2/3 are not the kernel's); without one it is <Q, false>."""
    from oflibnumpy_amd import device as dev
    nat, lib = of.native, of.native.load()
    B, H, W = fa.shape[:3]
    bufs = [dev.DeviceBuffer.from_host(x) for x in (fa, ma, fb, mb)]
    out, mout = dev.DeviceBuffer(fa.nbytes), dev.DeviceBuffer(ma.nbytes)
    stats = dev.DeviceBuffer.zeros(B * 8 * 4) if stats_on else None
    nat.check(lib.ofl_compose3_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, sign, H, W, B, out.ptr, mout.ptr,
                                   stats.ptr if stats_on else None, quant, None))
    res = out.to_host((B, H, W, 2), np.float32)
    msk = mout.to_host((B, H, W), np.uint8)
    words = stats.to_host((B, 8), np.uint32) if stats_on else None
    S = nat
    for b in range(B):
        o, m = oracle.compose3_raw(fa[b], ma[b], fb[b], mb[b], sign, quant)
        np.testing.assert_array_equal(res[b], o)
        np.testing.assert_array_equal(msk[b].astype(bool), m)
        if not stats_on:
            continue
        w = [bool(x) for x in words[b]]
        assert w[4] == (not oracle.is_zero_raw(fb[b], mb[b], False)), (b, words[b])
        assert w[5] == (not oracle.is_zero_raw(fb[b], mb[b], True)), (b, words[b])
        assert w[6] == (not oracle.is_zero_raw(fb[b], None, False)), (b, words[b])
        assert w[7] == (not oracle.is_zero_raw(fb[b], None, True)), (b, words[b])
        assert not w[2] and not w[3], (b, words[b])
        if w[0]:
            assert not oracle.is_zero_raw(fa[b], ma[b], False), (b, words[b])
        if w[1]:
            assert not oracle.is_zero_raw(fa[b], ma[b], True), (b, words[b])
        if not fa[b].any():
            assert not w[0] and not w[1], (b, words[b])
        elif all_gathered:                    # nearly every pixel gathers in bounds: the masked, non-zero fa is observed
            assert w[0] and w[1], (b, words[b])


@pytest.mark.parametrize("B,H,W", [(2, 16, 256), (3, 21, 200), (2, 13, 130), (1, 40, 384)])
@pytest.mark.parametrize("kind", ["random", "shift", "outside", "rotate", "clamp"])
def test_compose3_paths_bit_exact(gpu, oracle, B, H, W, kind):
    of = gpu
    rng = np.random.default_rng([B, H, W, len(kind)])
    fa = (rng.standard_normal((B, H, W, 2)) * 4).astype('f')
    fb = _flows(kind, B, H, W, rng)
    ma = (rng.random((B, H, W)) > 0.1).astype(np.uint8)
    mb = (rng.random((B, H, W)) > 0.1).astype(np.uint8)
    if B > 1:
        fa[1] = 0                            # one sampled field exactly zero (flag words stay clear)
    for quant in (of.native.QUANT_OPENCV, of.native.QUANT_EXACT):
        for sign in (-1, 1):
            for stats_on in (True, False):
                _run(of, oracle, fa, ma, fb, mb, sign, quant, stats_on, all_gathered=(kind == "shift"))


def test_compose3_8k_field(gpu, oracle):
    """7680 x 4320: the 32-bit field offsets near their largest values in a real size (rotated and scaled grids)."""
    of = gpu
    H, W = 4320, 7680
    f1 = of.Flow.from_transforms([['rotation', W / 2.0, H / 2.0, -30]], [H, W], 't')
    f2 = of.Flow.from_transforms([['scaling', W * 0.2, H * 0.3, 0.8]], [H, W], 't')
    rng = np.random.default_rng(8)
    m1, m2 = rng.random((H, W)) > 0.05, rng.random((H, W)) > 0.05
    for fa, fb in ((f1.vecs, f2.vecs), (f2.vecs, f1.vecs)):
        _run(of, oracle, fa[None].copy(), m1[None].astype(np.uint8), fb[None].copy(), m2[None].astype(np.uint8),
             -1, of.native.QUANT_OPENCV, True)
