"""Border waves of the tiled mode-3 compose kernel (compose3_xpose_kernel, streaming layout) at the smallest shapes that hold
each hazard of gathering a lane's pixel PAIR per round trip (c3_border_pair; QUANT_EXACT keeps the one-pixel loop), bit-exact
against the C oracle:

  (2, 16, 256)  whole tiles, two tile rows and columns, the second field's bases
  (2, 13, 130)  ragged both ways; W & 3 != 0, so the 2-byte mask store; pair group 1 inactive in the last tile column
  (1, 1, 128)   H < 2: every wave is a border wave and both tap rows clamp to row 0
  (1, 9, 2)     the narrowest even width: the clamped column is always 0

The cases prove their own reach WITHOUT a device (test_cases_reach_every_border_combination): the kernel's classification is
restated in NumPy below, and the pixels of the cases' border waves must show all 20 combinations of (column class, tap row 0
in the source, tap row 1 in the source), and border waves with pair group 0 / pair group 1 / neither wholly outside."""
import functools

import numpy as np
import pytest

QUANT_OPENCV, QUANT_EXACT = 0, 1
SHAPES = [(2, 16, 256), (2, 13, 130), (1, 1, 128), (1, 9, 2)]
TILE_W, TILE_H, XPOSE_ROWS = 128, 8, 6       # kC3TileW, kC3TileH (ofl_compose3.hip), kXposeRows (ofl_pairs.h)
COLUMN_CLASSES = ("left", "d-1", "d0", "d+1", "right")


def _sampling_fields(H, W):
    """name -> sampling field [H][W][2].  All keep the streaming layout: the vertical flow is constant along every row."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = {}
    # translations: half-pixel ones on one axis, integer ones (both fractions zero for c3_valid), half-pixel ones on both
    for u, v in [(1.5, 0), (-1.5, 0), (0, 1.5), (0, -1.5), (1, 1), (1, -1), (-1, 1), (-1, -1),
                 (0.5, 0.5), (0.5, -0.5), (-0.5, 0.5), (-0.5, -0.5)]:
        f = np.empty((H, W, 2), np.float32)
        f[..., 0], f[..., 1] = u, v
        out["shift({:+g},{:+g})".format(u, v)] = f
    # a row-wise step and its mirror: far-outside and inside pixels in one wave (the far half leaves on either sign)
    for name, far in (("step", xx < W // 2), ("step_mirror", xx >= W // 2)):
        f = np.full((H, W, 2), 0.25, np.float32)
        f[..., 0][far] = W + 3
        out[name] = f
    # 1.2 x magnification of the sample positions about an off-centre point (the benchmark's pattern in small), for either sign
    cx, cy = np.float32(0.3 * W), np.float32(0.4 * H)
    f = np.stack([np.float32(0.2) * (xx - cx), np.float32(0.2) * (yy - cy)], -1).astype(np.float32)
    out["magnify(sign+1)"], out["magnify(sign-1)"] = f, -f
    return out


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """(fa, ma, {name: fb}, mb) of one shape; computed once, shared, never written to"""
    rng = np.random.default_rng([B, H, W])
    fa = (rng.standard_normal((B, H, W, 2)) * 4).astype(np.float32)
    ma = (rng.random((B, H, W)) > 0.3).astype(np.uint8)           # about 30 % zeros
    mb = (rng.random((B, H, W)) > 0.5).astype(np.uint8)
    fbs = {k: np.broadcast_to(f, (B, H, W, 2)).copy() for k, f in _sampling_fields(H, W).items()}
    for x in (fa, ma, mb, *fbs.values()):
        x.setflags(write=False)
    return fa, ma, fbs, mb


# ------------------------------------------------------------------------- the kernel's classification, restated (QUANT_OPENCV)
def _taps(p):
    """c3_tap<QUANT_OPENCV>: top-left tap of float32 positions, rint(32 p) >> 5"""
    return np.rint(p * np.float32(32.0)).astype(np.int64) >> 5


def _reach(fb, sign):
    """One field fb [H][W][2] -> (set of (column class, row 0 in range, row 1 in range) over the active pixels of its border
    waves, set of 'g0' / 'g1' / 'none' over its border waves: which pair group is wholly outside or inactive)"""
    H, W = fb.shape[:2]
    ty_n, tx_n = -(-H // TILE_H), -(-W // TILE_W)
    hp, wp = ty_n * TILE_H, tx_n * TILE_W
    f = np.zeros((hp, wp, 2), np.float32)
    f[:H, :W] = fb
    xx = np.arange(wp, dtype=np.float32)[None, :]
    yy = np.arange(hp, dtype=np.float32)[:, None]
    ix = _taps(xx + f[..., 0] if sign >= 0 else xx - f[..., 0])      # c3_pos: one float32 operation
    iy = _taps(yy + f[..., 1] if sign >= 0 else yy - f[..., 1])
    act = (np.arange(hp)[:, None] < H) & (np.arange(wp)[None, :] < W)
    in_j = (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= H - 2) & (H >= 2)      # c3_classify; H < 2 is never inside
    out_j = (ix < -1) | (ix >= W) | (iy < -1) | (iy >= H)
    # the streaming layout (kernel body): |dv| over the tile's first row * 128 <= kXposeRows * its width
    for ty in range(ty_n):
        for tx in range(tx_n):
            x0, x1, y0 = tx * TILE_W, min(tx * TILE_W + TILE_W - 1, W - 1), min(ty * TILE_H, H - 1)
            assert not np.float32(abs(fb[y0, x1, 1] - fb[y0, x0, 1])) * np.float32(128.0) > np.float32(XPOSE_ROWS * (x1 - x0 + 1))

    def waves(a, cols=TILE_W):                # all() over a wave = tile rows (2 k, 2 k + 1) x 128 px, or over its 64-px halves
        return a.reshape(ty_n * 4, 2, wp // cols, cols).all(axis=(1, 3))
    outside = waves(out_j | ~act)
    border = ~outside & ~waves(in_j | ~act)
    d = ix - np.clip(ix, 0, max(W - 2, 0))    # c3_border_px: the tap column against its clamped load column
    cls = np.digitize(d, [-1, 0, 1, 2])       # 0: d < -1, 1: d = -1, 2: d = 0, 3: d = +1, 4: d > +1
    r0, r1 = (iy >= 0) & (iy < H), (iy + 1 >= 0) & (iy + 1 < H)
    px = act & np.repeat(np.repeat(border, 2, axis=0), TILE_W, axis=1)
    combos = {(COLUMN_CLASSES[c], bool(a), bool(b)) for c, a, b in zip(cls[px], r0[px], r1[px])}
    half_out = waves(out_j | ~act, 64)        # (wave row, 64-px half): pair group g of tile column t is half 2 t + g
    groups = set()
    for wy, tx in zip(*np.nonzero(border)):
        g0, g1 = half_out[wy, 2 * tx], half_out[wy, 2 * tx + 1]
        groups.add("g0" if g0 else "g1" if g1 else "none")      # (both would be an outside wave, not a border wave)
    return combos, groups


def test_cases_reach_every_border_combination():
    """No device: the union over the cases holds all 5 x 2 x 2 combinations and all three pair-group situations."""
    combos, groups, per_shape = set(), set(), {}
    for B, H, W in SHAPES:
        here = set()
        for name, fb in _case(B, H, W)[2].items():
            for sign in (-1, 1):
                c, g = _reach(fb[0], sign)
                here |= c
                groups |= g
        per_shape[(B, H, W)] = here
        combos |= here
    want = {(c, a, b) for c in COLUMN_CLASSES for a in (False, True) for b in (False, True)}
    assert combos == want, sorted(want - combos)
    assert groups == {"g0", "g1", "none"}, groups
    # what each small shape is there for
    assert all(not (a and b) for _, a, b in per_shape[(1, 1, 128)])                   # H < 2: never both tap rows in the source
    assert {c for c, _, _ in per_shape[(1, 9, 2)]} == set(COLUMN_CLASSES)              # W = 2: every class at load column 0


# ------------------------------------------------------------------------------------------------------------ on the device
def _launch(of, fa, ma, fb, mb, sign, quant, stats_on):
    """ofl_compose3_dev on device-resident stacks -> (vectors, mask, flag words or None): with a flag-word buffer the launch
    is compose3_xpose_kernel<quant, true>, without one <quant, false>"""
    from oflibnumpy_amd import device as dev
    nat, lib = of.native, of.native.load()
    B, H, W = fa.shape[:3]
    bufs = [dev.DeviceBuffer.from_host(x) for x in (fa, ma, fb, mb)]
    out, mout = dev.DeviceBuffer(fa.nbytes), dev.DeviceBuffer(ma.nbytes)
    stats = dev.DeviceBuffer.zeros(B * 8 * 4) if stats_on else None
    nat.check(lib.ofl_compose3_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, sign, H, W, B, out.ptr, mout.ptr,
                                   stats.ptr if stats_on else None, quant, None))
    return (out.to_host((B, H, W, 2), np.float32), mout.to_host((B, H, W), np.uint8),
            stats.to_host((B, 8), np.uint32) if stats_on else None)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_compose3_border_pairs_bit_exact(gpu, oracle, B, H, W):
    of = gpu
    fa, ma, fbs, mb = _case(B, H, W)
    for name, fb in fbs.items():
        zero = {(b, th): oracle.is_zero_raw(fb[b], mb[b], th) for b in range(B) for th in (False, True)}
        zero_all = {(b, th): oracle.is_zero_raw(fb[b], None, th) for b in range(B) for th in (False, True)}
        for quant in (QUANT_OPENCV, QUANT_EXACT):
            for sign in (-1, 1):
                want = [oracle.compose3_raw(fa[b], ma[b], fb[b], mb[b], sign, quant) for b in range(B)]
                for stats_on in (True, False):
                    res, msk, words = _launch(of, fa, ma, fb, mb, sign, quant, stats_on)
                    for b in range(B):
                        where = (name, quant, sign, stats_on, b)
                        o, m = want[b]
                        np.testing.assert_array_equal(res[b].view(np.uint32), o.view(np.uint32), err_msg=str(where))
                        np.testing.assert_array_equal(msk[b], m.astype(np.uint8), err_msg=str(where))
                        if not stats_on:
                            continue
                        w = [bool(x) for x in words[b]]
                        # fb: words 4 .. 7 exact; words 2 / 3 are not the kernel's
                        assert w[4:8] == [not zero[b, False], not zero[b, True], not zero_all[b, False], not zero_all[b, True]], (where, words[b])
                        assert not w[2] and not w[3], (where, words[b])
                        # fa: words 0 / 1 are certificates -- a set word means the oracle finds the masked fa non-zero
                        if w[0]:
                            assert not oracle.is_zero_raw(fa[b], ma[b], False), (where, words[b])
                        if w[1]:
                            assert not oracle.is_zero_raw(fa[b], ma[b], True), (where, words[b])
