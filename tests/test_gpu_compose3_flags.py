"""The zero-flow flag words of ofl_compose3_dev (compose3_xpose_kernel<Q, STATS=true>), word for word against predicates
computed in NumPy from the inputs.

A wave reads its field's flag row once at its top and only stores at its end ("Zero-flow early exits"), so what
is checked here is the row after the launch, never the order of anything inside it:
  words 4..7   exact predicates of fb / mb (non-zero where masked, >= 1e-3 where masked, non-zero anywhere, >= 1e-3 anywhere);
  words 0/1    certificates for fa / ma: set only if a masked vector of fa is non-zero / >= 1e-3, and SET when every such
               vector is gathered as a pixel's top-left tap (fb zero, or a shift below one pixel with fa's content interior);
  words 2/3    never written;
  a word that is 1 before the launch is 1 after it: pre-set rows, and two launches into one row without zeroing.
The rotated cases take the transposed layout (fb is a 35 degree rotation field wherever the case leaves fb free).  Values
only: nothing here can fault."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TH = np.float32(1e-3)
SIZES = [(50, 258), (64, 256)]            # ragged tiles / whole tiles (the field's last pixel is the last lane of the last wave)


def _rotation(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.deg2rad(35.0)
    cx, cy = W / 2.0, H / 2.0
    u = (np.cos(a) - 1) * (xx - cx) - np.sin(a) * (yy - cy)
    v = np.sin(a) * (xx - cx) + (np.cos(a) - 1) * (yy - cy)
    return np.stack([u, v], -1).astype('f')


def _free_fb(layout, H, W):
    """fb where the case does not prescribe it: a shift below one pixel (streaming layout) or a rotation (transposed)."""
    if layout == "rot":
        return _rotation(H, W)
    f = np.zeros((H, W, 2), 'f')
    f[..., 0], f[..., 1] = 0.3, 0.3
    return f


def _interior_fa(H, W, rng):
    """fa whose non-zero, masked content lies away from the edges, so that a sub-pixel shift gathers all of it."""
    fa = np.zeros((H, W, 2), 'f')
    fa[8:H - 8, 8:W - 8] = (rng.standard_normal((H - 16, W - 16, 2)) * 4).astype('f')
    return fa


def _case(name, layout, H, W, rng):
    """-> fa, ma, fb, mb, gathered (every masked vector of fa is some pixel's top-left tap)"""
    fa = _interior_fa(H, W, rng)
    ma = (rng.random((H, W)) > 0.1).astype(np.uint8)
    mb = (rng.random((H, W)) > 0.1).astype(np.uint8)
    fb = _free_fb(layout, H, W)
    gathered = layout == "shift"
    if name == "fb_zero":
        fb = np.zeros((H, W, 2), 'f')
        gathered = True
    elif name == "fb_one_pixel":                 # the field's last pixel: the last lane of the last wave of the last tile
        fb = np.zeros((H, W, 2), 'f')
        fb[H - 1, W - 1, 1] = -0.5
        mb[H - 1, W - 1] = 1
        gathered = True
    elif name == "fb_unmasked":                  # non-zero only where mb is 0
        mb = (rng.random((H, W)) > 0.5).astype(np.uint8)
        mb[::8, :] = 0                           # (the pixels the layout decision reads keep their rotation values)
        mb[:, ::128] = 0
        mb[:, 127::128] = 0
        mb[:, W - 1] = 0
        fb[mb != 0] = 0
        gathered = False
    elif name in ("th_below", "th_at", "th_above"):
        v = {"th_below": np.nextafter(TH, np.float32(0)), "th_at": TH, "th_above": np.nextafter(TH, np.float32(1))}[name]
        fb = np.zeros((H, W, 2), 'f')
        fb[H // 2, W // 3, 0] = v
        fb[H // 3, W // 2, 1] = -v
        mb[H // 2, W // 3] = 1
        mb[H // 3, W // 2] = 0
        gathered = True
    elif name == "fa_zero":
        fa = np.zeros((H, W, 2), 'f')
    elif name == "fa_unmasked":                  # non-zero only where ma is 0
        fa[ma != 0] = 0
    elif name != "plain":
        raise ValueError(name)
    return fa, ma, fb, mb, gathered


def _predicates(fa, ma, fb, mb):
    a, b = np.abs(fa).max(-1), np.abs(fb).max(-1)
    am, bm = a[ma != 0], b[mb != 0]
    fa_bound = [bool((am > 0).any()), bool((am >= TH).any())]
    fb_exact = [bool((bm > 0).any()), bool((bm >= TH).any()), bool((b > 0).any()), bool((b >= TH).any())]
    return fa_bound, fb_exact


def _launch(of, fields, sign, quant, words):
    """One ofl_compose3_dev launch of the stacked fields into the flag rows `words` (uint32 [B][8]); returns the rows after."""
    from oflibnumpy_amd import device as dev
    nat, lib = of.native, of.native.load()
    fa, ma, fb, mb = (np.ascontiguousarray(np.stack([f[i] for f in fields])) for i in range(4))
    B, H, W = fa.shape[:3]
    bufs = [dev.DeviceBuffer.from_host(x) for x in (fa, ma, fb, mb)]
    out, mout = dev.DeviceBuffer(fa.nbytes), dev.DeviceBuffer(ma.nbytes)
    stats = dev.DeviceBuffer.from_host(np.ascontiguousarray(words, dtype=np.uint32))
    nat.check(lib.ofl_compose3_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, sign, H, W, B, out.ptr, mout.ptr,
                                   stats.ptr, quant, None))
    return stats.to_host((B, 8), np.uint32)


def _check(got, before, fields, tag):
    """`fields`: per row, the list of (fa, ma, fb, mb, gathered) of every launch that wrote into it."""
    for b, launches in enumerate(fields):
        print(tag, "field", b, "before", before[b].tolist(), "after", got[b].tolist())
        bound, exact, must = [False, False], [False] * 4, [False, False]
        for fa, ma, fb, mb, gathered in launches:
            fa_bound, fb_exact = _predicates(fa, ma, fb, mb)
            bound = [x or y for x, y in zip(bound, fa_bound)]
            exact = [x or y for x, y in zip(exact, fb_exact)]
            if gathered:
                must = [x or y for x, y in zip(must, fa_bound)]
        assert set(got[b].tolist()) <= {0, 1}, (tag, b, got[b])
        for k in range(4):
            assert bool(got[b, 4 + k]) == (exact[k] or bool(before[b, 4 + k])), (tag, b, k, got[b], exact)
        for k in (2, 3):
            assert got[b, k] == before[b, k], (tag, b, k, got[b])
        for k in (0, 1):
            if before[b, k]:
                assert got[b, k] == 1, (tag, b, k, got[b])
                continue
            if got[b, k]:
                assert bound[k], (tag, b, k, got[b])
            if must[k]:
                assert got[b, k] == 1, (tag, b, k, got[b])


def _quants(of):
    return (of.native.QUANT_OPENCV, of.native.QUANT_EXACT)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("name,layout", [
    ("fb_zero", "shift"), ("fb_one_pixel", "shift"), ("fb_unmasked", "shift"), ("fb_unmasked", "rot"),
    ("th_below", "shift"), ("th_at", "shift"), ("th_above", "shift"),
    ("fa_zero", "shift"), ("fa_zero", "rot"), ("fa_unmasked", "shift"), ("fa_unmasked", "rot"),
    ("plain", "shift"), ("plain", "rot")])
def test_flag_words_single_field(gpu, name, layout, sign, H, W):
    of = gpu
    rng = np.random.default_rng([H, W, len(name), sign + 1])
    f = _case(name, layout, H, W, rng)
    for quant in _quants(of):
        before = np.zeros((1, 8), np.uint32)
        _check(_launch(of, [f], sign, quant, before), before, [[f]], f"{name}/{layout}/q{quant}")


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("names", [
    (("fb_zero", "shift"), ("plain", "rot"), ("th_below", "shift")),
    (("fa_zero", "rot"), ("fb_one_pixel", "shift"), ("fb_unmasked", "rot")),
    (("fa_unmasked", "shift"), ("th_at", "shift"), ("fb_zero", "shift"))])
def test_flag_words_batch_of_three(gpu, names, sign, H, W):
    """A different case per field: a row takes nothing from its neighbours (the waves of a launch run field after field)."""
    of = gpu
    rng = np.random.default_rng([H, W, sign + 1, len(names[0][0])])
    fs = [_case(n, l, H, W, rng) for n, l in names]
    for quant in _quants(of):
        before = np.zeros((3, 8), np.uint32)
        _check(_launch(of, fs, sign, quant, before), before, [[f] for f in fs], f"batch{names}/q{quant}")


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("layout", ["shift", "rot"])
def test_flag_words_preset_row(gpu, layout, sign, H, W):
    """Words 2, 3 and some of 4..7 (and of 0/1) set before the launch stay set; the others follow the predicates."""
    of = gpu
    rng = np.random.default_rng([H, W, sign + 1, len(layout)])
    fs = [_case("fb_unmasked", layout, H, W, rng), _case("fa_zero", layout, H, W, rng), _case("fb_zero", "shift", H, W, rng)]
    for quant in _quants(of):
        before = np.array([[0, 0, 1, 1, 1, 0, 0, 1], [1, 0, 1, 0, 0, 1, 0, 0], [0, 1, 0, 1, 0, 0, 1, 0]], np.uint32)
        _check(_launch(of, fs, sign, quant, before), before, [[f] for f in fs], f"preset/{layout}/q{quant}")


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("sign", [-1, 1])
@pytest.mark.parametrize("layout", ["shift", "rot"])
def test_flag_words_two_launches_one_row(gpu, layout, sign, H, W):
    """Two launches into the same rows without zeroing in between: the union of their predicates survives."""
    of = gpu
    rng = np.random.default_rng([H, W, sign + 1, len(layout), 2])
    first = [_case("th_below", "shift", H, W, rng), _case("fa_zero", layout, H, W, rng), _case("fb_zero", "shift", H, W, rng)]
    second = [_case("fa_unmasked", layout, H, W, rng), _case("fb_unmasked", layout, H, W, rng), _case("fb_zero", "shift", H, W, rng)]
    for quant in _quants(of):
        zero = np.zeros((3, 8), np.uint32)
        mid = _launch(of, first, sign, quant, zero)
        _check(mid, zero, [[f] for f in first], f"two/{layout}/q{quant}/first")
        _check(_launch(of, second, sign, quant, mid), zero, [[f, g] for f, g in zip(first, second)], f"two/{layout}/q{quant}/both")


@pytest.mark.parametrize("sign", [-1, 1])
def test_flag_words_1080p_one_pixel(gpu, sign):
    """1080 x 1920 (whole tiles): fb zero except the field's last pixel, the last lane of the last wave of the last tile."""
    of = gpu
    H, W = 1080, 1920
    f = _case("fb_one_pixel", "shift", H, W, np.random.default_rng(1080 + sign))
    before = np.zeros((1, 8), np.uint32)
    _check(_launch(of, [f], sign, of.native.QUANT_OPENCV, before), before, [[f]], "1080p")
