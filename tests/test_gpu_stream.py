"""The streaming kernels of ofl_stats.hip (K4 statistics, K5 axpy, flow extent, mask and, dtype conversion, grid offset, point
sampling) and the mask packing of ofl_compose3.hip against tests/stream_ref.py, bit for bit.  Nothing here has a tolerance:
words, mask bytes and the bits of every float -- NaN results with their sign and payload included -- are compared with
array_equal.  One thing is left open because NumPy leaves it open: the sign of a zero extreme of the flow extent (np.min does
not define it), so the extent alone is compared by value.

The raw entries are called on resident buffers; a case changes single pixels of them with small uploads, and every output
buffer has a pre-filled guard behind it that must come back unchanged."""
import numpy as np
import pytest

import oflibnumpy_amd as of
from oflibnumpy_amd import device as dev
from oflibnumpy_amd.batch import DeviceFlowBatch
import stream_ref as S

pytestmark = pytest.mark.gpu
nat = of.native
F32 = np.float32
GUARD = 0xA5
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def put(ptr, arr):
    """queue an upload of `arr` to the device address `ptr`; the caller keeps `arr` (or its base) alive until the next download"""
    assert arr.flags.c_contiguous
    nat.check(nat.load().ofl_upload(ptr, arr.ctypes.data, arr.nbytes, None))
    return arr


def fill(buf, byte=GUARD):
    nat.check(nat.load().ofl_memset(buf.ptr, byte, buf.nbytes, None))
    return buf


def same_bits(got, want, what=""):
    """equal bit patterns: signed zeros, subnormals and NaNs included"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_array_equal(got.view(UINT[got.dtype.itemsize]), want.view(UINT[want.dtype.itemsize]), err_msg=what)


def guard_intact(raw, start, what=""):
    assert (raw[start:] == GUARD).all() and raw[start:].size >= 16, what + ": bytes behind the output were written"


# ================================================================================================ K4: ofl_flow_stats_dev
KIND_NAMES = list(S.STATS_KINDS)
KIND_VECS = np.array([S.STATS_KINDS[k][0] for k in KIND_NAMES], F32)       # uploads read from these module-level tables
KIND_BYTES = [S.STATS_KINDS[k][1] for k in KIND_NAMES]
ZERO_VEC, BYTE0, BYTE1 = np.zeros(2, F32), np.zeros(1, np.uint8), np.ones(1, np.uint8)


def stats_into(d_v, d_m, n, word_ptr):
    nat.check(nat.load().ofl_flow_stats_dev(d_v.ptr, None if d_m is None else d_m.ptr, n, S.TH, word_ptr, None))


def zero_field(n):
    d_v, d_m = dev.DeviceBuffer.zeros(n * 8), dev.DeviceBuffer(n)
    fill(d_m, 1)
    return d_v, d_m


@pytest.mark.parametrize("n", S.STATS_SIZES)
def test_stats_single_cause_sweep(gpu, n):
    """a zero field under an all-ones mask with ONE pixel changed: every kind of cause at every edge position, with the
    mask and with mask = NULL; the words land in one buffer that is read back once"""
    d_v, d_m = zero_field(n)
    pos = S.stats_positions(n)
    d_w = fill(dev.DeviceBuffer(8 * len(pos) * len(KIND_NAMES)), 0xff)
    v, m = np.zeros((n, 2), F32), np.ones(n, np.uint8)
    want, label, slot = [], [], 0
    for p in pos:
        for k, kind in enumerate(KIND_NAMES):
            put(d_v.ptr + 8 * p, KIND_VECS[k])
            v[p], m[p] = KIND_VECS[k], KIND_BYTES[k]
            if not KIND_BYTES[k]:
                put(d_m.ptr + p, BYTE0)
            stats_into(d_v, d_m, n, d_w.ptr + 4 * slot)
            stats_into(d_v, None, n, d_w.ptr + 4 * slot + 4)
            want += [S.stats_word(v, m), S.stats_word(v, None)]
            label += ["pixel {} kind {} with the mask".format(p, kind), "pixel {} kind {} mask NULL".format(p, kind)]
            slot += 2
            put(d_v.ptr + 8 * p, ZERO_VEC)
            v[p], m[p] = 0, 1
            if not KIND_BYTES[k]:
                put(d_m.ptr + p, BYTE1)
    got = d_w.to_host((slot,), np.uint32)
    bad = np.flatnonzero(got != np.array(want, np.uint32))
    assert bad.size == 0, "n = {}: {} of {} words differ, first: {} gives {:#x}, expected {:#x}".format(
        n, bad.size, slot, label[bad[0]], int(got[bad[0]]), want[bad[0]])
    # the field is as it was
    stats_into(d_v, d_m, n, d_w.ptr)
    assert int(d_w.to_host((1,), np.uint32)[0]) == 0


def test_stats_merge_keeps_the_bits_of_every_workgroup(gpu):
    """40 961 pixels are ten workgroups of pixel pairs plus the odd pixel: a sub-threshold vector in one workgroup and a zero
    mask byte in another -- in the last pair for workgroup 0 -- give a word with both causes"""
    n = 40961
    groups = (n // 2 + 2047) // 2048
    assert groups == 10
    d_v, d_m = zero_field(n)
    d_w = fill(dev.DeviceBuffer(4 * 2 * groups), 0xff)
    v, m = np.zeros((n, 2), F32), np.ones(n, np.uint8)
    want = []
    for g in range(groups):
        pa = g * S.STATS_WG + 5
        pg = n - 2 if g == 0 else ((g + 5) % groups) * S.STATS_WG + 777          # n - 2: the last pixel of the last pair
        assert pa // S.STATS_WG != pg // S.STATS_WG
        put(d_v.ptr + 8 * pa, KIND_VECS[KIND_NAMES.index('a')])
        put(d_m.ptr + pg, BYTE0)
        v[pa], m[pg] = KIND_VECS[KIND_NAMES.index('a')], 0
        stats_into(d_v, d_m, n, d_w.ptr + 8 * g)
        stats_into(d_v, None, n, d_w.ptr + 8 * g + 4)
        want += [S.stats_word(v, m), S.stats_word(v, None)]
        put(d_v.ptr + 8 * pa, ZERO_VEC)
        put(d_m.ptr + pg, BYTE1)
        v[pa], m[pg] = 0, 1
    assert want == [S.NONZERO_MASKED | S.NONZERO | S.MASK_HAS_ZERO, S.NONZERO_MASKED | S.NONZERO] * groups
    np.testing.assert_array_equal(d_w.to_host((2 * groups,), np.uint32), np.array(want, np.uint32))


def test_stats_random_cases(gpu):
    cases = S.stats_cases()
    biggest = max(v.shape[0] for _, v, _ in cases)
    d_v, d_m = dev.DeviceBuffer(biggest * 8), dev.DeviceBuffer(biggest)
    d_w = fill(dev.DeviceBuffer(8 * len(cases)), 0xff)
    for k, (name, v, m) in enumerate(cases):
        put(d_v.ptr, v)
        put(d_m.ptr, m)
        stats_into(d_v, d_m, v.shape[0], d_w.ptr + 8 * k)
        stats_into(d_v, None, v.shape[0], d_w.ptr + 8 * k + 4)
    got = d_w.to_host((len(cases), 2), np.uint32)
    for k, (name, v, m) in enumerate(cases):
        assert (int(got[k, 0]), int(got[k, 1])) == (S.stats_word(v, m), S.stats_word(v, None)), name


def test_stats_entry_zeroes_its_word_and_no_other(gpu):
    n = 4097
    d_v, d_m = zero_field(n)
    v, m = np.zeros((n, 2), F32), np.ones(n, np.uint8)
    v[4000], m[4000] = (3, 0), 0
    put(d_v.ptr + 8 * 4000, v[4000:4001])
    put(d_m.ptr + 4000, BYTE0)
    d_w = fill(dev.DeviceBuffer(16), 0xff)
    stats_into(d_v, d_m, n, d_w.ptr + 4)
    want = S.stats_word(v, m)
    assert want == S.NONZERO | S.NONZERO_TH | S.MASK_HAS_ZERO
    assert d_w.to_host((3,), np.uint32).tolist() == [0xffffffff, want, 0xffffffff]
    fill(d_w, 0xff)
    stats_into(d_v, d_m, 0, d_w.ptr + 4)                     # no pixel: the word is zero, nothing is launched
    assert d_w.to_host((3,), np.uint32).tolist() == [0xffffffff, 0, 0xffffffff]


def batch_of_three():
    """three 37 x 53 fields (1961 px, an odd count) back to back: field 1 starts 8 bytes off a 16-byte boundary and its
    mask at an odd address, field 2 has its mask 2 bytes off a 4-byte boundary"""
    shape, rng = (37, 53), np.random.default_rng(11)
    n = shape[0] * shape[1]
    vecs = np.zeros((3,) + shape + (2,), F32)
    masks = np.ones((3,) + shape, np.uint8)
    vecs[0] = rng.standard_normal(shape + (2,)) * 4
    masks[0] = rng.random(shape) > 0.3
    vecs[1] = rng.uniform(-9e-4, 9e-4, shape + (2,))          # below the threshold, except one vector under mask 0
    vecs[1, 20, 30], masks[1, 20, 30] = (6.5, -7.25), 0
    vecs[1, 0, 0] = (7e-4, 7e-4)
    vecs[2, -1, -1], masks[2, -1, -1] = (0.0, -0.0), 0         # a zero field whose only zero mask byte is the odd tail pixel
    b = DeviceFlowBatch(3, shape, 't')
    put(b.vecs.ptr, vecs)
    put(b.mask.ptr, masks)
    dev.sync()
    assert (b.field(1).vecs.ptr % 16, b.field(1).mask.ptr % 2, b.field(2).mask.ptr % 4) == (8, 1, 2) and n % 2 == 1
    return b, vecs, masks


def test_stats_and_algebra_on_views_inside_a_batch(gpu):
    b, vecs, masks = batch_of_three()
    shape = b.shape
    views = [b.field(i) for i in range(3)]
    alone = [dev.DeviceFlow.from_host(vecs[i], 't', masks[i]) for i in range(3)]
    for i, (fv, fa) in enumerate(zip(views, alone)):
        assert fv.stats() == fa.stats() and fv.stats() & 63 == S.stats_word(vecs[i], masks[i]), i
        for thresholded in (True, False):
            for masked in (True, False):
                assert fv.is_zero(thresholded, masked) == fa.is_zero(thresholded, masked), (i, thresholded, masked)
        assert fv.get_padding() == fa.get_padding() == S.padding(vecs[i], masks[i], -1), i
    assert [f.stats() & 63 for f in views] == [15 | 32, 1 | 4 | 8 | 32, 32]
    assert views[1].get_padding() != S.padding(vecs[1], masks[1], -1, th=None)
    for i, j in ((1, 2), (2, 1), (0, 1)):
        for op, alpha in ((lambda x, y: x + y, 1.0), (lambda x, y: x - y, -1.0)):
            want_v, want_m = S.axpy(vecs[i], masks[i], vecs[j], masks[j], alpha)
            for got in (op(views[i], views[j]), op(alone[i], alone[j]), op(views[i], alone[j])):
                same_bits(got.vecs.to_host(shape + (2,), F32), want_v, "fields {} {} alpha {}".format(i, j, alpha))
                np.testing.assert_array_equal(got.mask.to_host(shape, np.uint8), want_m)
    for i in range(3):
        want_v, want_m = S.axpy(vecs[i], masks[i], None, None, -1.0)
        for got in (-views[i], -alone[i]):
            same_bits(got.vecs.to_host(shape + (2,), F32), want_v, "-field {}".format(i))
            np.testing.assert_array_equal(got.mask.to_host(shape, np.uint8), want_m)
    # the batch is unchanged
    same_bits(b.vecs.to_host(vecs.shape, F32), vecs)
    np.testing.assert_array_equal(b.mask.to_host(masks.shape, np.uint8), masks)


def test_stats_word_through_the_layers(gpu):
    shape = (33, 35)
    n = shape[0] * shape[1]
    assert n % 2 == 1
    m = np.ones(shape, np.uint8)
    m[-1, -1] = 0
    f = dev.DeviceFlow.from_host(np.zeros(shape + (2,), F32), 't', m)
    assert f._point_mask() is f.mask and f.stats() & 63 == S.MASK_HAS_ZERO          # the one zero byte is the odd tail pixel
    g = dev.DeviceFlow.from_host(np.zeros(shape + (2,), F32), 't', np.ones(shape, np.uint8))
    assert g._point_mask() is None and g.stats() & 63 == 0
    assert f._point_mask(consider_mask=False) is None
    for kind in ('b+', 'b-', 'c+', 'c-'):
        v = np.zeros(shape + (2,), F32)
        v[-1, -1] = S.STATS_KINDS[kind][0]
        word = S.stats_word(v, None)
        assert word == (15 if kind[0] == 'b' else 5)
        for thresholded, bit in ((True, S.NONZERO_TH), (False, S.NONZERO)):
            assert of.is_zero_flow(v, thresholded) == (not word & bit), (kind, thresholded)
            for masked in (True, False):
                assert of.Flow(v).is_zero(thresholded, masked) == (not word & bit), (kind, thresholded, masked)
            assert of.Flow(v, 't', m.astype(bool)).is_zero(thresholded, True) is True      # the pixel is masked out
            assert of.Flow(v, 't', m.astype(bool)).is_zero(thresholded, False) == (not word & bit)


# ================================================================================================ K5: ofl_axpy_dev
@pytest.mark.parametrize("n", S.AXPY_SIZES)
def test_axpy_every_variant(gpu, n):
    a, ma, b, mb = S.axpy_inputs(n)
    d_a, d_ma, d_b, d_mb = (dev.DeviceBuffer.from_host(x) for x in (a, ma, b, mb))
    d_out, d_mout = dev.DeviceBuffer((n + S.AXPY_UNIT) * 8), dev.DeviceBuffer(n + S.AXPY_UNIT)
    #            name                          b     mb    ma    mout  alphas
    variants = [("b and mb",                   True, True, True, True, S.AXPY_ALPHAS),
                ("neither b nor mb",           False, False, True, True, S.AXPY_ALPHAS),
                ("mb without b (_and_mask)",   False, True, True, True, [1.0]),
                ("no mout, with ma",           True, True, True, False, S.AXPY_ALPHAS),
                ("no mout, no ma",             True, False, False, False, S.AXPY_ALPHAS)]
    for name, with_b, with_mb, with_ma, with_mout, alphas in variants:
        for alpha in alphas:
            what = "n = {}, {}, alpha = {}".format(n, name, alpha)
            fill(d_out), fill(d_mout)
            nat.check(nat.load().ofl_axpy_dev(d_a.ptr, d_ma.ptr if with_ma else None, d_b.ptr if with_b else None,
                                              d_mb.ptr if with_mb else None, F32(alpha), n, d_out.ptr,
                                              d_mout.ptr if with_mout else None, None))
            want_v, want_m = S.axpy(a, ma if with_ma else None, b if with_b else None, mb if with_mb else None, alpha)
            raw = d_out.to_host(((n + S.AXPY_UNIT) * 8,), np.uint8)
            same_bits(raw[:n * 8].view(F32).reshape(n, 2), want_v, what)
            guard_intact(raw, n * 8, what)
            raw = d_mout.to_host((n + S.AXPY_UNIT,), np.uint8)
            if with_mout:
                np.testing.assert_array_equal(raw[:n], want_m, err_msg=what)
            guard_intact(raw, n if with_mout else 0, what)
    # the inputs are unchanged
    same_bits(d_a.to_host((n, 2), F32), a)
    same_bits(d_b.to_host((n, 2), F32), b)
    np.testing.assert_array_equal(d_ma.to_host((n,), np.uint8), ma)
    np.testing.assert_array_equal(d_mb.to_host((n,), np.uint8), mb)


# ================================================================================================ ofl_flow_extent_dev / get_padding
@pytest.mark.parametrize("shape", S.EXTENT_SHAPES)
def test_extent_and_get_padding(gpu, shape):
    h, w = shape
    n = h * w
    d_v, d_m, d_e = dev.DeviceBuffer(n * 8), dev.DeviceBuffer(n), dev.DeviceBuffer(32)

    def raw_extent(mask_ptr, sign, what):
        fill(d_e)
        nat.check(nat.load().ofl_flow_extent_dev(d_v.ptr, mask_ptr, h, w, sign, S.TH, d_e.ptr, None))
        raw = d_e.to_host((32,), np.uint8)
        guard_intact(raw, 16, what)
        return raw[:16].view(F32)

    for name, sign, v, m in S.extent_cases(shape):
        what = "{} {} sign {}".format(shape, name, sign)
        put(d_v.ptr, v)
        put(d_m.ptr, m)
        np.testing.assert_array_equal(raw_extent(d_m.ptr, sign, what), S.extent(v, m, sign), err_msg=what)      # by value
        field = dev.DeviceFlow(d_v, d_m, shape, 's' if sign == 1 else 't')
        if name == "none":
            assert np.isinf(S.extent(v, m, sign)).all()
            with pytest.raises(ValueError, match="zero-size array"):
                field.get_padding()
        else:
            assert field.get_padding() == S.padding(v, m, sign), what
        if name in ("random", "threshold", "none"):                  # mask = NULL: every pixel counts
            np.testing.assert_array_equal(raw_extent(None, sign, what), S.extent(v, None, sign), err_msg=what + " mask NULL")


# ================================================================================================ ofl_mask_and_dev
def test_mask_and_sizes_and_byte_offsets(gpu):
    biggest, rng = max(S.MASK_AND_SIZES), np.random.default_rng(3)
    a, b = rng.integers(0, 256, biggest, np.uint8), rng.integers(0, 256, biggest, np.uint8)
    a[:8], b[:8] = [0, 1, 1, 0, 255, 2, 128, 1], [0, 1, 0, 1, 15, 1, 128, 3]
    pad = 32
    d_a, d_b, d_out = dev.DeviceBuffer(biggest + pad), dev.DeviceBuffer(biggest + pad), dev.DeviceBuffer(biggest + pad)
    for off in (0, 1, 2, 3):
        put(d_a.ptr + off, a)
        put(d_b.ptr + off, b)
        for n in S.MASK_AND_SIZES:
            what = "n = {} at byte offset {}".format(n, off)
            fill(d_out)
            nat.check(nat.load().ofl_mask_and_dev(d_a.ptr + off, d_b.ptr + off, d_out.ptr + off, n, None))
            raw = d_out.to_host((biggest + pad,), np.uint8)
            np.testing.assert_array_equal(raw[off:off + n], a[:n] & b[:n], err_msg=what)
            assert (raw[:off] == GUARD).all(), what
            guard_intact(raw, off + n, what)
    # different offsets for the three buffers
    fill(d_out)
    put(d_a.ptr + 3, a)
    put(d_b.ptr + 2, b)
    nat.check(nat.load().ofl_mask_and_dev(d_a.ptr + 3, d_b.ptr + 2, d_out.ptr + 1, 1027, None))
    raw = d_out.to_host((biggest + pad,), np.uint8)
    np.testing.assert_array_equal(raw[1:1028], a[:1027] & b[:1027])
    guard_intact(raw, 1028)


# ================================================================================================ ofl_convert_dev
@pytest.mark.parametrize("src,dst", S.CONVERT_PAIRS)
def test_convert_supported_pairs(gpu, src, dst):
    s_dt, d_dt = np.dtype(S.DTYPES[src]), np.dtype(S.DTYPES[dst])
    biggest = max(S.CONVERT_SIZES)
    d_src, d_dst = dev.DeviceBuffer(biggest * s_dt.itemsize), dev.DeviceBuffer((biggest + 16) * d_dt.itemsize)
    for n in S.CONVERT_SIZES:
        what = "{} -> {}, n = {}".format(s_dt, d_dt, n)
        x = S.convert_input(src, dst, n)
        put(d_src.ptr, x)
        fill(d_dst)
        nat.check(nat.load().ofl_convert_dev(d_src.ptr, src, d_dst.ptr, dst, n, None))
        raw = d_dst.to_host(((n + 16) * d_dt.itemsize,), np.uint8)
        same_bits(raw[:n * d_dt.itemsize].view(d_dt), S.convert(x, d_dt), what)
        guard_intact(raw, n * d_dt.itemsize, what)
        if (src, dst) == (S.F32_CODE, S.F64_CODE):                   # exact: back to the same float32 bits
            back = raw[:n * 8].view(np.float64).astype(F32)
            same_bits(back, x, what + " and back")


def test_convert_refuses_every_other_pair(gpu):
    d_src, d_dst = fill(dev.DeviceBuffer(64), 1), fill(dev.DeviceBuffer(64))
    others = (S.U8, S.I16, S.U16, S.F64_CODE)
    for src in others:
        for dst in others:
            assert nat.load().ofl_convert_dev(d_src.ptr, src, d_dst.ptr, dst, 4, None) == nat.E_INVALID, (src, dst)
            assert "ofl_convert" in nat.last_error()
    for src, dst in ((7, S.F32_CODE), (S.F32_CODE, 7), (-1, S.F32_CODE), (S.F32_CODE, 5)):
        assert nat.load().ofl_convert_dev(d_src.ptr, src, d_dst.ptr, dst, 4, None) == nat.E_INVALID, (src, dst)
    assert nat.load().ofl_convert_dev(None, S.U8, d_dst.ptr, S.F32_CODE, 4, None) == nat.E_INVALID
    dev.sync()
    assert (d_dst.to_host((64,), np.uint8) == GUARD).all()            # nothing was launched


# ================================================================================================ ofl_grid_offset_dev
@pytest.mark.parametrize("shape", S.GRID_OFFSET_SHAPES)
def test_grid_offset(gpu, shape):
    h, w = shape
    n = h * w
    v = S.offset_field(shape)
    d_v, d_out = dev.DeviceBuffer.from_host(v), dev.DeviceBuffer(n * 8 + 32)
    for sign in (1, -1):
        what = "{} sign {}".format(shape, sign)
        fill(d_out)
        nat.check(nat.load().ofl_grid_offset_dev(d_v.ptr, sign, h, w, d_out.ptr, None))
        raw = d_out.to_host((n * 8 + 32,), np.uint8)
        same_bits(raw[:n * 8].view(F32).reshape(h, w, 2), S.grid_offset(v, sign), what)
        guard_intact(raw, n * 8, what)
    for sign in (0, 2):
        assert nat.load().ofl_grid_offset_dev(d_v.ptr, sign, h, w, d_out.ptr, None) == nat.E_INVALID


# ================================================================================================ ofl_sample_points_dev
@pytest.mark.parametrize("shape", S.SAMPLE_FIELDS)
def test_sample_points(gpu, shape):
    h, w = shape
    biggest = max(S.SAMPLE_COUNTS)
    d_p, d_out = dev.DeviceBuffer(biggest * 16), dev.DeviceBuffer(biggest * 16 + 32)
    d_f = None
    for n in S.SAMPLE_COUNTS:
        what = "{} field, {} points".format(shape, n)
        flow, pts = S.sample_case(shape, n)
        d_f = dev.DeviceBuffer.from_host(flow)
        put(d_p.ptr, pts)
        fill(d_out)
        nat.check(nat.load().ofl_sample_points_dev(d_f.ptr, h, w, d_p.ptr, n, d_out.ptr, None))
        raw = d_out.to_host((n * 16 + 32,), np.uint8)
        same_bits(raw[:n * 16].view(np.float64).reshape(n, 2), S.sample_points(flow, pts), what)
        guard_intact(raw, n * 16, what)


# ================================================================================================ ofl_mask_pack_dev / ofl_mask_unpack_dev
@pytest.mark.parametrize("W", S.PACK_WIDTHS)
def test_mask_pack_and_unpack(gpu, W):
    for H in S.PACK_HEIGHTS:
        for batch in S.PACK_BATCHES:
            n, words = batch * H * W, batch * H * ((W + 31) // 32)
            nbytes = dev.mask_bits_bytes(H, W, batch)
            assert nbytes == words * 4 + 16
            d_mask, d_bits, d_out = dev.DeviceBuffer(n), dev.DeviceBuffer(nbytes), dev.DeviceBuffer(n + 32)
            assert d_mask.ptr % 16 == 0                                # what stream_ref.pack_paths assumes
            for name, mask in S.pack_masks(H, W, batch):
                what = "{} x {} x {} {}".format(batch, H, W, name)
                want = S.pack_bits(mask, H, W, batch)
                put(d_mask.ptr, mask)
                fill(d_bits)
                nat.check(nat.load().ofl_mask_pack_dev(d_mask.ptr, H, W, batch, d_bits.ptr, None))
                raw = d_bits.to_host((nbytes,), np.uint8)
                np.testing.assert_array_equal(raw[:words * 4].view(np.uint32).reshape(want.shape), want, err_msg=what)
                guard_intact(raw, words * 4, what)                     # the 16 bytes of slack are not the kernel's to write
                # unpack the restatement's plane, not the device's
                put(d_bits.ptr, want)
                fill(d_out)
                nat.check(nat.load().ofl_mask_unpack_dev(d_bits.ptr, H, W, batch, d_out.ptr, None))
                raw = d_out.to_host((n + 32,), np.uint8)
                np.testing.assert_array_equal(raw[:n].reshape(mask.shape), (mask != 0).astype(np.uint8), err_msg=what)
                guard_intact(raw, n, what)
