"""GPU suite: the eight entry points that take host arrays (staged through csrc/ofl_host_stage.h) against their _dev twins
on the same inputs uploaded through DeviceBuffer -- byte for byte, NaN bits included -- over every combination of optional
arguments, at the smallest shapes at which staging can go wrong:

    1 x 1              the smallest field
    3 x 5, batch 1, 3  every part off the 16-byte grid; odd H * W with batch > 1: the narrow kernel routes
    8 x 130, batch 1, 2  even width, H * W % 4 == 0: the px2 / wide routes; more than one 128-column tile
    33 x 66

Every host output array has 64 guard bytes of 0xA5 behind it, which must come back unchanged.  Failing _dev entries hand
their code and message through the host entry, and the next call on the stream works."""
import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = [(1, 1), (3, 5), (8, 130), (33, 66)]
BATCHED = [(1, 1, 1), (3, 5, 1), (3, 5, 3), (8, 130, 1), (8, 130, 2), (33, 66, 1)]


@pytest.fixture(scope="module")
def env(gpu):
    from oflibnumpy_amd import device as dev
    return gpu.native, gpu.native.load(), dev.DeviceBuffer


def hp(a):
    return None if a is None else a.ctypes.data


def dp(b):
    return None if b is None else b.ptr


def guarded(shape, dtype):
    """A host output array, pre-filled with 0xA5 like the guard bytes behind it -> (array, the bytes with the guard)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.full(n + GUARD, 0xA5, np.uint8)
    return raw[:n].view(dtype).reshape(shape), raw


def intact(raw):
    return bool((raw[-GUARD:] == 0xA5).all())


def same_bytes(host, dev_buf):
    """host array == the first host.nbytes bytes of a device buffer"""
    got = dev_buf.to_host((host.nbytes,), np.uint8)
    return np.array_equal(np.ascontiguousarray(host).reshape(-1).view(np.uint8), got)


def field(rng, batch, h, w, scale=2.0):
    """float32 [batch][H][W][2] with NaN and Inf in a few vectors"""
    v = (rng.standard_normal((batch, h, w, 2)) * scale).astype(np.float32)
    flat = v.reshape(-1, 2)
    k = rng.choice(len(flat), size=min(3, len(flat)), replace=False)
    flat[k[0], 0] = np.nan
    if len(k) > 1:
        flat[k[1], 1] = np.inf
    if len(k) > 2:
        flat[k[2]] = -np.inf
    return v


def bits(rng, shape, p=0.7):
    return (rng.random(shape) < p).astype(np.uint8)


def subsets(names):
    """every combination of present / absent -> dicts name -> bool"""
    return [dict(zip(names, c)) for c in itertools.product((True, False), repeat=len(names))]


class Up:
    """uploads of one case's inputs and fresh device outputs, each with slack behind it"""

    def __init__(self, env):
        self.nat, self.lib, self.DeviceBuffer = env

    def __call__(self, a):
        a = np.ascontiguousarray(a)
        buf = self.DeviceBuffer(a.nbytes + GUARD)
        if a.nbytes:
            self.nat.check(self.lib.ofl_upload(buf.ptr, a.ctypes.data, a.nbytes, None))
            self.nat.check(self.lib.ofl_stream_sync(None))
        return buf

    def out(self, nbytes):
        return self.DeviceBuffer(nbytes + GUARD)

    def size(self, entry, *args):
        n = ctypes.c_size_t(0)
        self.nat.check(entry(*args, ctypes.byref(n)))
        return n.value


@pytest.mark.parametrize("h,w,batch", BATCHED)
def test_fill(env, h, w, batch):
    nat, lib, _ = env
    up = Up(env)
    rng = np.random.default_rng(h * 1000 + w + batch)
    vecs, mask, valid = field(rng, batch, h, w), bits(rng, (batch, h, w), 0.3), bits(rng, (batch, h, w), 0.8)
    dvecs, dmask, dvalid = up(vecs), up(mask), up(valid)
    n, wsb = batch * h * w, up.size(lib.ofl_fill_workspace_bytes, h, w, batch)
    ws, calls = up.out(wsb), 0
    for c in subsets(["vecs", "valid", "out_mask", "index", "d2"]):
        if not (c["vecs"] or c["index"] or c["d2"]):
            continue                    # check_fill_args: nothing to write
        ov, ov_raw = guarded((n, 2), np.float32) if c["vecs"] else (None, None)
        om, om_raw = guarded((n,), np.uint8) if c["out_mask"] else (None, None)
        ix, ix_raw = guarded((n,), np.int32) if c["index"] else (None, None)
        d2, d2_raw = guarded((n,), np.uint32) if c["d2"] else (None, None)
        nat.check(lib.ofl_fill(hp(vecs) if c["vecs"] else None, hp(mask), hp(valid) if c["valid"] else None, h, w, batch, 9,
                               hp(ov), hp(om), hp(ix), hp(d2)))
        dev = [None if a is None else up.out(a.nbytes) for a in (ov, om, ix, d2)]
        nat.check(lib.ofl_fill_dev(dp(dvecs) if c["vecs"] else None, dmask.ptr, dp(dvalid) if c["valid"] else None, h, w, batch, 9,
                                   ws.ptr, wsb, dp(dev[0]), dp(dev[1]), dp(dev[2]), dp(dev[3]), None))
        for name, a, raw, d in zip(("out_vecs", "out_mask", "index", "d2"), (ov, om, ix, d2), (ov_raw, om_raw, ix_raw, d2_raw), dev):
            if a is not None:
                assert same_bytes(a, d), (c, name)
                assert intact(raw), (c, name)
        calls += 1
    assert calls == 28


@pytest.mark.parametrize("h,w,batch", BATCHED)
def test_flow_error(env, h, w, batch):
    nat, lib, _ = env
    up = Up(env)
    rng = np.random.default_rng(h * 1000 + w + batch + 1)
    est, gt = field(rng, batch, h, w), field(rng, batch, h, w)
    em, gm = bits(rng, (batch, h, w)), bits(rng, (batch, h, w), 0.9)
    dest, dgt, dem, dgm = up(est), up(gt), up(em), up(gm)
    thr, edges = np.array([1, 3, 5, np.inf], np.float32), np.array([1, 2, 4], np.float32)
    n, wsb = batch * h * w, up.size(lib.ofl_flow_error_workspace_bytes, h, w, batch)
    ws = up.out(wsb)
    for c in subsets(["est_mask", "epe_map", "outlier_map"]):
        rec, rec_raw = guarded((batch * 96,), np.uint8)
        epe, epe_raw = guarded((n,), np.float32) if c["epe_map"] else (None, None)
        om, om_raw = guarded((n,), np.uint8) if c["outlier_map"] else (None, None)
        nat.check(lib.ofl_flow_error(hp(est), hp(em) if c["est_mask"] else None, hp(gt), hp(gm), h, w, batch, hp(thr), 3.0, 0.05,
                                     hp(edges), hp(rec), hp(epe), hp(om)))
        dev = [None if a is None else up.out(a.nbytes) for a in (rec, epe, om)]
        nat.check(lib.ofl_flow_error_dev(dest.ptr, dp(dem) if c["est_mask"] else None, dgt.ptr, dgm.ptr, h, w, batch, hp(thr), 3.0, 0.05,
                                         hp(edges), ws.ptr, wsb, dp(dev[0]), dp(dev[1]), dp(dev[2]), None))
        for name, a, raw, d in zip(("records", "epe_map", "outlier_map"), (rec, epe, om), (rec_raw, epe_raw, om_raw), dev):
            if a is not None:
                assert same_bytes(a, d), (c, name)
                assert intact(raw), (c, name)


@pytest.mark.parametrize("h,w,batch", BATCHED)
def test_consistency(env, h, w, batch):
    nat, lib, DeviceBuffer = env
    up = Up(env)
    rng = np.random.default_rng(h * 1000 + w + batch + 2)
    f, b = field(rng, batch, h, w), field(rng, batch, h, w)
    fm, bm = bits(rng, (batch, h, w)), bits(rng, (batch, h, w), 0.9)
    df, db, dfm, dbm = up(f), up(b), up(fm), up(bm)
    n = batch * h * w
    for quant in (nat.QUANT_OPENCV, nat.QUANT_EXACT):
        for c in subsets(["covered", "residual", "counts"]):
            con, con_raw = guarded((n,), np.uint8)
            cov, cov_raw = guarded((n,), np.uint8) if c["covered"] else (None, None)
            res, res_raw = guarded((n,), np.float32) if c["residual"] else (None, None)
            cnt, cnt_raw = guarded((batch, 2), np.uint32) if c["counts"] else (None, None)
            nat.check(lib.ofl_consistency(hp(f), hp(fm), hp(b), hp(bm), 1, h, w, batch, 0.01, 0.5, hp(con), hp(cov), hp(res), hp(cnt), quant))
            dev = [None if a is None else up.out(a.nbytes) for a in (con, cov, res)]
            dcnt = DeviceBuffer.zeros(batch * 8 + GUARD) if c["counts"] else None         # the launch adds to the counts
            nat.check(lib.ofl_consistency_dev(df.ptr, dfm.ptr, db.ptr, dbm.ptr, 1, h, w, batch, 0.01, 0.5, dp(dev[0]), dp(dev[1]), dp(dev[2]),
                                              dp(dcnt), quant, None))
            for name, a, raw, d in zip(("consistent", "covered", "residual", "counts"), (con, cov, res, cnt),
                                       (con_raw, cov_raw, res_raw, cnt_raw), dev + [dcnt]):
                if a is not None:
                    assert same_bytes(a, d), (quant, c, name)
                    assert intact(raw), (quant, c, name)


@pytest.mark.parametrize("h,w,batch", BATCHED)
def test_compose3(env, h, w, batch):
    nat, lib, _ = env
    up = Up(env)
    rng = np.random.default_rng(h * 1000 + w + batch + 3)
    fa, fb = field(rng, batch, h, w), field(rng, batch, h, w)
    fa[0] = 0                                                             # a zero field: the predicates differ between the fields
    ma, mb = bits(rng, (batch, h, w)), bits(rng, (batch, h, w), 0.9)
    dfa, dfb, dma, dmb = up(fa), up(fb), up(ma), up(mb)
    n, hw = batch * h * w, h * w
    for quant in (nat.QUANT_OPENCV, nat.QUANT_EXACT):
        for with_stats in (True, False):
            out, out_raw = guarded((n, 2), np.float32)
            mout, mout_raw = guarded((n,), np.uint8)
            st, st_raw = guarded((batch, 2), np.uint32) if with_stats else (None, None)
            nat.check(lib.ofl_compose3(hp(fa), hp(ma), hp(fb), hp(mb), -1, h, w, batch, hp(out), hp(mout), hp(st), quant))
            dout, dmout = up.out(out.nbytes), up.out(mout.nbytes)
            nat.check(lib.ofl_compose3_dev(dfa.ptr, dma.ptr, dfb.ptr, dmb.ptr, -1, h, w, batch, dout.ptr, dmout.ptr, None, quant, None))
            assert same_bytes(out, dout) and same_bytes(mout, dmout), (quant, with_stats)
            assert intact(out_raw) and intact(mout_raw), (quant, with_stats)
            if with_stats:
                # the host caller's exact predicates: one statistics pass per field and operand, the low four bits
                word = up.out(16)
                for k in range(batch):
                    for j, (dv, dm) in enumerate(((dfa, dma), (dfb, dmb))):
                        nat.check(lib.ofl_flow_stats_dev(dv.ptr + k * hw * 8, dm.ptr + k * hw, hw, np.float32(1e-3), word.ptr, None))
                        assert int(st[k, j]) == int(word.to_host((1,), np.uint32)[0]) & 15, (quant, k, j)
                assert intact(st_raw)


@pytest.mark.parametrize("h,w", SHAPES)
def test_gather_bilinear(env, h, w):
    nat, lib, _ = env
    up = Up(env)
    rng = np.random.default_rng(h * 1000 + w + 4)
    flow = field(rng, 1, h, w)
    smask, fmask = bits(rng, (h, w)), bits(rng, (h, w), 0.9)
    dflow, dsm, dfm = up(flow), up(smask), up(fmask)
    n = h * w
    img32 = rng.standard_normal((h, w, 2)).astype(np.float32)
    img32.reshape(-1)[rng.integers(img32.size)] = np.nan
    for src, code, C in ((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), nat.U8, 3), (img32, nat.F32, 2)):
        dsrc = up(src)
        for c in subsets(["smask", "fmask", "valid"]):
            dst, dst_raw = guarded(src.shape, src.dtype)
            val, val_raw = guarded((n,), np.uint8) if c["valid"] else (None, None)
            nat.check(lib.ofl_gather_bilinear(hp(src), code, C, h, w, hp(flow), h, w, 0, 0, -1, hp(smask) if c["smask"] else None,
                                              hp(fmask) if c["fmask"] else None, hp(dst), hp(val), nat.QUANT_OPENCV, nat.ARITH_NATIVE,
                                              nat.RULE_EQ1))
            ddst, dval = up.out(dst.nbytes), up.out(n) if c["valid"] else None
            nat.check(lib.ofl_gather_bilinear_dev(dsrc.ptr, code, C, h, w, dflow.ptr, h, w, 0, 0, -1, dp(dsm) if c["smask"] else None,
                                                  dp(dfm) if c["fmask"] else None, ddst.ptr, dp(dval), nat.QUANT_OPENCV,
                                                  nat.ARITH_NATIVE, nat.RULE_EQ1, None))
            assert same_bytes(dst, ddst) and intact(dst_raw), (code, c)
            if c["valid"]:
                assert same_bytes(val, dval) and intact(val_raw), (code, c)


def smooth_flow(h, w):
    """a gentle rotation plus a wobble: a mesh without folds, every warped position finite"""
    y, x = np.mgrid[:h, :w].astype(np.float32)
    return np.ascontiguousarray(np.stack([0.05 * (y - h / 2) + 0.4 * np.sin(x / 7) * np.cos(y / 5),
                                          -0.05 * (x - w / 2) + 0.3 * np.cos(x / 6) * np.sin(y / 8)], -1), np.float32)


@pytest.mark.parametrize("h,w", SHAPES)
def test_scatter_linear(env, h, w):
    """Point sets the _dev entry refuses (a single point, a masked set that is flat) must be refused by the host entry with the
    same code and message; everything else byte for byte."""
    nat, lib, _ = env
    up = Up(env)
    rng = np.random.default_rng(h * 1000 + w + 5)
    C, n = 2, h * w
    flow, vals = smooth_flow(h, w), rng.standard_normal((h, w, C)).astype(np.float32)
    vals.reshape(-1)[[0, vals.size - 1]] = np.nan, np.inf
    pmask, vmask = bits(rng, (h, w), 0.85), bits(rng, (h, w), 0.9)
    y, x = np.mgrid[:h, :w].astype(np.float32)
    query = np.ascontiguousarray(np.stack([x + 0.25, y - 0.5], -1), np.float32)
    dflow, dvals, dpm, dvm, dq = up(flow), up(vals), up(pmask), up(vmask), up(query)
    wsb = up.size(lib.ofl_scatter_workspace_bytes, h, w, C)
    ws, n_ok = up.out(wsb), 0
    for c in subsets(["pmask", "vmask", "query", "valid"]):
        out, out_raw = guarded((n, C), np.float32)
        val, val_raw = guarded((n,), np.uint8) if c["valid"] else (None, None)
        rc = lib.ofl_scatter_linear(hp(flow), 1, 0, hp(pmask) if c["pmask"] else None, hp(vals), C, hp(vmask) if c["vmask"] else None,
                                    h, w, hp(query) if c["query"] else None, hp(out), hp(val), 0)
        msg = nat.last_error() if rc else ""
        dout, dval = up.out(out.nbytes), up.out(n) if c["valid"] else None
        info = (ctypes.c_uint64 * 3)()
        rc_dev = lib.ofl_scatter_linear_dev(dflow.ptr, 1, 0, dp(dpm) if c["pmask"] else None, dvals.ptr, C, dp(dvm) if c["vmask"] else None,
                                            h, w, dp(dq) if c["query"] else None, dout.ptr, dp(dval), 0, ws.ptr, wsb, info, None)
        assert rc == rc_dev, (c, rc, rc_dev, msg, nat.last_error())
        assert intact(out_raw) and (val is None or intact(val_raw)), c
        if rc != nat.OK:
            assert msg == nat.last_error(), c
            continue
        n_ok += 1
        assert same_bytes(out, dout), c
        if c["valid"]:
            assert same_bytes(val, dval), c
    assert n_ok == 16 or h * w < 16, n_ok             # the two larger shapes: every combination is a triangulable set


@pytest.mark.parametrize("h,w", SHAPES)
def test_resize_flow(env, h, w):
    nat, lib, _ = env
    up = Up(env)
    rng = np.random.default_rng(h * 1000 + w + 6)
    vecs, mask = field(rng, 1, h, w), bits(rng, (h, w))
    dvecs, dmask = up(vecs), up(mask)
    for f in (0.5, 1.5):
        ho, wo = max(int(np.rint(h * f)), 1), max(int(np.rint(w * f)), 1)
        for with_mask in (True, False):
            out, out_raw = guarded((ho, wo, 2), np.float32)
            mout, mout_raw = guarded((ho, wo), np.uint8) if with_mask else (None, None)
            args = (h, w, ho, wo, 1.0 / f, 1.0 / f, float(np.float32(f)), float(np.float32(f)))
            nat.check(lib.ofl_resize_flow(hp(vecs), hp(mask) if with_mask else None, *args, hp(out), hp(mout)))
            dout, dmout = up.out(out.nbytes), up.out(ho * wo) if with_mask else None
            nat.check(lib.ofl_resize_flow_dev(dvecs.ptr, dmask.ptr if with_mask else None, *args, dout.ptr, dp(dmout), None))
            assert same_bytes(out, dout) and intact(out_raw), (f, with_mask)
            if with_mask:
                assert same_bytes(mout, dmout) and intact(mout_raw), f


@pytest.mark.parametrize("n_px", [0, 1, 2, 15, 33 * 66])
def test_flow_stats(env, n_px):
    nat, lib, _ = env
    up = Up(env)
    rng = np.random.default_rng(n_px + 7)
    vecs, mask = field(rng, 1, 1, max(n_px, 1)), bits(rng, (max(n_px, 1),))
    dvecs, dmask = up(vecs), up(mask)
    for with_mask in (True, False):
        word, raw = guarded((1,), np.uint32)
        nat.check(lib.ofl_flow_stats(hp(vecs), hp(mask) if with_mask else None, n_px, np.float32(1e-3), hp(word)))
        dword = up.out(16)
        nat.check(lib.ofl_flow_stats_dev(dvecs.ptr, dmask.ptr if with_mask else None, n_px, np.float32(1e-3), dword.ptr, None))
        assert same_bytes(word, dword) and intact(raw), with_mask
        assert n_px or int(word[0]) == 0


def test_failed_calls_pass_the_dev_entry_error_through_and_leave_the_stream_usable(env):
    nat, lib, _ = env
    h, w, C = 8, 130, 1
    rng = np.random.default_rng(8)
    flow, vals = smooth_flow(h, w), rng.standard_normal((h, w, C)).astype(np.float32)
    out, valid = np.empty((h, w, C), np.float32), np.empty((h, w), np.uint8)
    none = np.zeros((h, w), np.uint8)
    rc = lib.ofl_scatter_linear(hp(flow), 1, 0, hp(none), hp(vals), C, None, h, w, None, hp(out), hp(valid), 0)
    assert rc == nat.E_NOPOINTS, (rc, nat.last_error())
    nat.check(lib.ofl_scatter_linear(hp(flow), 1, 0, None, hp(vals), C, None, h, w, None, hp(out), hp(valid), 0))
    assert valid.any()

    vecs, mask = field(rng, 1, h, w), bits(rng, (h, w), 0.3)
    ov, om = np.empty((h, w, 2), np.float32), np.empty((h, w), np.uint8)
    rc = lib.ofl_fill(hp(vecs), hp(mask), None, h, w, 1, -2, hp(ov), hp(om), None, None)
    assert rc == nat.E_INVALID and "ofl_fill" in nat.last_error(), (rc, nat.last_error())
    nat.check(lib.ofl_fill(hp(vecs), hp(mask), None, h, w, 1, -1, hp(ov), hp(om), None, None))
    assert om.all()
