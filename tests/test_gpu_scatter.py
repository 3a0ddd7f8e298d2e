"""GPU parity tests of the scatter kernel K3 and everything built on it ('s'-reference apply, invert
s->s / t->t, switch_ref, valid_target('s'), valid_source('t'), combine_with modes 1 and 2), called through
the C ABI and the Flow API.

Expected values are (a) outputs of the REAL reference captured in tests/golden/ref_scipy_paths.npz and
(b) the oracle, which calls the same scipy.interpolate.griddata the reference calls.

Bars: validity masks bit-exact; interpolated float32 values within 1e-4 relative (BASELINE.json) -- in
practice ~1e-6 -- wherever SciPy's own Delaunay triangulation is unique (scatter_util.nonunique_nodes marks the
simplices with a fourth site on their circumcircle: exact squares of translations / axis-aligned scalings and the
~13 % of cells of a similarity transform whose float32 rounding is identical at all four corners; Qhull's choice
there is arbitrary -- inside them a node must equal the reference's output or be one of the admissible alternatives,
values and validity from one triangle: check_admissible / scatter_admissible.py).  Holes of the point mask, curved borders, folds and sheared cells are triangulated exactly
like SciPy does (round 2: certified mesh path + Delaunay path, see test_gpu_scatter_exact.py).
"""
import numpy as np
import pytest

from test_oracle import (golden_tags, k7_flows, K7_VALID_TARGET_S, K7_VALID_SOURCE_T,
                         K7_VALID_TARGET_S_MASKED, K7_VALID_SOURCE_T_MASKED)
from scatter_util import ambiguous_for, nonunique_nodes, reference_case, warped_points
import scatter_admissible as sa

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5


def ambiguous_nodes(flow, sign=1, tol=1e-9):
    """Grid nodes that lie in (the bounding box of) a warped cell whose four corners are co-circular to
    within `tol`: both diagonals are Delaunay there, Qhull picks one by its internal facet order and the
    kernel the other with equal right, so interpolated NON-AFFINE values may legitimately differ."""
    h, w = flow.shape[:2]
    y, x = np.mgrid[:h, :w].astype(np.float64)
    px, py = x + sign * flow[..., 0].astype(np.float64), y + sign * flow[..., 1].astype(np.float64)
    a = (px[:-1, :-1], py[:-1, :-1]); b = (px[:-1, 1:], py[:-1, 1:])
    c = (px[1:, 1:], py[1:, 1:]); d = (px[1:, :-1], py[1:, :-1])
    ax, ay, bx, by, cx, cy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    a2, b2, c2 = ax * ax + ay * ay, bx * bx + by * by, cx * cx + cy * cy
    ic = ax * (by * c2 - b2 * cy) - ay * (bx * c2 - b2 * cx) + a2 * (bx * cy - by * cx)
    amb = np.abs(ic) < tol
    out = np.zeros((h, w), bool)
    xs = np.stack([a[0], b[0], c[0], d[0]]); ys = np.stack([a[1], b[1], c[1], d[1]])
    x0 = np.clip(np.floor(xs.min(0)).astype(int), 0, w - 1); x1 = np.clip(np.ceil(xs.max(0)).astype(int), 0, w - 1)
    y0 = np.clip(np.floor(ys.min(0)).astype(int), 0, h - 1); y1 = np.clip(np.ceil(ys.max(0)).astype(int), 0, h - 1)
    for cy_, cx_ in zip(*np.nonzero(amb)):
        out[y0[cy_, cx_]:y1[cy_, cx_] + 1, x0[cy_, cx_]:x1[cy_, cx_] + 1] = True
    return out


def assert_close_outside_ambiguous(got, want, amb, tag=""):
    """Values agree everywhere except where SciPy's triangulation is not unique.  Returns the mismatching fraction."""
    bad = ~np.isclose(got, want, rtol=RTOL, atol=ATOL)
    if bad.ndim == 3:
        bad = bad.any(-1)
    assert not (bad & ~amb).any(), "{}: {} values differ outside non-unique simplices".format(tag, int((bad & ~amb).sum()))
    return bad.mean()


def run_product(of, g, tag):
    op = tag.split('/')[0]
    f = of.Flow(g[tag + '/in_vecs'], str(g[tag + '/in_ref']), g[tag + '/in_mask'])
    if op == 'invert':
        return f.invert()
    if op == 'switch_ref':
        return f.switch_ref()
    if op in ('valid_target', 'valid_target_nomask'):
        return f.valid_target(op == 'valid_target')
    if op in ('valid_source', 'valid_source_nomask'):
        return f.valid_source(op == 'valid_source')
    if op in ('apply_img', 'apply_img_nomask'):
        return f.apply(g['img_f32'], return_valid_area=True, consider_mask=(op == 'apply_img'))
    if op == 'apply_u8':
        return f.apply(g['img_u8'])
    if op.startswith('combine2'):
        return f.combine_with(of.Flow(g[tag + '/in2_vecs'], f.ref, g[tag + '/in2_mask']), 2)
    if op == 'k7':
        n = tag.split('/')[1]
        fn = f.valid_target if n.startswith('valid_target') else f.valid_source
        return fn(not n.endswith('nomask'))
    raise KeyError(tag)


def has_holes(g, tag):
    """True when SciPy received a point set with dropped points (consider_mask and a mask with False entries)."""
    op = tag.split('/')[0]
    if op.endswith('nomask') or tag.endswith('nomask') or op.startswith('combine2'):
        return False
    if op == 'apply_u8':
        return not g[tag + '/in_mask'].all()
    return not g[tag + '/in_mask'].all()


def case_ambiguity(golden, tag):
    """non-unique nodes of the point set SciPy received in this case"""
    sign = -1 if tag.startswith(('valid_source', 'k7/valid_source')) else 1
    if str(golden[tag + '/in_ref']) == 't' and tag.split('/')[0] in ('invert', 'switch_ref'):
        sign = -1                                   # t -> s / t -> t go through points x - f (flow_class.py:725, 753)
    keep = golden[tag + '/in_mask'] if has_holes(golden, tag) else None
    return ambiguous_for(golden[tag + '/in_vecs'], keep, sign)


def check_admissible(golden, tag, r, amb):
    """Inside the non-unique simplices, where the comparisons of check_case stop: the product's output equals the
    reference's or is one of the admissible alternatives (scatter_admissible), values and validity from one triangle."""
    c = reference_case(golden, tag)
    if c['queries'] is not None:            # mode 2 / 't': float32 points, scattered query positions
        amb = nonunique_nodes(c['points'], c['shape'], c['queries'])[0]
    if hasattr(r, 'vecs'):
        got, gv = r.vecs, r.mask
        if c['queries'] is not None:        # the stage that is interpolated: f3 - result
            got = golden[tag + '/in2_vecs'] - r.vecs
    elif isinstance(r, tuple):
        got, gv = r
    elif r.dtype == bool:
        got, gv = None, r
    else:
        got, gv = r, None
    return sa.assert_equal_or_admissible(tag, c['points'], c['values'], c['shape'], got, c['out'], amb, gv, c['out_valid'], c['rule'],
                                         c['queries'], rtol=RTOL, atol=ATOL, levels=c['levels'])


def check_case(of, golden, tag):
    r = run_product(of, golden, tag)
    amb = case_ambiguity(golden, tag)
    check_admissible(golden, tag, r, amb)
    speckled = not golden[tag + '/in_mask'].all()      # the mask VALUES are interpolated: which triangle covers a node matters
    if isinstance(r, of.Flow):
        assert r.ref == str(golden[tag + '/out_ref']), tag
        np.testing.assert_array_equal(r.mask, golden[tag + '/out_mask'], err_msg=tag)
        sel = ~amb if 'wobble' in tag else np.ones(r.mask.shape, bool)      # flow-valued data is affine for the affine fields
        np.testing.assert_allclose(r.vecs[sel], golden[tag + '/out_vecs'][sel], rtol=RTOL, atol=ATOL, err_msg=tag)
    elif isinstance(r, tuple):
        # random image content (not affine in position): exact wherever the triangulation is unique
        sel = ~amb if speckled else np.ones(amb.shape, bool)
        np.testing.assert_array_equal(r[1][sel], golden[tag + '/out_valid'][sel], err_msg=tag)
        assert_close_outside_ambiguous(r[0], golden[tag + '/out'], amb, tag)
    elif r.dtype == bool:
        sel = ~amb if speckled else np.ones(amb.shape, bool)
        np.testing.assert_array_equal(r[sel], golden[tag + '/out'][sel], err_msg=tag)
    else:   # uint8 image: a value that lands within 1e-6 of x.5 may round the other way
        d = np.abs(r.astype(int) - golden[tag + '/out'].astype(int)).max(-1)
        assert (d[~amb] <= 1).all() and (d[~amb] > 0).mean() < 1e-3, tag


def test_reference_outputs_without_holes(gpu, golden):
    """Every captured reference output whose point set is the full warped grid."""
    failures, n = [], 0
    for tag in golden_tags(golden):
        if has_holes(golden, tag):
            continue
        n += 1
        try:
            check_case(gpu, golden, tag)
        except AssertionError as e:
            failures.append("{}: {}".format(tag, str(e).strip().splitlines()[:6]))
    assert n >= 50
    assert not failures, "\n".join(failures)


def test_reference_outputs_with_holes(gpu, golden):
    """Point sets with dropped points (consider_mask=True and a mask with holes / speckle): SciPy triangulates
    across the gaps, and so does the Delaunay path.  Masks bit-exact; flow-valued AND image-valued results agree
    wherever SciPy's triangulation is unique."""
    of = gpu
    n = 0
    for tag in golden_tags(golden):
        if not has_holes(golden, tag):
            continue
        n += 1
        check_case(of, golden, tag)
    assert n >= 10


def test_known_answer_masks_scatter(gpu):
    """reference tests/test_flow_class.py:852-980, the four matrices that go through griddata without holes."""
    of = gpu
    f_s, f_sm, f_t, f_tm = k7_flows(lambda t, s, r, m=None: of.Flow.from_transforms(t, list(s), r, m))
    np.testing.assert_array_equal(f_s.valid_target(), K7_VALID_TARGET_S)
    np.testing.assert_array_equal(f_t.valid_source(), K7_VALID_SOURCE_T)
    np.testing.assert_array_equal(f_sm.valid_target(False), K7_VALID_TARGET_S_MASKED)
    np.testing.assert_array_equal(f_tm.valid_source(False), K7_VALID_SOURCE_T_MASKED)
    np.testing.assert_array_equal(of.valid_target(f_s.vecs, 's'), K7_VALID_TARGET_S)
    np.testing.assert_array_equal(of.valid_source(f_t.vecs, 't'), K7_VALID_SOURCE_T)


def test_translation_exact_s(gpu):
    """reference tests/test_utils.py:277-283, 's' branch: integer translation == ndimage.shift, exactly."""
    from scipy import ndimage
    of = gpu
    img = (np.random.default_rng(0).random((200, 240, 3)) * 255).astype(np.uint8)
    f = of.from_transforms([['translation', 10, 20]], [200, 240], 's')
    np.testing.assert_array_equal(of.apply_flow(f, img, 's'), ndimage.shift(img, [20, 10, 0]))


def test_invert_and_switch_ref_analytic(gpu):
    """reference tests/test_flow_class.py:501-573 at its own size (512 x 512) and tolerance (1e-3)."""
    of = gpu
    s = [512, 512]
    f_s = of.Flow.from_transforms([['rotation', 256, 256, 30]], s, 's')
    f_t = of.Flow.from_transforms([['rotation', 256, 256, 30]], s, 't')
    b_s = of.Flow.from_transforms([['rotation', 256, 256, -30]], s, 's')
    b_t = of.Flow.from_transforms([['rotation', 256, 256, -30]], s, 't')
    for got, want in ((f_s.invert(), b_s), (b_s.invert(), f_s), (f_s.invert('t'), b_t), (b_s.invert('t'), f_t),
                      (f_t.invert(), b_t), (b_t.invert(), f_t), (f_t.invert('s'), b_s), (b_t.invert('s'), f_s),
                      (f_t.switch_ref(), f_s), (f_s.switch_ref(), f_t)):
        assert got.ref == want.ref
        assert got.mask.sum() > 100000
        print("invert / switch_ref vs analytic: max abs error", float(np.abs(got.vecs[got.mask] - want.vecs[got.mask]).max()))
        # (the reference's own bar is 1e-3, tests/test_flow_class.py:528-572; measured: 1.5e-5 = one float32 ulp of a 180-px vector)
        np.testing.assert_allclose(got.vecs[got.mask], want.vecs[got.mask], rtol=1e-4, atol=1e-4)
    np.testing.assert_array_equal(of.invert_flow(f_s.vecs, 's'), f_s.invert().vecs)
    np.testing.assert_array_equal(of.switch_flow_ref(f_t.vecs, 't'), f_t.switch_ref().vecs)


@pytest.mark.parametrize("ref", ['s', 't'])
def test_combine_modes_analytic(gpu, ref):
    """reference tests/test_flow_class.py:1020-1057: all three modes recover the analytic third flow."""
    of = gpu
    shape = [512, 512]
    tr = [['rotation', 255.5, 255.5, -30], ['scaling', 100, 100, 0.8]]
    f1, f2, f3 = (of.Flow.from_transforms(t, shape, ref) for t in (tr[:1], tr[1:], tr))
    for got, want in ((f2.combine_with(f3, 1), f1), (f1.combine_with(f3, 2), f2), (f1.combine_with(f2, 3), f3)):
        assert isinstance(got, of.Flow) and got.ref == ref
        m = got.mask & want.mask
        assert m.sum() > 20000
        np.testing.assert_allclose(got.vecs[m], want.vecs[m], atol=5e-2)
    np.testing.assert_array_equal(of.combine_flows(f2.vecs, f3.vecs, 1, ref), f2.combine_with(f3, 1).vecs)


@pytest.mark.parametrize("ref", ['s', 't'])
def test_combine_modes_vs_oracle(gpu, oracle, ref):
    """Modes 1 and 2 against the oracle (same SciPy griddata as the reference) on a 96 x 128 field."""
    of = gpu
    shape = [96, 128]
    tr = [['rotation', 60, 50, -12], ['scaling', 30, 40, 0.9]]
    f2, f3 = of.Flow.from_transforms(tr[1:], shape, ref), of.Flow.from_transforms(tr, shape, ref)
    f1 = of.Flow.from_transforms(tr[:1], shape, ref)
    for mode, (a, b) in ((1, (f2, f3)), (2, (f1, f3))):
        got = a.combine_with(b, mode)
        want = oracle.OFlow(a.vecs, ref, a.mask).combine_with(oracle.OFlow(b.vecs, ref, b.mask), mode)
        both = got.mask & want.mask
        diff = got.mask ^ want.mask
        print("mode", mode, ref, "mask mismatches", int(diff.sum()), "of", diff.size, np.argwhere(diff)[:8].tolist())
        # mode 2 / ref 't' triangulates float32-ROUNDED points (flow_class.py:1398-1400): the warped border is ragged at
        # the 1e-6 px level, and a query position inside that band (here one: 4e-7 px inside the convex hull) is found
        # or not by Qhull's handling of the sliver facets there; everything else is exact
        assert diff.sum() <= (1 if (mode, ref) == (2, 't') else 0), (mode, ref, int(diff.sum()))
        assert both.sum() > 0.5 * want.mask.sum()
        np.testing.assert_allclose(got.vecs[both], want.vecs[both], rtol=RTOL, atol=ATOL)      # every node; stage by stage: test_gpu_chains.py


@pytest.mark.parametrize("ref", ['s', 't'])
def test_config3_mode1_full_size(gpu, ref):
    """BASELINE config 3 at full size (2160 x 3840): f2.combine_with(f3, mode=1) recovers the analytic rotation within
    the reference's own tolerance (tests/test_flow_class.py:1020-1057: atol 5e-2 inside both masks).  'sigma' = 1 scatter
    + 2 gathers (flow_class.py:1369-1370), 't' = 4 scatters + 1 gather (:1383-1385); HBM-resident end to end."""
    of = gpu
    shape = [2160, 3840]
    t_rot, t_scale = [['rotation', 1920, 1080, -20]], [['scaling', 1000, 800, 0.9]]
    f1 = of.Flow.from_transforms(t_rot, shape, ref)
    f2 = of.Flow.from_transforms(t_scale, shape, ref).to_device()
    f3 = of.Flow.from_transforms(t_rot + t_scale, shape, ref).to_device()
    got = f2.combine_with(f3, 1)
    assert got.ref == ref
    vecs, mask = got.to_host()
    assert mask.mean() > 0.3
    m = mask & f1.mask
    np.testing.assert_allclose(vecs[m], f1.vecs[m], atol=5e-2)
    # every scatter of the chain runs on a certified mesh or on the Delaunay path: no owner-map fallback
    assert f2.mesh_cert(+1 if ref == 's' else -1).certified == 1


def test_scatter_raw_abi(gpu, oracle):
    """ofl_scatter_linear (host entry): values, validity rules, query points and the no-points error."""
    import ctypes
    of = gpu
    nat, lib = of.native, of.native.load()
    H, W, C = 40, 56, 3
    rng = np.random.default_rng(2)
    flow = of.from_transforms([['rotation', 20, 25, 17], ['scaling', 20, 20, 0.9]], [H, W], 's')
    y, x = np.mgrid[:H, :W].astype('f')          # smooth non-affine part: every cell has a unique Delaunay diagonal
    flow = flow + np.stack([0.4 * np.sin(x / 7) * np.cos(y / 5), 0.3 * np.cos(x / 6) * np.sin(y / 8)], -1).astype('f')
    vals = rng.standard_normal((H, W, C)).astype('f')
    out = np.empty((H, W, C), np.float32)
    valid = np.empty((H, W), np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    nat.check(lib.ofl_scatter_linear(p(flow), 1, 0, None, p(vals), C, None, H, W, None, p(out), p(valid), 0))
    want = oracle.scatter_griddata(flow, vals, None)
    hull = oracle.scatter_griddata(flow, np.ones((H, W), 'f'), None) == 1
    # a non-affine flow bends the border of the warped grid: the pockets between the mesh and its convex hull are
    # triangulated like SciPy triangulates them -- every node agrees
    v = valid.astype(bool)
    np.testing.assert_array_equal(v, hull)
    assert not ambiguous_for(flow).any()
    np.testing.assert_allclose(out, want, rtol=RTOL, atol=ATOL)
    none = np.zeros((H, W), np.uint8)
    rc = lib.ofl_scatter_linear(p(flow), 1, 0, p(none), p(vals), C, None, H, W, None, p(out), p(valid), 0)
    assert rc == nat.E_NOPOINTS
    with pytest.raises(ValueError):
        of.Flow(flow, 's', none.astype(bool)).valid_target()


def test_scatter_4k_invert(gpu):
    """BASELINE config 3 geometry at full size: invert an 's' scaling flow at 2160 x 3840 and check it against
    the analytic inverse inside the result mask (size-independent property; SciPy would need minutes)."""
    of = gpu
    shape = [2160, 3840]
    f = of.Flow.from_transforms([['scaling', 1000, 800, 0.9]], shape, 's')
    inv = f.invert()
    want = of.Flow.from_transforms([['scaling', 1000, 800, 1 / 0.9]], shape, 's')
    assert inv.mask.mean() > 0.75
    print("4K invert vs analytic: max abs error", float(np.abs(inv.vecs[inv.mask] - want.vecs[inv.mask]).max()))
    np.testing.assert_allclose(inv.vecs[inv.mask], want.vecs[inv.mask], rtol=1e-4, atol=2e-4)      # measured 3e-5: one ulp of a 400-px vector
    # round trip: inverting twice returns the original inside the doubly valid area
    back = inv.invert()
    m = back.mask
    print("4K invert round trip: max abs error", float(np.abs(back.vecs[m] - f.vecs[m]).max()))
    np.testing.assert_allclose(back.vecs[m], f.vecs[m], rtol=1e-4, atol=2e-4)


def test_track_pts_matches_reference(gpu, golden):
    """Sparse point tracking (reference utils.py:547-622, tests/test_utils.py:543-571) against
    outputs of the real reference: bilinear 's' mode bit-exact (float64, same operation order, including the
    reference's swapped b/c pairing), 't' mode and s_exact_mode through the scatter kernel's query pass."""
    of = gpu
    g = golden
    pf, pi = g['track/pts_f'], g['track/pts_i']
    for name in ('rot', 'wob'):
        for ref in ('s', 't'):
            tag = 'track/{}_{}'.format(name, ref)
            flow = g[tag + '/flow']
            got = of.track_pts(flow, ref, pf)
            assert got.dtype == np.float64
            if ref == 's':
                np.testing.assert_array_equal(got, g[tag + '/float'])
                np.testing.assert_array_equal(of.track_pts(flow, ref, pi), g[tag + '/int'])
                ex = of.track_pts(flow, ref, pf, s_exact_mode=True)
                # regular grid: every cell is an exact square (both diagonals Delaunay); affine flow -> equal up to
                # otherwise within the reference's own "order of 0.01 px" remark (utils.py:596-598)
                np.testing.assert_allclose(ex, g[tag + '/exact'], rtol=0, atol=1e-6 if name == 'rot' else 2e-2)   # float32 flow noise ~1e-7
            else:
                np.testing.assert_allclose(got, g[tag + '/float'], rtol=1e-9, atol=1e-9)
            r = of.track_pts(flow, ref, pf, int_out=True)
            np.testing.assert_array_equal(r, g[tag + '/float_int_out'])
            assert r.dtype == g[tag + '/float_int_out'].dtype
    ft = of.Flow(g['track/status_t/flow'], 't', g['track/status_t/mask'])
    warped, status = ft.track(g['track/status_t/pts'], get_valid_status=True)
    np.testing.assert_array_equal(status, g['track/status_t/status'])
    np.testing.assert_allclose(warped, g['track/status_t/warped'], rtol=1e-9, atol=1e-9)
    # reference tests/test_utils.py:545-571 at its own size and tolerances
    f_s = of.from_transforms([['rotation', 0, 0, 30]], [512, 512], 's')
    f_t = of.from_transforms([['rotation', 0, 0, 30]], [512, 512], 't')
    pts = np.array([[20.5, 10.5], [8.3, 7.2], [120.4, 160.2]])
    want = [[12.5035207776, 19.343266740], [3.58801085141, 10.385382907], [24.1694586156, 198.93726969]]
    np.testing.assert_allclose(of.track_pts(f_s, 's', pts), want, atol=1e-1, rtol=1e-2)
    np.testing.assert_allclose(of.track_pts(f_s, 's', pts, s_exact_mode=True), want, rtol=1e-7)
    np.testing.assert_allclose(of.track_pts(f_t, 't', pts), want, atol=1e-6, rtol=1e-6)
    r = of.track_pts(f_t, 't', pts, int_out=True)
    np.testing.assert_array_equal(r, np.round(want))
    f = of.from_transforms([['translation', 10, 20]], [512, 512], 's')
    np.testing.assert_array_equal(of.track_pts(f, 's', np.array([[20, 10], [8, 7]])), [[40, 20], [28, 17]])
    with pytest.raises(IndexError):
        of.track_pts(f_s, 's', np.array([[600.5, 10.5]]))
    with pytest.raises(TypeError):
        of.Flow(f_s, 's').track(pts, True, get_valid_status='test')


def test_apply_with_padding_both_refs(gpu, oracle):
    """Flow.apply(padding=..., cut=...) (reference flow_class.py:588-595, 636-664, 673-678): a flow smaller than
    its target, 't' (zero padding, one gather launch with offsets) and 's' (edge padding, scatter kernel),
    with valid areas, cut and uncut, against the oracle's literal restatement."""
    of = gpu
    rng = np.random.default_rng(6)
    H, W, pad = 70, 90, [6, 9, 11, 4]
    fh, fw = H - pad[0] - pad[1], W - pad[2] - pad[3]
    img = rng.random((H, W, 3), dtype=np.float32)
    tmask = rng.random((H, W)) > 0.1
    for ref in ('t', 's'):
        v = of.from_transforms([['rotation', 20, 25, 9], ['scaling', 30, 20, 0.95]], [fh, fw], ref)
        y, x = np.mgrid[:fh, :fw].astype('f')
        v = (v + np.stack([0.5 * np.sin(x / 7), 0.4 * np.cos(y / 6)], -1)).astype('f')   # unique Delaunay diagonals
        f, o = of.Flow(v, ref), oracle.OFlow(v, ref)
        for cut in (True, False):
            for tm in (None, tmask):
                gw, gv = f.apply(img, tm, return_valid_area=True, padding=pad, cut=cut)
                ow, ov = o.apply(img, tm, return_valid_area=True, padding=pad, cut=cut)
                assert gw.shape == ow.shape and gv.shape == ov.shape
                if ref == 't':
                    np.testing.assert_array_equal(gw, ow)
                    np.testing.assert_array_equal(gv, ov)
                else:
                    np.testing.assert_array_equal(gv, ov)
                    np.testing.assert_allclose(gw, ow, rtol=RTOL, atol=ATOL)
        g2 = f.apply(img, padding=pad)
        o2 = o.apply(img, padding=pad)
        if ref == 't':
            np.testing.assert_array_equal(g2, o2)
        else:
            np.testing.assert_allclose(g2, o2, rtol=RTOL, atol=ATOL)


def test_discontinuous_fields_vs_reference(gpu, golden):
    """Motion boundaries (a block moving over a static background; outputs of the real reference): the cells along
    the boundary stretch or fold.  The Delaunay path triangulates the points globally like SciPy: masks bit-exact
    and values equal wherever SciPy's triangulation is unique.  (The static background is an exact lattice -- every
    cell co-circular -- so for image values these two fixtures leave little to compare; the generic-background case
    of test_gpu_scatter_exact.py::test_exact_path_matches_reference_outputs[block_generic] has no such cells.)"""
    from test_oracle import disc_tags
    of = gpu
    for tag in disc_tags(golden):
        op, name = tag.split('/')
        vecs = golden[tag + '/in_vecs']
        f = of.Flow(vecs, 's', golden[tag + '/in_mask'])
        amb = ambiguous_for(vecs)
        if op == 'disc_apply':
            w, v = f.apply(golden['disc/' + name + '/img'], return_valid_area=True)
            np.testing.assert_array_equal(v, golden[tag + '/out_valid'], err_msg=tag)
            np.testing.assert_allclose(w[~amb], golden[tag + '/out'][~amb], rtol=RTOL, atol=ATOL, err_msg=tag)
            n = check_admissible(golden, tag, (w, v), amb)
            assert n['judged'] >= amb.sum() > 1900 and n['not_judged'] == 0      # the lattice background: nearly every node is judged here
        elif op == 'disc_invert':
            r = f.invert()
            np.testing.assert_array_equal(r.mask, golden[tag + '/out_mask'], err_msg=tag)
            np.testing.assert_allclose(r.vecs[~amb], golden[tag + '/out_vecs'][~amb], rtol=RTOL, atol=1e-5, err_msg=tag)
            check_admissible(golden, tag, r, amb)
        else:
            np.testing.assert_array_equal(f.valid_target(), golden[tag + '/out'], err_msg=tag)


def test_apply_entry_points_agree_both_refs(gpu):
    """Restates reference tests/test_flow_class.py:417-438 (Flow.apply == apply_flow for 3-D, 2-D and Flow targets,
    with and without a mask, both references) and tests/test_utils.py:267-283 (rotation vs scipy.ndimage.rotate,
    loose; translation vs scipy.ndimage.shift, exact) on a smooth synthetic uint8 image."""
    from scipy import ndimage
    of = gpu
    yy, xx = np.mgrid[:512, :512]
    img = np.stack([127 + 100 * np.sin(xx / 23.0) * np.cos(yy / 31.0), 127 + 90 * np.cos(xx / 17.0 + yy / 41.0),
                    (xx + yy) / 4.0], -1).astype(np.uint8)
    for ref in ('t', 's'):
        flow = of.Flow.from_transforms([['rotation', 30, 50, 30]], img.shape[:2], ref)
        mask = np.ones(img.shape[:2], bool)
        want = of.apply_flow(flow.vecs, img, ref)
        np.testing.assert_array_equal(flow.apply(img), want)
        np.testing.assert_array_equal(flow.apply(img, mask, return_valid_area=True)[0], want)
        want2 = of.apply_flow(flow.vecs, img[..., 0], ref)
        assert want2.shape == img.shape[:2]
        np.testing.assert_array_equal(flow.apply(img[..., 0]), want2)
        np.testing.assert_array_equal(flow.apply(img[..., 0], mask, return_valid_area=True)[0], want2)
        np.testing.assert_array_equal(want2, want[..., 0])
        np.testing.assert_array_equal(flow.apply(flow).vecs, of.apply_flow(flow.vecs, flow.vecs, ref))
        rot = of.Flow.from_transforms([['rotation', 255.5, 255.5, -30]], img.shape[:2], ref).vecs
        control = ndimage.rotate(img[..., 0], -30, reshape=False)
        np.testing.assert_allclose(control[200:300, 200:300], of.apply_flow(rot, img[..., 0], ref)[200:300, 200:300], atol=20, rtol=0.05)
        tr = of.Flow.from_transforms([['translation', 10, 20]], img.shape[:2], ref).vecs
        np.testing.assert_array_equal(of.apply_flow(tr, img, ref), ndimage.shift(img, [20, 10, 0]))


def test_scatter_row_bands_equal_full_result(gpu):
    """ofl_scatter_rows_dev: one field split into row bands over several GPUs (replicated inputs, disjoint output
    rows).  The concatenated bands equal the single-GPU result bit for bit -- smooth field with a speckled point
    mask (gap fill across the band seams), a discontinuous field, and the tiled-Sintel geometry of config 5."""
    import os
    of = gpu
    from oflibnumpy_amd import device as dev, sharding
    rng = np.random.default_rng(31)
    h, w = 203, 296
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    smooth = of.Flow.from_transforms([['rotation', 100, 80, 17], ['scaling', 50, 60, 0.93]], [h, w], 's').vecs + \
        np.stack([1.5 * np.sin(xx / 19) * np.cos(yy / 23), 1.2 * np.cos(xx / 17)], -1).astype(np.float32)
    block = np.zeros((h, w, 2), np.float32)
    block[60:140, 90:210] = [11.0, -7.0]
    flo = of.load_sintel(os.path.join(os.path.dirname(__file__), "golden", "sintel.flo"))
    tiled = np.tile(flo, (21, 15, 1))[:h, :w]
    img = rng.random((h, w, 3), dtype=np.float32)
    for name, vecs, pm in (("smooth+speckle", smooth, rng.random((h, w)) > 0.15), ("block", block, None), ("tiled sintel", tiled, None)):
        f = dev.DeviceBuffer.from_host(np.ascontiguousarray(vecs, np.float32))
        vals = dev.DeviceBuffer.from_host(img)
        pmb = dev.DeviceBuffer.from_host(pm.astype(np.uint8)) if pm is not None else None
        vm = dev.DeviceBuffer.from_host((rng.random((h, w)) > 0.1).astype(np.uint8))
        out, valid = dev.DeviceBuffer(h * w * 12), dev.DeviceBuffer(h * w)
        dev.scatter_linear(f, +1, pmb, vals, 3, vm, h, w, None, out, valid, 0)
        full, fullv = out.to_host((h, w, 3), np.float32), valid.to_host((h, w), np.uint8)
        for world in (8, 3):
            parts, vparts = [], []
            for r in range(world):
                r0, r1 = sharding.row_band(h, r, world)
                ob, vb = dev.DeviceBuffer((r1 - r0) * w * 12), dev.DeviceBuffer((r1 - r0) * w)
                dev.scatter_rows(f, +1, pmb, vals, 3, vm, h, w, r0, r1 - r0, ob, vb)
                parts.append(ob.to_host((r1 - r0, w, 3), np.float32))
                vparts.append(vb.to_host((r1 - r0, w), np.uint8))
            np.testing.assert_array_equal(np.concatenate(parts), full, err_msg=name)
            np.testing.assert_array_equal(np.concatenate(vparts), fullv, err_msg=name)
        assert fullv.mean() > 0.2, name


def test_strong_magnification_all_triangles_large(gpu):
    """A field that magnifies 40x turns EVERY cell triangle into a large one (bounding boxes of ~1 700 nodes): 2.4
    million of them at 1100 x 1100, more than any fixed-size list -- the large-triangle list is sized for the whole
    mesh.  The inverse of the scaling is the scaling by 1/40 (analytic, as reference tests/test_flow_class.py:528-572)."""
    of = gpu
    s = (1100, 1100)
    f = of.Flow.from_transforms([['scaling', 550, 550, 40.0]], s, 's')
    inv = f.invert()
    want = of.Flow.from_transforms([['scaling', 550, 550, 1 / 40.0]], s, 's')
    assert inv.mask.mean() > 0.99
    print("40x magnification vs analytic: max abs error", float(np.abs(inv.vecs[inv.mask] - want.vecs[inv.mask]).max()))
    np.testing.assert_allclose(inv.vecs[inv.mask], want.vecs[inv.mask], rtol=1e-4, atol=1e-4)      # measured: exact
    assert f.valid_target().mean() > 0.99


def test_speckled_mask_with_dropped_corners(gpu, oracle):
    """A random point mask that also drops image corners.  Validity masks equal SciPy's bit for bit and flow-valued
    results agree inside the mask; the 4K case bounds the time of the exact (Delaunay) path with 5 % dropped points."""
    import time
    of, O = gpu, oracle
    rng = np.random.default_rng(17)
    shape = (60, 84)
    for tr in ([['rotation', 30, 40, 25]], [['scaling', 20, 30, 0.8]]):
        m = rng.random(shape) > 0.1
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = False
        m[1, 0] = m[0, 1] = False
        f = of.Flow.from_transforms(tr, shape, 's', m)
        o = O.OFlow(f.vecs, 's', m)
        np.testing.assert_array_equal(f.valid_target(), o.valid_target())
        got, want = f.invert(), o.invert()
        np.testing.assert_array_equal(got.mask, want.mask)
        np.testing.assert_allclose(got.vecs[got.mask], want.vecs[got.mask], rtol=1e-4, atol=1e-4)
    h, w = 2160, 3840
    m = rng.random((h, w)) > 0.05
    m[0, 0] = m[-1, -1] = False
    d = of.Flow.from_transforms([['rotation', 1920, 1080, -20], ['scaling', 1000, 800, 0.9]], [h, w], 's', m).to_device()
    d.stats()
    d.invert()
    t0 = time.perf_counter()
    r = d.invert()
    of.native.check(of.native.load().ofl_device_sync())
    assert time.perf_counter() - t0 < 0.2, "the Delaunay path fell off the device"
    assert r.to_host()[1].mean() > 0.5


def test_randomised_bands_masks_and_folds(gpu):
    """Seeded sweep over ragged shapes (2 .. 90 x 2 .. 140), smooth / shifted / folded fields, random point and value
    masks, 1-3 channels, both signs: the scatter result is finite, and row bands (1 .. 5 ranks) of the scatter AND of the
    gather (uint8 / float32 / int16 images) concatenate to the full result bit for bit."""
    of = gpu
    from oflibnumpy_amd import device as dev, sharding
    rng = np.random.default_rng(123)
    n_ok = 0
    for it in range(60):
        h, w = int(rng.integers(2, 90)), int(rng.integers(2, 140))
        yy, xx = np.mgrid[:h, :w].astype(np.float32)
        amp = rng.uniform(0, 6)
        vecs = np.stack([amp * np.sin(xx / rng.uniform(3, 30) + yy / rng.uniform(5, 40)), amp * np.cos(xx / rng.uniform(4, 25))], -1).astype(np.float32)
        vecs += rng.uniform(-8, 8, 2).astype(np.float32)
        if it % 4 == 0:
            vecs[rng.random((h, w)) < 0.05] += 15          # discontinuities / folds
        pm = None if it % 3 == 0 else (rng.random((h, w)) > rng.uniform(0, 0.5))
        if pm is not None and pm.sum() < 3:
            pm = None
        vm = rng.random((h, w)) > 0.2
        C = int(rng.integers(1, 4))
        img = rng.random((h, w, C), dtype=np.float32)
        f = dev.DeviceBuffer.from_host(vecs)
        vals = dev.DeviceBuffer.from_host(img)
        pmb = dev.DeviceBuffer.from_host(pm.astype(np.uint8)) if pm is not None else None
        vmb = dev.DeviceBuffer.from_host(vm.astype(np.uint8))
        out, valid = dev.DeviceBuffer(h * w * C * 4), dev.DeviceBuffer(h * w)
        sign = 1 if it % 2 else -1
        dev.scatter_linear(f, sign, pmb, vals, C, vmb, h, w, None, out, valid, 0)
        full, fullv = out.to_host((h, w, C), np.float32), valid.to_host((h, w), np.uint8)
        assert np.isfinite(full).all()
        world = int(rng.integers(1, 6))
        parts, vparts = [], []
        for r in range(world):
            r0, r1 = sharding.row_band(h, r, world)
            if r1 <= r0:
                continue
            ob, vb = dev.DeviceBuffer((r1 - r0) * w * C * 4), dev.DeviceBuffer((r1 - r0) * w)
            dev.scatter_rows(f, sign, pmb, vals, C, vmb, h, w, r0, r1 - r0, ob, vb)
            parts.append(ob.to_host((r1 - r0, w, C), np.float32)); vparts.append(vb.to_host((r1 - r0, w), np.uint8))
        assert np.array_equal(np.concatenate(parts), full), (it, h, w, world)
        assert np.array_equal(np.concatenate(vparts), fullv), (it, h, w, world)
        # gather bands, several dtypes
        if w % 2 == 0:
            for dt in (np.uint8, np.float32, np.int16):
                im = (rng.random((h, w, C)) * 200).astype(dt)
                dimg = dev.DeviceImage.from_host(im)
                fm = dev.DeviceBuffer.from_host((rng.random((h, w)) > 0.1).astype(np.uint8))
                fd, fv = dev.gather_bilinear(dimg, f, (h, w), -1, smask=vmb, fmask=fm, want_valid=True)
                fd, fv = fd.to_host(), fv.to_host((h, w), np.uint8)
                ps, vs = [], []
                for r in range(world):
                    r0, r1 = sharding.row_band(h, r, world)
                    if r1 <= r0:
                        continue
                    fr = dev.DeviceBuffer.from_host(np.ascontiguousarray(vecs[r0:r1]))
                    fmr = dev.DeviceBuffer.from_host(np.ascontiguousarray(fm.to_host((h, w), np.uint8)[r0:r1]))
                    d, v = dev.gather_rows(dimg, r0, r1 - r0, fr, -1, smask=vmb, fmask_rows=fmr, want_valid=True)
                    ps.append(d.to_host()); vs.append(v.to_host((r1 - r0, w), np.uint8))
                assert np.array_equal(np.concatenate(ps), fd) and np.array_equal(np.concatenate(vs), fv), (it, h, w, dt)
        n_ok += 1
    assert n_ok == 60


def test_randomised_masks_against_scipy(gpu, oracle):
    """Seeded sweep against the SciPy oracle on small ragged shapes: similarity transforms with and without a smooth
    non-affine term, speckled point masks: valid_target() and the mask of invert() -- hull membership, dropped points,
    gap fill -- are bit-exact.  (valid_target(consider_mask=False) interpolates the speckled mask VALUES, which depends
    on the Delaunay diagonal of co-circular cells -- deviation (a) -- and is covered by the reference-output tests.)"""
    of, O = gpu, oracle
    rng = np.random.default_rng(321)
    for it in range(45):
        h, w = int(rng.integers(6, 120)), int(rng.integers(6, 160))
        kind = it % 3
        if kind == 0:
            tr = [['rotation', rng.uniform(0, w), rng.uniform(0, h), rng.uniform(-40, 40)], ['scaling', rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.7, 1.3)]]
        elif kind == 1:
            tr = [['translation', rng.uniform(-6, 6), rng.uniform(-6, 6)], ['scaling', rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.8, 1.2)]]
        else:
            tr = [['rotation', w / 2, h / 2, rng.uniform(-15, 15)]]
        m = rng.random((h, w)) > rng.uniform(0, 0.2)
        if it % 5 == 0:
            m[:] = True
        if it % 4 == 1:                                 # a rectangular hole, possibly deeper than the ring search
            hh, hw = int(rng.integers(2, max(3, h // 2))), int(rng.integers(2, max(3, w // 2)))
            y0, x0 = int(rng.integers(1, h - hh)), int(rng.integers(1, w - hw))
            m[y0:y0 + hh, x0:x0 + hw] = False
        f = of.Flow.from_transforms(tr, [h, w], 's', m)
        if it % 2:
            yy, xx = np.mgrid[:h, :w].astype(np.float32)
            f = of.Flow(f.vecs + np.stack([0.4 * np.sin(xx / 9) * np.cos(yy / 7), 0.3 * np.cos(xx / 8)], -1).astype(np.float32), 's', m)
        o = O.OFlow(f.vecs, 's', m)
        np.testing.assert_array_equal(f.valid_target(), o.valid_target(), err_msg=str((it, h, w, tr)))
        np.testing.assert_array_equal(f.invert().mask, o.invert().mask, err_msg=str((it, h, w, tr)))


def test_large_hole_in_point_mask_matches_scipy(gpu, oracle):
    """A hole of the point mask much wider than any ring search (70 x 100 px in 160 x 220): SciPy bridges it with long
    triangles and reports the bridged nodes valid; the Delaunay path builds the same triangles (the rim points finish
    in the wave / workgroup star passes).  Masks are bit-exact; an affine field is reproduced across the hole; row bands
    still concatenate to the full result."""
    of, O = gpu, oracle
    from oflibnumpy_amd import device as dev, sharding
    shape = (160, 220)
    m = np.ones(shape, bool)
    m[40:110, 60:160] = False
    m[5:9, 200:215] = False                                      # and a shallow one
    for tr in ([['rotation', 100, 70, 12], ['scaling', 30, 40, 0.95]], [['translation', 4.5, -3.25]]):
        f = of.Flow.from_transforms(tr, shape, 's', m)
        o = O.OFlow(f.vecs, 's', m)
        np.testing.assert_array_equal(f.valid_target(), o.valid_target())
        got, want = f.invert(), o.invert()
        np.testing.assert_array_equal(got.mask, want.mask)
        assert got.mask[60:90, 90:130].all()                      # the middle of the hole is bridged
        np.testing.assert_allclose(got.vecs[got.mask], want.vecs[got.mask], rtol=1e-4, atol=2e-4)
    # bands vs full with the deep fill
    rng = np.random.default_rng(4)
    h, w = shape
    img = rng.random((h, w, 2), dtype=np.float32)
    fb, vals = dev.DeviceBuffer.from_host(f.vecs), dev.DeviceBuffer.from_host(img)
    pm = dev.DeviceBuffer.from_host(m.astype(np.uint8))
    out, valid = dev.DeviceBuffer(h * w * 8), dev.DeviceBuffer(h * w)
    dev.scatter_linear(fb, +1, pm, vals, 2, pm, h, w, None, out, valid, 0)
    full, fullv = out.to_host((h, w, 2), np.float32), valid.to_host((h, w), np.uint8)
    parts, vparts = [], []
    for r in range(4):
        r0, r1 = sharding.row_band(h, r, 4)
        ob, vb = dev.DeviceBuffer((r1 - r0) * w * 8), dev.DeviceBuffer((r1 - r0) * w)
        dev.scatter_rows(fb, +1, pm, vals, 2, pm, h, w, r0, r1 - r0, ob, vb)
        parts.append(ob.to_host((r1 - r0, w, 2), np.float32)); vparts.append(vb.to_host((r1 - r0, w), np.uint8))
    np.testing.assert_array_equal(np.concatenate(parts), full)
    np.testing.assert_array_equal(np.concatenate(vparts), fullv)
    assert fullv[60:90, 90:130].all()


def test_float64_targets_keep_their_precision(gpu, oracle):
    """apply_flow(.., 's') of a float64 image: griddata interpolates in float64 and the reference returns
    result.astype(float64) (utils.py:253-258) -- the float64 scatter entry reproduces SciPy to 1e-11 where the
    triangulation is unique (a smooth non-affine field), float32 images to float32 rounding."""
    of, O = gpu, oracle
    rng = np.random.default_rng(9)
    shape = (48, 64)
    yy, xx = np.mgrid[:shape[0], :shape[1]].astype(np.float32)
    vecs = of.Flow.from_transforms([['rotation', 30, 20, 11], ['scaling', 10, 10, 0.93]], shape, 's').vecs + \
        np.stack([0.7 * np.sin(xx / 9) * np.cos(yy / 7), 0.5 * np.cos(xx / 8)], -1).astype(np.float32)
    img = rng.random(shape + (3,)) * 1e3 + 1e-7 * rng.random(shape + (3,))
    f = of.Flow(vecs, 's')
    got, valid = f.apply(img, return_valid_area=True)
    want, wvalid = O.OFlow(vecs, 's').apply(img, return_valid_area=True)
    assert got.dtype == np.float64
    # The reference compares the interpolated mask channel with 1 in the TARGET's dtype (flow_class.py:668): in float64
    # the sum c0 + c1 + (1 - c0 - c1) misses 1.0 by one ulp at ~3 % of the nodes, which SciPy's own rounding decides.
    # The kernel applies the float32 rule to every dtype: its valid area is the float32 one, a superset of that noise.
    v32 = f.apply(img.astype(np.float32), return_valid_area=True)[1]
    np.testing.assert_array_equal(valid, v32)
    np.testing.assert_array_equal(v32, O.OFlow(vecs, 's').apply(img.astype(np.float32), return_valid_area=True)[1])
    assert not (wvalid & ~valid).any() and (valid & ~wvalid).mean() < 0.08
    np.testing.assert_allclose(got[valid], want[valid], rtol=1e-11, atol=1e-9)
    got32 = f.apply(img.astype(np.float32))
    assert got32.dtype == np.float32
    np.testing.assert_allclose(got32[valid], want[valid], rtol=2e-6, atol=1e-4)


def test_integer_targets_valid_area_s(gpu, oracle):
    """'s' warp of integer images with a valid area: the reference concatenates the mask into the integer array, so the
    interpolated mask is np.round-ed before `== 1` (utils.py:256-257, flow_class.py:644, 668) -- looser than the float
    rule.  Default (int8) and boolean target masks, uint8 / int16 images, speckled flow mask, against the oracle."""
    of, O = gpu, oracle
    rng = np.random.default_rng(13)
    shape = (40, 56)
    yy, xx = np.mgrid[:shape[0], :shape[1]].astype(np.float32)
    vecs = of.Flow.from_transforms([['rotation', 20, 30, 9], ['scaling', 10, 10, 1.05]], shape, 's').vecs + \
        np.stack([0.6 * np.sin(xx / 9) * np.cos(yy / 7), 0.5 * np.cos(xx / 8)], -1).astype(np.float32)
    fm = rng.random(shape) > 0.08
    f, o = of.Flow(vecs, 's', fm), O.OFlow(vecs, 's', fm)
    tm = np.ones(shape, bool)
    tm[10:22, 15:40] = False            # a solid invalid region: its outline is where the rounded rule and the float rule differ
    # nodes in simplices SciPy itself cannot pin (none on this non-affine field unless the speckle leaves co-circular sites):
    # everything else is compared exactly -- no band around the outline, no tolerance on counts
    amb_kept, amb_all = ambiguous_for(vecs, fm), ambiguous_for(vecs)
    print("non-unique nodes: {} with the speckled point set, {} with every point".format(int(amb_kept.sum()), int(amb_all.sum())))
    for dt in (np.uint8, np.int16):
        img = (rng.random(shape + (3,)) * 200).astype(dt)
        for tmask in (None, tm):
            got, valid = f.apply(img, tmask, return_valid_area=True)
            want, wvalid = o.apply(img, tmask, return_valid_area=True)
            np.testing.assert_array_equal(valid[~amb_kept], wvalid[~amb_kept], err_msg=str((dt, tmask is None)))
            d = np.abs(got.astype(int) - want.astype(int)).max(-1)[~amb_kept & wvalid]
            assert (d <= 1).all() and (d > 0).mean() < 1e-3, (dt, tmask is None)       # a value within 1e-6 of x.5 may round the other way
            both = fm if tmask is None else fm & tmask
            rows = np.concatenate([img, both[..., None]], -1).reshape(-1, 4)[fm.ravel()]
            sa.assert_equal_or_admissible(str((dt, tmask is None)), warped_points(vecs, fm), rows, shape, got, want, amb_kept, valid, wvalid,
                                          sa.rule_eq1_rounded, rtol=RTOL, atol=ATOL, levels=True)
        # the rounding rule really is looser than the float rule along the outline -- and the kernel follows it node for node
        w_int = o.apply(img, tm, return_valid_area=True)[1]
        w_flt = o.apply(img.astype(np.float32), tm, return_valid_area=True)[1]
        assert w_int.sum() > w_flt.sum() + 20
        # values with all points kept
        got, valid = of.Flow(vecs, 's').apply(img, tm, return_valid_area=True)
        want, wvalid = O.OFlow(vecs, 's').apply(img, tm, return_valid_area=True)
        np.testing.assert_array_equal(valid[~amb_all], wvalid[~amb_all])
        inner = of.Flow(vecs, 's').valid_target() & ~amb_all
        d = np.abs(got.astype(int) - want.astype(int)).max(-1)
        assert (d[inner] <= 1).all() and (d[inner] > 0).mean() < 1e-3
        sa.assert_equal_or_admissible(str(dt), warped_points(vecs), np.concatenate([img, tm[..., None]], -1).reshape(-1, 4), shape, got, want,
                                      amb_all, valid, wvalid, sa.rule_eq1_rounded, rtol=RTOL, atol=ATOL, levels=True)


def test_track_pts_t_positions_outside_the_image(gpu, oracle):
    """track_pts(..., 't') interpolates on the points x - f (utils.py:610-615); a flow that carries them out of the image
    leaves query positions that are inside their convex hull but next to no grid node the triangulation covers.  griddata
    interpolates there, and so does the query pass: its walk is seeded from the point set when no owned node is near
    (a non-affine field, so the Delaunay path with its visibility walk answers, not the certified mesh)."""
    of, O = gpu, oracle
    shape = (64, 80)
    yy, xx = np.mgrid[:shape[0], :shape[1]].astype(np.float32)
    vecs = np.stack([-100 + 0.8 * np.sin(xx / 9) * np.cos(yy / 7), 0.6 * np.cos(xx / 8) * np.sin(yy / 6)], -1).astype(np.float32)
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(2, 60, 40), rng.uniform(103, 176, 40)], 1)          # (row, col): columns 103 .. 176 of an 80-column image
    pts = np.concatenate([pts, [[30.0, 40.0], [-5.0, 120.0], [30.0, 500.0]]])          # and three positions outside the hull
    got = of.track_pts(vecs, 't', pts)
    want = O.track_pts(vecs, 't', pts.copy())
    assert np.abs(want[:40] - pts[:40]).max() > 50                                      # they are interpolated, not dropped
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-7)
