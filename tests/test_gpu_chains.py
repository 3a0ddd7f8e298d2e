"""GPU parity of the COMPOSED paths -- combine_with modes 1 / 2, invert, switch_ref -- at north_star's tolerance
(1e-4 relative, here rtol 1e-4 / atol 2e-5) instead of the looser bars the chains carried in rounds 1-2.

A chain is a sequence of stages (negation, sum, 't' gather = cv2.remap, 's' scatter = scipy griddata); the oracle
(oracle/np_oracle.py: the reference's operation sequence, flow_class.py:697-753, 1357-1410) records every stage.  Two
kinds of comparison, both per stage:

* ISOLATED: the product runs ONE stage on the oracle's inputs of that stage.  Gathers and sums must be bit-exact, a
  scatter within the tolerance, masks included, on EVERY node: the data of these chains are flow vectors of affine fields,
  which no choice among co-circular diagonals (scatter_util.nonunique_nodes, counted and printed) can change.  The one
  exemption is scatter_util.hull_band: positions within 1e-5 px of the border of the convex hull of the stage's point set,
  where Qhull's sliver facets decide hull membership (one node of mode 2 / 't' in the first case).
* NATIVE: the product runs the whole chain on its own intermediates.  A node may leave the tolerance only for a
  reason that is a property of the reference's arithmetic, and every such node is attributed to its stage and printed:
  (i) a 't' gather whose sampling coordinate snaps to a different 1/32-px step (cv2.remap's INTER_BITS = 5) because
  the two sampling fields differ in their last float32 bits -- the sample then moves by 1/32 px, the value by
  gradient / 32; (ii) a scatter node in a non-unique simplex; (iii) anything downstream of (i) / (ii): a tap, a
  summand, a scattered point within reach of the node.  Nodes with no such reason must agree.
"""
import numpy as np
import pytest

from scatter_util import nonunique_nodes, warped_points, hull_band
import scatter_admissible as sa

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5

# (result, op, operands): 'a' = self, 'b' = the other operand of combine_with
CHAINS = {
    ('mode1', 's'): [('g', 'invert_t', 'b'), ('sw', 'switch_ref', 'a'), ('ga', 'apply', 'g', 'sw'), ('h', 'add', 'g', 'ga'),
                     ('ha', 'apply', 'h', 'a'), ('res', 'sub', 'b', 'ha')],                       # flow_class.py:1369-1370
    ('mode1', 't'): [('as', 'switch_ref', 'a'), ('bs', 'switch_ref', 'b'), ('ai', 'invert_t', 'as'), ('bi', 'invert_s', 'b'),
                     ('aa', 'apply', 'ai', 'bi'), ('h', 'add', 'as', 'aa'), ('ha', 'apply', 'h', 'as'), ('r', 'sub', 'bs', 'ha'),
                     ('res', 'switch_ref', 'r')],                                                 # :1383-1385
    ('mode2', 's'): [('d', 'sub', 'b', 'a'), ('res', 'apply', 'a', 'd')],                         # :1390
    ('mode2', 't'): [('rs', 'resample', 'a', 'b'), ('res', 'sub', 'b', 'rs')],                    # :1398-1410
    ('invert', 's'): [('n', 'neg', 'a'), ('res', 'apply', 'a', 'n')],                             # :746
    ('invert', 't'): [('n', 'invert_s', 'a'), ('res', 'switch_ref', 'n')],                        # :753
    ('switch', 's'): [('res', 'switch_ref', 'a')],                                                # :716-726
    ('switch', 't'): [('res', 'switch_ref', 'a')],
}


class OracleBackend:
    def __init__(self, O):
        self.O = O

    def flow(self, v, r, m):
        return self.O.OFlow(v, r, m)

    def resample(self, a, b):
        from oracle.np_oracle import _mode2_t_resample
        return _mode2_t_resample(a, b)


class ProductBackend:
    def __init__(self, of):
        self.of = of

    def flow(self, v, r, m):
        return self.of.Flow(v, r, m)

    def resample(self, a, b):
        """the inline griddata of mode 2 / 't' has no public method of its own: f3 - (f3 - resampled) is not exact, so the
        device layer's stage is called (DeviceFlow._resample_to, the only caller is combine_with)"""
        return self.of.Flow.from_device(a.to_device()._resample_to(b.to_device()))


def run_stage(be, op, xs):
    if op == 'neg':
        return -xs[0]
    if op == 'invert_t':
        return xs[0].invert('t')
    if op == 'invert_s':
        return xs[0].invert('s')
    if op == 'switch_ref':
        return xs[0].switch_ref()
    if op == 'apply':
        return xs[0].apply(xs[1])
    if op == 'add':
        return xs[0] + xs[1]
    if op == 'sub':
        return xs[0] - xs[1]
    if op == 'resample':
        return be.resample(xs[0], xs[1])
    raise KeyError(op)


def triple(f):
    return np.asarray(f.vecs), f.ref, np.asarray(f.mask)


def run_chain(be, chain, a, b):
    env = {'a': be.flow(*a), 'b': be.flow(*b)}
    for name, op, *args in chain:
        env[name] = run_stage(be, op, [env[k] for k in args])
    return {k: triple(v) for k, v in env.items()}


def stage_kind(op, xs):
    """'scatter' (with the sign of its point set), 'gather' or 'exact' for a stage with operand triples xs"""
    if op == 'switch_ref':
        return ('scatter', +1 if xs[0][1] == 's' else -1)
    if op == 'apply':
        return ('scatter', +1) if xs[0][1] == 's' else ('gather', -1)
    if op == 'resample':
        return ('scatter', -1)
    return ('exact', 0)


def scatter_ambiguity(op, sign, xs, shape):
    """(nodes -- for the resample stage: query positions -- in a non-unique simplex of this stage's point set,
        nodes within 1e-5 px of the border of its convex hull)"""
    v, _, m = xs[0]
    if op == 'resample':            # float32 points x - f1, every point kept, queried at x - f3 (flow_class.py:1398-1406)
        yy, xx = np.mgrid[:shape[0], :shape[1]].astype(np.float32)
        pts = np.stack([(xx - v[..., 0]).ravel(), (yy - v[..., 1]).ravel()], 1).astype(np.float64)
        q3 = xs[1][0]
        q = np.stack([(xx - q3[..., 0]).ravel(), (yy - q3[..., 1]).ravel()], 1).astype(np.float64)
        return nonunique_nodes(pts, shape, queries=q)[0], hull_band(pts, shape, q)
    pts = warped_points(v, None if m.all() else m, sign)
    return nonunique_nodes(pts, shape)[0], hull_band(pts, shape)


def scatter_status(op, sign, xs, result, shape, only):
    """scatter_admissible's verdict on the nodes `only` of one scatter stage's result, from the stage's OWN operand triples xs:
    is the value there one of the alternatives SciPy's non-unique simplices allow (values and validity from one triangle)?
    Returns (status, inside the hull)."""
    v, _, m = xs[0]
    if op == 'resample':            # value rows f1 | mask of every point, validity = interpolated mask > 0.99 (flow_class.py:1398-1410)
        yy, xx = np.mgrid[:shape[0], :shape[1]].astype(np.float32)
        pts = np.stack([(xx - v[..., 0]).ravel(), (yy - v[..., 1]).ravel()], 1).astype(np.float64)
        q3 = xs[1][0]
        q = np.stack([(xx - q3[..., 0]).ravel(), (yy - q3[..., 1]).ravel()], 1).astype(np.float64)
        rows = np.concatenate([v, m[..., None]], -1).reshape(-1, 3)
        return sa.admissible_nodes(pts, rows, shape, result[0], result[2], sa.rule_gt099, q, rtol=RTOL, atol=ATOL, only=only, with_inside=True)
    tv, _, tm = xs[-1]              # switch_ref warps the flow itself, apply its second operand; the masks are and-ed (flow_class.py:643)
    rows = np.concatenate([tv, (m & tm)[..., None]], -1).reshape(-1, 3)[m.ravel()]
    return sa.admissible_nodes(warped_points(v, m, sign), rows, shape, result[0], result[2], sa.rule_eq1, rtol=RTOL, atol=ATOL, only=only,
                               with_inside=True)


def close(got, want):
    bad = ~np.isclose(got[0], want[0], rtol=RTOL, atol=ATOL).all(-1)
    return bad | (got[2] != want[2])


def snapped(field):
    """cv2.remap's 1/32-px coordinate steps of the sampling positions grid - field"""
    h, w = field.shape[:2]
    yy, xx = np.mgrid[:h, :w]
    px = (xx - field[..., 0].astype(np.float64)).astype(np.float32)
    py = (yy - field[..., 1].astype(np.float64)).astype(np.float32)
    return np.rint(px * np.float32(32)).astype(np.int64), np.rint(py * np.float32(32)).astype(np.int64)


def taps_touch(dev, sx, sy):
    """does any of the 2 x 2 taps at the snapped positions touch a node of `dev`?"""
    h, w = dev.shape
    ix, iy = sx >> 5, sy >> 5
    out = np.zeros((h, w), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = ix + dx, iy + dy
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            out |= ok & dev[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
    return out


def scatter_reach(dev_src, vecs, sign, shape, radius):
    """target nodes within `radius` px of where a deviating source node lands"""
    from scipy import ndimage
    h, w = shape
    ys, xs = np.nonzero(dev_src)
    out = np.zeros(shape, bool)
    if len(ys) == 0:
        return out
    px = np.rint(xs + sign * vecs[ys, xs, 0]).astype(int)
    py = np.rint(ys + sign * vecs[ys, xs, 1]).astype(int)
    ok = (px >= -radius) & (px < w + radius) & (py >= -radius) & (py < h + radius)
    out[np.clip(py[ok], 0, h - 1), np.clip(px[ok], 0, w - 1)] = True
    return ndimage.binary_dilation(out, iterations=radius)


CASES = {
    # (transforms of f1, f2; f3 = f1 then f2) at sizes SciPy finishes in seconds
    'rot+scale 96x128': ((96, 128), [['rotation', 60, 50, -12]], [['scaling', 30, 40, 0.9]]),
    'scale+rot 120x90': ((120, 90), [['scaling', 20, 70, 1.08]], [['rotation', 40, 60, 9]]),
}


def operands(of, case, kind, ref, rng):
    shape, t1, t2 = CASES[case]
    f1, f2, f3 = (of.Flow.from_transforms(t, list(shape), ref) for t in (t1, t2, t1 + t2))
    if kind == 'mode1':
        a, b = f2, f3
    elif kind == 'mode2':
        a, b = f1, f3
    else:
        a, b = f3, f3
    return triple(a), triple(b)


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("kind", ['mode1', 'mode2', 'invert', 'switch'])
@pytest.mark.parametrize("case", sorted(CASES))
def test_chain_stage_by_stage(gpu, oracle, case, kind, ref):
    of = gpu
    chain = CHAINS[(kind, ref)]
    shape = CASES[case][0]
    a, b = operands(of, case, kind, ref, None)
    O, P = OracleBackend(oracle), ProductBackend(of)
    want = run_chain(O, chain, a, b)

    # ---- isolated stages: the product on the ORACLE's operands
    ambs = {}
    for name, op, *args in chain:
        xs = [want[k] for k in args]
        got = triple(run_stage(P, op, [P.flow(*x) for x in xs]))
        assert got[1] == want[name][1], (name, op)
        k, sign = stage_kind(op, xs)
        if k == 'scatter':
            amb, band = ambs[name] = scatter_ambiguity(op, sign, xs, shape)
            bad = close(got, want[name])
            print("{} {} {}: isolated scatter '{}' beyond tolerance: {} outside / {} inside the {} non-unique nodes; {} of them among "
                  "the {} nodes within 1e-5 px of the hull border".format(case, kind, ref, name, int((bad & ~amb).sum()), int((bad & amb).sum()),
                                                                          int(amb.sum()), int((bad & band).sum()), int(band.sum())))
            # flow-valued data of these (affine) fields is affine to float rounding, so the choice among co-circular diagonals
            # does not show either: EVERY node must agree, bar the hull-border noise band
            bad &= ~band
            if bad.any():
                y, x = np.argwhere(bad)[0]
                pytest.fail("stage '{}' ({}) node ({}, {}): got {} {}, want {} {}".format(
                    name, op, y, x, got[0][y, x], got[2][y, x], want[name][0][y, x], want[name][2][y, x]))
        else:
            np.testing.assert_array_equal(got[2], want[name][2], err_msg="{} mask".format(name))
            np.testing.assert_array_equal(got[0], want[name][0], err_msg="{} ({}) is not bit-exact on equal inputs".format(name, op))

    # ---- native chain: every deviation has a reason
    got = run_chain(P, chain, a, b)
    dev = {'a': np.zeros(shape, bool), 'b': np.zeros(shape, bool)}
    why = []
    for name, op, *args in chain:
        xs_w, xs_g = [want[k] for k in args], [got[k] for k in args]
        k, sign = stage_kind(op, xs_w)
        d = close(got[name], want[name])
        if k == 'exact':
            ok = np.zeros(shape, bool)
            for kk in args:
                ok |= dev[kk]
            reason = "operand"
        elif k == 'gather':
            sw, sg = snapped(xs_w[0][0]), snapped(xs_g[0][0])
            flip = (sw[0] != sg[0]) | (sw[1] != sg[1])
            ok = flip | dev[args[0]] | taps_touch(dev[args[1]], *sw) | taps_touch(dev[args[1]], *sg)
            reason = "1/32-px snap flips at {} nodes".format(int(flip.sum()))
        else:
            amb, band = ambs[name]
            src = dev[args[0]].copy()
            for kk in args[1:]:
                src |= dev[kk]
            ok = band | scatter_reach(src, xs_w[0][0], sign, shape, 3)
            if op == 'resample':
                ok |= dev[args[1]]
            # a non-unique simplex explains a deviation only if the value IS one of its alternatives
            ask = d & amb & ~ok
            st, inside = scatter_status(op, sign, xs_g, got[name], shape, ask)
            unjudged = st == sa.NOT_JUDGED                           # counted, bounded by 0.1 % of the nodes inside the hull
            assert unjudged.sum() <= 1e-3 * inside.sum(), (name, op, int(unjudged.sum()), int(inside.sum()))
            ok |= ask & ((st == sa.ADMISSIBLE) | unjudged)
            reason = "{} non-unique, {} of them admissible, {} not judged; {} hull-border nodes".format(
                int(amb.sum()), int((st == sa.ADMISSIBLE).sum()), int(unjudged.sum()), int(band.sum()))
        unexplained = d & ~ok
        if d.any():
            why.append("  stage '{}' ({}): {} nodes beyond tolerance ({}), first {}".format(
                name, op, int(d.sum()), reason, np.argwhere(d)[0].tolist()))
        if unexplained.any():
            y, x = np.argwhere(unexplained)[0]
            pytest.fail("native chain, stage '{}' ({}): node ({}, {}) differs without a reason: got {} {}, want {} {}\n{}".format(
                name, op, y, x, got[name][0][y, x], got[name][2][y, x], want[name][0][y, x], want[name][2][y, x], "\n".join(why)))
        dev[name] = d
    print("{} {} {}: native chain, {} of {} result nodes beyond tolerance".format(case, kind, ref, int(dev['res'].sum()), dev['res'].size))
    print("\n".join(why))
    # few nodes may deviate at all: each snap flip touches one node and what lands around it
    assert dev['res'].mean() < 0.02, "\n".join(why)

    # ---- and the public one-call form gives what the explicit stages give
    A, B = P.flow(*a), P.flow(*b)
    if kind.startswith('mode'):
        r = A.combine_with(B, int(kind[-1]))
    else:
        r = A.invert() if kind == 'invert' else A.switch_ref()
    assert r.ref == got['res'][1]
    np.testing.assert_array_equal(r.mask, got['res'][2])
    np.testing.assert_array_equal(r.vecs, got['res'][0])


@pytest.mark.parametrize("ref", ['s', 't'])
def test_invert_and_switch_ref_vs_oracle_512(gpu, oracle, ref):
    """The reference's own size for these tests (tests/test_flow_class.py:501-573: 512 x 512, rotation by 30 degrees),
    against the oracle instead of the analytic flow: masks bit-exact, vectors within 1e-4 / 2e-5 on every node
    (flow-valued data of an affine field is affine, so non-unique diagonals give the same values)."""
    of = gpu
    s = [512, 512]
    f = of.Flow.from_transforms([['rotation', 256, 256, 30]], s, ref)
    o = oracle.OFlow(f.vecs, ref, f.mask)
    for got, want in ((f.invert(), o.invert()), (f.switch_ref(), o.switch_ref())):
        assert got.ref == want.ref
        np.testing.assert_array_equal(got.mask, want.mask)
        assert got.mask.sum() > 100000
        np.testing.assert_allclose(got.vecs, want.vecs, rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
def test_soak_seed_mesh_fan_with_a_site_inside(gpu, oracle):
    """tools/soak_chains.py, seed 78000073 (mode 1 't', 90 x 136, rippled fields, a fifth of the points masked out): the last
    stage -- res.switch_ref(), a scatter on the Delaunay path -- holds a grid cell whose corner a lies INSIDE the triangle of
    its other three corners (an outlier vector next to a masked region).  The mesh-fan pass chose that cell's diagonal by the
    in-circle sign of a convex cell and took corner a on trust: its sites' stars held the triangle (b, c, d) with site a in it,
    and one node came out 0.6 px off SciPy (all paths alike: grid, query positions, bands).  star_fan now refuses a whole cell
    that is not convex, as cell_verify does."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import soak_chains
    n, bad, msgs = soak_chains.one_case(gpu, oracle, sys.modules[__name__], 78000073, 120, 160)
    assert n > 100000 and bad == 0, msgs
