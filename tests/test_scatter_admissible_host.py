"""CPU suite: tests/scatter_admissible.py -- the checker the GPU scatter tests apply inside non-unique simplices -- pinned
before anything trusts it: (a) every output of the REAL reference in tests/golden/ is admissible, whatever order Qhull is fed
the sites in; (b) hand-built cells with known answers; (c) corrupted reference outputs are flagged, by literal counts."""
import os

import numpy as np
import pytest

import scatter_admissible as sa
from scatter_admissible import OUTSIDE, ADMISSIBLE, INADMISSIBLE, NOT_JUDGED, NOT_ASKED
from scatter_util import nonunique_nodes, reference_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DELAUNAY_TAGS = ["affine_generic", "affine_generic_hole", "block_generic", "curved", "curved_in", "hole_img", "shear", "speckle_img",
                 "wobble3", "sintel4x4"]
PATH_OPS = ('apply_img', 'apply_img_nomask', 'apply_u8', 'invert', 'switch_ref', 'disc_apply', 'disc_invert', 'combine2', 'combine2_wobble',
            # and the cases whose output is a validity plane alone (the warped mask)
            'valid_target', 'valid_target_nomask', 'valid_source', 'valid_source_nomask', 'k7', 'disc_valid_target')


@pytest.fixture(scope="module")
def g_delaunay():
    return np.load(os.path.join(GOLDEN, "ref_delaunay_cases.npz"))


@pytest.fixture(scope="module")
def g_paths():
    return np.load(os.path.join(GOLDEN, "ref_scipy_paths.npz"))


def judge(c, out=None, out_valid=None, order=None, only=None):
    p, v = c['points'], c['values']
    if order is not None:
        p, v = p[order], v[order]
    return sa.admissible_nodes(p, v, c['shape'], c['out'] if out is None else out, c['out_valid'] if out_valid is None else out_valid,
                               c['rule'], c['queries'], levels=c['levels'], only=only)


def reference_is_admissible(c, tag):
    """first pass: every node, sites as the fixture has them; second pass: the non-unique nodes (the only ones an order can
    change) with the sites permuted, so that Qhull's diagonals -- and the duplicates met first -- are other ones"""
    amb, inside = nonunique_nodes(c['points'], c['shape'], c['queries'])
    st = judge(c)
    assert np.array_equal(st != OUTSIDE, inside), tag
    assert (st == INADMISSIBLE).sum() == 0, (tag, np.argwhere(st == INADMISSIBLE)[:5].tolist())
    assert (st == NOT_JUDGED).sum() <= 1e-3 * inside.sum(), (tag, int((st == NOT_JUDGED).sum()), int(inside.sum()))
    if amb.any():
        st2 = judge(c, order=np.random.default_rng(11).permutation(len(c['points'])), only=amb)
        assert ((st2 == NOT_ASKED) == ~amb).all() and (st2 == INADMISSIBLE).sum() == 0, (tag, "permuted")
        assert (st2 == NOT_JUDGED).sum() <= 1e-3 * inside.sum(), (tag, "permuted")
    return st, amb


# --------------------------------------------------------------------------------------------- (a) the reference's own outputs
@pytest.mark.parametrize("name", DELAUNAY_TAGS)
def test_reference_delaunay_fixtures_are_admissible(g_delaunay, name):
    for op in ('apply', 'invert'):
        st, amb = reference_is_admissible(reference_case(g_delaunay, name + '/' + op), name + '/' + op)
    if name == "shear":                     # two nodes in hull slivers whose circle holds 51 and 61 sites
        assert (st == NOT_JUDGED).sum() == 2
    else:
        assert (st == NOT_JUDGED).sum() == 0


def test_reference_path_fixtures_are_admissible(g_paths):
    tags = sorted({'/'.join(k.split('/')[:2]) for k in g_paths.files if k.split('/')[0] in PATH_OPS})
    assert len(tags) == 93
    n_amb = 0
    for tag in tags:
        st, amb = reference_is_admissible(reference_case(g_paths, tag), tag)
        assert (st == NOT_JUDGED).sum() == 0, tag
        n_amb += int(amb.sum())
    assert n_amb > 15000                    # the share today's suite exempts


@pytest.mark.parametrize("name", ["hole_img", "sintel4x4"])
def test_both_evaluation_paths_agree(g_delaunay, name):
    """the acceptance rule exists twice in admissible_nodes (all simplices without duplicated sites at once / simplex by simplex):
    the same verdicts on the reference's output and on a corrupted one, values and validity"""
    c = reference_case(g_delaunay, name + '/apply')
    rng = np.random.default_rng(3)
    flip = rng.random(c['shape']) < 0.3
    bad = np.where(flip[..., None], np.roll(c['out'], 1, 1), c['out'])
    bad_valid = c['out_valid'] ^ (rng.random(c['shape']) < 0.1)
    for out, valid in ((c['out'], c['out_valid']), (bad, bad_valid)):
        a, b = (sa.admissible_nodes(c['points'], c['values'], c['shape'], out, valid, c['rule'], vectorise=v) for v in (True, False))
        np.testing.assert_array_equal(a, b)
    assert (a == INADMISSIBLE).sum() > 1000 and (a == ADMISSIBLE).sum() > 1000


# --------------------------------------------------------------------------------------------- (b) known answers
#   c(0,1) d(1,1) f(2,1)
#   a(0,0) b(1,0) e(2,0)          values 1, 2, 4, 8 | 16, 32
CELL = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [2, 0], [2, 1]], np.float64)
CELL_V = np.array([1, 2, 4, 8, 16, 32], np.float64)[:, None]


def at(q, pts, vals, got, valid=None, rule=None, **kw):
    return int(sa.admissible_nodes(pts, vals, (1, 1), np.reshape(got, (1, 1, -1)), None if valid is None else np.reshape(valid, (1, 1)),
                                   rule, np.reshape(q, (1, 2)), **kw)[0, 0])


def test_square_both_diagonals_and_nothing_else():
    centre = (0.5, 0.5)
    assert at(centre, CELL, CELL_V, (1 + 8) / 2) == ADMISSIBLE                    # diagonal a-d
    assert at(centre, CELL, CELL_V, (2 + 4) / 2) == ADMISSIBLE                    # diagonal b-c
    assert at(centre, CELL, CELL_V, (1 + 2 + 4 + 8) / 4) == INADMISSIBLE          # the four-corner mean is neither
    assert at(centre, CELL, CELL_V, 16.0) == INADMISSIBLE                         # a corner of the neighbouring cell
    assert at(centre, CELL, CELL_V, (2 + 32) / 2) == INADMISSIBLE                 # ... or its diagonal
    # off the centre: triangles a b c (0.3, 0.3, 0.4) and a c d (0.6, 0.1, 0.3) hold (0.3, 0.4); a b d and b c d do not
    q = (0.3, 0.4)
    assert at(q, CELL, CELL_V, 0.3 * 1 + 0.3 * 2 + 0.4 * 4) == ADMISSIBLE
    assert at(q, CELL, CELL_V, 0.6 * 1 + 0.1 * 4 + 0.3 * 8) == ADMISSIBLE
    assert at(q, CELL, CELL_V, 0.5 * (2.5 + 3.4)) == INADMISSIBLE                 # a blend of the two
    assert at(q, CELL, CELL_V, 0.7 * 1 - 0.1 * 2 + 0.4 * 8) == INADMISSIBLE      # a b d, extrapolated: does not hold q
    assert at(q, CELL, CELL_V, 2.5 + 3e-4) == INADMISSIBLE and at(q, CELL, CELL_V, 2.5 + 2e-4) == ADMISSIBLE   # rtol 1e-4, atol 2e-5
    assert at((5.0, 5.0), CELL, CELL_V, 0.0) == OUTSIDE
    # whole rows: every channel from ONE triangle
    two = np.concatenate([CELL_V, CELL_V[::-1]], 1)                              # second channel: 32, 16, 8, 4, 2, 1
    assert at(centre, CELL, two, [4.5, 18.0]) == ADMISSIBLE and at(centre, CELL, two, [3.0, 12.0]) == ADMISSIBLE
    assert at(centre, CELL, two, [4.5, 12.0]) == INADMISSIBLE
    # max_sites: the cell cannot be judged with fewer than its four sites, and says so
    assert at(centre, CELL, CELL_V, 4.5, max_sites=3) == NOT_JUDGED


def test_duplicated_site_either_value_not_their_mean():
    pts = np.array([[0, 0], [1, 0], [0, 1], [0, 1], [1.3, 1.2]], np.float64)
    vals = np.array([1, 2, 4, 64, 9], np.float64)[:, None]
    q = (0.25, 0.5)                                                               # in a b c: 0.25, 0.25, 0.5
    assert at(q, pts, vals, 0.25 * 1 + 0.25 * 2 + 0.5 * 4) == ADMISSIBLE
    assert at(q, pts, vals, 0.25 * 1 + 0.25 * 2 + 0.5 * 64) == ADMISSIBLE
    assert at(q, pts, vals, 0.25 * 1 + 0.25 * 2 + 0.5 * 34) == INADMISSIBLE       # Qhull keeps ONE site: no averaging
    assert at(q, pts, vals, 0.25 * 1 + 0.25 * 2 + 0.5 * 68) == INADMISSIBLE       # ... and no summing
    assert at(q, pts, vals, 0.25 * 1 + 0.25 * 2 + 0.5 * 4, max_alternatives=1) == NOT_JUDGED
    # the order of the duplicates does not matter
    o = [3, 0, 4, 2, 1]
    assert at(q, pts[o], vals[o], 0.25 * 1 + 0.25 * 2 + 0.5 * 4) == ADMISSIBLE and at(q, pts[o], vals[o], 0.75 + 32) == ADMISSIBLE


def test_node_on_a_shared_edge():
    pts = np.array([[0, 0], [2, 0], [0, 2], [2.5, 2.75], [-1.5, 0.5]], np.float64)   # no four sites co-circular
    vals = np.array([[1, 1], [2, 0], [4, 1], [8, 1], [16, 1]], np.float64)
    for t in (0.25, 0.5, 0.9):                                                     # on the edge b-c, whichever side find_simplex names
        q = (2 - 2 * t, 2 * t)
        want = (1 - t) * 2 + t * 4
        assert at(q, pts, vals, want, False, sa.rule_eq1) == ADMISSIBLE
        assert at(q, pts, vals[:, :1], want) == ADMISSIBLE
        assert at(q, pts, vals[:, :1], want + 0.01) == INADMISSIBLE
    # on the edge a-c both neighbours (a b c and a c e) give the edge's value
    assert at((0.0, 0.5), pts, vals[:, :1], 0.75 * 1 + 0.25 * 4) == ADMISSIBLE
    assert at((0.0, 0.5), pts, vals, 0.75 * 1 + 0.25 * 4, True, sa.rule_eq1) == ADMISSIBLE


def test_values_and_validity_from_the_same_triangle():
    m = np.array([1, 0, 1, 1, 1, 1], np.float64)[:, None]                          # b is masked out
    vals = np.concatenate([CELL_V, m], 1)
    centre = (0.5, 0.5)                      # diagonal b-c: 3.0 with mask 0.5 (invalid); diagonal a-d: 4.5 with mask 1 (valid)
    assert at(centre, CELL, vals, 4.5, True, sa.rule_eq1) == ADMISSIBLE
    assert at(centre, CELL, vals, 3.0, False, sa.rule_eq1) == ADMISSIBLE
    assert at(centre, CELL, vals, 3.0, True, sa.rule_eq1) == INADMISSIBLE         # the values of one diagonal, the validity of the other
    assert at(centre, CELL, vals, 3.75, True, sa.rule_eq1) == INADMISSIBLE
    assert at(centre, CELL, vals, 123.0, False, sa.rule_eq1) == ADMISSIBLE        # invalid: only the validity is compared, as today
    # the other rules: mask 0.5 rounds to 0 (np.round, half to even) and is not > 0.99
    assert at(centre, CELL, vals, 3.0, True, sa.rule_eq1_rounded) == INADMISSIBLE
    assert at(centre, CELL, vals, 3.0, True, sa.rule_gt099) == INADMISSIBLE
    q = (0.9, 0.05)                          # a b c (0.05, 0.9, 0.05): mask 0.1; a b d (0.1, 0.85, 0.05): mask 0.15 -- both round to 0
    assert at(q, CELL, vals, 0.0, False, sa.rule_eq1_rounded) == ADMISSIBLE
    m2 = np.array([1, 1, 1, 0, 1, 1], np.float64)[:, None]                         # d masked out: a b c all valid, a b d 0.95 -> rounds to 1
    vals2 = np.concatenate([CELL_V, m2], 1)
    assert at(q, CELL, vals2, 0.1 * 1 + 0.85 * 2 + 0.05 * 8, True, sa.rule_eq1_rounded) == ADMISSIBLE      # a b d, rounded rule
    assert at(q, CELL, vals2, 0.1 * 1 + 0.85 * 2 + 0.05 * 8, True, sa.rule_eq1) == INADMISSIBLE            # the float rule says invalid there
    assert at(q, CELL, vals2, 0.05 * 1 + 0.9 * 2 + 0.05 * 4, True, sa.rule_eq1) == ADMISSIBLE              # a b c


def test_integer_levels():
    v = CELL_V * 10
    assert at((0.5, 0.5), CELL, v, 45, levels=True) == ADMISSIBLE and at((0.5, 0.5), CELL, v, 31, levels=True) == ADMISSIBLE
    assert at((0.5, 0.5), CELL, v, 37, levels=True) == INADMISSIBLE and at((0.5, 0.5), CELL, v, 47, levels=True) == INADMISSIBLE


# --------------------------------------------------------------------------------------------- (c) corruptions
def other_triangle_values(c, amb):
    """at the nodes of simplices whose S is four distinct, unduplicated sites: the value row extrapolated from a triangle of S
    that does NOT hold the node -- what a kernel returns that walks into the right cell and evaluates the wrong half"""
    from scipy.spatial import Delaunay, cKDTree
    import itertools
    pts, vals, shape = c['points'], c['values'], c['shape']
    upts, idx, counts = np.unique(pts, axis=0, return_index=True, return_counts=True)
    d, tree = Delaunay(upts), cKDTree(upts)
    q = sa._grid(shape)
    s = d.find_simplex(q)
    out = np.array(c['out'], np.float64).reshape(len(q), -1)
    touched = np.zeros(len(q), bool)
    cen, rad = sa._circumcircles(upts, d.simplices)
    for n in np.flatnonzero(amb.ravel() & (s >= 0)):
        S = sa.cocircular_sites(upts, tree, [int(v) for v in d.simplices[s[n]]], cen[s[n]], float(rad[s[n]]), 1e-9)
        if len(S) != 4 or (counts[S] > 1).any():
            continue
        tri = np.array(list(itertools.combinations(S, 3)))
        lam = sa._barycentric(upts, tri, q[n:n + 1])[0]
        wrong = np.flatnonzero((lam < -1e-3).any(1))
        if len(wrong):
            t = wrong[0]
            out[n] = lam[t] @ vals[idx[tri[t]], :out.shape[1]]
            touched[n] = True
    return out.reshape(np.shape(c['out'])), touched.reshape(shape)


# literal counts of this file's own run: in-hull, valid and non-unique nodes, then the nodes flagged by each corruption (and, for
# the two that touch non-unique nodes only, how many they touched: on sintel4x4 the nearest site's value is right AT the lattice
# sites, and only 219 nodes lie in a cell of four distinct, unduplicated sites)
CORRUPTIONS = {
    "sintel4x4": dict(inside=3200, valid=3200, amb=2116, roll=3200, swap=3198, nearest=1139, nearest_touched=1139, other=219, other_touched=219),
    "hole_img": dict(inside=3875, valid=3875, amb=627, roll=3875, swap=3873, nearest=627, nearest_touched=627, other=627, other_touched=627),
}


@pytest.mark.parametrize("name", sorted(CORRUPTIONS))
def test_corrupted_reference_outputs_are_flagged(g_delaunay, name):
    from scipy.spatial import cKDTree
    c = reference_case(g_delaunay, name + '/apply')
    out, valid, shape = c['out'], c['out_valid'], c['shape']
    amb, inside = nonunique_nodes(c['points'], shape)
    flagged = lambda st: int((st == INADMISSIBLE).sum())
    n = dict(inside=int(inside.sum()), valid=int(valid.sum()), amb=int(amb.sum()))
    # 1. the whole result one pixel to the right.  Wherever the result or the shifted one is valid the node must be flagged
    #    (random image values: no neighbour's value is an alternative of this node)
    st = judge(c, np.roll(out, 1, 1), np.roll(valid, 1, 1))
    n['roll'] = flagged(st)
    assert ((st == INADMISSIBLE) == (inside & (valid | np.roll(valid, 1, 1)))).all()
    # 2. channels 0 and 1 swapped, validity untouched: every valid node whose two channels differ by more than the tolerance
    st = judge(c, out[..., [1, 0, 2]])
    n['swap'] = flagged(st)
    same = np.isclose(out[..., 1], out[..., 0], rtol=1e-4, atol=2e-5) & np.isclose(out[..., 0], out[..., 1], rtol=1e-4, atol=2e-5)
    assert ((st == INADMISSIBLE) == (inside & valid & ~same)).all()
    # 3. non-unique nodes: the nearest site's value -- no interpolation at all.  Right only AT a site.
    dist, near = cKDTree(c['points']).query(sa._grid(shape))
    bad = out.copy()
    bad[amb] = c['values'][near.reshape(shape)[amb]][:, :3]
    touched = amb & valid & (dist.reshape(shape) > 1e-3)
    st = judge(c, bad, only=amb)
    n['nearest'], n['nearest_touched'] = flagged(st), int(touched.sum())
    assert not (touched & (st != INADMISSIBLE)).any()
    # 4. non-unique nodes: the triangle of S that does not hold the node
    bad, touched = other_triangle_values(c, amb)
    touched &= valid
    st = judge(c, bad, only=amb)
    n['other'], n['other_touched'] = flagged(st), int(touched.sum())
    assert not (touched & (st != INADMISSIBLE)).any() and not ((st == INADMISSIBLE) & ~touched).any()
    print(name, n)
    assert n == CORRUPTIONS[name]
