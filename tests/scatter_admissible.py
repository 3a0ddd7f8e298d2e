"""Is a scatter output ADMISSIBLE where SciPy's triangulation is not unique?  (test side only: NumPy and SciPy, nothing of the
package under test)

scatter_util.nonunique_nodes marks the nodes whose covering simplex T of SciPy's own triangulation has a fourth site on its
circumcircle, or a duplicated site: Qhull's diagonal -- and the duplicate it keeps -- is arbitrary there, so the reference's
output is ONE of several right answers.  This module enumerates them:

  * S = T's three sites plus every site whose distance to T's circumcentre c is within tol * max(r, 1) of the radius r (the
    rule and the tol of test_delaunay_core.unique_simplices).  All of S lies on one empty circle, so every triangle with corners
    in S is a Delaunay triangle of some valid triangulation.
  * Qhull keeps one site of a duplicated position (option Qc) and drops the others; each corner may carry the value row of
    any of its duplicates.

An output at q is admissible iff for ONE triple of S that contains q (barycentric coordinates >= -eps) and ONE choice of
duplicate per corner the barycentric interpolation of the whole value row equals the output within rtol / atol AND -- where the
row ends in a mask channel -- the validity rule applied to the same interpolated row equals the output's validity.  Where that
triangle's validity is false only the validity is compared.
"""
import itertools

import numpy as np

OUTSIDE, ADMISSIBLE, INADMISSIBLE, NOT_JUDGED = 0, 1, 2, 3
NOT_ASKED = -1                      # only with `only`: a node the caller has compared directly

_CHUNK = 1 << 21                    # elements of one block of candidate rows


def rule_eq1(m):
    """apply_flow('s') interpolates in float64 and returns the target's dtype, float32 (utils.py:253-258); flow_class.py:668 then
    compares the mask channel with 1"""
    return m.astype(np.float32) == 1


def rule_eq1_rounded(m):
    """integer targets: the interpolated mask channel is np.round-ed with the image before `== 1` (utils.py:256-257)"""
    return np.round(m) == 1


def rule_gt099(m):
    """combine_with mode 2, ref 't' (flow_class.py:1410)"""
    return m > .99


def _grid(shape):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)


def _circumcircles(p, tri):
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    bx, by, cx, cy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
    d = 2 * (bx * cy - by * cx)
    with np.errstate(divide='ignore', invalid='ignore'):
        ux = (cy * (bx * bx + by * by) - by * (cx * cx + cy * cy)) / d
        uy = (bx * (cx * cx + cy * cy) - cx * (bx * bx + by * by)) / d
    return np.stack([a[:, 0] + ux, a[:, 1] + uy], 1), np.hypot(ux, uy)


def cocircular_sites(upts, tree, verts, centre, r, tol):
    """S of one simplex: indices into the unique sites, the simplex's own three first"""
    band = tol * max(r, 1.0)
    near = np.asarray(tree.query_ball_point(centre, r + band), np.int64)
    dist = np.hypot(upts[near, 0] - centre[0], upts[near, 1] - centre[1])
    near = near[np.abs(dist - r) <= band]
    return list(verts) + [int(j) for j in near if j not in verts]


def _barycentric_each(p, tri, q):
    """q [...][2], each in its own triangle tri [...][3] of p -> [...][3]; NaN for a flat triangle"""
    a, b, c = p[tri[..., 0]], p[tri[..., 1]], p[tri[..., 2]]
    det = (b[..., 1] - c[..., 1]) * (a[..., 0] - c[..., 0]) + (c[..., 0] - b[..., 0]) * (a[..., 1] - c[..., 1])
    dx, dy = q[..., 0] - c[..., 0], q[..., 1] - c[..., 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        l0 = ((b[..., 1] - c[..., 1]) * dx + (c[..., 0] - b[..., 0]) * dy) / det
        l1 = ((c[..., 1] - a[..., 1]) * dx + (a[..., 0] - c[..., 0]) * dy) / det
        return np.stack([l0, l1, 1.0 - l0 - l1], -1)


def _barycentric(p, tri, q):
    """q [m][2] in the triangles tri [t][3] of p -> [m][t][3]; NaN for a flat triple"""
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    det = (b[:, 1] - c[:, 1]) * (a[:, 0] - c[:, 0]) + (c[:, 0] - b[:, 0]) * (a[:, 1] - c[:, 1])
    dx, dy = q[:, None, 0] - c[None, :, 0], q[:, None, 1] - c[None, :, 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        l0 = ((b[:, 1] - c[:, 1]) * dx + (c[:, 0] - b[:, 0]) * dy) / det
        l1 = ((c[:, 1] - a[:, 1]) * dx + (a[:, 0] - c[:, 0]) * dy) / det
        return np.stack([l0, l1, 1.0 - l0 - l1], -1)


def alternatives(dup_lists, S):
    """every triple of S [t][3] (indices of distinct sites) and, per triple, every choice of duplicate per corner: [cand][3]
    ORIGINAL point indices"""
    tri = np.array(list(itertools.combinations(S, 3)), np.int64)
    if all(len(dup_lists(i)) == 1 for i in S):
        first = {i: dup_lists(i)[0] for i in S}
        return tri, [np.array([[first[i], first[j], first[k]]], np.int64) for i, j, k in tri]
    rows = [np.stack(np.meshgrid(dup_lists(i), dup_lists(j), dup_lists(k), indexing='ij'), -1).reshape(-1, 3) for i, j, k in tri]
    return tri, rows


def _one_triple(lam, vrows, got, gv, C, valid_rule, close):
    """nodes [m] that one triple holds (lam [m][3]) against its candidate rows vrows [cand][3][K] -> admissible [m].  The mask
    channel and the first value channel are evaluated for every (node, candidate); the other channels only for the pairs that
    are still open -- with many duplicates of one site nearly none."""
    open_ = np.ones((len(lam), len(vrows)), bool)
    settled = np.zeros(len(lam), bool)
    if valid_rule is not None:
        cv = valid_rule(lam @ vrows[:, :, C].T)
        open_ = cv == gv[:, None]
        settled = (open_ & ~cv).any(1)                                         # an invalid alternative: only the validity counts
        open_ &= cv
    elif gv is not None:                                                       # no mask channel: valid = inside the hull
        open_ &= gv[:, None]
    if C:
        open_ &= close(got[:, :1, None], (lam @ vrows[:, :, 0].T)[:, None])[:, 0]
        if C > 1:
            mi, ci = np.nonzero(open_)
            rest = np.einsum('pi,pik->pk', lam[mi], vrows[ci][:, :, 1:C])
            open_[mi, ci] = close(got[mi, 1:], rest).all(-1)
    return settled | open_.any(1)


def admissible_nodes(points, values, shape, got, got_valid=None, valid_rule=None, queries=None, tol=1e-9, rtol=1e-4, atol=2e-5,
                     max_sites=8, eps=1e-7, only=None, levels=False, max_alternatives=1 << 16, with_inside=False, vectorise=True):
    """points [N][2] (x, y) as SciPy received them, duplicates included; values [N][K] their value rows (K = C, or C + 1 with
    the mask channel last when `valid_rule` is given); got [H][W][C] and got_valid [H][W]: the output to judge at the grid
    nodes, or at `queries` [H * W][2].  `only` [H][W] bool: judge these nodes alone (the rest: NOT_ASKED).  `levels`: the
    output is an integer image -- admissible within 1 of the rounded alternative (a value within rounding of x.5 may go either
    way).  Returns the int8 status plane [H][W]: OUTSIDE the hull, ADMISSIBLE, INADMISSIBLE, or NOT_JUDGED (|S| > max_sites,
    more than max_alternatives candidate rows, or no finite circumradius) -- counted by the callers, never passed.  `with_inside`:
    return (status, inside the hull [H][W]) instead.
    Two things go beyond the four codes: NOT_ASKED marks the nodes that `only` leaves out (the callers have compared them with
    the reference directly), and max_alternatives bounds the duplicate choices of one simplex (a site with thousands of
    duplicates next to two more duplicated ones would not fit in memory) -- such a simplex is NOT_JUDGED like one with too many
    sites.  The acceptance rule is written twice: for simplices without a duplicated site all nodes are judged in one go per
    |S|, the others simplex by simplex (_one_triple).  The two must stay equivalent; `vectorise=False` sends everything
    through the second, and test_scatter_admissible_host.py::test_both_evaluation_paths_agree compares them."""
    from scipy.spatial import Delaunay, cKDTree
    points = np.asarray(points, np.float64)
    values = np.asarray(values, np.float64).reshape(len(points), -1)
    n = shape[0] * shape[1]
    got = np.zeros((n, 0)) if got is None else np.asarray(got, np.float64).reshape(n, -1)       # (None: a validity plane alone)
    C = got.shape[1]
    assert values.shape[1] == C + (valid_rule is not None), (values.shape, C)
    gv = None if got_valid is None else np.asarray(got_valid, bool).ravel()
    upts, idx, inv, counts = np.unique(points, axis=0, return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(idx)                   # the distinct sites in the order of `points`: Qhull's diagonals follow it
    rank = np.empty(len(idx), np.int64)
    rank[by_first] = np.arange(len(idx))
    upts, counts, inv = upts[by_first], counts[by_first], rank[inv.ravel()]
    order = np.argsort(inv, kind='stable')
    start = np.concatenate([[0], np.cumsum(counts)])
    dup_lists = lambda u: order[start[u]:start[u + 1]]
    d = Delaunay(upts)
    q = _grid(shape) if queries is None else np.asarray(queries, np.float64).reshape(n, 2)
    s = d.find_simplex(q)
    ask = np.ones(n, bool) if only is None else np.asarray(only, bool).ravel()
    status = np.full(n, NOT_ASKED, np.int8)
    status[ask & (s < 0)] = OUTSIDE
    todo = np.flatnonzero(ask & (s >= 0))
    todo = todo[np.argsort(s[todo], kind='stable')]
    simp, first = np.unique(s[todo], return_index=True)
    last = np.append(first[1:], len(todo))
    centre, radius = _circumcircles(upts, d.simplices[simp])
    finite = np.isfinite(radius)
    band = tol * np.maximum(radius, 1.0)
    # S of every simplex with a small circle at once: the sites within the band of the circle, bar its own three (the few
    # large circles -- hull slivers -- hold thousands of sites each and are searched one by one below)
    tree = cKDTree(upts)
    small = finite & (radius <= 64)
    near = tree.query_ball_point(centre[small], (radius + band)[small]) if small.any() else []
    owner = np.repeat(np.flatnonzero(small), [len(x) for x in near])
    site = np.fromiter(itertools.chain.from_iterable(near), np.int64, len(owner))
    on = np.abs(np.hypot(upts[site, 0] - centre[owner, 0], upts[site, 1] - centre[owner, 1]) - radius[owner]) <= band[owner]
    on &= ~(site[:, None] == d.simplices[simp][owner]).any(1)
    owner, site = owner[on], site[on]
    n_more = np.bincount(owner, minlength=len(simp))
    more_at = np.concatenate([[0], np.cumsum(n_more)])
    if levels:
        close = lambda a, b: np.abs(a - np.round(b)) <= 1
    else:
        close = lambda a, b: np.isclose(a, b, rtol=rtol, atol=atol)
    # simplices whose S has no duplicated site, grouped by |S|: the triples of all of them, and all of their nodes, in one go
    # (|S| = 3: the uniquely Delaunay ones, with the one alternative)
    nodup = vectorise & small & (counts[d.simplices[simp]] == 1).all(1) & (np.bincount(owner, counts[site] > 1, len(simp)) == 0)
    of_node = np.repeat(np.arange(len(simp)), last - first)
    done = np.zeros(len(simp), bool)
    for g in range(max_sites - 2):
        grp = np.flatnonzero(nodup & (n_more == g))
        if len(grp) == 0:
            continue
        done[grp] = True
        S = np.concatenate([d.simplices[simp[grp]], site[more_at[grp][:, None] + np.arange(g)].reshape(len(grp), g)], 1)
        triples = S[:, np.array(list(itertools.combinations(range(3 + g), 3)))]           # [simplex][t][3]
        pos = np.full(len(simp), -1)
        pos[grp] = np.arange(len(grp))
        sel = np.flatnonzero(pos[of_node] >= 0)
        step = max(1, _CHUNK // (triples.shape[1] * 3 * values.shape[1]))
        for m0 in range(0, len(sel), step):
            nd = todo[sel[m0:m0 + step]]
            tri = triples[pos[of_node[sel[m0:m0 + step]]]]                                 # [m][t][3]
            lam = _barycentric_each(upts, tri, q[nd][:, None])
            holds = (lam >= -eps).all(-1)
            interp = np.einsum('mti,mtik->mtk', np.nan_to_num(lam), values[order[start[tri]]])
            ok = holds & close(got[nd][:, None], interp[..., :C]).all(-1)
            if valid_rule is not None:
                cv = valid_rule(interp[..., C])
                ok = (ok | (holds & ~cv)) & (cv == gv[nd][:, None])
            elif gv is not None:
                ok &= gv[nd][:, None]
            status[nd] = np.where(ok.any(1), ADMISSIBLE, INADMISSIBLE)
    cache = {}
    for k in np.flatnonzero(~done):
        nodes = todo[first[k]:last[k]]
        verts = [int(v) for v in d.simplices[simp[k]]]
        if small[k]:
            S = verts + [int(v) for v in site[more_at[k]:more_at[k + 1]]]
        elif finite[k]:
            S = cocircular_sites(upts, tree, verts, centre[k], float(radius[k]), tol)
        if not finite[k] or len(S) > max_sites:
            status[nodes] = NOT_JUDGED
            continue
        key = tuple(sorted(S))
        if key not in cache:
            n_alt = sum(int(counts[i] * counts[j] * counts[k]) for i, j, k in itertools.combinations(S, 3))
            cache[key] = alternatives(dup_lists, key) if n_alt <= max_alternatives else None
        if cache[key] is None:
            status[nodes] = NOT_JUDGED
            continue
        tri, rows = cache[key]
        lam = _barycentric(upts, tri, q[nodes])                                # [m][t][3]; NaN for a flat triple: holds nothing
        holds = (lam >= -eps).all(-1)
        ok = np.zeros(len(nodes), bool)
        for t in range(len(tri)):
            inn = np.flatnonzero(holds[:, t] & ~ok)
            vrows = values[rows[t]]                                            # [cand][3][K]
            step = max(1, _CHUNK // len(vrows))
            for m0 in range(0, len(inn), step):
                ii = inn[m0:m0 + step]
                nd = nodes[ii]
                ok[ii] = _one_triple(lam[ii, t], vrows, got[nd], None if gv is None else gv[nd], C, valid_rule, close)
        status[nodes] = np.where(ok, ADMISSIBLE, INADMISSIBLE)
    return (status.reshape(shape), (s >= 0).reshape(shape)) if with_inside else status.reshape(shape)


def equal_or_admissible(points, values, shape, got, want, amb, got_valid=None, want_valid=None, valid_rule=None, queries=None,
                        tol=1e-9, rtol=1e-4, atol=2e-5, levels=False, **kw):
    """The rule of the GPU tests: a node equals the reference output `want` (the vectorised comparison they have always made:
    isclose for floats, within one level for integer images, validity bit for bit and no values where it is false), or it is
    admissible.  The alternatives are
    enumerated only at nodes that are `amb` or failed the direct comparison.  Returns (equal [H][W], status [H][W], counts):
    inside = nodes in the hull, judged = nodes the enumeration ran on, inadmissible = nodes neither equal nor admissible
    (outside the hull nothing is admissible), not_judged = judged nodes whose alternatives could not be enumerated."""
    n = shape[0] * shape[1]
    if got is None:
        equal = np.ones(shape, bool)
    elif levels:
        equal = (np.abs(np.asarray(got).reshape(n, -1).astype(np.int64) - np.asarray(want).reshape(n, -1).astype(np.int64)) <= 1).all(-1).reshape(shape)
    else:
        equal = np.isclose(np.asarray(got).reshape(n, -1), np.asarray(want).reshape(n, -1), rtol=rtol, atol=atol).all(-1).reshape(shape)
    if got_valid is not None:                # (an invalid node has no value to compare: the rule of admissible_nodes)
        equal = (equal | ~np.asarray(want_valid, bool)) & (np.asarray(got_valid, bool) == np.asarray(want_valid, bool))
    ask = np.asarray(amb, bool) | ~equal
    status, inside = admissible_nodes(points, values, shape, got, got_valid, valid_rule, queries, tol, rtol, atol, only=ask,
                                      levels=levels, with_inside=True, **kw)
    counts = dict(inside=int(inside.sum()), judged=int((status > OUTSIDE).sum()),
                  inadmissible=int((~equal & ((status == INADMISSIBLE) | (status == OUTSIDE))).sum()),
                  not_judged=int((status == NOT_JUDGED).sum()))
    return equal, status, counts


def assert_equal_or_admissible(tag, *args, **kw):
    """equal_or_admissible, asserted: no node that is neither equal to the reference nor admissible, and at most 0.1 % of the
    nodes inside the hull not judged.  Returns the counts."""
    equal, status, n = equal_or_admissible(*args, **kw)
    bad = ~equal & ((status == INADMISSIBLE) | (status == OUTSIDE))
    assert not bad.any(), "{}: {} nodes neither equal the reference nor are admissible, first {}".format(tag, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert n['not_judged'] <= 1e-3 * n['inside'], "{}: {} of {} nodes inside the hull could not be judged".format(tag, n['not_judged'], n['inside'])
    return n
