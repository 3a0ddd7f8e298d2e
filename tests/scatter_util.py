"""Helpers shared by the GPU scatter tests: where is SciPy's own triangulation unique?"""
import numpy as np


def warped_points(vecs, keep=None, sign=1):
    h, w = vecs.shape[:2]
    yy, xx = np.mgrid[:h, :w]
    p = np.stack([(xx + sign * vecs[..., 0].astype(np.float64)).ravel(), (yy + sign * vecs[..., 1].astype(np.float64)).ravel()], 1)
    return p if keep is None else p[np.asarray(keep, bool).ravel()]


def nonunique_nodes(points, shape, queries=None, tol=1e-9):
    """Grid nodes whose covering simplex of SciPy's own triangulation is NOT uniquely Delaunay (a fourth site within
    `tol` (relative) of its circumcircle, or a duplicated site): Qhull's choice among the co-circular alternatives is arbitrary
    there, and non-affine data (image values, speckled masks) can tell the alternatives apart.  Everywhere else the
    Delaunay triangulation -- and with it griddata's result -- is unique.  `queries` (N x 2, (x, y), N = H * W): scattered
    query positions instead of the grid nodes (mode 2 / 't', flow_class.py:1407).  Returns (ambiguous, inside_hull).
    (Qhull merges facets that are coplanar within ITS roundoff, which grows with the coordinates: on a 248 x 411
    similarity field it splits a cell whose fourth corner is 1.1e-9 px OUTSIDE the circle along the other diagonal -- and
    along the right one when x and y are swapped; tools/soak_scatter.py therefore scales `tol` with the field.)"""
    from scipy.spatial import Delaunay
    from test_delaunay_core import unique_simplices
    upts, inv, counts = np.unique(points, axis=0, return_inverse=True, return_counts=True)
    d = Delaunay(upts)
    uniq = unique_simplices(upts, d.simplices, tol)
    dup_vertex = (counts[d.simplices] > 1).any(1)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    q = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64) if queries is None else np.asarray(queries, np.float64)
    s = d.find_simplex(q).reshape(shape)
    amb = np.zeros(shape, bool)
    inside = s >= 0
    amb[inside] = ~uniq[s[inside]] | dup_vertex[s[inside]]
    return amb, inside


def ambiguous_for(vecs, keep=None, sign=1):
    return nonunique_nodes(warped_points(vecs, keep, sign), vecs.shape[:2])[0]


def hull_band(points, shape, queries=None, width=1e-5):
    """Grid nodes (or query positions) within `width` px of the border of the convex hull of `points`: whether such a
    position is inside is decided by Qhull's handling of the sliver facets along a border that is straight only up to
    float rounding (find_simplex fails on positions 4e-7 px INSIDE the hull of float32-rounded points) -- rounding
    noise of the reference, not a rule."""
    from scipy.spatial import ConvexHull
    hull = ConvexHull(np.unique(points, axis=0))
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    q = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64) if queries is None else np.asarray(queries, np.float64)
    d = (q @ hull.equations[:, :2].T + hull.equations[:, 2]).max(1)          # signed distance to the nearest facet, < 0 inside
    return (np.abs(d) < width).reshape(shape)


def reference_case(g, tag):
    """What SciPy received and what the reference returned for one image- or flow-valued case of the two fixture files
    (tests/golden/make_golden.py), as scatter_admissible wants it: dict(points [N][2], values [N][K], shape, out, out_valid,
    rule, levels, queries).  `tag` of ref_delaunay_cases.npz: '<name>/apply' or '<name>/invert'."""
    import scatter_admissible as sa
    parts = tag.split('/')
    op, levels, queries, rule = parts[0], False, None, sa.rule_eq1
    if tag + '/in_vecs' not in g.files:                                   # ref_delaunay_cases.npz
        name, op = parts
        vecs, mask = g[name + '/in_vecs'], g[name + '/in_mask']
        if op == 'apply':
            rows, out, out_valid = g[name + '/img'], g[name + '/apply'], g[name + '/apply_valid']
        else:
            rows, out, out_valid = -vecs, g[name + '/invert_vecs'], g[name + '/invert_mask']
        pts, keep, vm = warped_points(vecs), mask, mask
    else:
        vecs, mask = g[tag + '/in_vecs'], g[tag + '/in_mask']
        ref = str(g[tag + '/in_ref'])
        sign = 1 if ref == 's' else -1
        pts, keep, vm = warped_points(vecs, None, sign), mask, mask
        if op in ('apply_img', 'apply_img_nomask', 'disc_apply'):
            rows = g['disc/' + parts[1] + '/img'] if op == 'disc_apply' else g['img_f32']
            out, out_valid = g[tag + '/out'], g[tag + '/out_valid']
            if op == 'apply_img_nomask':
                keep = np.ones_like(mask)
        elif op.startswith(('valid_', 'k7', 'disc_valid')):               # flow_class.py:1113-1195: the mask alone is warped
            nomask = parts[-1].endswith('nomask') or op.endswith('nomask')
            rows, out, out_valid = np.zeros(mask.shape + (0,)), None, g[tag + '/out']
            if nomask:
                keep = np.ones_like(mask)
        elif op == 'apply_u8':
            rows, out, out_valid, rule, levels = g['img_u8'], g[tag + '/out'], None, None, True
        elif op in ('invert', 'disc_invert', 'switch_ref'):               # flow_class.py:697-753
            rows, out, out_valid = (vecs if op == 'switch_ref' else -vecs), g[tag + '/out_vecs'], g[tag + '/out_mask']
        elif op.startswith('combine2') and ref == 's':                    # self.apply(flow - self), flow_class.py:1390
            rows, vm = g[tag + '/in2_vecs'] - vecs, mask & g[tag + '/in2_mask']
            out, out_valid = g[tag + '/out_vecs'], g[tag + '/out_mask']
        elif op.startswith('combine2'):                                   # flow - resampled f1, flow_class.py:1398-1410: float32 positions
            h, w = vecs.shape[:2]
            f3 = g[tag + '/in2_vecs']
            assert g[tag + '/in2_mask'].all()
            c1 = np.copy(-vecs); c1[:, :, 0] += np.arange(w); c1[:, :, 1] += np.arange(h)[:, None]
            c3 = np.copy(-f3); c3[:, :, 0] += np.arange(w); c3[:, :, 1] += np.arange(h)[:, None]
            pts, queries, keep = c1.reshape(-1, 2).astype(np.float64), c3.reshape(-1, 2).astype(np.float64), np.ones_like(mask)
            rows, out, out_valid, rule = vecs, f3 - g[tag + '/out_vecs'], g[tag + '/out_mask'], sa.rule_gt099
        else:
            raise KeyError(tag)
    k = keep.ravel()
    values = rows.reshape(len(k), -1).astype(np.float64)
    if rule is not None:
        values = np.concatenate([values, vm.reshape(-1, 1).astype(np.float64)], 1)
    return dict(points=pts[k], values=values[k], shape=vecs.shape[:2], out=out, out_valid=out_valid, rule=rule, levels=levels, queries=queries)
