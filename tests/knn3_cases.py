"""The cases of the k-NN search (N14): the smallest shapes at which a ring search on a cell grid can go wrong.  Each case is a dict
    name, supports f32[ns,3], s_lens, queries f32[nq,3], q_lens, radius (the grid is built at it), cells (cells_per_elem, 0 = default),
    ks (the k's to run), order (None, or a permutation of the queries).
Every array is made once; the tests leave them unchanged."""
import numpy as np


def _case(name, supports, s_lens, radius, ks, queries=None, q_lens=None, cells=0, order=None):
    s = np.ascontiguousarray(supports, np.float32).reshape(-1, 3)
    q = s if queries is None else np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    return dict(name=name, supports=s, s_lens=np.asarray(s_lens, np.int32), queries=q,
                q_lens=np.asarray(s_lens if q_lens is None else q_lens, np.int32), radius=float(radius), ks=tuple(ks), cells=int(cells),
                order=order)


def lattice():
    g = np.arange(5, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)


def _cloud(seed, n, scale=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * scale + offset).astype(np.float32)


# (radius, [coordinates whose f = (double(q) - 0) * (1 / (double(radius) * 1.00001)) is 1, 2, 3]) in the build's own arithmetic, found by a
# search over fp32 radii: EXACT puts the query on the inner face m itself (f == m: it belongs to cell m, the face is the LOWER face of its
# own cell), BELOW a few 2^-53 under it (cell m - 1, the face is the UPPER face of its own cell, inside the bound's 2^-50 margin)
FACES_EXACT = (0.06854534149169922, (0.06854602694511414, 0.13709205389022827, 0.2056380808353424))
FACES_BELOW = (0.05811452865600586, (0.05811510980129242, 0.11623021960258484, 0.17434532940387726))


def face_f(radius, q):
    """the build's cell coordinate of q on an axis whose box starts at 0"""
    return np.float64(np.float32(q)) * (1.0 / (np.float64(np.float32(radius)) * 1.00001))


def _face_cases(name, spec, seed, below):
    """A 4 x 4 x 4 grid whose box starts at the origin, queries ON its inner faces (every axis, m = 1, 2, 3) and, for every query, a
    support 1e-4 edges across that face: the true nearest neighbour lies in the neighbouring cell, at a distance far below the edge, so
    a search that trusts ring 0 returns a point of the query's own cell instead.  -> a foreign-query case and a self-query case"""
    radius, faces = spec
    edge = float(np.float32(radius)) * 1.00001
    for m, q in enumerate(faces, 1):                             # the fixture is what it says: checked at import
        f = face_f(radius, q)
        assert (m - 2.0 ** -50 * (2 * m + 1) <= f < m) if below else f == m, (name, m, f)
    rng = np.random.default_rng(seed)
    cloud = (rng.random((300, 3)) * 3.6 * edge).astype(np.float32)
    cloud[0] = 0.0                                               # the box starts at the origin on every axis
    cloud[1] = np.float32(3.6 * edge)                            # ... and is 4 cells wide
    qs, partners = [], []
    for axis in range(3):
        for m, q in enumerate(faces, 1):
            for _ in range(3):
                p = (rng.random(3) * 3.4 * edge + 0.1 * edge).astype(np.float32)
                p[axis] = np.float32(q)
                o = p.copy()
                o[axis] = np.float32(q + (1e-4 if below else -1e-4) * edge)
                qs.append(p)
                partners.append(o)
    qs, partners = np.array(qs, np.float32), np.array(partners, np.float32)
    # keep the cloud away from the queries: the partner across the face is the nearest support by far
    far = (np.abs(cloud[:, None, :] - qs[None, :, :]).max(2) > 0.02 * edge).all(1)
    far[:2] = True
    sup = np.concatenate([cloud[far], partners])
    both = np.concatenate([sup, qs])
    return [_case(name + '_foreign', sup, [len(sup)], radius, (1, 2, 8), queries=qs, q_lens=[len(qs)]),
            _case(name + '_self', both, [len(both)], radius, (2, 9))]


def all_cases():
    out = []
    # 1. the integer lattice, cell edge ~ 1: ties on every ring face (k = 8: the 8th and 9th neighbour tie in 117 of 125 rows)
    lat = lattice()
    out.append(_case('lattice', lat, [125], 1.0, (8, 9, 27, 64)))
    # 2. fewer points than k; k = 1 and k = 64
    out.append(_case('five_points', _cloud(1, 5), [5], 0.2, (8, 1, 64)))
    out.append(_case('k1_k64', _cloud(2, 400), [400], 0.15, (1, 64)))
    # 3. three stacked clouds 300 / 0 / 7 that overlap in space
    st = np.concatenate([_cloud(3, 300), _cloud(4, 7)])
    out.append(_case('stacked_300_0_7', st, [300, 0, 7], 0.1, (1, 10, 16)))
    # 4. a hundred identical points: every row is 0 .. 9
    out.append(_case('identical', np.full((100, 3), 0.25, np.float32), [100], 0.1, (10,)))
    # 5. one cell for 300 points; a radius far below the spacing (auto-coarsened table)
    out.append(_case('one_cell', _cloud(5, 300), [300], 0.05, (20, 64), cells=1))
    out.append(_case('tiny_radius', _cloud(6, 500, 10.0), [500], 1e-6, (5, 30)))
    # 6. a cluster and one point 50 cell edges away; a cloud flat in one axis
    far = np.concatenate([_cloud(7, 200, 0.3), np.array([[5.3, 0.15, 0.15]], np.float32)])
    out.append(_case('far_point', far, [201], 0.1, (4, 32)))
    flat = _cloud(8, 400)
    flat[:, 2] = 0.5
    out.append(_case('flat_axis', flat, [400], 0.08, (12,)))
    line = np.zeros((300, 3), np.float32)
    line[:, 0] = np.sort(np.random.default_rng(9).random(300)).astype(np.float32)
    out.append(_case('line', line, [300], 0.01, (6,)))
    # 7. foreign queries: inside the box, beside cell faces (within 3e-7 cells: the fp32 cast moves them off; 7b holds the exact ones),
    #    outside the box by 1, 3 and 100 edges
    s = _cloud(10, 600)
    edge = 0.1 * 1.00001
    mn, mx = s.min(0), s.max(0)
    inside = _cloud(11, 40)
    faces = (mn[None, :].astype(np.float64) + edge * np.random.default_rng(12).integers(0, 9, (40, 3))).astype(np.float32)
    outside = []
    for d in (1.0, 3.0, 100.0):
        for axis in range(3):
            for side in (0, 1):
                q = _cloud(13 + axis, 4)
                q[:, axis] = mn[axis] - np.float32(d * edge) if side == 0 else mx[axis] + np.float32(d * edge)
                outside.append(q)
    corner = np.array([[-10.0, -10.0, -10.0], [11.0, 11.0, 11.0], [-3.0, 0.5, 12.0]], np.float32)
    fq = np.concatenate([inside, faces, corner] + outside)
    out.append(_case('foreign_queries', s, [600], 0.1, (1, 7, 30), queries=fq, q_lens=[len(fq)]))
    # 7b. queries on inner cell faces EXACTLY, in the build's arithmetic, with the nearest support across the face
    out += _face_cases('faces_exact', FACES_EXACT, 30, below=False)
    out += _face_cases('faces_below', FACES_BELOW, 31, below=True)
    r, q = 0.05029141902923584, 0.05029192194342613              # the smallest such scene: 4 x 1 x 1 cells, f = 1 exactly
    assert face_f(r, q) == 1.0
    line4 = np.array([[0, 0, 0], [0.0502, 0, 0], [0.06, 0, 0], [0.16, 0, 0]], np.float32)
    out.append(_case('face_minimal', line4, [4], r, (1, 2), queries=np.array([[q, 0, 0]], np.float32), q_lens=[1]))
    out.append(_case('face_minimal_self', np.concatenate([line4, np.array([[q, 0, 0]], np.float32)]), [5], r, (2,)))
    # 8. NaN and +-inf rows among the supports and among the queries
    bad = _cloud(14, 200)
    bad[5] = np.nan
    bad[17, 1] = np.inf
    bad[40, 0] = -np.inf
    bad[41, 2] = np.nan
    bq = _cloud(15, 30)
    bq[3] = np.nan
    bq[4, 0] = np.inf
    bq[9, 2] = -np.inf
    out.append(_case('non_finite_supports', bad, [200], 0.12, (1, 9)))
    out.append(_case('non_finite_queries', bad, [200], 0.12, (9,), queries=bq, q_lens=[30]))
    # 9. a random processing order over two stacked clouds
    two = np.concatenate([_cloud(16, 350), _cloud(17, 250, 1.0, 0.3)])
    out.append(_case('random_order', two, [350, 250], 0.1, (8, 30), order=np.random.default_rng(18).permutation(600).astype(np.int32)))
    # 10. random clouds at three scales: faces are met closely
    for i, scale in enumerate((1e-3, 1.0, 1e3)):
        c = _cloud(20 + i, 2000, scale)
        out.append(_case(f'random_scale_{scale:g}', c, [2000], 0.07 * scale, (20, 30)))
    return out


CASES = all_cases()
# the lattice case is there for its ties: with k = 8 the 8th and 9th neighbour tie in 117 of the 125 rows
_d2 = np.sort(((lattice()[:, None, :] - lattice()[None, :, :]) ** 2).sum(2), axis=1)
assert int((_d2[:, 7] == _d2[:, 8]).sum()) == 117
