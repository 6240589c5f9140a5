"""Inputs shared by tests/test_radius_ref_cpu.py and tests/test_radius_grid_gpu.py: small seeded clouds, each named for the capacity
of the cell-grid kernels (buffer_amd/csrc/radius.hip) it reaches.

    row capacity CAP of the group kernels   64 (k <= 32), 128 (k > 32)         row_caps, stage_512
    LDS stage of the cell-centric kernel    192 (k <= 32), 512 (k > 32)        stage_192, stage_512, one_cell_*, outlier
    column KL of the lane-per-query pass    32 (k <= 32), 64 (k > 32): further sweeps from rows longer than KL
    element counts                          multiples of 8 (block remap), 130 (second offsets launch)      elements_*

A case is a Case tuple; its reference rows (radius_ref.brute_force) are computed once per process and are read-only.
"""
import collections
import functools

import numpy as np

import radius_ref

Case = collections.namedtuple('Case', 'supports s_lens queries q_lens grid_radius query_radius cells_per_elem self_query finite order_grid')

KS = (0, 1, 16, 32, 33, 64, 65, 128, 129)          # and Kmax + 3: both sides of every k-switch of the dispatch, and past the longest row


def _case(s, s_lens, q=None, q_lens=None, r=0.1, rq=None, cells=0, order_grid=True):
    s = np.ascontiguousarray(s, np.float32)
    s_lens = np.asarray(s_lens, np.int32)
    self_query = q is None
    if self_query:
        q, q_lens = s, s_lens
    q = np.ascontiguousarray(q, np.float32)
    q_lens = np.asarray(q_lens, np.int32)
    assert s_lens.sum() == len(s) and q_lens.sum() == len(q) and len(q_lens) == len(s_lens)
    for a in (s, s_lens, q, q_lens):
        a.setflags(write=False)
    finite = bool(np.isfinite(s).all() and np.isfinite(q).all())
    return Case(s, s_lens, q, q_lens, float(r), float(r if rq is None else rq), int(cells), self_query, finite, bool(order_grid))


def _uniform(seed=1):
    rng = np.random.default_rng(seed)
    return rng.random((2400, 3)).astype(np.float32), [1500, 900]


def uniform():
    return _case(*_uniform())


def row_caps():
    """clumps whose rows are exactly 63 .. 150 long (both sides of CAP 64 and 128), one of them 150 copies of one point (every d2 equal:
    the order is the index order alone), and a sparse background; one element, shuffled"""
    rng = np.random.default_rng(2)
    parts = []
    for i, n in enumerate(ROW_CAP_LENGTHS):
        parts.append(np.array([float(i), 0.0, 0.0]) + rng.normal(scale=0.004, size=(n, 3)))
    parts.append(np.tile(np.array([[float(len(ROW_CAP_LENGTHS)), 0.0, 0.0]]), (150, 1)))
    parts.append(rng.random((400, 3)) * np.array([8.0, 2.0, 2.0]) + np.array([0.0, 2.0, 0.0]))
    s = np.concatenate(parts).astype(np.float32)
    return _case(s[rng.permutation(len(s))], [len(s)])


ROW_CAP_LENGTHS = (63, 64, 65, 127, 128, 129, 150)
STAGE_192_N = 1000
STAGE_512_N = 3400


def _cube(seed, n):
    return (np.random.default_rng(seed).random((n, 3)) * 0.5).astype(np.float32)


def stage_192():
    """27-cell sets above the 192-candidate stage while the rows stay within CAP 64: stage overflow without row overflow"""
    return _case(_cube(3, STAGE_192_N), [STAGE_192_N])


def stage_512():
    """27-cell sets above the 512-candidate stage, rows above 64 and above 128"""
    return _case(_cube(4, STAGE_512_N), [STAGE_512_N])


def one_cell(cells):
    return _case(*_uniform(), cells=cells)


def small_radius(rq):
    return _case(*_uniform(), rq=rq)


def offset():
    rng = np.random.default_rng(5)
    s = rng.random((2000, 3)) * np.array([3.0, 3.0, 0.5]) + np.array([1000.0, -2000.0, 50.0])
    return _case(s, [2000], r=0.3)


def _lattice():
    g = np.arange(8) * 0.25
    s = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    return s[np.random.default_rng(6).permutation(len(s))]


def lattice():
    """pitch 0.25 (exact in float32): many equal d2 at different indices and in different distance buckets"""
    return _case(_lattice(), [512], r=0.6)


def lattice_edge():
    """r = 0.5: the points two pitches apart along an axis sit at d2 == r * r exactly, and are no neighbours"""
    return _case(_lattice(), [512], r=0.5)


def outside():
    """a flat cloud (dim z = 1) with queries pushed off every face of its box by just under r, just over r, and by one to three cells
    more, and queries a million units away (a grid built over these queries still fits within 60 coarsening steps); a one-point and
    a two-point element"""
    rng = np.random.default_rng(7)
    r = 0.1
    flat = rng.random((500, 3)) * np.array([1.0, 0.7, 0.0]) + np.array([0.2, -0.4, 0.3])
    flat = flat.astype(np.float32)
    mn, mx = flat.min(0), flat.max(0)
    qs = []
    for axis in range(3):
        by = np.argsort(flat[:, axis], kind='stable')
        for side in (0, 1):
            near = flat[by[:40] if side == 0 else by[-40:]]           # the supports closest to that face
            for d in OUTSIDE_STEPS:
                q = near.copy()
                q[:, axis] = mn[axis] - np.float32(d * r) if side == 0 else mx[axis] + np.float32(d * r)
                qs.append(q)
    far = np.array([[1e6, 0, 0.3], [0.5, -1e6, 0.3], [0.5, 0, 1e6], [-1e6, -1e6, -1e6], [1e6, 1e6, 1e6], [0.5, 0.0, -1e6]])
    q0 = np.concatenate(qs + [far, flat[:100]]).astype(np.float32)
    one = np.array([[5.0, 5.0, 5.0]], np.float32)
    q1 = one + np.array([[0, 0, 0], [0.0999, 0, 0], [0.1001, 0, 0], [0, -0.0999, 0], [0, 0, 0.1001], [0.25, 0.25, 0.25], [-0.15, 0, 0]])
    two = np.array([[-3.0, 1.0, 2.0], [-3.0, 1.0, 2.15]], np.float32)
    q2 = np.concatenate([two, two + np.array([0.0, 0.0, -0.0999]), two + np.array([0.0, 0.0, 0.1001]), two + np.array([0.0999, 0, 0]),
                         two + np.array([0, -0.1001, 0]), two.mean(0, keepdims=True), two + np.array([0.0, 0.0, 0.5])])
    return _case(np.concatenate([flat, one, two]), [500, 1, 2], np.concatenate([q0, q1, q2]), [len(q0), len(q1), len(q2)], r=r)


def far_queries():
    """queries at 1e30 and near the float32 maximum against an ordinary cloud: they find no cell.  order_grid = False: NO grid is ever
    built over these queries (their box would need some 390 coarsening steps, a regime that is checked on the host only)"""
    rng = np.random.default_rng(10)
    s = rng.random((400, 3)).astype(np.float32)
    far = np.array([[0.5, 0, 1e30], [-1e30, -1e30, -1e30], [3e38, 3e38, 3e38], [0.5, 0.5, -3e38], [1e30, 0.5, 0.5], [0.5, -3e38, 0.5]])
    q = np.concatenate([s[:60], far, s[60:100] + np.float32(0.01)]).astype(np.float32)
    return _case(s, [400], q, [len(q)], order_grid=False)


OUTSIDE_STEPS = (0.5, 0.999, 1.001, 1.5, 2.2, 3.5)     # in radii: cells -1 (inside and outside r), -2 and beyond; dim, dim + 1 and beyond


def outlier():
    """one support a million radii away: the edge is coarsened 58 times and the cloud proper falls into one cell"""
    s, lens = _uniform()
    s = np.concatenate([s[:1500], np.full((1, 3), 1e6, np.float32), s[1500:]])
    return _case(s, [1501, 900], r=0.05)


def elements(nb):
    """nb clouds in the same unit cube (a neighbour leaked from another element would show), ragged, an empty and a one-point
    element among them"""
    rng = np.random.default_rng(100 + nb)
    lens = rng.integers(2, 2600 // nb + 2, size=nb)
    lens[[1, nb - 1]] = 0, 1
    return _case(rng.random((int(lens.sum()), 3)), lens, r=0.2)


def elements_cross():
    """8 elements whose query and support lengths differ: supports without queries, queries without supports"""
    rng = np.random.default_rng(200)
    s_lens = np.array([300, 0, 150, 1, 400, 200, 0, 77])
    q_lens = np.array([100, 50, 0, 30, 1, 333, 0, 129])
    return _case(rng.random((int(s_lens.sum()), 3)), s_lens, rng.random((int(q_lens.sum()), 3)), q_lens, r=0.15)


def _nonfinite_supports():
    rng = np.random.default_rng(8)
    s = rng.random((600, 3)).astype(np.float32)
    bad = rng.permutation(600)[:24]
    vals = [np.nan, np.inf, -np.inf]
    for j, i in enumerate(bad):
        s[i, j % 3] = vals[(j // 3) % 3]
    s[bad[0]] = np.nan
    s[bad[1]] = np.inf
    s[bad[2]] = (-np.inf, np.inf, np.nan)
    dead = np.array([[np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf], [-np.inf, 0.5, 0.5], [0.5, np.nan, 0.5]] * 5, np.float32)
    return np.concatenate([s, dead]), [600, len(dead)]


def nonfinite():
    """NaN and +-inf coordinates among the supports and among the queries; the second element has no finite support at all"""
    s, s_lens = _nonfinite_supports()
    rng = np.random.default_rng(9)
    q = rng.random((330, 3)).astype(np.float32)
    q[5] = np.nan
    q[17, 0] = np.inf
    q[40, 1] = -np.inf
    q[41, 2] = np.nan
    q[99] = (np.inf, -np.inf, np.inf)
    q[310, 1] = np.nan
    q[320] = np.inf
    return _case(s, s_lens, q, [300, 30], r=0.15)


def nonfinite_self():
    s, s_lens = _nonfinite_supports()
    return _case(s, s_lens, r=0.15)


CASES = {
    'uniform': uniform,
    'row_caps': row_caps,
    'stage_192': stage_192,
    'stage_512': stage_512,
    'one_cell_1': functools.partial(one_cell, 1),
    'one_cell_8': functools.partial(one_cell, 8),
    'one_cell_27': functools.partial(one_cell, 27),
    'small_radius_0.1': functools.partial(small_radius, 0.1),
    'small_radius_0.04': functools.partial(small_radius, 0.04),
    'small_radius_0': functools.partial(small_radius, 0.0),
    'offset': offset,
    'lattice': lattice,
    'lattice_edge': lattice_edge,
    'outside': outside,
    'far_queries': far_queries,
    'outlier': outlier,
    'elements_3': functools.partial(elements, 3),
    'elements_8': functools.partial(elements, 8),
    'elements_9': functools.partial(elements, 9),
    'elements_16': functools.partial(elements, 16),
    'elements_130': functools.partial(elements, 130),
    'elements_cross': elements_cross,
    'nonfinite': nonfinite,
    'nonfinite_self': nonfinite_self,
}


def built_boxes(name):
    """every box a GPU test builds a grid over for this case -> (what, extent f64[3], radius, table slots per element): the supports
    at the grid radius, and -- where the case allows an order grid -- the queries at twice that radius (the `other_grid` path)"""
    c = get(name)
    sets = [('supports', c.supports, c.s_lens, c.grid_radius, c.cells_per_elem)]
    if c.order_grid:
        sets.append(('queries', c.queries, c.q_lens, 2 * c.grid_radius, 0))
    for what, pts, lens, r, cells in sets:
        cells = cells or radius_ref.default_cells(len(pts), len(lens))
        off = 0
        for b, n in enumerate(lens):
            yield f'{name} {what}[{b}]', radius_ref.finite_box(pts[off:off + n])[1], r, cells
            off += n


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(table, counts, max_count) of the all-pairs search at the case's QUERY radius; computed once, read-only"""
    c = get(name)
    table, counts, mc = radius_ref.brute_force(c.queries, c.supports, c.q_lens, c.s_lens, c.query_radius)
    table.setflags(write=False)
    counts.setflags(write=False)
    return table, counts, mc
