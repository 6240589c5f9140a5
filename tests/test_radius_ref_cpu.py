"""The yardstick of tests/test_radius_grid_gpu.py, checked without a GPU: the all-pairs reference (tests/radius_ref.py) against the
plain-C oracle, every named case (tests/radius_cases.py) against the capacity it is named for, and the host export of the cell rule
(buf_grid_cell_dims) against its restatement and on boxes that need far more than 200 coarsening steps."""
import math

import numpy as np
import pytest

import radius_cases
import radius_ref

FINITE = [n for n in radius_cases.CASES if radius_cases.get(n).finite]


@pytest.mark.parametrize('name', FINITE)
def test_reference_equals_oracle(name, oracle):
    """two independent implementations (all pairs in numpy; a cell grid in C) agree bit for bit before either judges the GPU"""
    c = radius_cases.get(name)
    table, counts, mc = radius_cases.reference(name)
    want = oracle.radius_neighbors(c.queries, c.supports, c.q_lens, c.s_lens, c.query_radius)
    assert table.shape == want.shape == (len(c.queries), mc)
    assert np.array_equal(table, want)
    assert np.array_equal(counts, (want < len(c.supports)).sum(1))


@pytest.mark.parametrize('name', list(radius_cases.CASES))
def test_reference_rows_are_well_formed(name):
    """what the table promises, from the definition alone: counts, padding, indices inside the query's own element"""
    c = radius_cases.get(name)
    table, counts, mc = radius_cases.reference(name)
    ns = len(c.supports)
    assert table.dtype == np.int32 and counts.dtype == np.int32 and table.shape == (len(c.queries), mc)
    assert mc == (counts.max() if len(counts) else 0)
    cols = np.arange(mc)[None, :]
    assert (table[cols >= counts[:, None]] == ns).all()
    s_off = np.concatenate([[0], np.cumsum(c.s_lens)])
    elem = np.repeat(np.arange(len(c.q_lens)), c.q_lens)
    valid = cols < counts[:, None]
    assert (table >= s_off[elem][:, None])[valid].all() and (table < s_off[elem + 1][:, None])[valid].all()
    if c.self_query and c.query_radius > 0:
        finite = np.isfinite(c.supports).all(1)
        assert (counts[finite] >= 1).all() and (counts[~finite] == 0).all()       # a finite point finds itself, at d2 = 0
    if name in ('nonfinite', 'nonfinite_self'):
        assert not c.finite and (counts[~np.isfinite(c.queries).all(1)] == 0).all() and counts.max() > 0
        bad = np.flatnonzero(~np.isfinite(c.supports).all(1))
        assert not np.isin(table, bad).any()
        last = len(c.q_lens) - 1
        assert (counts[elem == last] == 0).all() and c.q_lens[last] > 0          # the element without a finite support


def test_reference_ties_and_strict_bound():
    """lattice: equal d2 in ascending index; lattice_edge: d2 == r * r is no neighbour"""
    for name in ('lattice', 'lattice_edge'):
        c = radius_cases.get(name)
        table, counts, _ = radius_cases.reference(name)
        s = c.supports.astype(np.float64)
        ties = 0
        for i in (0, 100, 511):
            row = table[i, :counts[i]]
            d2 = ((s[row] - s[i]) ** 2).sum(1)                                   # exact: the lattice is in quarters
            assert (np.diff(d2) >= 0).all()
            same = np.diff(d2) == 0
            ties += int(same.sum())
            assert (np.diff(row)[same] > 0).all()
        assert ties > 20
    c = radius_cases.get('lattice_edge')
    table, counts, _ = radius_cases.reference('lattice_edge')
    s = c.supports.astype(np.float64)
    d2 = ((s[:, None, :] - s[None, :, :]) ** 2).sum(2)
    r2 = np.float32(c.query_radius) * np.float32(c.query_radius)
    on_edge = d2 == float(r2)
    assert on_edge.sum() >= 512 and r2 == 0.25
    assert np.array_equal(counts, (d2 < 0.25).sum(1))                            # none of them counted


# ---- every case reaches what it is named for -------------------------------------------------------------------------------------
def _sets(name):
    c = radius_cases.get(name)
    return radius_ref.candidate_sets(c.supports, c.s_lens, c.grid_radius, c.cells_per_elem)


def test_uniform_rows_are_short():
    counts = radius_cases.reference('uniform')[1]
    sets, _ = _sets('uniform')
    assert counts.max() <= 32 and sets.max() <= 192          # neither a row nor a stage capacity: the plain path of every kernel


def test_row_caps_reaches_every_length():
    counts = radius_cases.reference('row_caps')[1]
    have = set(counts.tolist())
    assert set(radius_cases.ROW_CAP_LENGTHS) <= have
    assert max(have - set(radius_cases.ROW_CAP_LENGTHS)) < 32          # the background: nothing else near a capacity
    c = radius_cases.get('row_caps')
    _, inverse, copies = np.unique(c.supports, axis=0, return_inverse=True, return_counts=True)
    dup = copies[inverse.reshape(-1)] == 150                           # the clump of exact duplicates: rows of 150, all at d2 = 0
    assert dup.sum() == 150 and (counts[dup] == 150).all()
    table = radius_cases.reference('row_caps')[0]
    assert all(np.array_equal(table[i], np.flatnonzero(dup)) for i in np.flatnonzero(dup))


def test_stage_192_overflows_the_stage_not_the_rows():
    sets, _ = _sets('stage_192')
    counts = radius_cases.reference('stage_192')[1]
    share = float(np.mean(sets > 192))
    print('stage_192: n =', len(sets), 'share of 27-cell sets above 192 =', share, 'longest row =', counts.max())
    assert share >= 0.10
    assert counts.max() <= 64
    assert (sets <= 512).all()


def test_stage_512_overflows_stage_and_rows():
    sets, _ = _sets('stage_512')
    counts = radius_cases.reference('stage_512')[1]
    share = float(np.mean(sets > 512))
    print('stage_512: n =', len(sets), 'share of 27-cell sets above 512 =', share, 'rows above 64:', float(np.mean(counts > 64)),
          'rows above 128:', int(np.sum(counts > 128)))
    assert share >= 0.10 and float(np.mean(sets <= 512)) >= 0.10      # both sides of the stage
    assert np.mean(counts > 64) >= 0.5 and np.sum(counts > 128) >= 10 and np.sum(counts <= 64) >= 10


@pytest.mark.parametrize('cells', [1, 8])
def test_one_cell_sets_are_whole_elements(cells):
    name = f'one_cell_{cells}'
    c = radius_cases.get(name)
    sets, dims = _sets(name)
    assert np.array_equal(sets, np.repeat(c.s_lens, c.s_lens))
    assert all(math.prod(d) == cells for d in dims)


def test_one_cell_27_is_three_cells_a_side():
    """27 slots give a 3 x 3 x 3 table: only its centre cell sees the whole element, so "every set equals the element size" cannot hold
    here (it is asserted for 1 and 8 slots above).  What this variant adds is both sides of the 512 stage in one cloud."""
    sets, dims = _sets('one_cell_27')
    assert dims == [[3, 3, 3], [3, 3, 3]]
    assert (sets > 192).all() and (sets > 512).any() and (sets <= 512).any()


def test_small_radius_shrinks_the_rows():
    full, some, none = (radius_cases.reference(f'small_radius_{r}')[1] for r in ('0.1', '0.04', '0'))
    assert np.array_equal(full, radius_cases.reference('uniform')[1])
    assert (some <= full).all() and some.sum() < full.sum() and some.max() > 1
    assert not none.any()
    for r in ('0.04', '0'):
        c = radius_cases.get(f'small_radius_{r}')
        assert c.query_radius < c.grid_radius == 0.1


def test_offset_is_far_from_the_origin():
    c = radius_cases.get('offset')
    assert np.abs(c.supports).min(0).tolist() >= [1000.0, 1997.0, 50.0]
    assert radius_cases.reference('offset')[2] > 32


def test_outside_queries_land_in_every_cell_off_the_box():
    c = radius_cases.get('outside')
    flat, q = c.supports[:c.s_lens[0]], c.queries[:c.q_lens[0]]
    mn, ext = radius_ref.finite_box(flat)
    edge, dims, _ = radius_ref.cell_rule(ext, c.grid_radius, radius_ref.default_cells(len(c.supports), 3))
    assert dims[2] == 1 and dims[0] > 3 and dims[1] > 3
    close = np.abs(q).max(1) < 1e5
    cq = radius_ref.cell_coords(q[close], mn, edge)
    for axis in range(3):
        seen = set(cq[:, axis].tolist())
        assert {-3, -2, -1, dims[axis], dims[axis] + 1, dims[axis] + 2} <= seen, (axis, sorted(seen))
    counts = radius_cases.reference('outside')[1]
    off_box = ((cq < 0) | (cq >= np.array(dims))).any(1)
    near = counts[:len(q)][close]
    assert near[off_box].max() > 0 and (near[off_box] == 0).any()      # just under r, and just over
    for axis in range(3):                                              # neighbours found from cell -1 of every axis, and from cell dim
        assert near[cq[:, axis] == -1].max() > 0                       # (not on z: its one cell is wider than r and starts at the cloud)
        assert axis == 2 or near[cq[:, axis] == dims[axis]].max() > 0
    assert (~close).sum() == 6 and (counts[:len(q)][~close] == 0).all()
    assert c.s_lens.tolist() == [500, 1, 2]
    o = c.q_lens[0]
    assert counts[o:].max() == 2 and (counts[o:] == 0).any() and (counts[o:] == 1).any()


def test_outlier_needs_58_steps():
    c = radius_cases.get('outlier')
    _, ext = radius_ref.finite_box(c.supports[:c.s_lens[0]])
    _, dims, steps = radius_ref.cell_rule(ext, c.grid_radius, radius_ref.default_cells(len(c.supports), 2))
    assert 50 <= steps < 200, steps               # far, but inside what the loop did before it was unbounded
    sets, _ = _sets('outlier')
    assert (sets[:1500] == 1500).all() and sets[1500] == 1


@pytest.mark.parametrize('nb', [3, 8, 9, 16, 130])
def test_elements_counts_and_ragged_lengths(nb):
    c = radius_cases.get(f'elements_{nb}')
    assert len(c.s_lens) == nb and 0 in c.s_lens and 1 in c.s_lens and len(set(c.s_lens.tolist())) > 2
    table, counts, mc = radius_cases.reference(f'elements_{nb}')
    # leakage would show: ignoring the elements, the same clouds give strictly more neighbours
    n = len(c.supports)
    merged = radius_ref.brute_force(c.queries, c.supports, [n], [n], c.query_radius)[1]
    assert (merged >= counts).all() and merged.sum() > counts.sum()


def test_elements_cross_has_one_sided_elements():
    c = radius_cases.get('elements_cross')
    assert len(c.s_lens) == 8 and not c.self_query
    assert ((c.s_lens == 0) & (c.q_lens > 0)).any() and ((c.s_lens > 0) & (c.q_lens == 0)).any() and ((c.s_lens == 0) & (c.q_lens == 0)).any()


# ---- the host export of the cell rule -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    from buffer_amd import build, ops
    build.build()                      # (a no-op where the in-tree library is newer than its sources)
    return ops


def _boxes():
    for name in radius_cases.CASES:
        yield from radius_cases.built_boxes(name)


def test_every_grid_a_gpu_test_builds_fits_within_200_steps():
    """the regime past 200 coarsening steps is checked on the host only: no GPU test builds such a grid, over supports or over queries"""
    worst = 0
    for what, ext, r, cells in _boxes():
        steps = radius_ref.cell_rule(ext, r, cells)[2]
        assert steps < 200, (what, steps)
        worst = max(worst, steps)
    assert 50 <= worst < 100                       # `outlier` is the farthest any of them goes
    c = radius_cases.get('far_queries')            # the case that is kept away from the order grid, and why
    assert not c.order_grid and np.abs(c.queries).max() > 1e38
    assert radius_ref.cell_rule(radius_ref.finite_box(c.queries)[1], 2 * c.grid_radius, radius_ref.default_cells(len(c.queries), 1))[2] > 200
    assert all(radius_cases.get(n).order_grid for n in radius_cases.CASES if n != 'far_queries')


def test_cell_dims_export_equals_the_restatement_on_every_case(ops):
    seen = 0
    for what, ext, r, cells in _boxes():
        edge, dims, steps = radius_ref.cell_rule(ext, r, cells)
        assert steps < 200, what
        got_edge, got_dims = ops.grid_cell_dims(ext, r, cells)
        assert got_edge == edge and list(got_dims) == dims, what
        seen += 1
    assert seen > 300


@pytest.mark.parametrize('ext,radius,cells', [
    ((1e30, 1e30, 1e30), 0.07, 84752),
    ((1.0, 1e30, 0.5), 0.07, 65536 + 16),
    ((6e38, 6e38, 6e38), 0.07, 1 << 24),
    ((6e38, 0.0, 6e38), 0.07, 1),
    ((1.0, 1.0, 1.0), 1e-42, 100000),             # a subnormal float32 radius
    ((1.0, 1.0, 1.0), 1.401298464324817e-45, 27),
])
def test_cell_dims_export_fits_the_table_however_many_steps(ext, radius, cells, ops):
    """boxes that need far more than the 200 steps the loop used to stop at: the table fits, every dim >= 1"""
    edge, dims, steps = radius_ref.cell_rule(ext, radius, cells)
    assert steps > 200
    got_edge, got_dims = ops.grid_cell_dims(ext, radius, cells)
    assert all(d >= 1 for d in got_dims) and math.prod(got_dims) <= cells
    assert got_edge > max(ext) / cells and math.isfinite(got_edge)
    assert got_edge == edge and list(got_dims) == dims
    # not coarser than needed: one step back does not fit
    back = [math.floor(e / (got_edge / 1.25)) + 1 for e in ext]
    assert math.prod(back) > cells


def test_cell_dims_export_edges(ops):
    from buffer_amd import _lib
    assert ops.grid_cell_dims((0.0, 0.0, 0.0), 0.1, 1) == (float(np.float32(0.1)) * 1.00001, (1, 1, 1))
    assert ops.grid_cell_dims((3.5, 0.0, 1.0), 0.0, 1000) == (1.0, (4, 1, 2))          # r <= 0: unit cells
    assert ops.grid_cell_dims((3.5, 0.0, 1.0), -1.0, 1000) == (1.0, (4, 1, 2))
    assert ops.grid_cell_dims((1.0, 1.0, 1.0), math.inf, 1000)[1] == (1, 1, 1)
    for bad in (((math.inf, 1.0, 1.0), 0.1, 10), ((-1.0, 1.0, 1.0), 0.1, 10), ((math.nan, 1.0, 1.0), 0.1, 10), ((1.0, 1.0, 1.0), math.nan, 10),
                ((1.0, 1.0, 1.0), 0.1, 0)):
        with pytest.raises(_lib.BufferHipError):
            ops.grid_cell_dims(*bad)


def test_far_queries_find_no_cell():
    c = radius_cases.get('far_queries')
    counts = radius_cases.reference('far_queries')[1]
    far = np.abs(c.queries).max(1) > 1e29
    assert far.sum() == 6 and (counts[far] == 0).all() and (counts[~far] >= 1).all()
