"""The cell-grid radius search (buffer_amd/csrc/radius.hip) against the all-pairs reference of tests/radius_ref.py: every named case of
tests/radius_cases.py through every query path, at every k around the switches of the dispatch.  Rows (cut at k, padded with ns), the
untruncated counts and max_count are compared with np.array_equal: there is no tolerance in this file.

    wave        no order                                  k_grid_query_wave<64|128>
    cell        the grid's own supports in its own order  k_grid_query_cell<64,192|128,512>; stage and row overflows -> lane-per-query pass
    other_grid  the order of a second grid over the queries, at twice the radius (stays inside every element; buffer_amd/pyramid.py)
    perm        a seeded permutation of all queries (crosses elements: those slots go to the lane-per-query pass)
    one_call    ops.radius_neighbors(k=None): count, then fill
    c_abi       the header's contract for a self query in cell order without a todo workspace, k_out = 0: counts only
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import radius_cases
import radius_ref

pytestmark = pytest.mark.gpu

PATHS = ('wave', 'cell', 'other_grid', 'perm', 'one_call', 'c_abi')


def _applies(name, path):
    c = radius_cases.get(name)
    if path in ('cell', 'c_abi'):
        return c.self_query                                                   # the grid's own order orders the grid's own supports
    if path == 'other_grid':
        return c.order_grid                                                   # far_queries: no grid is built over those queries
    if path == 'one_call':
        return c.cells_per_elem == 0 and c.query_radius == c.grid_radius      # the one-call form takes neither
    return True


PARAMS = [(n, p) for n in radius_cases.CASES for p in PATHS if _applies(n, p)]


@functools.lru_cache(maxsize=None)
def _device(name):
    c = radius_cases.get(name)
    dev = torch.device('cuda:0')
    return torch.from_numpy(c.supports.copy()).to(dev), torch.from_numpy(c.queries.copy()).to(dev)


def _grid(name):
    from buffer_amd import ops
    c = radius_cases.get(name)
    return ops.CellGrid(_device(name)[0], c.s_lens, c.grid_radius, cells_per_elem=c.cells_per_elem)


def _check(name, path, k, got, cnt, mc):
    c = radius_cases.get(name)
    ref = radius_cases.reference(name)
    what = f'{name} / {path} / k = {k}'
    assert np.array_equal(cnt, ref[1]), what + ': counts'
    assert mc == ref[2], what + ': max_count'
    if got is not None:
        assert got.shape == (len(c.queries), k), what
        assert np.array_equal(got, radius_ref.expected(ref, k, len(c.supports))), what + ': rows'


@pytest.mark.parametrize('name,path', PARAMS)
def test_grid_query_equals_all_pairs(name, path, dev):
    from buffer_amd import _lib, ops
    c = radius_cases.get(name)
    S, Q = _device(name)
    kmax = radius_cases.reference(name)[2]
    nq = len(c.queries)

    if path == 'one_call':
        got = ops.radius_neighbors(Q, S, c.q_lens, c.s_lens, c.grid_radius).cpu().numpy()
        want = radius_cases.reference(name)[0]
        assert got.shape == want.shape, f'{name} / one_call'
        assert np.array_equal(got, want), f'{name} / one_call'
        return

    grid = _grid(name)
    if path == 'c_abi':
        # include/buffer_hip.h, todo_ws: null is allowed for a self query at k_out == 0
        cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
        mc = torch.zeros(1, dtype=torch.int32, device=dev)
        assert grid.supports.data_ptr() == grid.g.supports and grid.ns == nq
        rc = _lib.lib().buf_grid_query(C.byref(grid.g), C.c_void_p(grid.g.supports), nq, C.c_void_p(grid.s_lengths.ctypes.data),
                                       C.c_void_p(grid.g.order), c.query_radius, 0, None, C.c_void_p(cnt.data_ptr()),
                                       C.c_void_p(mc.data_ptr()), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, 'buf_grid_query')
        _check(name, path, 0, None, cnt.cpu().numpy(), int(mc.item()))
        return

    other = None
    if path == 'wave':
        queries, order = Q, None
    elif path == 'cell':
        queries, order = grid.supports, grid.order
        # the pointer identities the library recognises a self query by: without them this path would run the group kernel and pass
        assert order.data_ptr() == grid.g.order and queries.data_ptr() == grid.g.supports and grid.ns == nq
    elif path == 'other_grid':
        other = ops.CellGrid(Q, c.q_lens, 2 * c.grid_radius)
        queries, order = Q, other.order
    else:
        queries = Q
        order = torch.from_numpy(np.random.default_rng(len(name)).permutation(nq).astype(np.int32)).to(dev)

    for k in radius_cases.KS + (kmax + 3,):
        mc = torch.zeros(1, dtype=torch.int32, device=dev)
        out, cnt = grid.query(queries, c.q_lens, k, radius=c.query_radius, q_order=order, counts=True, max_count=mc)
        _check(name, path, k, out.cpu().numpy(), cnt.cpu().numpy(), int(mc.item()))
        out.fill_(-7)           # the allocator hands these blocks to the next call: a row it leaves unwritten must not find the
        cnt.fill_(-7)           # right answer of this one there
    del other


@pytest.mark.parametrize('name', list(radius_cases.CASES))
def test_grid_order_is_a_stable_permutation_inside_elements(name, dev):
    """two builds of the same grid give the same order; the order permutes every element's rows inside that element's range"""
    c = radius_cases.get(name)
    a, b = _grid(name), _grid(name)
    oa, ob = a.order.cpu().numpy(), b.order.cpu().numpy()
    assert np.array_equal(oa, ob)
    off = np.concatenate([[0], np.cumsum(c.s_lens)])
    for e in range(len(c.s_lens)):
        assert np.array_equal(np.sort(oa[off[e]:off[e + 1]]), np.arange(off[e], off[e + 1])), (name, e)
