"""buf_grid_knn (N14) against the all-pairs restatement of tests/knn3_ref.py on the cases of tests/knn3_cases.py: identical indices,
d2_out bit-equal to sqdist3 of the reported index, agreement with CellGrid.query wherever its row holds k entries, independence of the
processing order and of the batch, and every BUF_EINVAL through the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn3_ref
from knn3_cases import CASES

pytestmark = pytest.mark.gpu

_REF = {}
EINVAL = -1            # BUF_EINVAL (include/buffer_hip.h)


def _ref(case, k):
    key = (case['name'], k)
    if key not in _REF:
        _REF[key] = knn3_ref.brute_force(case['queries'], case['supports'], case['q_lens'], case['s_lens'], k)
    return _REF[key]


def _run(case, k, dev, order=None):
    from buffer_amd import ops
    grid = ops.CellGrid(torch.from_numpy(case['supports']).to(dev), case['s_lens'], case['radius'], case['cells'])
    q = torch.from_numpy(case['queries']).to(dev)
    if order is not None:
        order = torch.from_numpy(order).to(dev)
    nbr, d2 = grid.knn(q, case['q_lens'], k, q_order=order, return_d2=True)
    return grid, q, nbr, d2


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_rows_equal_the_restatement(case, dev):
    ns = len(case['supports'])
    for k in case['ks']:
        want_nbr, want_d2 = _ref(case, k)
        grid, q, nbr, d2 = _run(case, k, dev, case['order'])
        nbr, d2 = nbr.cpu().numpy(), d2.cpu().numpy()
        assert nbr.shape == (len(case['queries']), k) and nbr.dtype == np.int32 and d2.dtype == np.float32
        assert np.array_equal(nbr, want_nbr), (case['name'], k, np.argwhere(nbr != want_nbr)[:5])
        # d2_out: the bits of sqdist3 of the reported index, +inf in the padding
        assert np.array_equal(d2.view(np.uint32), knn3_ref.d2_of(case['queries'], case['supports'], nbr).view(np.uint32))
        assert np.array_equal(d2.view(np.uint32), want_d2.view(np.uint32))
        assert np.array_equal(nbr == ns, np.isinf(d2))
        # the same rows without d2_out, and wherever the ball of CellGrid.query holds k entries its first k columns
        assert torch.equal(grid.knn(q, case['q_lens'], k), torch.from_numpy(want_nbr).to(dev))
        rows, cnt = grid.query(q, case['q_lens'], k, counts=True)
        full = (cnt >= k).cpu().numpy()
        assert np.array_equal(rows.cpu().numpy()[full], want_nbr[full])


def test_padding_and_identical_points(dev):
    five = next(c for c in CASES if c['name'] == 'five_points')
    _, _, nbr, d2 = _run(five, 8, dev)
    assert bool((nbr[:, 5:] == 5).all()) and bool(torch.isinf(d2[:, 5:]).all()) and bool((nbr[:, :5] < 5).all())
    assert torch.equal(nbr[:, 0].cpu(), torch.arange(5, dtype=torch.int32))
    same = next(c for c in CASES if c['name'] == 'identical')
    _, _, nbr, d2 = _run(same, 10, dev)
    assert torch.equal(nbr.cpu(), torch.arange(10, dtype=torch.int32).repeat(100, 1)) and bool((d2 == 0).all())


def test_rows_stay_inside_their_cloud_and_do_not_depend_on_the_batch(dev):
    from buffer_amd import ops
    case = next(c for c in CASES if c['name'] == 'stacked_300_0_7')
    _, _, nbr, d2 = _run(case, 16, dev)
    nbr = nbr.cpu().numpy()
    ns = 307
    assert ((nbr[:300] < 300) | (nbr[:300] == ns)).all() and ((nbr[300:] >= 300)).all()
    assert (nbr[300:, 7:] == ns).all() and (nbr[300:, :7] < ns).all()
    # each cloud alone: the same rows (indices shifted by the cloud's offset), the same d2 bits
    for lo, hi in ((0, 300), (300, 307)):
        pts = torch.from_numpy(case['supports'][lo:hi]).to(dev)
        a_nbr, a_d2 = ops.CellGrid(pts, [hi - lo], case['radius']).knn(pts, [hi - lo], 16, return_d2=True)
        a_nbr = a_nbr.cpu().numpy()
        want = np.where(nbr[lo:hi] == ns, hi - lo, nbr[lo:hi] - lo)
        assert np.array_equal(a_nbr, want)
        assert torch.equal(a_d2.view(torch.int32), d2[lo:hi].view(torch.int32))
    # an empty element on the query side as well, and no queries at all
    g = ops.CellGrid(torch.from_numpy(case['supports']).to(dev), case['s_lens'], case['radius'])
    q = torch.from_numpy(case['supports'][:4]).to(dev)
    r = g.knn(q, [0, 4, 0], 3)                                   # four queries of the empty element: padded rows
    assert bool((r == ns).all())
    assert g.knn(q[:0], [0, 0, 0], 3).shape == (0, 3)


def test_processing_order_does_not_change_a_bit(dev):
    case = next(c for c in CASES if c['name'] == 'random_order')
    for k in case['ks']:
        grid, q, nbr, d2 = _run(case, k, dev, case['order'])
        for order in (None, grid.order):
            n2, e2 = grid.knn(q, case['q_lens'], k, q_order=order, return_d2=True)
            assert torch.equal(nbr, n2) and torch.equal(d2.view(torch.int32), e2.view(torch.int32))


def test_einval_through_the_c_abi(dev):
    from buffer_amd import _lib, ops
    L = _lib.lib()
    pts = torch.rand((50, 3), device=dev)
    grid = ops.CellGrid(pts, [50], 0.2)
    out = torch.empty((50, 64), dtype=torch.int32, device=dev)
    lens, bad_lens, neg = (C.c_int * 1)(50), (C.c_int * 1)(49), (C.c_int * 1)(-1)
    P = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)

    def call(g=True, q=P(pts), nq=50, ql=lens, k=8, o=P(out)):
        rc = L.buf_grid_knn(C.byref(grid.g) if g else None, q, nq, ql, null, k, o, null, null)
        return rc, L.buf_last_error().decode()

    assert call()[0] == 0
    for k in (0, -1, 65, 1 << 20):
        rc, msg = call(k=k)
        assert rc == EINVAL and f'buf_grid_knn: k={k} (1 <= k <= 64)' in msg
    rc, msg = call(nq=-1)
    assert rc == EINVAL and 'buf_grid_knn: nq=-1' in msg
    for kw in (dict(g=False), dict(ql=null)):
        rc, msg = call(**kw)
        assert rc == EINVAL and 'buf_grid_knn: null argument' in msg
    rc, msg = call(ql=bad_lens)
    assert rc == EINVAL and 'buf_grid_knn: batch lengths sum to 49, expected 50' in msg
    rc, msg = call(ql=neg)
    assert rc == EINVAL and 'buf_grid_knn: negative batch length' in msg
    rc, msg = call(q=null)
    assert rc == EINVAL and 'buf_grid_knn: null queries' in msg
    rc, msg = call(o=null)
    assert rc == EINVAL and 'buf_grid_knn: null nbr_out' in msg
    assert call(nq=0, ql=(C.c_int * 1)(0), q=null, o=null)[0] == 0
    torch.cuda.synchronize()
