"""The plain-C oracle (oracle/buffer_oracle.c: A1 grid subsample, A2 radius neighbours) against the reference's OWN compiled
cores (oracle/_ref = neighbors.cpp + grid_subsampling.cpp + cloud.cpp built in place from /root/reference by oracle/Makefile)
at 3DMatch size: the whole 3-level pyramid of a stacked 3DMatch-shape pair (≈21k / 5k / 1.4k points, all seven query shapes),
the KITTI shape, and ragged / tiny batch elements.  Neighbour tables index-exact except inside groups of exactly equal d2
(the reference's order there is what std::sort leaves of the KD-tree traversal); subsampled layers the same multiset of rows,
bit for bit.  Where oracle/_ref could not be built (the reference tree is not present), the oracle is checked against the
reference cores' results stored as digests in tests/golden/oracle_vs_ref.json: sha256 of every neighbour table with each row
in (d2, index) order -- equal exactly when the tables agree up to the order inside groups of equal d2 -- and of every
subsampled layer with its rows sorted per batch element.  Where oracle/_ref exists, the live comparison runs and the
reference's digests must equal the stored ones.  `python tests/test_oracle_vs_ref.py` rewrites that file from oracle/_ref."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from buffer_amd import synth  # noqa: E402
from util import assert_neighbors_equal_mod_ties as nbr_eq, d2_table  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'oracle_vs_ref.json')


def _canon(a):
    return a[np.lexsort(a.T[::-1])]


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(str(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _nbr_digest(tab, q, s):
    """a neighbour table with every row in (d2, index) order"""
    tab = np.asarray(tab).astype('<i4')
    order = np.lexsort((tab, d2_table(q, s, tab)))
    return _digest(np.take_along_axis(tab, order, 1))


def _sub_digest(sub, sl):
    """a subsampled layer: its batch lengths and each element's rows sorted"""
    lo, parts = 0, [np.asarray(sl).astype('<i4')]
    for n in sl:
        parts.append(_canon(sub[lo:lo + n]).view(np.uint32).astype('<u4'))
        lo += n
    return _digest(*parts)


class _Check:
    """one case: the live comparison with oracle/_ref where it was built, the stored digests of the reference's results elsewhere"""

    def __init__(self, o, case, record=None):
        self.o, self.live = o, o.have_ref()
        self.want = None
        if record is None:
            with open(GOLDEN) as f:
                self.want = json.load(f)[case]
        self.record, self.i = record, 0

    def _next(self, digest):
        if self.record is not None:
            self.record.append(digest)
        else:
            assert digest == self.want[self.i], f'call {self.i}: the reference cores\' stored result differs'
        self.i += 1

    def nbr(self, q, s, qb, sb, r):
        a = self.o.radius_neighbors(q, s, qb, sb, r)
        if self.live:
            b = self.o.ref_radius_neighbors(q, s, qb, sb, r)
            nbr_eq(a, b, q, s)
            self._next(_nbr_digest(b, q, s))
        else:
            # the digest fixes each row's set of (d2, index) entries; the live comparison's order (ascending d2, ties free) and
            # duplicate-free rows are checked here
            self._next(_nbr_digest(a, q, s))
            d2 = d2_table(q, s, a)
            assert (d2[:, 1:] >= d2[:, :-1]).all(), 'rows not in ascending d2 order'
            for row in a:
                real = row[row < len(s)]
                assert len(np.unique(real)) == len(real)
        return a

    def sub(self, pts, lens, r):
        sub, sl = self.o.grid_subsample_batch(pts, lens, r)
        if self.live:
            rsub, rsl = self.o.ref_grid_subsample_batch(pts, lens, r)
            assert np.array_equal(sl, rsl)
            lo = 0
            for n in sl:                                               # same rows per batch element, the reference in hash order
                assert np.array_equal(_canon(sub[lo:lo + n]).view(np.uint32), _canon(rsub[lo:lo + n]).view(np.uint32))
                lo += n
            self._next(_sub_digest(rsub, rsl))
        else:
            self._next(_sub_digest(sub, sl))
        return sub, sl

    def done(self):
        assert self.record is not None or self.i == len(self.want)


def _pyramid_both_ways(c, pts, lens, r0, layers=3):
    r = r0
    for l in range(layers):
        c.nbr(pts, pts, lens, lens, r)
        if l == layers - 1:
            break
        sub, sl = c.sub(pts, lens, r)
        c.nbr(sub, pts, sl, lens, r)
        c.nbr(pts, sub, lens, sl, 2 * r)
        pts, lens, r = sub, sl, 2 * r
    c.done()


@pytest.fixture(scope="module")
def o(oracle):
    return oracle


def _case_3dmatch(o, record=None):
    s = synth.make_pair(4)
    pts = np.concatenate([s['src_sds_pts'][:, :3], s['tgt_sds_pts'][:, :3]]).astype(np.float32)
    lens = np.array([len(s['src_sds_pts']), len(s['tgt_sds_pts'])], np.int32)
    assert pts.shape[0] > 15000
    _pyramid_both_ways(_Check(o, '3dmatch', record), pts, lens, 0.07)


def _case_kitti(o, record=None):
    s = synth.make_kitti_pair(2)
    pts = np.concatenate([s['src_sds_pts'][:, :3], s['tgt_sds_pts'][:, :3]]).astype(np.float32)
    lens = np.array([len(s['src_sds_pts']), len(s['tgt_sds_pts'])], np.int32)
    _pyramid_both_ways(_Check(o, 'kitti', record), pts, lens, 0.6)    # KITTI: 0.30 m voxels, wrapped voxel keys at dl = 0.6


def _case_ragged(o, record=None):
    rng = np.random.default_rng(0)
    p = (rng.random((3000, 3)) * [1.5, 1.0, 0.2] + 0.4).astype(np.float32)
    # tiny elements.  (An EMPTY element is not compared: neighbors.cpp:268-283 advances one batch element per query, so the
    # first query after an empty element is searched in the wrong tree -- never reached by BUFFER, whose fragments are not
    # empty; the oracle and the kernels give every point of the following element its own neighbours.)
    _pyramid_both_ways(_Check(o, 'ragged', record), p, np.array([1, 2, 1500, 1497], np.int32), 0.07, layers=2)


def test_oracle_equals_reference_cores_at_3dmatch_size(o):
    _case_3dmatch(o)


def test_oracle_equals_reference_cores_on_kitti_shape_and_ragged_batches(o):
    _case_kitti(o)
    _case_ragged(o)


if __name__ == '__main__':                                             # rewrite the stored digests from oracle/_ref
    from oracle import cpu
    cpu.build(ref=True)
    assert cpu.have_ref(), 'oracle/_ref not built (needs the reference tree at build time)'
    rec = {}
    for name, fn in (('3dmatch', _case_3dmatch), ('kitti', _case_kitti), ('ragged', _case_ragged)):
        rec[name] = []
        fn(cpu, rec[name])
    with open(GOLDEN, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('wrote', GOLDEN)
