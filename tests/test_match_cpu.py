"""The float32 twin of the descriptor-matching contract (tests/match_ref.py) pinned on the CPU -- against the float64 twin of
fpfh.match where the two rankings agree, and on the non-finite, single-row and ratio rules by hand -- and the host-side pieces of the
operator: the ctypes signature, the header, the --match-ratio option, the stand-in's entry.  No device."""
import ctypes as C
import os

import numpy as np
import pytest

import fpfh_ref
import match_ref

# forward matches, and those the mutual filter, the ratio filter (0.8) and both keep, per case of match_ref.CASES + WIDE_CASES (the
# twin's own figures on the seeded inputs: they pin the generator, and show that each filter keeps some matches and drops others)
COUNTS = {(1, 130, 257, 33): (130, 85, 65, 57), (2, 64, 65, 33): (64, 33, 32, 24), (3, 257, 130, 32): (257, 101, 129, 82),
          (5, 200, 200, 7): (200, 106, 127, 84), (6, 65, 64, 36): (65, 34, 33, 27), (7, 63, 129, 40): (63, 41, 32, 29),
          (8, 70, 131, 64): (70, 44, 35, 32)}


@pytest.mark.parametrize('case', match_ref.CASES + match_ref.WIDE_CASES, ids=lambda c: 'seed%d-%dx%d-d%d' % c)
def test_twin_equals_the_float64_match_where_the_rankings_agree(case):
    a, b = match_ref.make_pair(*case)
    s = match_ref.ssd(a, b)
    assert s.dtype == np.float32 and np.array_equal(s, match_ref.ssd(b, a).T)               # ssd(i, j) is the bits of ssd(j, i)
    pad = lambda x: np.concatenate([x, np.zeros((len(x), 3), np.float32)], 1)
    assert np.array_equal(s, match_ref.ssd(pad(a), pad(b)))                                 # zero dimensions change nothing
    # the fp64 ranking of fpfh_ref.match and the fp32 ranking of the twin agree on this case, in both directions: asserted, not assumed
    d64 = ((a.astype(np.float64)[:, None, :] - b.astype(np.float64)[None, :, :]) ** 2).sum(2)
    assert np.array_equal(d64.argmin(1), match_ref.two_nearest(a, b)[0][:, 0])
    assert np.array_equal(d64.argmin(0), match_ref.two_nearest(b, a)[0][:, 0])
    for mutual in (True, False):
        assert np.array_equal(match_ref.match(a, b, mutual)['corr'], fpfh_ref.match(a, b, mutual))
    got = tuple(len(match_ref.match(a, b, m, r)['corr']) for m, r in ((False, None), (True, None), (False, match_ref.RATIO),
                                                                      (True, match_ref.RATIO)))
    assert got == COUNTS[case]
    f, mu, ra, both = got
    assert 0 < mu < f and 0 < ra < f and 0 < both < min(mu, ra)                             # a filter that drops nothing tests nothing
    # the filtered lists are sub-lists of the forward matches, in order
    fw = [tuple(r) for r in match_ref.match(a, b, False)['corr']]
    for m, r in ((True, None), (False, match_ref.RATIO), (True, match_ref.RATIO)):
        rows = [tuple(x) for x in match_ref.match(a, b, m, r)['corr']]
        assert set(rows) <= set(fw) and rows == sorted(rows)


def test_second_nearest_ties_and_keys():
    b = np.repeat(np.random.default_rng(0).random((5, 4)).astype(np.float32), 2, 0)         # rows 2k and 2k + 1 are twins
    a = b[[4, 5, 0]]
    nn, sd = match_ref.two_nearest(a, b)
    assert nn.tolist() == [[4, 5], [4, 5], [0, 1]] and not sd.any()                          # ties go to the lower row, then the next
    m = match_ref.match(a, b, True)['corr']
    assert m.tolist() == [[0, 4], [2, 0]]                                                    # b[4]'s nearest row of a is 0, not 1


def test_non_finite_rows_match_nobody_and_are_matched_by_nobody():
    rng = np.random.default_rng(4)
    b = rng.random((9, 5)).astype(np.float32)
    a = (b[[3, 3, 7, 1, 2]] + np.float32(0.01)).astype(np.float32)
    a[1, 2], a[3, 0] = np.nan, np.inf
    b[7, 4], b[0, 0] = -np.inf, np.nan
    r = match_ref.match(a, b, False)
    assert r['nn'][1].tolist() == [-1, -1] and r['nn'][3].tolist() == [-1, -1] and np.isinf(r['ssd'][[1, 3]]).all()
    assert not np.isin(r['nn'], [0, 7]).any()                                                # nobody is matched to a non-finite row
    assert r['corr'][:, 0].tolist() == [0, 2, 4] and r['nn'][0, 0] == 3 and r['nn'][4, 0] == 2 and r['nn'][2, 0] not in (-1, 7)
    back = match_ref.two_nearest(b, a)[0]
    assert back[7].tolist() == [-1, -1] and back[0].tolist() == [-1, -1] and not np.isin(back, [1, 3]).any()
    assert match_ref.match(a[[1, 3]], b, True)['corr'].shape == (0, 2)
    # a finite row whose sum overflows is ranked like any other
    big = np.array([[3e38, -3e38]], np.float32)
    r = match_ref.match(big, np.array([[-3e38, 3e38], [3e38, -3e38]], np.float32), False, 0.5)
    assert r['nn'].tolist() == [[1, 0]] and r['ssd'][0, 0] == 0 and np.isinf(r['ssd'][0, 1]) and len(r['corr']) == 1


def test_single_row_and_empty_sides():
    a = np.random.default_rng(2).random((6, 33)).astype(np.float32)
    r = match_ref.match(a, a[2:3], False, match_ref.RATIO)
    assert r['nn'].tolist() == [[0, -1]] * 6 and np.isinf(r['ssd'][:, 1]).all()
    assert r['corr'].tolist() == [[i, 0] for i in range(6)]                                  # no second neighbour: the test passes
    assert match_ref.match(a, a[2:3], True, match_ref.RATIO)['corr'].tolist() == [[2, 0]]
    for x, y in ((a[:0], a), (a, a[:0])):
        r = match_ref.match(x, y, True, match_ref.RATIO)
        assert r['corr'].shape == (0, 2) and r['nn'].shape == (len(x), 2) and (r['nn'] == -1).all()
    st = match_ref.match_batch([(a, a[2:3]), (a[:0], a), (a[:3], a)], True)
    assert st['counts'].tolist() == [1, 0, 3] and st['corr'].tolist() == [[2, 0], [0, 0], [1, 1], [2, 2]] and st['nn'].shape == (9, 2)


def test_ratio_rule_by_hand():
    b = np.array([[0.0], [1.0], [10.0]], np.float32)
    a = np.array([[0.4], [0.5], [9.0]], np.float32)                                          # ssd1 / ssd2: .16/.36, .25/.25, 1/64
    assert match_ref.ratio_squared(0.8) == np.float32(np.float64(np.float32(0.8)) ** 2)
    assert match_ref.match(a, b, False, 0.8)['corr'].tolist() == [[0, 0], [2, 2]]          # 0.16 <= 0.64 * 0.36 = 0.2304; 0.25 > 0.16
    assert match_ref.match(a, b, False, 0.6)['corr'].tolist() == [[2, 2]]                  # 0.16 > 0.36 * 0.36
    assert match_ref.match(a, b, False, 0.0)['corr'].tolist() == match_ref.match(a, b, False)['corr'].tolist()
    z = np.zeros((2, 1), np.float32)
    assert match_ref.match(z[:1], z, False, 0.5)['corr'].tolist() == [[0, 0]]              # 0 <= r2 * 0


def test_ctypes_signature_and_header():
    from buffer_amd import _lib
    assert {'buf_feature_match', 'buf_feature_match_ws_bytes'} <= set(_lib.exported_symbols())
    L = _lib.lib()
    fn = L.buf_feature_match
    assert fn.restype is C.c_int
    want = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert list(fn.argtypes) == want
    ws = L.buf_feature_match_ws_bytes
    assert ws.restype is C.c_size_t and list(ws.argtypes) == [C.c_longlong, C.c_longlong, C.c_int]
    # meta ints | two keys per row of A | two per row of B | a flag per row of A, each piece on a 256-byte boundary
    assert ws(1000, 2000, 3) >= 4 * 15 + 16 * 1000 + 16 * 2000 + 1000 and ws(0, 0, 0) >= 1 and ws(1 << 33, 1 << 33, 1) > 1 << 38
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'buffer_hip.h')).read()
    assert 'int     buf_feature_match(const float* fa, const int* a_lengths_host, const float* fb, const int* b_lengths_host,' in hdr
    assert 'size_t  buf_feature_match_ws_bytes(long long na_total, long long nb_total, int pairs);' in hdr
    assert 'forward direction only' in hdr
    # the argument checks that need no device
    null = C.c_void_p(0)
    one = (C.c_int * 1)(4)
    assert fn(null, one, null, one, 1, 33, 1, 1.0, null, null, null, null, null, 0, null) == -1 and b'ratio' in L.buf_last_error()
    assert fn(null, one, null, one, 1, 33, 1, float('nan'), null, null, null, null, null, 0, null) == -1
    assert fn(null, one, null, one, 1, 65, 1, 0.0, null, null, null, null, null, 0, null) == -1 and b'd=65' in L.buf_last_error()
    assert fn(null, one, null, one, -1, 33, 1, 0.0, null, null, null, null, null, 0, null) == -1
    assert fn(null, null, null, null, 0, 33, 1, 0.0, null, null, null, null, null, 0, null) == 0      # no pairs: nothing to do


def test_match_ratio_option(capsys):
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r'])
        assert a.match_ratio is None
        a, _ = mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--match-ratio', '0.8', '--estimator', 'fgr'])
        assert a.match_ratio == 0.8 and a.descriptor == 'fpfh' and a.estimator == 'fgr'
        with pytest.raises(SystemExit) as e:
            mod.parse_args(['--root', 'r', '--match-ratio', '0.8'])
        assert e.value.code == 2 and '--match-ratio 0.8' in capsys.readouterr().err
        for bad in ('0', '1', '1.5', '-0.2', 'nan'):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(['--root', 'r', '--descriptor', 'fpfh', '--match-ratio', bad])
            assert e.value.code == 2 and '(0, 1)' in capsys.readouterr().err


def test_python_entries_and_standin():
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    from buffer_amd import fpfh, ops
    from buffer_amd.config import THREEDMATCH
    regm = o3d.pipelines.registration
    assert callable(ops.feature_match) and callable(fpfh.match_batch) and callable(regm.correspondences_from_features)
    assert 'correspondences_from_features' in o3d.__doc__
    empty = regm.correspondences_from_features(regm.Feature(np.zeros((33, 0))), regm.Feature(np.zeros((33, 5))), True)
    assert empty.shape == (0, 2) and empty.dtype == np.int32                                 # empty in, empty out: no device
    with pytest.raises(ValueError):
        regm.correspondences_from_features(regm.Feature(np.zeros((33, 2))), regm.Feature(np.zeros((32, 2))))
    for bad in (0.0, 1.0, float('nan')):
        with pytest.raises(ValueError):
            fpfh.FpfhRegistration(THREEDMATCH, 'cuda:0', match_ratio=bad)
