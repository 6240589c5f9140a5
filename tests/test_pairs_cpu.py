"""Host side of buffer_amd/pairs.py: the information matrix from moments, the gt.log / gt.info writer, the bounding-box prefilter and
the command line's errors.  No device needed."""
import json
import os

import numpy as np
import pytest

import pairs_ref


def _moments(p):
    terms = np.stack([p[:, 0], p[:, 1], p[:, 2], p[:, 0] * p[:, 0], p[:, 0] * p[:, 1], p[:, 0] * p[:, 2], p[:, 1] * p[:, 1],
                      p[:, 1] * p[:, 2], p[:, 2] * p[:, 2]], 1)
    return terms.sum(0), terms


@pytest.mark.parametrize("n,scale,shift", [(5000, 1.0, 0.0), (1, 2.0, 1.0), (20000, 30.0, 5.0), (257, 0.05, -3.0)])
def test_information_matrix_from_moments(n, scale, shift):
    """Both conventions from (n, sum u, sum u u^T) equal the explicit per-point sums.  Both sides are fp64 sums of the same n terms in
    different orders, so entry by entry |diff| <= 2 (N - 1) 2^-53 sum|term| with N the number of terms of the entry: n for the entries
    that are +-1, +-2 or 4 times one moment (the scaling is exact), 2n for a diagonal rotation entry (yy + zz and the like)."""
    from buffer_amd import pairs, synth
    rng = np.random.default_rng(n)
    p = rng.normal(size=(n, 3)) * scale + shift
    m, terms = _moments(p)
    b = pairs_ref.sum_bound(terms)                       # per moment: x y z xx xy xz yy yz zz
    bs, buu = b[:3], b[3:]
    cross_b = np.array([[0, bs[2], bs[1]], [bs[2], 0, bs[0]], [bs[1], bs[0], 0]])
    two = lambda a, c: pairs_ref.sum_bound(np.concatenate([terms[:, a], terms[:, c]])[:, None])[0]      # an entry of 2n terms
    rot_b = np.array([[two(6, 8), buu[1], buu[2]], [buu[1], two(3, 8), buu[4]], [buu[2], buu[4], two(3, 6)]])

    got = pairs.information_matrix(n, m[:3], m[3:], '3dmatch')
    want = synth.information_matrix(p)
    bound = np.zeros((6, 6))
    bound[:3, 3:], bound[3:, :3], bound[3:, 3:] = 2 * cross_b, 2 * cross_b.T, 4 * rot_b
    assert got[0, 0] == n and np.all(np.abs(got - want) <= bound), np.abs(got - want) - bound

    G = np.zeros((n, 3, 6))                               # the three rows of open3d's G per target point (x, y, z)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    G[:, 0, 1], G[:, 0, 2], G[:, 0, 3] = z, -y, 1.0       # [ 0,  z, -y, 1, 0, 0]
    G[:, 1, 0], G[:, 1, 2], G[:, 1, 4] = -z, x, 1.0       # [-z,  0,  x, 0, 1, 0]
    G[:, 2, 0], G[:, 2, 1], G[:, 2, 5] = y, -x, 1.0       # [ y, -x,  0, 0, 0, 1]
    want = np.einsum('nij,nik->jk', G, G)
    got = pairs.information_matrix(n, m[:3], m[3:], 'open3d')
    bound = np.zeros((6, 6))
    bound[:3, 3:], bound[3:, :3], bound[:3, :3] = cross_b, cross_b.T, rot_b
    assert got[5, 5] == n and np.all(np.abs(got - want) <= bound), np.abs(got - want) - bound
    with pytest.raises(ValueError):
        pairs.information_matrix(n, m[:3], m[3:], 'colmap')


def _fake_pairs(rng, keys):
    from buffer_amd import synth
    out = []
    for i, j in keys:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = synth.random_rotation(rng), rng.normal(size=3)
        info = synth.information_matrix(rng.normal(size=(50, 3)))
        out.append(dict(i=i, j=j, T=T, info=info, overlap=0.4, overlap_i=0.4, overlap_j=0.5, matched_i=40, matched_j=50, inlier_rmse=0.01))
    return out


def test_write_gt_round_trip_and_overwrite(tmp_path):
    from buffer_amd import evaluate, pairs, threedmatch as tdm
    rng = np.random.default_rng(1)
    ps = _fake_pairs(rng, [(1, 4), (0, 2), (0, 1), (2, 3)])            # given out of order: written ascending by (i, j)
    gt = str(tmp_path / 'gt')
    pairs.write_gt(gt, ps, 5, voxel=0.025, radius=0.0375)
    ordered = sorted(ps, key=lambda p: (p['i'], p['j']))
    log = tdm.load_gt_log(gt)
    assert list(log) == [f"{p['i']}_{p['j']}" for p in ordered]
    for p in ordered:
        assert np.array_equal(log[f"{p['i']}_{p['j']}"], p['T'])        # repr(float) round-trips fp64 exactly
    keys, traj = evaluate.read_trajectory(os.path.join(gt, 'gt.log'))
    assert [tuple(k) for k in keys] == [(str(p['i']), str(p['j']), '5') for p in ordered]
    assert np.array_equal(traj, np.array([p['T'] for p in ordered]).astype(np.float32))       # (the reader keeps fp32)
    n_frag, info = evaluate.read_trajectory_info(os.path.join(gt, 'gt.info'))
    assert n_frag == 5 and np.array_equal(info, np.array([p['info'] for p in ordered]).astype(np.float32))
    meta = json.load(open(os.path.join(gt, 'gt_overlap.json')))
    assert meta['voxel'] == 0.025 and meta['radius'] == 0.0375 and [(p['i'], p['j']) for p in meta['pairs']] == [(p['i'], p['j']) for p in ordered]
    assert meta['pairs'][0]['overlap_i'] == 0.4 and meta['pairs'][0]['matched_j'] == 50
    with pytest.raises(FileExistsError):
        pairs.write_gt(gt, ps[:1], 5)
    assert len(tdm.load_gt_log(gt)) == 4                                 # untouched by the refused call
    pairs.write_gt(gt, ps[:1], 5, force=True)
    assert list(tdm.load_gt_log(gt)) == ['1_4']


def test_box_prefilter_never_drops_a_pair_with_a_match():
    """random boxes of random small clouds under random poses: whenever brute force finds a match within the radius, boxes_within
    says True; and it does drop pairs that are far apart."""
    from buffer_amd import pairs, synth
    rng = np.random.default_rng(2)
    dropped = with_match = 0
    for trial in range(400):
        a = rng.uniform(-1, 1, (40, 3)) * rng.uniform(0.05, 1.0, 3)
        b = rng.uniform(-1, 1, (40, 3)) * rng.uniform(0.05, 1.0, 3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = synth.random_rotation(rng), rng.normal(size=3) * rng.choice([0.3, 1.0, 3.0])
        radius = float(rng.choice([0.02, 0.1, 0.4]))
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        box = lambda c: np.stack([c.min(0), c.max(0)]).astype(np.float64)
        keep = pairs.boxes_within(box(a32), box(b32), T, radius)
        matched = pairs_ref.pair_ref(b32, a32, T, radius)['matched']
        with_match += matched > 0
        dropped += not keep
        assert keep or matched == 0, (trial, matched)
    assert dropped > 20 and with_match > 20, (dropped, with_match)


def _cli_root(tmp_path, n=3):
    from buffer_amd import threedmatch as tdm
    root = str(tmp_path / 'data')
    for k in range(n):
        tdm.write_ply(os.path.join(root, 'test', '3DMatch', 'fragments', 'room', f'cloud_bin_{k}.ply'), np.zeros((4, 3), np.float32))
    return root


def _write_traj(path, n):
    with open(path, 'w') as f:
        for k in range(n):
            f.write(f'{k}\t{k}\t{n}\n')
            for row in np.eye(4):
                f.write('\t'.join(repr(float(x)) for x in row) + '\n')


def test_cli_errors(tmp_path, capsys):
    from buffer_amd import pairs
    root = _cli_root(tmp_path)
    with pytest.raises(SystemExit):                                  # no --poses and no cloud_bin_<k>.pose.npy
        pairs.main(['--root', root, '--scene', 'room'])
    assert 'pose.npy is missing' in capsys.readouterr().err
    with pytest.raises(SystemExit):                                  # a poses file that is not there
        pairs.main(['--root', root, '--scene', 'room', '--poses', str(tmp_path / 'none.log')])
    assert 'no such poses file' in capsys.readouterr().err
    _write_traj(str(tmp_path / 'two.log'), 2)
    with pytest.raises(SystemExit):                                  # 2 poses for 3 fragments
        pairs.main(['--root', root, '--scene', 'room', '--poses', str(tmp_path / 'two.log')])
    assert '2 poses for 3 fragments' in capsys.readouterr().err
    _write_traj(str(tmp_path / 'three.log'), 3)
    with pytest.raises(SystemExit):
        pairs.main(['--root', root, '--scene', 'room', '--poses', str(tmp_path / 'three.log'), '--dataset', '3DNoMatch'])
    assert 'unknown data set' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pairs.main(['--root', root, '--scene', 'nowhere', '--poses', str(tmp_path / 'three.log')])
    assert 'no cloud_bin_0.ply' in capsys.readouterr().err
    assert not os.path.exists(os.path.join(root, 'test', '3DMatch', 'gt_result'))


def test_header_lists_the_pair_statistics_entry_points():
    """the two new entry points are declared in the header and bound by the ctypes table (tests/test_host_cpu.py compares the whole
    header with the table)"""
    from buffer_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'buffer_hip.h')).read()
    for name in ('buf_pair_stats_ws_bytes', 'buf_pair_stats'):
        assert name + '(' in header and name in _lib.exported_symbols()


def test_bands():
    from buffer_amd import pairs
    assert [pairs.band_of(x) for x in (0.0, 0.0999, 0.1, 0.2999, 0.3, 0.5999, 0.6, 1.0)] == [0, 0, 1, 1, 2, 2, 3, 3]
