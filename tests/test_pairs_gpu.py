"""Device pair statistics (csrc/pairstats.hip, buffer_amd/pairs.py) against the numpy restatement of tests/pairs_ref.py: matches and
nearest rows EQUAL, fp64 sums within the summation bound 2 (n - 1) 2^-53 sum|term|; batch independence bit for bit; the existing ICP
kernel's evaluation of the same transform; the scene tool and the 3DMatch driver end to end on what it writes."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import pairs_ref

pytestmark = pytest.mark.gpu


# ---- data ----------------------------------------------------------------------------------------------------------------------
def _room_views(seed, offsets=(0.0, 0.45, 0.9), size=(2.4, 1.9, 1.7), width=1.5, n_raw=260_000):
    """slabs of one synth.make_scene room along x (the three-view room of tests/test_threedmatch_driver.py::_mini_dataset for the
    default arguments) -> (raw fragments f32[n,3], each in its own frame, poses world -> fragment)"""
    from buffer_amd import synth
    rng = np.random.default_rng(seed)
    rects = synth.make_scene(rng, size, 6)
    frags, poses = [], []
    for lo in offsets:
        pts, _ = synth.sample_scene(rng, rects, n_raw)
        pts = pts[(pts[:, 0] >= lo) & (pts[:, 0] <= lo + width)]
        sensor = np.array([lo + 0.5 * width, 0.55 * size[1], 0.5 * size[2]])
        R = synth.random_rotation(rng, 0.6)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, -R @ sensor
        poses.append(T)
        frags.append((pts @ R.T + T[:3, 3]).astype(np.float32))
    return frags, poses


@pytest.fixture(scope="module")
def room():
    """the three views voxelised at 0.025 m on the host (f32), with T[(a, b)] mapping view a into view b"""
    from buffer_amd import synth
    frags, poses = _room_views(5)
    down = [synth.voxel_down_sample(f.astype(np.float64), 0.025).astype(np.float32) for f in frags]
    T = {(a, b): poses[b] @ np.linalg.inv(poses[a]) for a in range(3) for b in range(3)}
    return down, T


def _run(dev, clouds, prs, Ts, radius, **kw):
    from buffer_amd import pairs
    cl = [torch.from_numpy(np.ascontiguousarray(c, np.float32).reshape(-1, 3)).to(dev) for c in clouds]
    return pairs.pair_statistics(cl, prs, np.asarray(Ts, np.float64).reshape(-1, 4, 4), radius, correspondences=True, **kw)


def _check(dev, clouds, prs, Ts, radius, **kw):
    """device == restatement for every pair -> (device result, [restatement per pair])"""
    st = _run(dev, clouds, prs, Ts, radius, **kw)
    refs = []
    for k, (a, b) in enumerate(prs):
        ref = pairs_ref.pair_ref(clouds[a], clouds[b], Ts[k], radius)
        refs.append(ref)
        print(f'pair {k} ({a}->{b}): n_src={ref["n_src"]} matched device={int(st["matched"][k])} restated={ref["matched"]}')
        assert int(st['n_src'][k]) == ref['n_src']
        assert int(st['matched'][k]) == ref['matched']
        assert np.array_equal(st['nn'][k], ref['nn'])
        pairs_ref.check_moments(np.concatenate([[st['sum_d2'][k]], st['sum_u'][k], st['sum_uu'][k]]), ref)
        assert st['overlap'][k] == (ref['matched'] / ref['n_src'] if ref['n_src'] else 0.0)
        assert st['inlier_rmse'][k] == (np.sqrt(st['sum_d2'][k] / ref['matched']) if ref['matched'] else 0.0)
    return st, refs


# ---- 6. against the restatement ---------------------------------------------------------------------------------------------------
def test_threedmatch_shape_fragments(dev, room):
    down, T = room
    prs = [(1, 0), (2, 0), (2, 1), (0, 2)]
    st, _ = _check(dev, down, prs, [T[p] for p in prs], 0.0375)
    assert np.all(st['overlap'] > 0.2) and np.all(st['overlap'] < 0.9)            # (partial overlaps: the case is not degenerate)


def test_kitti_shape_scans(dev):
    from buffer_amd import synth
    s = synth.make_kitti_pair(3)
    clouds = [s['src_fds_pts'].astype(np.float32), s['tgt_fds_pts'].astype(np.float32)]
    st, _ = _check(dev, clouds, [(0, 1), (1, 0)], [s['relt_pose'], np.linalg.inv(s['relt_pose'])], 0.075)
    assert np.all(st['matched'] > 0)


def test_self_pair_under_the_identity(dev, room):
    c = room[0][0]
    assert np.unique(c, axis=0).shape[0] == c.shape[0]                            # no duplicate rows
    st, _ = _check(dev, [c], [(0, 0)], [np.eye(4)], 0.0375)
    assert st['overlap'][0] == 1.0 and st['inlier_rmse'][0] == 0.0 and np.array_equal(st['nn'][0], np.arange(c.shape[0]))


def test_disjoint_empty_and_no_pairs(dev, room):
    from buffer_amd import pairs
    c = room[0][0][:5000]
    far = c + np.float32(100.0)
    empty = np.zeros((0, 3), np.float32)
    st, _ = _check(dev, [c, far, empty], [(0, 1), (2, 0), (0, 2), (2, 2)], [np.eye(4)] * 4, 0.0375)
    assert not st['matched'].any() and not st['sum_uu'].any() and not st['overlap'].any() and not st['inlier_rmse'].any()
    assert st['n_src'].tolist() == [5000, 0, 5000, 0]
    none = _run(dev, [c], [], np.zeros((0, 4, 4)), 0.0375)
    assert none['matched'].shape == (0,) and none['sum_u'].shape == (0, 3) and len(none['nn']) == 0
    sym = pairs.pair_statistics([torch.from_numpy(c).to(dev)], [], np.zeros((0, 4, 4)), 0.0375, symmetric=True)
    assert sym['matched'].shape == (0,) and sym['reverse']['matched'].shape == (0,)


def test_non_finite_source_rows_are_skipped_but_counted(dev, room):
    down, T = room
    src = down[1][:6000].copy()
    src[[0, 17, 255, 256, 5999]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, 1, 1]]
    st, refs = _check(dev, [src, down[0]], [(0, 1)], [T[(1, 0)]], 0.0375)
    assert st['n_src'][0] == 6000 and np.all(st['nn'][0][[0, 17, 255, 256, 5999]] == -1) and 0 < st['matched'][0] <= 5995
    huge = np.eye(4)
    huge[0, 3] = 1e300                                                            # finite rows whose fp32 search point is not
    st, _ = _check(dev, [down[1][:300], down[0]], [(0, 1)], [huge], 0.0375)
    assert st['matched'][0] == 0


def test_duplicate_targets_tie_to_the_smaller_row(dev):
    rng = np.random.default_rng(0)
    base = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    tgt = np.concatenate([base, base[::-1], base])                                # every point three times
    src = base + rng.normal(scale=0.004, size=base.shape).astype(np.float32)
    st, _ = _check(dev, [src, tgt], [(0, 1)], [np.eye(4)], 0.05)
    assert st['matched'][0] == 500 and np.all(st['nn'][0] < 500)
    first = {}
    for r, p in enumerate(map(bytes, tgt)):
        first.setdefault(p, r)
    assert all(first[bytes(tgt[j])] == j for j in st['nn'][0])


def test_distance_exactly_r_is_not_a_match(dev):
    r = 0.25                                                                      # r, r*r and every coordinate below are exact in fp32
    src = np.array([[0, 0, 0], [10, 0, 0], [0, 20, 0], [0, 0, -30]], np.float32)
    tgt = np.array([[0.25, 0, 0], [10.25 - 2.0 ** -20, 0, 0], [0, 20.25, 0], [0, 0, -30.25 + 2.0 ** -19]], np.float32)
    assert tgt[1, 0] < 10.25 and tgt[3, 2] > -30.25
    st, _ = _check(dev, [src, tgt], [(0, 1)], [np.eye(4)], r)
    assert st['nn'][0].tolist() == [-1, 1, -1, 3]


def test_coarsened_grid_and_split_calls_change_nothing(dev, room):
    """a table share far smaller than the box (the cell edge coarsens by 1.25 until it fits), a radius that makes the grid one cell,
    and a table budget that splits the job into several calls: the same bits as the default call"""
    from buffer_amd import ops, pairs
    down, T = room
    prs = [(1, 0), (2, 0), (2, 1), (0, 1)]
    Ts = np.array([T[p] for p in prs])
    want = _run(dev, down, prs, Ts, 0.0375)
    pts = torch.from_numpy(np.concatenate(down)).to(dev)
    m, mo, nn = ops.pair_stats(pts, [c.shape[0] for c in down], [p[0] for p in prs], [p[1] for p in prs], torch.from_numpy(Ts).to(dev),
                               0.0375, correspondences=True, cells_per_elem=512)
    assert np.array_equal(m.cpu().numpy(), want['matched'])
    assert np.array_equal(mo.cpu().numpy(), np.concatenate([want['sum_d2'][:, None], want['sum_u'], want['sum_uu']], 1))
    assert np.array_equal(nn.cpu().numpy(), np.concatenate(list(want['nn'])))
    split = _run(dev, down, prs, Ts, 0.0375, table_cells=1 << 10)                 # at most two clouds per call, coarsened as well
    for k in ('matched', 'sum_d2', 'sum_u', 'sum_uu'):
        assert np.array_equal(split[k], want[k]), k
    assert all(np.array_equal(a, b) for a, b in zip(split['nn'], want['nn']))
    small = [c[:3000] for c in down]
    _check(dev, small, prs, Ts, 5.0)                                              # radius > the clouds: one cell, every row a candidate


def test_rejected_arguments(dev, room):
    from buffer_amd import _lib, ops, pairs
    c = torch.from_numpy(room[0][0][:100]).to(dev)
    eye = torch.eye(4, dtype=torch.float64, device=dev)[None]
    for bad in ([1], [-1]):
        with pytest.raises(_lib.BufferHipError, match='outside'):
            ops.pair_stats(c, [100], [0], bad, eye, 0.05)
    for r in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(_lib.BufferHipError, match='radius'):
            ops.pair_stats(c, [100], [0], [0], eye, r)
    with pytest.raises(_lib.BufferHipError):
        ops.pair_stats(c.cpu(), [100], [0], [0], eye, 0.05)
    with pytest.raises(_lib.BufferHipError):
        pairs.pair_statistics([c.cpu()], [(0, 0)], np.eye(4)[None], 0.05)
    with pytest.raises(ValueError):
        pairs.pair_statistics([c], [(0, 1)], np.eye(4)[None], 0.05)


# ---- 7. batch independence ----------------------------------------------------------------------------------------------------------
def test_batch_independence_bit_for_bit(dev):
    from buffer_amd import synth
    frags, poses = _room_views(9, offsets=(0.0, 0.2, 0.4, 0.6, 0.8, 0.9), n_raw=60_000)
    clouds = [synth.voxel_down_sample(f.astype(np.float64), 0.04).astype(np.float32) for f in frags]
    rng = np.random.default_rng(1)
    prs, Ts = [], []
    for k in range(40):
        a, b = (int(x) for x in rng.integers(0, 6, 2))
        dT = np.eye(4)
        dT[:3, :3], dT[:3, 3] = synth.random_rotation(rng, 0.02), rng.normal(scale=0.01, size=3)
        prs.append((a, b))
        Ts.append(dT @ poses[b] @ np.linalg.inv(poses[a]))
    keys = ('matched', 'sum_d2', 'sum_u', 'sum_uu')
    batch = _run(dev, clouds, prs, Ts, 0.06)
    again = _run(dev, clouds, prs, Ts, 0.06)
    rev = _run(dev, clouds, prs[::-1], Ts[::-1], 0.06)
    assert batch['matched'].sum() > 1000
    for k in range(40):
        alone = _run(dev, [clouds[prs[k][0]], clouds[prs[k][1]]], [(0, 1)], [Ts[k]], 0.06)
        for other, j in ((again, k), (rev, 39 - k), (alone, 0)):
            for key in keys:
                assert np.array_equal(batch[key][k], other[key][j]), (k, key)
            assert np.array_equal(batch['nn'][k], other['nn'][j]), k


# ---- 8. against the ICP kernel's evaluation of the same transform -------------------------------------------------------------------
def test_equals_icp_batched_without_iterations(dev, room):
    from buffer_amd import icp, synth
    down, T = room
    rng = np.random.default_rng(4)
    prs = [(1, 0), (2, 0), (2, 1), (0, 1), (0, 0)]
    Ts = []
    for p in prs:
        dT = np.eye(4)
        dT[:3, :3], dT[:3, 3] = synth.random_rotation(rng, 0.01), rng.normal(scale=0.005, size=3)
        Ts.append(dT @ T[p])
    st, refs = _check(dev, down, prs, Ts, 0.0375)
    cl = [torch.from_numpy(c).to(dev) for c in down]
    res = icp.icp_batched([cl[a] for a, _ in prs], [cl[b] for _, b in prs], 0.0375, inits=Ts, max_iteration=0, return_correspondences=True)
    for k, r in enumerate(res):
        assert r['iterations'] == 0 and np.array_equal(r['T'], Ts[k])
        nn = st['nn'][k]
        hit = np.flatnonzero(nn >= 0)
        assert np.array_equal(r['correspondences'], np.stack([hit, nn[hit]], 1))
        assert r['fitness'] == st['matched'][k] / st['n_src'][k]
        m = float(st['matched'][k])
        bound = pairs_ref.sum_bound(refs[k]['terms'][:, :1])[0] + 8 * pairs_ref.U * st['sum_d2'][k]     # (+ sqrt, division, squaring)
        print(f'pair {k}: rmse icp={r["inlier_rmse"]!r} pair_stats={st["inlier_rmse"][k]!r}')
        assert abs(r['inlier_rmse'] ** 2 * m - st['sum_d2'][k]) <= bound


# ---- 9. symmetric ---------------------------------------------------------------------------------------------------------------------
def test_symmetric_equals_two_directional_calls(dev, room):
    down, T = room
    prs = [(1, 0), (2, 0), (2, 1)]
    Ts = np.array([T[p] for p in prs])
    sym = _run(dev, down, prs, Ts, 0.0375, symmetric=True)
    fwd = _run(dev, down, prs, Ts, 0.0375)
    bwd = _run(dev, down, [(b, a) for a, b in prs], np.linalg.inv(Ts), 0.0375)
    for key in ('n_src', 'matched', 'overlap', 'inlier_rmse', 'sum_d2', 'sum_u', 'sum_uu'):
        assert np.array_equal(sym[key], fwd[key]) and np.array_equal(sym['reverse'][key], bwd[key]), key
    for k in range(3):
        assert np.array_equal(sym['nn'][k], fwd['nn'][k]) and np.array_equal(sym['reverse']['nn'][k], bwd['nn'][k])


# ---- 10. scene tool + driver, end to end ------------------------------------------------------------------------------------------------
# slabs of width 1.5 m at 0 / 0.205 / 1.179 / 1.669 / 1.883 m, picked on the host (KD-tree overlaps at voxel 0.02 m, radius 0.03 m: 0.80, 0.55,
# 0.38, 0.79 in the 3DMatch band, 0.16, 0.26 in the 3DLoMatch band, the rest below 0.03) so that no pair lies within 0.04 of a band edge
# 0.1 / 0.3 / 0.6; the test checks 0.02 on the restated figures before using a pair.  Ordered so that three of the four 3DMatch-band pairs
# are non-consecutive fragments, the only ones the Registration Recall counts.
OFFSETS = (0.0, 1.179, 0.205, 1.883, 1.669)


def _read_info(path):
    lines = open(path).read().splitlines()
    return {tuple(int(x) for x in lines[k].split()[:2]): np.array([[float(x) for x in ln.split()] for ln in lines[k + 1:k + 7]])
            for k in range(0, len(lines), 7)}


def test_scene_pairs_write_gt_and_driver_end_to_end(tmp_path, dev, capsys):
    from buffer_amd import evaluate, pairs, synth, threedmatch as tdm
    from buffer_amd.config import THREEDMATCH
    frags, poses = _room_views(21, offsets=OFFSETS, size=(3.5, 1.9, 1.7))
    n = len(frags)
    W = [np.linalg.inv(P) for P in poses]                                         # fragment -> world
    root = str(tmp_path / 'data')
    first = os.path.join(root, 'test', '3DMatch', 'fragments', tdm.SCENES[0])
    for k, f in enumerate(frags):
        tdm.write_ply(os.path.join(first, f'cloud_bin_{k}.ply'), f)
    for scene in tdm.SCENES[1:]:                                                  # the driver reads all eight scenes: the same room eight times
        shutil.copytree(first, os.path.join(root, 'test', '3DMatch', 'fragments', scene))
    traj = str(tmp_path / 'poses.log')
    with open(traj, 'w') as f:
        for k in range(n):
            f.write(f'{k}\t{k}\t{n}\n')
            for row in W[k]:
                f.write('\t'.join(repr(float(x)) for x in row) + '\n')

    # the restatement: the tool's own voxelisation (an existing, tested operator), then tests/pairs_ref.py in both directions
    voxel, radius = THREEDMATCH.downsample, 1.5 * THREEDMATCH.downsample
    down = [c.cpu().numpy() for c in pairs.downsample_clouds(frags, voxel, dev)]
    want = {}
    for i in range(n):
        for j in range(i + 1, n):
            Tij = np.linalg.inv(W[i]) @ W[j]
            fj = pairs_ref.pair_ref(down[j], down[i], Tij, radius)                # fragment j into fragment i
            fi = pairs_ref.pair_ref(down[i], down[j], np.linalg.inv(Tij), radius)  # fragment i into fragment j: matched points of j
            ov = min(fj['matched'] / fj['n_src'], fi['matched'] / fi['n_src'])
            print(f'pair ({i}, {j}): restated overlaps {fi["matched"] / fi["n_src"]:.4f} / {fj["matched"] / fj["n_src"]:.4f}')
            assert all(abs(ov - e) > 0.02 for e in (0.1, 0.3, 0.6)), (i, j, ov)      # no pair near a band edge
            want[(i, j)] = dict(T=Tij, overlap=ov, ref=fi)
    bands = {'3DMatch': (0.3, 1.01), '3DLoMatch': (0.1, 0.3)}
    expect = {d: sorted(p for p, w in want.items() if lo <= w['overlap'] < hi) for d, (lo, hi) in bands.items()}
    assert len(expect['3DMatch']) >= 4 and len(expect['3DLoMatch']) >= 2, expect

    for dataset in ('3DMatch', '3DLoMatch'):
        for scene in tdm.SCENES:
            pairs.main(['--root', root, '--scene', scene, '--poses', traj, '--dataset', dataset])
            line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
            assert line['pairs'] == len(expect[dataset]) and line['fragments'] == n and sum(line['overlap_histogram'].values()) == line['pairs']
        gt_dir = os.path.join(root, 'test', '3DMatch', 'gt_result', tdm.SCENES[0]) if dataset == '3DMatch' else os.path.join(root, 'test', dataset, tdm.SCENES[0])
        log = tdm.load_gt_log(gt_dir)
        assert list(log) == [f'{i}_{j}' for i, j in expect[dataset]]              # exactly the pairs of the band, ascending
        info = _read_info(os.path.join(gt_dir, 'gt.info'))
        meta = {(p['i'], p['j']): p for p in json.load(open(os.path.join(gt_dir, 'gt_overlap.json')))['pairs']}
        for p in expect[dataset]:
            w = want[p]
            assert np.array_equal(log['%d_%d' % p], w['T'])
            assert min(meta[p]['overlap_i'], meta[p]['overlap_j']) == w['overlap'] and meta[p]['matched_i'] == w['ref']['matched']
            u = w['ref']['matched_pts']
            ref_info = synth.information_matrix(u)
            # the bound of the CPU test, entry by entry over the terms of J^T J; repr(float) keeps fp64 exactly, so the text adds nothing
            bound = pairs_ref.info_bound(u)
            assert info[p][0, 0] == u.shape[0] and np.all(np.abs(info[p] - ref_info) <= bound), np.abs(info[p] - ref_info).max()
            # what the matrix means to the evaluator: for a small residual transform E acting on fragment j's frame,
            # transformation_error(E, info) = er^T info er / info[0,0] is the mean squared displacement of the matched points.  The
            # matrix linearises the rotation (t + 2 q x u against t + (R - I) u): at 0.01 rad and |u| < 4 m the displacements differ
            # by < theta^2 |u| / 2 = 2e-4 m against ~0.03 m, under 1 % of the displacement, so 3 % of its square covers it.
            E = np.eye(4)
            E[:3, :3], E[:3, 3] = synth.random_rotation(np.random.default_rng(p[0] * 7 + p[1]), 0.01), [0.02, -0.01, 0.015]
            msd = float((((u @ E[:3, :3].T + E[:3, 3]) - u) ** 2).sum(1).mean())
            assert abs(evaluate.transformation_error(E, info[p]) - msd) <= 0.03 * msd
        with pytest.raises(SystemExit):                                           # a second run refuses to replace gt.log
            pairs.main(['--root', root, '--scene', tdm.SCENES[0], '--poses', traj, '--dataset', dataset])
        capsys.readouterr()

    log_root = str(tmp_path / 'logs')
    common = ['--root', root, '--dataset', '3DMatch', '--log-root', log_root, '--batch', '8', '--stage-metrics']
    tdm.main(common + ['--log-name', 'plain.log'])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    plain_rows = json.load(open(os.path.join(log_root, 'stage_metrics.json')))
    tdm.main(common + ['--log-name', 'bands.log', '--by-overlap', '--limits', ','.join(str(x) for x in plain['limits'])])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    rows = json.load(open(os.path.join(log_root, 'stage_metrics.json')))
    print('driver:', {k: out[k] for k in ('pairs', 'dgr_recall', 'registration_recall')}, out['by_overlap'])
    # 12. without the option nothing new appears; with it exactly `by_overlap` and the per-pair `overlap`
    assert 'by_overlap' not in plain and set(out) == set(plain) | {'by_overlap'}
    assert all(set(r) == {'id', 'counts'} for r in plain_rows['pairs']) and all(set(r) == {'id', 'counts', 'overlap'} for r in rows['pairs'])
    assert out['pairs'] == 8 * len(expect['3DMatch'])
    rr, _ = evaluate.registration_recall(os.path.join(root, 'test', '3DMatch', 'gt_result'), log_root, 'bands.log')
    assert out['registration_recall'] == rr                                       # computed with the written gt.info matrices
    assert 0.0 < rr <= 1.0, rr          # (0, 2) shares 80 % of its surface: the existing mini data set asks for RR >= 0.85 at 70 % / 40 %
    assert out['dgr_recall'] >= 0.5, out                                          # (the driver did register the pairs it was given)
    assert list(out['by_overlap']) == ['[0.0, 0.1)', '[0.1, 0.3)', '[0.3, 0.6)', '[0.6, 1.0]']
    per_band = np.bincount([pairs.band_of(want[p]['overlap']) for p in expect['3DMatch']], minlength=4) * 8
    assert [out['by_overlap'][k]['pairs'] for k in out['by_overlap']] == per_band.tolist()
    assert all('stage' in v and 'dgr_recall' in v for v in out['by_overlap'].values())
    ds = tdm.ThreeDMatchTestSet(root, '3DMatch')
    for r, (s, t) in zip(rows['pairs'], ds.files):
        p = (int(s.split('_')[-1]), int(t.split('_')[-1]))
        assert r['overlap'] == want[p]['overlap'], (p, r['overlap'])
    # the 3DLoMatch files through the data set class and the driver; --by-overlap alone (no stage rows to split)
    lo_ds = tdm.ThreeDMatchTestSet(root, '3DLoMatch')
    assert len(lo_ds) == 8 * len(expect['3DLoMatch'])
    assert [(int(s.split('_')[-1]), int(t.split('_')[-1])) for s, t in lo_ds.files[:len(expect['3DLoMatch'])]] == expect['3DLoMatch']
    tdm.main(['--root', root, '--dataset', '3DLoMatch', '--log-root', str(tmp_path / 'lo'), '--log-name', 'lo.log', '--batch', '8', '--by-overlap',
              '--limits', ','.join(str(x) for x in plain['limits'])])
    lo = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert lo['pairs'] == len(lo_ds) and 'stage' not in lo and not os.path.exists(str(tmp_path / 'lo' / 'stage_metrics.json'))
    assert [v['pairs'] for v in lo['by_overlap'].values()] == [0, len(lo_ds), 0, 0] and all(set(v) == {'pairs', 'dgr_recall'} for v in lo['by_overlap'].values())


# ---- 11. the open3d stand-in ---------------------------------------------------------------------------------------------------------
def test_open3d_standin_calls(dev, room):
    import buffer_amd.shims as shims
    from buffer_amd import pairs
    shims.install()
    import open3d as o3d
    down, T = room
    src, tgt = o3d.geometry.PointCloud(), o3d.geometry.PointCloud()
    src.points, tgt.points = o3d.utility.Vector3dVector(down[1]), o3d.utility.Vector3dVector(down[0])
    reg = o3d.pipelines.registration
    st = _run(dev, [down[1], down[0]], [(0, 1)], [T[(1, 0)]], 0.0375)
    r = reg.evaluate_registration(src, tgt, 0.0375, T[(1, 0)])
    hit = np.flatnonzero(st['nn'][0] >= 0)
    assert r.fitness == st['overlap'][0] and r.inlier_rmse == st['inlier_rmse'][0] and 0.5 < r.fitness < 0.9
    assert np.array_equal(np.asarray(r.correspondence_set), np.stack([hit, st['nn'][0][hit]], 1)) and np.array_equal(r.transformation, T[(1, 0)])
    info = reg.get_information_matrix_from_point_clouds(src, tgt, 0.0375, T[(1, 0)])
    assert info.dtype == np.float64 and np.array_equal(info, pairs.information_matrix(st['matched'][0], st['sum_u'][0], st['sum_uu'][0], 'open3d'))
    ident = reg.evaluate_registration(tgt, tgt, 0.0375)                           # transformation defaults to the identity
    assert ident.fitness == 1.0 and ident.inlier_rmse == 0.0


# ---- 12. the other two drivers: --by-overlap adds one key and nothing else --------------------------------------------------------------
def test_eth_driver_by_overlap_keys(tmp_path, dev, capsys):
    from buffer_amd import eth, pairs, synth
    root = str(tmp_path / 'eth')
    scenes = ('gazebo_summer', 'wood_autmn')
    synth.make_eth_root(root, scenes=scenes, stations=3, n_raw=60_000)
    common = ['--root', root, '--scenes', *scenes, '--batch', '3', '--stage-metrics']
    eth.main(common + ['--log-root', str(tmp_path / 'a')])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    eth.main(common + ['--log-root', str(tmp_path / 'b'), '--by-overlap', '--limits', ','.join(str(x) for x in plain['limits'])])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(out) == set(plain) | {'by_overlap'} and sum(v['pairs'] for v in out['by_overlap'].values()) == out['pairs'] == 6
    a = json.load(open(tmp_path / 'a' / 'stage_metrics.json'))
    b = json.load(open(tmp_path / 'b' / 'stage_metrics.json'))
    assert set(a) == set(b) and all(set(r) == {'id', 'counts'} for r in a['pairs']) and all(set(r) == {'id', 'counts', 'overlap'} for r in b['pairs'])
    ds = eth.ETHTestSet(root, scenes)
    ov = pairs.dataset_overlaps(ds, range(len(ds)), dev)
    assert [r['overlap'] for r in b['pairs']] == ov.tolist()
    i = 1                                                                          # one pair against the restatement (voxel = downsample)
    down = [c.cpu().numpy() for c in pairs.downsample_clouds(ds.raw_pair(i), ds.downsample, dev)]
    G = ds.meta(i)['relt_pose']
    f = pairs_ref.pair_ref(down[0], down[1], G, 1.5 * ds.downsample)
    g = pairs_ref.pair_ref(down[1], down[0], np.linalg.inv(G), 1.5 * ds.downsample)
    assert ov[i] == min(f['matched'] / f['n_src'], g['matched'] / g['n_src'])


def test_kitti_driver_by_overlap_keys(tmp_path, dev, capsys):
    from buffer_amd import kitti
    from test_kitti_driver import _mini_sequence
    root = str(tmp_path / 'kitti')
    for drive in kitti.TEST_DRIVES:
        _mini_sequence(root, drive=drive, frames=26, seed=drive)
    common = ['--root', root, '--batch', '2', '--allow-odometry-gt', '--stage-metrics']
    kitti.main(common + ['--log-root', str(tmp_path / 'a')])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    kitti.main(common + ['--log-root', str(tmp_path / 'b'), '--by-overlap', '--limits', ','.join(str(x) for x in plain['limits'])])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(out) == set(plain) | {'by_overlap'} and sum(v['pairs'] for v in out['by_overlap'].values()) == out['pairs'] > 0
    a = json.load(open(tmp_path / 'a' / 'stage_metrics.json'))
    b = json.load(open(tmp_path / 'b' / 'stage_metrics.json'))
    assert set(a) == set(b) and all(set(r) == {'id', 'counts'} for r in a['pairs']) and all(set(r) == {'id', 'counts', 'overlap'} for r in b['pairs'])
    assert all(0.0 < r['overlap'] <= 1.0 for r in b['pairs'])                      # scans 10 m apart on one street do overlap


# ---- the grid's bounding box skips non-finite coordinates: pinned through the operators that shared it before ----------------------------
def test_inf_and_nan_support_rows_match_nothing_in_radius_search_and_icp(dev, room):
    """A support / target row with an inf or NaN coordinate takes no part in the grid's box and is never a neighbour: the radius search
    and the ICP give what they give with those rows moved far away (finite), where the grid was always well defined."""
    from buffer_amd import icp, ops
    down, T = room
    bad_rows = [3, 500, 1999]
    sup = down[0][:2000].copy()
    far = sup.copy()
    sup[bad_rows] = [[np.inf, 0, 0], [0.5, -np.inf, np.nan], [np.nan, 1, 1]]
    far[bad_rows] = [[900.0, 0, 0], [0.5, -900.0, 900.0], [900.0, 1, 1]]
    q = down[0][2000:2600]
    a = ops.radius_neighbors(torch.from_numpy(q).to(dev), torch.from_numpy(sup).to(dev), [600], [2000], 0.08).cpu().numpy()
    b = ops.radius_neighbors(torch.from_numpy(q).to(dev), torch.from_numpy(far).to(dev), [600], [2000], 0.08).cpu().numpy()
    assert a.shape == b.shape and np.array_equal(a, b) and (a < 2000).sum() > 600 and not np.isin(a, bad_rows).any()
    src = torch.from_numpy(down[1][:4000]).to(dev)
    tg, tf = down[0].copy(), down[0].copy()
    tg[bad_rows], tf[bad_rows] = sup[bad_rows], far[bad_rows]
    ra = icp.icp_batched([src], [torch.from_numpy(tg).to(dev)], 0.0375, inits=[T[(1, 0)]], max_iteration=5, return_correspondences=True)[0]
    rb = icp.icp_batched([src], [torch.from_numpy(tf).to(dev)], 0.0375, inits=[T[(1, 0)]], max_iteration=5, return_correspondences=True)[0]
    assert np.array_equal(ra['T'], rb['T']) and ra['fitness'] == rb['fitness'] > 0.0 and ra['correspondences'].shape[0] > 500 and ra['inlier_rmse'] == rb['inlier_rmse']
    assert np.array_equal(ra['correspondences'], rb['correspondences']) and not np.isin(ra['correspondences'][:, 1], bad_rows).any()
