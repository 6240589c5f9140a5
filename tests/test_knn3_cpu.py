"""N14 / N15 without a device: the exported symbols, the pinned version, the host-side argument errors of the new functions, the
drivers' --denoise options and their misuse, and prepare_fragments' default."""
import inspect

import numpy as np
import pytest


def test_case_fixtures_are_what_they_say():
    import knn3_cases as kc                                      # (its import asserts the lattice's 117 tied rows and the face coordinates)
    import knn3_ref
    d2 = np.sort(knn3_ref.sqdist3(kc.lattice(), kc.lattice()), axis=1)
    assert int((d2[:, 7] == d2[:, 8]).sum()) == 117
    exact = [kc.face_f(kc.FACES_EXACT[0], q) for q in kc.FACES_EXACT[1]]
    below = [kc.face_f(kc.FACES_BELOW[0], q) for q in kc.FACES_BELOW[1]]
    assert exact == [1.0, 2.0, 3.0] and all(m - 2.0 ** -50 * (2 * m + 1) <= f < m for m, f in enumerate(below, 1))
    # in the face cases the nearest support of every foreign query lies in ANOTHER cell than the query (box from the origin, 4 cells)
    for c in kc.CASES:
        if c['name'] in ('faces_exact_foreign', 'faces_below_foreign'):
            edge = float(np.float32(c['radius'])) * 1.00001
            assert (c['supports'].min(0) == 0).all() and (np.floor(c['supports'].max(0).astype(np.float64) / edge) == 3).all()
            nbr, _ = knn3_ref.brute_force(c['queries'], c['supports'], c['q_lens'], c['s_lens'], 1)
            cq = np.floor(c['queries'].astype(np.float64) * (1.0 / edge))
            cs = np.floor(c['supports'][nbr[:, 0]].astype(np.float64) * (1.0 / edge))
            assert len(cq) == 27 and (cq != cs).any(1).all()


def test_symbols_and_version():
    from buffer_amd import _lib
    L = _lib.lib()
    for name in ('buf_grid_knn', 'buf_outlier_statistical', 'buf_outlier_statistical_ws_bytes'):
        assert name in _lib.exported_symbols() and hasattr(L, name)
    assert L.buf_version() == 670
    assert L.buf_outlier_statistical_ws_bytes(3) >= 16 and L.buf_outlier_statistical_ws_bytes(3) % 256 == 0


def test_c_abi_argument_errors_need_no_device():
    import ctypes as C
    from buffer_amd import _lib
    L = _lib.lib()
    lens = (C.c_int * 1)(0)
    null = C.c_void_p(0)
    assert L.buf_grid_knn(None, null, 0, lens, null, 8, null, null, null) == -1
    assert 'buf_grid_knn: null argument' in L.buf_last_error().decode()
    one = C.c_void_p(256)                                        # never dereferenced: every call below fails its argument checks
    for kw, msg in ((dict(n=-1), 'n=-1'), (dict(k=0), 'k=0'), (dict(nc=0), 'nc=0'), (dict(ratio=float('nan')), 'std_ratio is NaN'),
                    (dict(lens=null), 'null argument'), (dict(ws=null), 'null argument'), (dict(n=4, d2=null), 'null d2, mean_out or keep_out'),
                    (dict(ws_bytes=0), 'workspace 0 <')):
        a = dict(d2=one, n=0, k=4, lens=lens, nc=1, ratio=2.0, ws=one, ws_bytes=4096)
        a.update(kw)
        rc = L.buf_outlier_statistical(a['d2'], a['n'], a['k'], a['lens'], a['nc'], a['ratio'], one, one, one, one, a['ws'], a['ws_bytes'], null)
        assert rc in (-1, -3) and 'buf_outlier_statistical: ' + msg in L.buf_last_error().decode(), (kw, L.buf_last_error())


def test_host_side_argument_errors():
    from buffer_amd import ops, preprocess as pp
    with pytest.raises(ValueError, match='grid_knn: grid is not a CellGrid'):
        ops.grid_knn(None, None, [1], 3)
    for k in (0, 65, 2.5):
        with pytest.raises(ValueError, match=r'knn_search: k=.* \(1 <= k <= 64\)'):
            pp.knn_search(None, k)
        with pytest.raises(ValueError, match=r'estimate_normals_knn: knn='):
            pp.estimate_normals_knn(None, k)
        with pytest.raises(ValueError, match=r'remove_statistical_outlier: nb_neighbors='):
            pp.remove_statistical_outlier(None, k)
    for cell in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='knn_search: cell='):
            pp.knn_search(None, 3, cell=cell)
    for ratio in (0.0, -2.0, float('nan')):
        with pytest.raises(ValueError, match='remove_statistical_outlier: std_ratio='):
            pp.remove_statistical_outlier(None, 20, ratio)
    for nb in (-1, 1.5):
        with pytest.raises(ValueError, match='remove_radius_outlier: nb_points='):
            pp.remove_radius_outlier(None, nb, 0.1)
    for r in (0.0, -0.1, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='remove_radius_outlier: radius='):
            pp.remove_radius_outlier(None, 3, r)
    with pytest.raises(ValueError, match="denoise: method='median'"):
        pp.denoise_clouds(None, None, dict(method='median'))
    with pytest.raises(ValueError, match="needs a radius"):
        pp.denoise_clouds(None, None, dict(method='radius'))
    with pytest.raises(ValueError, match=r"unknown option\(s\) \['radius'\]"):
        pp.denoise_clouds(None, None, dict(method='statistical', radius=0.1))
    # a host array is no device tensor: the library has no CPU path
    from buffer_amd._lib import BufferHipError
    with pytest.raises(BufferHipError, match='expected a tensor in device memory'):
        pp.knn_search(np.zeros((4, 3), np.float32), 2)


def test_prepare_fragments_default_is_no_denoising():
    from buffer_amd import fpfh, preprocess as pp
    for fn in (pp.prepare_fragments, pp.prepare_fragment):
        assert inspect.signature(fn).parameters['denoise'].default is None
    assert inspect.signature(fpfh.FpfhRegistration.__init__).parameters['iss_resolution'].default == 'voxel'
    assert pp.prepare_fragments([], 0.02, 0.04, denoise=dict(method='statistical')) == []


def test_denoise_options_on_all_three_drivers(capsys):
    from buffer_amd import driver, eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r'])
        assert (a.denoise, a.denoise_neighbors, a.denoise_std_ratio, a.denoise_radius) == (None, None, None, None)
        assert driver.denoise_option(a) is None
        a, _ = mod.parse_args(['--root', 'r', '--denoise', 'statistical'])
        assert driver.denoise_option(a) == dict(method='statistical', nb_neighbors=20, std_ratio=2.0)
        a, _ = mod.parse_args(['--root', 'r', '--denoise', 'statistical', '--denoise-neighbors', '12', '--denoise-std-ratio', '1.5'])
        assert driver.denoise_option(a) == dict(method='statistical', nb_neighbors=12, std_ratio=1.5)
        a, _ = mod.parse_args(['--root', 'r', '--denoise', 'radius', '--denoise-radius', '0.1'])
        assert driver.denoise_option(a) == dict(method='radius', nb_points=16, radius=0.1)
        a, _ = mod.parse_args(['--root', 'r', '--denoise', 'radius', '--denoise-radius', '0.1', '--denoise-neighbors', '0'])
        assert driver.denoise_option(a) == dict(method='radius', nb_points=0, radius=0.1)
        for argv, msg in ((['--denoise', 'median'], 'invalid choice'),
                          (['--denoise-neighbors', '5'], '--denoise-neighbors 5 is a setting of --denoise: it needs --denoise'),
                          (['--denoise-std-ratio', '1.0'], '--denoise-std-ratio 1.0 is a setting of --denoise'),
                          (['--denoise-radius', '0.1'], '--denoise-radius 0.1 is a setting of --denoise'),
                          (['--denoise', 'radius'], '--denoise radius needs --denoise-radius'),
                          (['--denoise', 'radius', '--denoise-radius', '0'], '--denoise-radius 0.0: must be finite and > 0'),
                          (['--denoise', 'radius', '--denoise-radius', '0.1', '--denoise-std-ratio', '2'], 'is the ratio of --denoise statistical'),
                          (['--denoise', 'radius', '--denoise-radius', '0.1', '--denoise-neighbors', '-1'], '--denoise-neighbors -1: must be >= 0'),
                          (['--denoise', 'statistical', '--denoise-radius', '0.1'], 'is the ball of --denoise radius'),
                          (['--denoise', 'statistical', '--denoise-neighbors', '0'], '--denoise-neighbors 0: must be in 1..64'),
                          (['--denoise', 'statistical', '--denoise-neighbors', '65'], '--denoise-neighbors 65: must be in 1..64'),
                          (['--denoise', 'statistical', '--denoise-std-ratio', '0'], '--denoise-std-ratio 0.0: must be finite and > 0')):
            with pytest.raises(SystemExit):
                mod.parse_args(['--root', 'r'] + argv)
            assert msg in capsys.readouterr().err, (mod.__name__, argv)


class _Consts:
    downsample, voxel_size_0, max_num_pts = 0.02, 0.04, 30000


def test_pack_pairs_hands_the_option_on(monkeypatch):
    from buffer_amd import driver, preprocess as pp
    seen = []

    def fake(raws, downsample, voxel_size_0, max_num_pts=30000, seeds=None, with_normals=True, denoise=None):
        seen.append(denoise)
        return [dict(fds_pts=i, sds_pts=i, **({} if denoise is None else {'denoise_removed': 0.25})) for i, _ in enumerate(raws)]

    monkeypatch.setattr(pp, 'prepare_fragments', fake)
    c = _Consts()
    driver.pack_pairs([0, 1], [0, 1], [{}], c)
    driver.pack_pair([0, 1], [0, 1], {}, c)
    assert seen == [None, None, None]
    c.denoise, c.denoise_log = dict(method='statistical'), []
    driver.pack_pairs([0, 1], [0, 1], [{}], c)
    driver.pack_pair([0, 1], [0, 1], {}, c)
    assert seen[3:] == [c.denoise] * 3 and c.denoise_log == [0.25] * 4
