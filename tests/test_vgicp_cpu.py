"""Voxelized Generalized ICP, the parts that need no device: the float64 restatement (tests/vgicp_ref.py) pinned on its scene together
with the margin conditions of everything tests/test_vgicp_gpu.py compares exactly, a hand-computed voxel map, the Python argument
checks, the driver flags and the size functions of the C ABI."""
import math

import numpy as np
import pytest

import gicp_ref
import vgicp_ref

SIZES = [(0, 1800), (1, 1500), (255, 1700), (256, 1800), (257, 1234), (900, 1800)]      # tests/test_gicp_gpu.py's sub-clouds


@pytest.fixture(scope="module")
def vmap():
    sc = vgicp_ref.scene()
    return vgicp_ref.build_map(sc['tgt'], sc['tgt_normals'], vgicp_ref.VOXEL)


@pytest.fixture(scope="module")
def runs(vmap):
    """the restatement on its scene from the identity, 50 updates at most, at 1 / 7 / 27 neighbours, each with its trace"""
    sc = vgicp_ref.scene()
    out = {}
    for nb in (1, 7, 27):
        tr = []
        out[nb] = (vgicp_ref.vgicp(sc['src'], vmap, nb, sc['src_normals'], None, 50, trace=tr), tr)
    return out


def test_scene_is_the_shifted_one():
    sc, base = vgicp_ref.scene(), gicp_ref.scene()
    assert sc['src'].dtype == np.float32 and np.array_equal(sc['tgt'], base['tgt'] + np.float32(0.1))
    on = sc['src'].astype(np.float64) @ sc['T'][:3, :3].T + sc['T'][:3, 3] - float(np.float32(0.1))
    assert np.abs(on).min(1).max() < 6 * gicp_ref.SIGMA + 1e-6                       # the planted pose still puts the source on the walls


@pytest.mark.parametrize("nb", [1, 7, 27])
def test_restatement_reaches_the_planted_pose(runs, nb):
    """Measured with this file: 1 neighbour 0.0359 deg / 0.53 mm in 4 updates, 7: 0.0277 deg / 0.48 mm in 5, 27: 0.0289 deg / 0.57 mm
    in 5.  The bound is the one tests/test_gicp_cpu.py puts on Generalized ICP."""
    r, _ = runs[nb]
    rot, tr = gicp_ref.pose_error(r['T'], vgicp_ref.scene()['T'])
    print(f'voxelized, {nb} neighbours: {rot:.4f} deg {tr * 1e3:.3f} mm in {r["iterations"]}, fitness {r["fitness"]}, rmse {r["inlier_rmse"]:.4f}')
    assert 0 < r['iterations'] < 50 and r['fitness'] == 1.0 and r['solvable']
    assert rot < 0.051 and tr < 0.92e-3


@pytest.mark.parametrize("nb", [1, 7, 27])
def test_margins_of_the_exact_comparisons(runs, nb):
    """what the GPU tests compare exactly (rows, term counts, update counts) holds only if no transformed coordinate sits within rounding
    of a voxel face and no stop decision within rounding of relative_rmse"""
    _, tr = runs[nb]
    face, stop = vgicp_ref.face_margin(tr, vgicp_ref.VOXEL), vgicp_ref.stop_margin(tr)
    print(f'{nb} neighbours: nearest face {face:.3g} voxels, nearest stop decision {stop:.3g}')
    assert face >= 1e-9 and stop >= 1e-9


@pytest.mark.parametrize("init", ["identity", "start"])
def test_margins_of_the_one_step_cases(vmap, init):
    sc = vgicp_ref.scene()
    for nb in (1, 7, 27):
        tr = []
        r = vgicp_ref.vgicp(sc['src'], vmap, nb, sc['src_normals'], None if init == "identity" else vgicp_ref.start(), 1, trace=tr)
        assert r['iterations'] == 1 and vgicp_ref.face_margin(tr, vgicp_ref.VOXEL) >= 1e-9


def test_margins_of_the_sub_cloud_cases():
    sc = vgicp_ref.scene()
    for n, m in SIZES[2:]:
        tr = []
        vm = vgicp_ref.build_map(sc['tgt'][:m], sc['tgt_normals'][:m], vgicp_ref.VOXEL)
        r = vgicp_ref.vgicp(sc['src'][:n], vm, 7, sc['src_normals'][:n], None, 40, trace=tr)
        assert 0 < r['iterations'] < 40, (n, m)
        assert vgicp_ref.face_margin(tr, vgicp_ref.VOXEL) >= 1e-9 and vgicp_ref.stop_margin(tr) >= 1e-9, (n, m)
    one = vgicp_ref.vgicp(sc['src'][:1], vgicp_ref.build_map(sc['tgt'][:1500], sc['tgt_normals'][:1500], vgicp_ref.VOXEL), 7, sc['src_normals'][:1])
    assert one['iterations'] == 0 and one['terms'] == 4                                # fewer than 6 terms: no system


def test_hand_computed_map():
    pts = vgicp_ref.HAND_POINTS
    nrm = np.zeros_like(pts)
    nrm[:, 2] = 1.0
    nrm[3] = [np.nan, 0, 0]                                                        # no normal: C = I
    m = vgicp_ref.build_map(pts, nrm, vgicp_ref.HAND_VOXEL, 0.5)
    k, ok = vgicp_ref.voxel_of(pts.astype(np.float64), vgicp_ref.HAND_VOXEL)
    assert k[:4, 0].tolist() == [2, -1, 0, 0] and k[4, 0] == -1
    assert ok.tolist() == [True] * 5 + [False] * 3 + [True] * 3
    assert m['keys'].tolist() == [vgicp_ref.key_of(c) for c in vgicp_ref.HAND_KEYS] and (np.diff(m['keys']) > 0).all()
    assert m['counts'].tolist() == vgicp_ref.HAND_COUNTS
    assert m['keys'][2] == (1 << 62) | (1 << 41) | (1 << 20)                       # voxel (0, 0, 0)
    assert np.array_equal(m['means'][1], [(-0.25 - 0.125) / 2, 0, 0]) and np.array_equal(m['means'][2], [0, 0, 0])
    assert np.array_equal(m['covs'][1], [1, 0, 0, 1, 0, 0.5])                      # I - 0.5 z z^T, twice
    assert np.array_equal(m['covs'][2], [1, 0, 0, 1, 0, 0.75])                     # (C(z) + I) / 2


# ---------------------------------------------------------------------------------------------------- Python, no device
class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def test_python_checks_come_before_the_device_check():
    from buffer_amd import icp, ops
    assert sorted(ops.ICP_METHODS) == ['generalized', 'point_to_plane', 'point_to_point'] and ops.VGICP_NEIGHBORS == (1, 7, 27)
    s, t = [_Shape(5, 3)], [_Shape(7, 3)]
    for v in (None, 0.0, -0.2, math.nan, math.inf):
        with pytest.raises(ValueError, match="voxel"):
            icp.vgicp_batched(s, t, voxel=v)
        with pytest.raises(ValueError, match="voxel"):
            icp.voxel_map(t, v)
        with pytest.raises(ValueError, match="voxel"):
            icp.icp_voxelized(None, None, None, None, v)
    for eps in (0.0, -1.0, 1.5, math.nan):
        with pytest.raises(ValueError, match="epsilon"):
            icp.vgicp_batched(s, t, voxel=0.2, epsilon=eps)
        with pytest.raises(ValueError, match="epsilon"):
            icp.voxel_map(t, 0.2, epsilon=eps)
    for nb in (0, 6, 26, 28):
        with pytest.raises(ValueError, match="neighbors"):
            icp.vgicp_batched(s, t, voxel=0.2, neighbors=nb)
    with pytest.raises(ValueError, match="src_normals"):
        icp.vgicp_batched(s, t, voxel=0.2, src_normals=[_Shape(6, 3)])
    with pytest.raises(ValueError, match="tgt_normals"):
        icp.vgicp_batched(s, t, voxel=0.2, tgt_normals=[])
    with pytest.raises(ValueError, match="tgt_normals"):
        icp.voxel_map(t, 0.2, tgt_normals=[_Shape(6, 3)])
    with pytest.raises(ValueError, match="no target"):
        icp.voxel_map([], 0.2)
    with pytest.raises(ValueError, match="initial"):
        icp.vgicp_batched(s, t, voxel=0.2, inits=[])
    with pytest.raises(ValueError, match="targets"):
        icp.vgicp_batched(s + s, t, voxel=0.2)
    for pt in ([1], [-1], [0, 0]):
        with pytest.raises(ValueError, match="pair_target"):
            icp.vgicp_batched(s, t, voxel=0.2, pair_target=pt)
    with pytest.raises(RuntimeError, match="device"):                     # well-formed arguments reach the device check
        icp.vgicp_batched(s, t, voxel=0.2, src_normals=s, tgt_normals=t)
    with pytest.raises(RuntimeError, match="device"):
        icp.voxel_map(t, 0.2, t)


def test_refine_batch_method_check():
    import torch
    from buffer_amd.pipeline import BufferPipeline
    pipe = BufferPipeline.__new__(BufferPipeline)                          # the checks need no state
    pipe.device = torch.device('cpu')
    with pytest.raises(ValueError, match="unknown method"):
        pipe.refine_batch([], [], method='colored')
    with pytest.raises(ValueError, match="neighbors"):
        pipe.refine_batch([], [], method='voxelized', neighbors=5)
    out = pipe.refine_batch([], [], method='voxelized', voxel=0.3, neighbors=27)       # an empty batch: the empty result, no device
    assert out['poses'].shape == (0, 4, 4) and out['iterations'].shape == (0,)


def test_driver_flags():
    from buffer_amd import eth, kitti, threedmatch
    for mod in (threedmatch, kitti, eth):
        a, _ = mod.parse_args(['--root', 'r'])
        assert (a.refine, a.refine_dist, a.refine_iters, a.refine_voxel, a.refine_neighbors) == (None, None, 30, None, 7)
        a, _ = mod.parse_args(['--root', 'r', '--refine', 'voxelized', '--refine-voxel', '0.4', '--refine-neighbors', '27'])
        assert (a.refine, a.refine_voxel, a.refine_neighbors) == ('voxelized', 0.4, 27)
        a, _ = mod.parse_args(['--root', 'r', '--refine', 'voxelized'])
        assert (a.refine_voxel, a.refine_neighbors) == (None, 7)
        for bad in (['--refine-neighbors', '9'], ['--refine', 'colored'], ['--refine', 'voxelized', '--refine-voxel', '0'],
                    ['--refine', 'voxelized', '--descriptor', 'fpfh']):
            with pytest.raises(SystemExit):
                mod.parse_args(['--root', 'r'] + bad)


# ---------------------------------------------------------------------------------------------------- C ABI, no device
def test_symbols_and_size_functions():
    from buffer_amd import _lib, build
    build.build()
    lib = _lib.lib()
    names = _lib.exported_symbols()
    for f in ("buf_voxel_map_bytes", "buf_voxel_map_ws_bytes", "buf_voxel_map_build", "buf_voxel_map_export", "buf_vgicp_ws_bytes",
              "buf_vgicp_batched"):
        assert f in names
    assert lib.buf_version() == 670
    a, b = lib.buf_voxel_map_bytes(100_000, 4, 1 << 20), lib.buf_voxel_map_bytes(200_000, 4, 1 << 20)
    assert 0 < a < b and b - a >= 88 * 100_000
    assert lib.buf_voxel_map_bytes(100_000, 4, 1 << 21) - a >= 4 << 20
    assert lib.buf_voxel_map_ws_bytes(100_000, 4, 1 << 20) > 0
    assert lib.buf_voxel_map_bytes(-1, 4, 1 << 20) == 0 and lib.buf_voxel_map_bytes(10, 0, 1 << 20) == 0 and lib.buf_voxel_map_bytes(10, 1, 0) == 0
    assert lib.buf_vgicp_ws_bytes(100_000, 16) > lib.buf_vgicp_ws_bytes(1_000, 16) > 0
    assert lib.buf_vgicp_ws_bytes(-1, 4) == 0 and lib.buf_vgicp_ws_bytes(10, 0) == 0
    assert lib.buf_icp_ws_bytes(100_000, 100_000, 4, 3) == 0                   # the ICP entry points keep refusing other methods
