"""Batched ICP, the parts that need no device: the C ABI of buf_icp_ws_bytes / buf_icp_batched (argument checks come before any
device call) and the open3d stand-in's point-to-plane estimation class."""
import ctypes as C
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from buffer_amd import _lib, build
    build.build()
    return _lib.lib()


def test_icp_ws_bytes_is_exported_and_grows_with_every_argument(lib):
    from buffer_amd import _lib
    assert "buf_icp_ws_bytes" in _lib.exported_symbols() and "buf_icp_batched" in _lib.exported_symbols()
    base = lib.buf_icp_ws_bytes(100_000, 100_000, 4, 0)
    assert base > 0
    assert lib.buf_icp_ws_bytes(200_000, 100_000, 4, 0) > base
    assert lib.buf_icp_ws_bytes(100_000, 200_000, 4, 0) > base
    assert lib.buf_icp_ws_bytes(100_000, 100_000, 64, 0) > base
    assert lib.buf_icp_ws_bytes(100_000, 100_000, 4, 1) > base            # point-to-plane records are longer
    assert lib.buf_icp_ws_bytes(100_000, 100_000, 4, 7) == 0              # unknown method
    assert lib.buf_icp_ws_bytes(-1, 100_000, 4, 0) == 0


def _call(lib, method=0, max_dist=0.2, normals=True, src_len=(10, 20), tgt_len=(30, 40)):
    """buf_icp_batched with placeholder device pointers: only argument checks may run (they precede any device call)."""
    fake = C.c_void_p(0x1000)
    sl, tl = np.array(src_len, np.int32), np.array(tgt_len, np.int32)
    rc = lib.buf_icp_batched(fake, C.c_void_p(sl.ctypes.data), fake, fake if normals else C.c_void_p(0), C.c_void_p(tl.ctypes.data),
                             len(sl), method, max_dist, fake, 30, 1e-6, 1e-6, fake, fake, fake, fake, C.c_void_p(0), fake, 1 << 30,
                             C.c_void_p(0))
    return rc, lib.buf_last_error().decode()


@pytest.mark.parametrize("max_dist", [0.0, -0.2, math.nan, math.inf])
def test_icp_batched_rejects_a_bad_distance(lib, max_dist):
    rc, msg = _call(lib, max_dist=max_dist)
    assert rc == -1 and "max_dist" in msg


def test_icp_batched_rejects_point_to_plane_without_normals(lib):
    rc, msg = _call(lib, method=1, normals=False)
    assert rc == -1 and "normals" in msg
    rc, msg = _call(lib, method=2)
    assert rc == -1 and "method" in msg


def test_icp_batched_rejects_negative_lengths(lib):
    rc, msg = _call(lib, src_len=(10, -1))
    assert rc == -1 and "negative" in msg
    rc, msg = _call(lib, tgt_len=(-5, 40))
    assert rc == -1 and "negative" in msg


def test_icp_batched_python_checks():
    from buffer_amd import icp
    with pytest.raises(ValueError):
        icp.icp_batched([None, None], [None], 0.2)
    with pytest.raises(ValueError):
        icp.icp_batched([None], [None], 0.2, method='point_to_plane')
    with pytest.raises(ValueError):
        icp.icp_batched([None], [None], 0.2, method='generalized')


def test_open3d_standin_has_point_to_plane():
    import buffer_amd.shims as shims
    shims.install()
    import open3d as o3d
    reg = o3d.pipelines.registration
    est = reg.TransformationEstimationPointToPlane()
    assert est.kernel is None
    pcd0 = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(np.zeros((4, 3))))
    pcd1 = o3d.geometry.PointCloud(o3d.utility.Vector3dVector(np.ones((4, 3))))
    with pytest.raises(RuntimeError, match="estimate_normals"):          # refused before any device work
        reg.registration_icp(pcd0, pcd1, 0.2, np.eye(4), est)
