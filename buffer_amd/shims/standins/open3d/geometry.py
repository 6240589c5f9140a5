import numpy as np

from .utility import Vector3dVector


class KDTreeSearchParamKNN:
    def __init__(self, knn=30):
        self.knn = int(knn)


class KDTreeSearchParamRadius:
    def __init__(self, radius):
        self.radius = float(radius)


class KDTreeSearchParamHybrid:
    def __init__(self, radius, max_nn):
        self.radius, self.max_nn = float(radius), int(max_nn)


def _device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("open3d stand-in (buffer_amd): this call runs on a HIP device and none is visible")
    return torch.device("cuda", torch.cuda.current_device())


class PointCloud:
    def __init__(self, points=None):
        self._points = Vector3dVector()
        self._normals = Vector3dVector()
        self._colors = Vector3dVector()
        self._covariances = np.zeros((0, 3, 3), np.float64)
        if points is not None:
            self.points = points

    points = property(lambda s: s._points, lambda s, v: setattr(s, "_points", Vector3dVector(v)))
    normals = property(lambda s: s._normals, lambda s, v: setattr(s, "_normals", Vector3dVector(v)))
    colors = property(lambda s: s._colors, lambda s, v: setattr(s, "_colors", Vector3dVector(v)))
    covariances = property(lambda s: s._covariances, lambda s, v: setattr(s, "_covariances", np.asarray(v, np.float64).reshape(-1, 3, 3)))

    def has_points(self):
        return len(self._points) > 0

    def has_normals(self):
        return len(self._normals) > 0 and len(self._normals) == len(self._points)

    def has_colors(self):
        return len(self._colors) > 0 and len(self._colors) == len(self._points)

    def paint_uniform_color(self, color):
        self._colors = Vector3dVector(np.repeat(np.asarray(color, np.float64).reshape(1, 3), len(self._points), 0))
        return self

    def transform(self, T):
        T = np.asarray(T, np.float64)
        self._points = Vector3dVector(np.asarray(self._points) @ T[:3, :3].T + T[:3, 3])
        if self.has_normals():
            self._normals = Vector3dVector(np.asarray(self._normals) @ T[:3, :3].T)
        return self

    def voxel_down_sample(self, voxel_size):
        """-> new PointCloud of voxel means (csrc/preprocess.hip buf_voxel_downsample; fp64 means like open3d's)."""
        import torch
        from buffer_amd import preprocess
        dev = _device()
        pts = torch.from_numpy(np.asarray(self._points)).to(dev)
        out = PointCloud()
        if self.has_normals():
            m, nm = preprocess.voxel_down_sample(pts, voxel_size, normals=torch.from_numpy(np.asarray(self._normals)).to(dev))
            out._normals = Vector3dVector(nm.cpu().numpy())
        else:
            m = preprocess.voxel_down_sample(pts, voxel_size)
        out._points = Vector3dVector(m.cpu().numpy())
        if self.has_colors():                                # colours are display only in the reference: uniform paint kept
            out._colors = Vector3dVector(np.repeat(np.asarray(self._colors)[:1], len(out._points), 0))
        return out

    def _radius_search(self, search_param, what):
        """(radius, max_nn or None) of a Hybrid / Radius neighbourhood"""
        if isinstance(search_param, KDTreeSearchParamHybrid):
            return search_param.radius, search_param.max_nn
        if isinstance(search_param, KDTreeSearchParamRadius):
            return search_param.radius, None
        raise NotImplementedError(f"open3d stand-in: {what} takes a KDTreeSearchParamHybrid or KDTreeSearchParamRadius neighbourhood"
                                  + (" (or KDTreeSearchParamKNN)" if what == "estimate_normals" else ""))

    def estimate_normals(self, search_param=None, fast_normal_computation=True):
        """PCA normals; orientation is left as computed.  KDTreeSearchParamKNN (default: 30-NN): csrc/preprocess.hip buf_knn_normals;
        KDTreeSearchParamHybrid(radius, max_nn) / KDTreeSearchParamRadius(radius): csrc/normals.hip buf_row_normals
        (preprocess.estimate_normals_radius; include/buffer_hip.h N13 lists the deviations)."""
        import torch
        from buffer_amd import preprocess
        knn = search_param is None or isinstance(search_param, KDTreeSearchParamKNN)
        if not knn:
            radius, max_nn = self._radius_search(search_param, "estimate_normals")
        pts = torch.from_numpy(np.asarray(self._points, np.float32).reshape(-1, 3)).to(_device())
        if knn:
            nrm = preprocess.estimate_normals(pts, knn=search_param.knn if search_param is not None else 30, orient=False)
        else:
            nrm = preprocess.estimate_normals_radius(pts, radius, max_nn, orient=False)
        self._normals = Vector3dVector(nrm.cpu().numpy())
        return self

    def estimate_covariances(self, search_param=None):
        """per-point covariances of the neighbourhoods (KDTreeSearchParamHybrid / KDTreeSearchParamRadius; open3d's default is
        KDTreeSearchParamKNN(30), which is not provided) -> self.covariances f64[n,3,3] (preprocess.estimate_covariances, N13)."""
        import torch
        from buffer_amd import preprocess
        radius, max_nn = self._radius_search(search_param, "estimate_covariances")
        pts = torch.from_numpy(np.asarray(self._points, np.float32).reshape(-1, 3)).to(_device())
        c = preprocess.estimate_covariances(pts, radius, max_nn).cpu().numpy()
        self._covariances = c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
        return self

    def has_covariances(self):
        return len(self._covariances) > 0 and len(self._covariances) == len(self._points)

    def orient_normals_towards_camera_location(self, camera_location=(0.0, 0.0, 0.0)):
        if not self.has_normals():
            raise RuntimeError("[Open3D Error] No normals in the PointCloud. Call EstimateNormals() first.")
        p, n = np.asarray(self._points), np.asarray(self._normals).copy()
        cam = np.asarray(camera_location, np.float64).reshape(1, 3)
        zero = np.linalg.norm(n, axis=1) == 0.0                 # open3d: a zero normal becomes the view direction
        view = cam - p
        n[zero] = view[zero] / np.maximum(np.linalg.norm(view[zero], axis=1, keepdims=True), 1e-300)
        flip = (n * view).sum(1) < 0.0
        n[flip] *= -1.0
        self._normals = Vector3dVector(n)
        return self


def _compute_iss_keypoints(input, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """open3d geometry.keypoint.compute_iss_keypoints -> PointCloud of the keypoints, in row order, with their normals if the input
    has them (buffer_amd/keypoints.py iss_keypoints, csrc/iss.hip; restated from the published algorithm, unpinned: include/buffer_hip.h
    N11 lists the deviations).  A radius of 0 is open3d's heuristic: 6 x (salient) / 4 x (non-max) the cloud's resolution = the mean
    distance of a point to its nearest other point (ops.knn at k = 2, fp32)."""
    import torch
    from buffer_amd import keypoints, ops
    out = PointCloud()
    if not input.has_points():
        return out
    pts_h = np.asarray(input.points).reshape(-1, 3)
    pts = torch.from_numpy(pts_h.astype(np.float32)).to(_device())
    if salient_radius == 0.0 or non_max_radius == 0.0:
        res = 0.0
        if len(pts_h) >= 2:
            res = float(ops.knn(pts[None], pts[None], 2)[0][0, :, 1].double().mean())
        salient_radius, non_max_radius = 6.0 * res, 4.0 * res
    if not (salient_radius > 0.0 and non_max_radius > 0.0):     # a single point, or all points coincident: nothing is salient
        return out
    idx = keypoints.iss_keypoints(pts, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)[0].cpu().numpy()
    out._points = Vector3dVector(pts_h[idx])
    if input.has_normals():
        out._normals = Vector3dVector(np.asarray(input.normals)[idx])
    return out


class keypoint:
    """open3d.geometry.keypoint"""
    compute_iss_keypoints = staticmethod(_compute_iss_keypoints)
