import numpy as np


class TransformationEstimationPointToPoint:
    def __init__(self, with_scaling=False):
        self.with_scaling = bool(with_scaling)


class TransformationEstimationPointToPlane:
    """L2 point-to-plane ICP step (open3d's, restated, unpinned): needs target normals."""

    def __init__(self, kernel=None):
        if kernel is not None:
            raise NotImplementedError("open3d stand-in: robust kernels other than L2 are not provided")
        self.kernel = None


class TransformationEstimationForGeneralizedICP:
    """Generalized ICP step (plane-to-plane; csrc/icp.hip, restated, unpinned): covariances I - (1 - epsilon) n n^T from the normals."""

    def __init__(self, epsilon=1e-3, kernel=None):
        if kernel is not None:
            raise NotImplementedError("open3d stand-in: robust kernels other than L2 are not provided")
        self.epsilon, self.kernel = float(epsilon), None


class CorrespondenceCheckerBasedOnEdgeLength:
    def __init__(self, similarity_threshold=0.9):
        self.similarity_threshold = float(similarity_threshold)


class CorrespondenceCheckerBasedOnDistance:
    def __init__(self, distance_threshold):
        self.distance_threshold = float(distance_threshold)


class RANSACConvergenceCriteria:
    def __init__(self, max_iteration=100000, confidence=0.999):
        self.max_iteration, self.confidence = int(max_iteration), float(confidence)


class ICPConvergenceCriteria:
    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
        self.relative_fitness, self.relative_rmse, self.max_iteration = float(relative_fitness), float(relative_rmse), int(max_iteration)


class RegistrationResult:
    def __init__(self, transformation=None, fitness=0.0, inlier_rmse=0.0, correspondence_set=None):
        self.transformation = np.eye(4) if transformation is None else np.asarray(transformation, np.float64)
        self.fitness, self.inlier_rmse = float(fitness), float(inlier_rmse)
        self.correspondence_set = np.zeros((0, 2), np.int32) if correspondence_set is None else correspondence_set

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, "
                f"and correspondence_set size of {len(self.correspondence_set)}")


def _device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("open3d stand-in (buffer_amd): this call runs on a HIP device and none is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _ransac_settings(max_correspondence_distance, estimation_method, ransac_n, checkers, criteria):
    """what the two RANSAC entry points accept -> (edge similarity, hypothesis budget); everything else is refused"""
    from buffer_amd.config import THREEDMATCH
    est = estimation_method or TransformationEstimationPointToPoint(False)
    if est.with_scaling or int(ransac_n) != 3:
        raise NotImplementedError("open3d stand-in: rigid point-to-point estimation from 3-point samples only")
    edge, dist = 0.0, float(max_correspondence_distance)       # no checker = nothing rejected
    for c in checkers:
        if isinstance(c, CorrespondenceCheckerBasedOnEdgeLength):
            edge = c.similarity_threshold
        elif isinstance(c, CorrespondenceCheckerBasedOnDistance):
            if abs(c.distance_threshold - dist) > 1e-12:          # the kernel checks samples and scores candidates with ONE distance
                raise NotImplementedError("open3d stand-in: the distance checker must use max_correspondence_distance")
        else:
            raise NotImplementedError(f"open3d stand-in: checker {type(c).__name__}")
    nhyp = THREEDMATCH.ransac_hypotheses
    if criteria is not None:
        nhyp = max(1, min(nhyp, criteria.max_iteration))
    return edge, nhyp


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance,
                                                estimation_method=None, ransac_n=3, checkers=(), criteria=None, seed=0):
    """models/BUFFER.py:318-326 -> buf_ransac_kabsch (csrc/registration.hip): a fixed budget of seeded 3-point
    hypotheses, each pre-checked by the edge-length and distance checkers, Kabsch, ranked by inlier count then RMSE
    within `max_correspondence_distance`.  `criteria.max_iteration` caps the budget (default budget 4096);
    `confidence` early termination does not apply to a batch that is evaluated at once."""
    import torch
    from buffer_amd import ops
    edge, nhyp = _ransac_settings(max_correspondence_distance, estimation_method, ransac_n, checkers, criteria)
    dev = _device()
    src = torch.from_numpy(np.asarray(source.points, np.float32)).to(dev)
    tgt = torch.from_numpy(np.asarray(target.points, np.float32)).to(dev)
    corr = np.asarray(corres, np.int32).reshape(-1, 2)
    if len(corr) < 3:
        return RegistrationResult()
    T, info = ops.ransac_kabsch(src, tgt, torch.from_numpy(corr).to(dev), nhyp=nhyp, seed=seed,
                                max_dist=float(max_correspondence_distance), edge_similarity=edge)
    T = T.cpu().numpy().astype(np.float64)
    p = np.asarray(source.points)[corr[:, 0]] @ T[:3, :3].T + T[:3, 3]
    d = np.linalg.norm(p - np.asarray(target.points)[corr[:, 1]], axis=1)
    inl = d < max_correspondence_distance
    return RegistrationResult(T, inl.mean() if len(inl) else 0.0, float(np.sqrt((d[inl] ** 2).mean())) if inl.any() else 0.0,
                              corr[inl])


class Feature:
    """open3d.pipelines.registration.Feature: `data` f64[dimension, num], one column per point"""

    def __init__(self, data=None):
        self.data = np.zeros((0, 0), np.float64) if data is None else np.ascontiguousarray(data, dtype=np.float64)

    def dimension(self):
        return int(self.data.shape[0])

    def num(self):
        return int(self.data.shape[1])

    def resize(self, dim, n):
        self.data = np.zeros((int(dim), int(n)), np.float64)

    def __repr__(self):
        return f"Feature class with dimension = {self.dimension()} and num = {self.num()}"


def compute_fpfh_feature(input, search_param):
    """open3d compute_fpfh_feature -> Feature with data f64[33, n] (buffer_amd/fpfh.py compute_fpfh, csrc/fpfh.hip; restated from
    the published algorithm, unpinned: include/buffer_hip.h N6 lists the deviations).  The neighbourhood is
    KDTreeSearchParamHybrid(radius, max_nn) with max_nn <= 128; the cloud needs normals."""
    import torch
    from buffer_amd import fpfh
    from ..geometry import KDTreeSearchParamHybrid
    if not input.has_normals():
        raise RuntimeError("[Open3D Error] Failed because input point cloud has no normal.")
    if not isinstance(search_param, KDTreeSearchParamHybrid):
        raise NotImplementedError("open3d stand-in: compute_fpfh_feature takes a KDTreeSearchParamHybrid(radius, max_nn) neighbourhood only")
    dev = _device()
    pts = torch.from_numpy(np.asarray(input.points, np.float32).reshape(-1, 3)).to(dev)
    nrm = torch.from_numpy(np.asarray(input.normals, np.float32).reshape(-1, 3)).to(dev)
    return Feature(fpfh.compute_fpfh(pts, nrm, search_param.radius, search_param.max_nn).cpu().numpy().T)


def correspondences_from_features(source_features, target_features, mutual_filter=False, mutual_consistency_ratio=0.1):
    """open3d correspondences_from_features -> int32[m,2] rows (source column, its nearest target column), ascending by source column:
    the 1-NN matches of the source features among the target features (ops.feature_match, csrc/match.hip: exact fp32 squared
    distances, ties to the lower column; restated, unpinned: include/buffer_hip.h N12 is the specification).  mutual_filter keeps the
    matches that are nearest in both directions -- unless they are fewer than mutual_consistency_ratio x the forward matches: then, as
    in open3d, the forward matches are returned."""
    import torch
    from buffer_amd import ops
    if source_features.dimension() != target_features.dimension():
        raise ValueError("open3d stand-in: the two feature sets differ in dimension")
    na, nb = source_features.num(), target_features.num()
    if na == 0 or nb == 0:
        return np.zeros((0, 2), np.int32)
    dev = _device()
    fa = torch.from_numpy(np.ascontiguousarray(source_features.data.T)).to(dev)
    fb = torch.from_numpy(np.ascontiguousarray(target_features.data.T)).to(dev)
    mutual, _, nn, _ = ops.feature_match(fa, [na], fb, [nb], mutual=True, return_nn=True)      # nn: the forward matches, filter or not
    nn = nn[:, 0].cpu().numpy()
    rows = np.flatnonzero(nn >= 0)
    forward = np.stack([rows, nn[rows]], 1).astype(np.int32)
    if not mutual_filter:
        return forward
    mutual = mutual.cpu().numpy()
    return mutual if len(mutual) >= float(mutual_consistency_ratio) * len(forward) else forward


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, estimation_method=None, ransac_n=3, checkers=(),
                                                  criteria=None, seed=0):
    """open3d registration_ransac_based_on_feature_matching: 1-NN matches of the source features among the target features
    (buffer_amd/fpfh.py match; mutual_filter keeps the mutual ones, without open3d's fall-back to all matches when fewer than
    ransac_n are mutual), then the RANSAC of registration_ransac_based_on_correspondence on them, with the same refusals."""
    import torch
    from buffer_amd import fpfh
    edge, nhyp = _ransac_settings(max_correspondence_distance, estimation_method, ransac_n, checkers, criteria)
    if source_feature.num() != len(source.points) or target_feature.num() != len(target.points):
        raise ValueError("open3d stand-in: a feature set does not have one column per point of its cloud")
    dev = _device()
    src = torch.from_numpy(np.asarray(source.points, np.float32).reshape(-1, 3)).to(dev)
    tgt = torch.from_numpy(np.asarray(target.points, np.float32).reshape(-1, 3)).to(dev)
    fa = torch.from_numpy(np.ascontiguousarray(source_feature.data.T)).to(dev)
    fb = torch.from_numpy(np.ascontiguousarray(target_feature.data.T)).to(dev)
    corr_dev = fpfh.match(fa, fb, bool(mutual_filter))
    corr = corr_dev.cpu().numpy()
    if len(corr) < 3:
        return RegistrationResult()
    T = fpfh.ransac_on_matches(src, tgt, corr_dev, nhyp, seed, float(max_correspondence_distance), edge)
    T = T.cpu().numpy().astype(np.float64)
    p = np.asarray(source.points)[corr[:, 0]] @ T[:3, :3].T + T[:3, 3]
    d = np.linalg.norm(p - np.asarray(target.points)[corr[:, 1]], axis=1)
    inl = d < max_correspondence_distance
    return RegistrationResult(T, inl.mean() if len(inl) else 0.0, float(np.sqrt((d[inl] ** 2).mean())) if inl.any() else 0.0,
                              corr[inl])


class FastGlobalRegistrationOption:
    """open3d's option holder, with its names and defaults (buffer_amd/fgr.py FgrOptions carries them to the kernel)"""

    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000):
        self.division_factor, self.use_absolute_scale, self.decrease_mu = float(division_factor), bool(use_absolute_scale), bool(decrease_mu)
        self.maximum_correspondence_distance, self.iteration_number = float(maximum_correspondence_distance), int(iteration_number)
        self.tuple_scale, self.maximum_tuple_count = float(tuple_scale), int(maximum_tuple_count)

    def __repr__(self):
        return ("FastGlobalRegistrationOption class with " + ", ".join(f"{k}={v}" for k, v in vars(self).items()))


def registration_fast_based_on_feature_matching(source, target, source_feature, target_feature, option=None, seed=0):
    """open3d registration_fast_based_on_feature_matching: the MUTUAL 1-NN matches of the two feature sets (buffer_amd/fpfh.py match;
    open3d's own matching adds a cross-check fall-back this one has not), then Fast Global Registration on them (buffer_amd/fgr.py,
    csrc/fgr.hip; restated from the published algorithm, unpinned: include/buffer_hip.h N7 lists the deviations).
    option.maximum_correspondence_distance is read in normalised units, as open3d reads it, both for the annealing floor and for the
    result's inliers: the residual of a match is divided by the pair's scale D before it is compared.  use_absolute_scale=True is
    refused.  `seed` seeds the tuple draw (open3d draws from its global generator)."""
    import torch
    from buffer_amd import fgr, fpfh
    opt = option or FastGlobalRegistrationOption()
    if opt.use_absolute_scale:
        raise NotImplementedError("open3d stand-in: FastGlobalRegistrationOption.use_absolute_scale=True is not provided")
    if source_feature.num() != len(source.points) or target_feature.num() != len(target.points):
        raise ValueError("open3d stand-in: a feature set does not have one column per point of its cloud")
    dev = _device()
    sp, tp = np.asarray(source.points, np.float32).reshape(-1, 3), np.asarray(target.points, np.float32).reshape(-1, 3)
    src, tgt = torch.from_numpy(sp).to(dev), torch.from_numpy(tp).to(dev)
    fa = torch.from_numpy(np.ascontiguousarray(source_feature.data.T)).to(dev)
    fb = torch.from_numpy(np.ascontiguousarray(target_feature.data.T)).to(dev)
    corr_dev = fpfh.match(fa, fb, True)
    corr = corr_dev.cpu().numpy()
    res = fgr.fast_global_registration(src, [len(sp)], tgt, [len(tp)], corr_dev, [len(corr)], seeds=[seed], options=fgr.FgrOptions(
        **{k: getattr(opt, k) for k in ('division_factor', 'use_absolute_scale', 'decrease_mu', 'maximum_correspondence_distance',
                                        'iteration_number', 'tuple_scale', 'maximum_tuple_count')}))
    T = res['poses'][0].cpu().numpy()
    if len(corr) == 0:
        return RegistrationResult(T)
    fin = [c[np.isfinite(c).all(1)].astype(np.float64) for c in (sp, tp)]
    D = max(float(np.linalg.norm(c - c.mean(0), axis=1).max()) if len(c) else 0.0 for c in fin)
    p = sp[corr[:, 0]].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d = np.linalg.norm(p - tp[corr[:, 1]], axis=1)
    inl = d / D < opt.maximum_correspondence_distance if D > 0 else np.zeros(len(d), bool)
    return RegistrationResult(T, inl.mean(), float(np.sqrt((d[inl] ** 2).mean())) if inl.any() else 0.0, corr[inl])


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """KITTI/dataset.py:104-107: ICP on the device (buffer_amd/icp.py, csrc/icp.hip).  TransformationEstimationPointToPlane uses
    the target's normals; a target without normals raises RuntimeError (open3d would hand back the initial transform unrefined:
    refused here rather than returning an unrefined pose)."""
    import torch
    from buffer_amd import icp
    est = estimation_method or TransformationEstimationPointToPoint(False)
    plane = isinstance(est, TransformationEstimationPointToPlane)
    if not plane and est.with_scaling:
        raise NotImplementedError("open3d stand-in: rigid point-to-point ICP only")
    if plane and not target.has_normals():
        raise RuntimeError("open3d stand-in: point-to-plane ICP needs target normals; call target.estimate_normals() first")
    cr = criteria or ICPConvergenceCriteria()
    dev = _device()
    clouds = [source.points, target.points] + ([target.normals] if plane else [])
    run = icp.icp_point_to_plane if plane else icp.icp_point_to_point
    T, fit, rmse, corr = run(*(torch.from_numpy(np.asarray(c, np.float32)).to(dev) for c in clouds), float(max_correspondence_distance),
                             np.eye(4) if init is None else np.asarray(init, np.float64),
                             cr.max_iteration, cr.relative_fitness, cr.relative_rmse)
    return RegistrationResult(T, fit, rmse, corr)


def registration_generalized_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """Generalized ICP on the device (buffer_amd/icp.py icp_generalized).  A cloud without normals gets them from a copy's
    estimate_normals() (30-NN) first, as open3d estimates a cloud's covariances itself; the clouds passed in are left as they are.
    inlier_rmse is Euclidean, as for registration_icp (open3d reports the Mahalanobis residual here)."""
    import torch
    from buffer_amd import icp
    from ..geometry import PointCloud
    est = estimation_method or TransformationEstimationForGeneralizedICP()
    if not isinstance(est, TransformationEstimationForGeneralizedICP):
        raise TypeError("open3d stand-in: registration_generalized_icp takes a TransformationEstimationForGeneralizedICP")
    cr = criteria or ICPConvergenceCriteria()
    dev = _device()
    clouds = []
    for pcd in (source, target):
        if not pcd.has_normals() and len(pcd.points) > 0:
            pcd = PointCloud(pcd.points)
            pcd.estimate_normals()
        clouds += [pcd.points, pcd.normals]
    T, fit, rmse, corr = icp.icp_generalized(*(torch.from_numpy(np.asarray(c, np.float32).reshape(-1, 3)).to(dev) for c in clouds),
                                             float(max_correspondence_distance),
                                             np.eye(4) if init is None else np.asarray(init, np.float64),
                                             cr.max_iteration, cr.relative_fitness, cr.relative_rmse, est.epsilon)
    return RegistrationResult(T, fit, rmse, corr)


def _one_pair_statistics(source, target, max_correspondence_distance, transformation, correspondences):
    """source / target PointClouds -> pairs.pair_statistics of the one pair (source -> target under `transformation`)"""
    import torch
    from buffer_amd import pairs
    dev = _device()
    T = np.eye(4) if transformation is None else np.asarray(transformation, np.float64).reshape(4, 4)
    clouds = [torch.from_numpy(np.asarray(c.points, np.float32).reshape(-1, 3)).to(dev) for c in (source, target)]
    return T, pairs.pair_statistics(clouds, [(0, 1)], T[None], float(max_correspondence_distance), correspondences=correspondences)


def evaluate_registration(source, target, max_correspondence_distance, transformation=None):
    """open3d evaluate_registration: fitness (matched source points / source points), inlier RMSE and the correspondence set of
    `transformation` itself, nothing refined (buffer_amd/pairs.py, csrc/pairstats.hip)."""
    T, st = _one_pair_statistics(source, target, max_correspondence_distance, transformation, True)
    nn = st['nn'][0]
    hit = np.flatnonzero(nn >= 0)
    return RegistrationResult(T, st['overlap'][0], st['inlier_rmse'][0], np.stack([hit, nn[hit]], 1).astype(np.int32))


def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation):
    """open3d get_information_matrix_from_point_clouds -> f64[6,6], order [rotation, translation], over the matched target points
    (restated from the upstream source as recalled, unpinned)."""
    from buffer_amd import pairs
    _, st = _one_pair_statistics(source, target, max_correspondence_distance, transformation, False)
    return pairs.information_matrix(st['matched'][0], st['sum_u'][0], st['sum_uu'][0], 'open3d')
