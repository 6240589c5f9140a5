"""TEST INFRASTRUCTURE: a float64 numpy restatement of the Generalized ICP loop of csrc/icp.hip (include/buffer_hip.h, N2) and the one
scene the Generalized ICP tests use.  Host code only.

The scene: three unit-square wall patches on the coordinate planes (z = 0, y = 0, x = 0, a room corner), every point uniform on
its patch (point i lies on wall i % 3) with Gaussian noise of sigma = 1 mm along the wall's normal, normals analytic.  Target: 1 800
points, seed 0.  Source: an independent sampling of 900 points, seed 1, moved by the inverse of the planted pose
R = Rz(3 deg) Ry(-2 deg) Rx(1.5 deg), t = (0.02, -0.03, 0.015), so that the planted pose maps it onto the target.  Clouds and normals
are rounded through fp32.  Correspondence distance 0.10."""
import numpy as np

MAX_DIST = 0.10
SIGMA = 1e-3


def rot(ax, ay, az):
    """Rz(az) Ry(ay) Rx(ax)"""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def planted_pose():
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(*np.deg2rad([1.5, -2.0, 3.0])), [0.02, -0.03, 0.015]
    return T


def walls(n, seed):
    """n points on the three wall patches -> (points f64[n,3], normals f64[n,3])"""
    rng = np.random.default_rng(seed)
    uv, h = rng.uniform(0.0, 1.0, (n, 2)), rng.normal(0.0, SIGMA, n)
    axis = (2 - np.arange(n) % 3)                       # wall 0: z = 0, wall 1: y = 0, wall 2: x = 0
    pts, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for a in range(3):
        m = axis == a
        pts[np.ix_(m, [c for c in range(3) if c != a])] = uv[m]
        pts[m, a] = h[m]
        nrm[m, a] = 1.0
    return pts, nrm


_SCENE = []


def scene():
    """-> dict(src, src_normals f32[900,3], tgt, tgt_normals f32[1800,3], T f64[4,4] the planted pose src -> tgt); made once, shared:
    callers copy before they write."""
    if not _SCENE:
        T = planted_pose()
        R, t = T[:3, :3], T[:3, 3]
        tgt, tn = walls(1800, 0)
        s, sn = walls(900, 1)
        out = dict(src=((s - t) @ R).astype(np.float32), src_normals=(sn @ R).astype(np.float32),      # R^T (x - t), R^T n
                   tgt=tgt.astype(np.float32), tgt_normals=tn.astype(np.float32), T=T)
        for v in out.values():
            v.setflags(write=False)
        _SCENE.append(out)
    return _SCENE[0]


def moved(src, T):
    """the kernel's fp64 transform ((T0 x + T1 y) + T2 z) + T3 per row, and its fp32 rounding for the search"""
    s = np.asarray(src, np.float32).astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):                      # (NaN / inf rows stay what they are)
        p = np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], 1)
        return p, p.astype(np.float32)


def brute_nn(q32, tgt, dist):
    """nearest target row with fp32 d2 = ((dx*dx + dy*dy) + dz*dz) < r2 (strict, every operation rounded: sqdist3), ties to the lowest
    index, -1 = none; a non-finite query matches nothing"""
    tgt = np.asarray(tgt, np.float32)
    r2 = np.float32(dist) * np.float32(dist)
    out = np.full(len(q32), -1, np.int64)
    if len(tgt) == 0:
        return out
    with np.errstate(invalid='ignore', over='ignore'):
        for lo in range(0, len(q32), 512):
            q = q32[lo:lo + 512]
            dx, dy, dz = (q[:, None, c] - tgt[None, :, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(d2 < r2, d2, np.float32(np.inf))
            j = np.argmin(d2, 1)                                           # first of the minima = lowest index
            ok = np.isfinite(d2[np.arange(len(q)), j]) & np.isfinite(q).all(1)
            out[lo:lo + 512] = np.where(ok, j, -1)
    return out


def usable_normals(n):
    """fp64 rows; a row with | |n|^2 - 1 | >= 1e-3 or a non-finite component -> zero"""
    n = np.asarray(n, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = np.abs(l2 - 1.0) < 1e-3
    return np.where(ok[:, None], n, 0.0)


def _skew(p):
    S = np.zeros((len(p), 3, 3))
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -p[:, 2], p[:, 1], p[:, 2], -p[:, 0], -p[:, 1], p[:, 0]
    return S


def step_generalized(p, q, ns, nq, R, eps):
    """matched rows p = T s, q, their normals (zero = none) -> x f64[6] solving H x = -g, or None when H is not positive definite"""
    w = 1.0 - eps
    I = np.eye(3)
    Cq = I - w * nq[:, :, None] * nq[:, None, :]
    Cs = I - w * ns[:, :, None] * ns[:, None, :]
    M = np.linalg.inv(Cq + R @ Cs @ R.T)
    J = np.concatenate([-_skew(p), np.broadcast_to(I, (len(p), 3, 3))], 2)          # [k,3,6]
    JtM = np.einsum('kij,kil->kjl', J, M)
    H = np.einsum('kjl,klm->jm', JtM, J)
    g = np.einsum('kjl,kl->j', JtM, p - q)
    return _solve(H, g)


def _solve(H, g):
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None
    x = np.linalg.solve(H, -g)
    return x if np.isfinite(x).all() else None


def step_kabsch(p, q):
    """the point-to-point update: the rigid dT minimising sum |dT p - q|^2"""
    pc, qc = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((p - pc).T @ (q - qc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    dT = np.eye(4)
    dT[:3, :3] = Vt.T @ D @ U.T
    dT[:3, 3] = qc - dT[:3, :3] @ pc
    return dT


def icp(src, tgt, max_dist=MAX_DIST, init=None, max_iteration=30, method='generalized', src_normals=None, tgt_normals=None,
        epsilon=1e-3, relative_fitness=1e-6, relative_rmse=1e-6):
    """The loop of k_icp_correspond / k_icp_update for one pair, method 'generalized' or 'point_to_point' (Kabsch)
    -> dict(T, fitness, inlier_rmse, iterations, correspondences int64[k,2])."""
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).reshape(4, 4).copy()
    tgt64 = tgt.astype(np.float64)
    if method == 'generalized':
        ns_all, nq_all = usable_normals(src_normals), usable_normals(tgt_normals)
    it, prev = 0, (0.0, 0.0)
    while True:
        p, q32 = moved(src, T)
        nn = brute_nn(q32, tgt, max_dist)
        hit = np.flatnonzero(nn >= 0)
        d = p[hit] - tgt64[nn[hit]]
        fit = hit.size / len(src) if len(src) else 0.0
        rmse = float(np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum() / hit.size)) if hit.size else 0.0
        if it > 0 and abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
        if it >= max_iteration or hit.size < (6 if method == 'generalized' else 3):
            break
        if method == 'generalized':
            x = step_generalized(p[hit], tgt64[nn[hit]], ns_all[hit], nq_all[nn[hit]], T[:3, :3], epsilon)
            if x is None:
                break
            dT = np.eye(4)
            dT[:3, :3], dT[:3, 3] = rot(x[0], x[1], x[2]), x[3:]
        else:
            dT = step_kabsch(p[hit], tgt64[nn[hit]])
        T = dT @ T
        it += 1
        prev = (fit, rmse)
    return dict(T=T, fitness=fit, inlier_rmse=rmse, iterations=it, correspondences=np.stack([hit, nn[hit]], 1))


def pose_error(T, T_true):
    """-> (rotation error in degrees, translation error in metres)"""
    c = (np.trace(T[:3, :3].T @ T_true[:3, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
