"""TEST INFRASTRUCTURE: a float64 numpy restatement of voxelized Generalized ICP as include/buffer_hip.h (N9) specifies it (csrc/vgicp.hip):
the voxel map as a dictionary of voxels with sequential sums in input order, and the registration loop with numpy's inverse and solve.
Host code only.

The scene is tests/gicp_ref.py's with np.float32(0.1) added to every coordinate of source and target in fp32: the walls then sit
mid-voxel at voxel 0.2 (at the original coordinates they lie on voxel faces, where 1 mm of noise decides the voxel).  With o the
offset, the planted pose becomes Tr(o) T Tr(-o)."""
import numpy as np

import gicp_ref

VOXEL = 0.2
EPSILON = 1e-3
KLIM = 1 << 20
OFFSETS = {1: [(0, 0, 0)],
           7: [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
           27: [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]}

_SCENE = []


def scene():
    """-> gicp_ref.scene() moved by +0.1 on every axis (fp32 sum), T = Tr(o) T Tr(-o); made once, shared: callers copy before they write"""
    if not _SCENE:
        sc = gicp_ref.scene()
        o = np.float32(0.1)
        Tr = np.eye(4)
        Tr[:3, 3] = float(o)
        Ti = np.eye(4)
        Ti[:3, 3] = -float(o)
        out = dict(src=sc['src'] + o, tgt=sc['tgt'] + o, src_normals=sc['src_normals'], tgt_normals=sc['tgt_normals'], T=Tr @ sc['T'] @ Ti)
        for v in out.values():
            v.setflags(write=False)
        _SCENE.append(out)
    return _SCENE[0]


def start():
    """the start pose of tests/test_gicp_gpu.py: a few milliradians / millimetres off the identity"""
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = gicp_ref.rot(0.004, -0.003, 0.005), [0.004, 0.002, -0.003]
    return T0


def voxel_of(p, voxel):
    """p f64[n,3] -> (k int64[n,3], ok bool[n]): k = floor(p / voxel), ok = finite and every |k| < 2^20"""
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        kd = np.floor(np.asarray(p, np.float64) / float(voxel))
        ok = (np.abs(kd) < KLIM).all(1)                                    # (NaN and inf fail the comparison)
    return np.where(ok[:, None], kd, 0.0).astype(np.int64), ok


def key_of(k):
    return ((int(k[2]) + KLIM) << 42) | ((int(k[1]) + KLIM) << 21) | (int(k[0]) + KLIM)


def build_map(pts, normals, voxel, epsilon=EPSILON):
    """one cloud -> dict(keys int64[R], counts int32[R], means f64[R,3], covs f64[R,6], index {(kx,ky,kz): row}, voxel, epsilon): rows in
    ascending key order, sums sequential in input order"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    nrm = gicp_ref.usable_normals(normals) if normals is not None else np.zeros_like(pts)
    w = 1.0 - float(epsilon)
    k, ok = voxel_of(pts, voxel)
    cells = {}
    for i in np.flatnonzero(ok):
        cells.setdefault(tuple(int(c) for c in k[i]), []).append(i)
    order = sorted(cells, key=key_of)
    R = len(order)
    keys, counts = np.zeros(R, np.int64), np.zeros(R, np.int32)
    means, covs = np.zeros((R, 3)), np.zeros((R, 6))
    for r, c in enumerate(order):
        sm, sc = np.zeros(3), np.zeros(6)
        for i in cells[c]:
            n = nrm[i]
            sm = sm + pts[i]
            C = [(1.0 if a == b else 0.0) - (w * n[a]) * n[b] for a in range(3) for b in range(a, 3)]
            sc = sc + np.array(C)
        N = float(len(cells[c]))
        keys[r], counts[r], means[r], covs[r] = key_of(c), len(cells[c]), sm / N, sc / N
    return dict(keys=keys, counts=counts, means=means, covs=covs, index={c: r for r, c in enumerate(order)}, voxel=float(voxel),
                epsilon=float(epsilon))


def _sym(c6):
    return np.array([[c6[0], c6[1], c6[2]], [c6[1], c6[3], c6[4]], [c6[2], c6[4], c6[5]]])


def terms(src, src_normals, vmap, T, neighbors):
    """one pass -> dict(p f64[n,3], rows int64[n] (own voxel's row or -1), pt int64[t] / row int64[t] (the terms: source point, map row, in
    point then offset order), k int64[n,3], ok bool[n])"""
    p, _ = gicp_ref.moved(src, T)
    k, ok = voxel_of(p, vmap['voxel'])
    rows = np.full(len(p), -1, np.int64)
    pt, row = [], []
    for i in np.flatnonzero(ok):
        kk = tuple(int(c) for c in k[i])
        rows[i] = vmap['index'].get(kk, -1)
        for d in OFFSETS[neighbors]:
            r = vmap['index'].get((kk[0] + d[0], kk[1] + d[1], kk[2] + d[2]), -1)
            if r >= 0:
                pt.append(i)
                row.append(r)
    return dict(p=p, rows=rows, pt=np.array(pt, np.int64), row=np.array(row, np.int64), k=k, ok=ok)


def step(t, src_normals, vmap, T):
    """the Gauss-Newton system of one pass's terms -> (H f64[6,6], g f64[6])"""
    w = 1.0 - vmap['epsilon']
    R = T[:3, :3]
    p = t['p'][t['pt']]
    ns = gicp_ref.usable_normals(src_normals)[t['pt']] if src_normals is not None else np.zeros_like(p)
    I = np.eye(3)
    Cs = I - w * ns[:, :, None] * ns[:, None, :]
    Cv = np.stack([_sym(c) for c in vmap['covs'][t['row']]]) if len(p) else np.zeros((0, 3, 3))
    M = np.linalg.inv(Cv + R @ Cs @ R.T)
    J = np.concatenate([-gicp_ref._skew(p), np.broadcast_to(I, (len(p), 3, 3))], 2)
    N = vmap['counts'][t['row']].astype(np.float64)
    JtM = np.einsum('kij,kil->kjl', J, M) * N[:, None, None]
    H = np.einsum('kjl,klm->jm', JtM, J)
    g = np.einsum('kjl,kl->j', JtM, p - vmap['means'][t['row']])
    return H, g


def vgicp(src, vmap, neighbors=7, src_normals=None, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, trace=None):
    """The loop of k_vg_terms / k_vg_update for one pair -> dict(T, fitness, inlier_rmse, iterations, rows int64[n], terms, solvable).
    trace: a list that receives, per pass, dict(p, k, ok, dfit, drmse, stopped) for the margin conditions of the exact comparisons."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).reshape(4, 4).copy()
    it, prev, solvable = 0, (0.0, 0.0), True
    while True:
        t = terms(src, src_normals, vmap, T, neighbors)
        nt = len(t['pt'])
        d = t['p'][t['pt']] - vmap['means'][t['row']] if nt else np.zeros((0, 3))
        fit = len(np.unique(t['pt'])) / len(src) if len(src) else 0.0
        rmse = float(np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum() / nt)) if nt else 0.0
        conv = it > 0 and abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse
        if trace is not None:
            trace.append(dict(p=t['p'], k=t['k'], ok=t['ok'], dfit=abs(prev[0] - fit), drmse=abs(prev[1] - rmse), it=it, stopped=conv))
        if conv or it >= max_iteration or nt < 6:
            break
        x = gicp_ref._solve(*step(t, src_normals, vmap, T))
        if x is None:
            solvable = False
            break
        dT = np.eye(4)
        dT[:3, :3], dT[:3, 3] = gicp_ref.rot(x[0], x[1], x[2]), x[3:]
        T = dT @ T
        it += 1
        prev = (fit, rmse)
    return dict(T=T, fitness=fit, inlier_rmse=rmse, iterations=it, rows=t['rows'], terms=nt, solvable=solvable)


def face_margin(trace, voxel):
    """smallest distance, in voxels, of a transformed finite coordinate from a voxel face over all passes of a trace"""
    m = np.inf
    for t in trace:
        q = t['p'][t['ok']] / voxel
        if q.size:
            m = min(m, float(np.abs(q - np.round(q)).min()))
    return m


def stop_margin(trace, relative_rmse=1e-6):
    """smallest |(|d rmse|) - relative_rmse| over the passes after the first update: how far every stop decision was from flipping"""
    return min([abs(t['drmse'] - relative_rmse) for t in trace if t['it'] > 0] or [np.inf])


# the hand-computed map of the tests: voxel 0.25; x = 0.5, -0.25, 0.0, -0.0 lie exactly on faces and land in voxels 2, -1, 0, 0
HAND_VOXEL = 0.25
HAND_POINTS = np.array([[0.5, 0.0, 0.0],            # voxel (2, 0, 0)
                        [-0.25, 0.0, 0.0],          # voxel (-1, 0, 0): a face belongs to the voxel above it
                        [0.0, 0.0, 0.0],            # voxel (0, 0, 0)
                        [-0.0, -0.0, -0.0],         # voxel (0, 0, 0) as well
                        [-0.125, 0.0, 0.0],         # a negative coordinate inside voxel (-1, 0, 0)
                        [np.nan, 0.0, 0.0],         # left out
                        [0.0, 0.25 * (1 << 20), 0.0],   # |k| = 2^20: left out
                        [0.0, -0.25 * (1 << 20), 0.0],  # k = -2^20: left out
                        [0.0, 0.25 * ((1 << 20) - 1), 0.0],   # k = 2^20 - 1: the last voxel kept
                        [0.0, 0.0, -0.25],          # voxel (0, 0, -1): the lowest key
                        [0.0, 0.3, 0.0]], np.float32)     # voxel (0, 1, 0)
HAND_KEYS = [(0, 0, -1), (-1, 0, 0), (0, 0, 0), (2, 0, 0), (0, 1, 0), (0, (1 << 20) - 1, 0)]     # ascending key: z, then y, then x
HAND_COUNTS = [1, 2, 2, 1, 1, 1]
