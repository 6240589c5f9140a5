"""Synthetic fragment pairs of 3DMatch / KITTI shape.

The datasets are not available offline, so the benchmark and the parity tests
run on seeded synthetic scenes that reproduce the *shape* of what
ThreeDMatch/dataset.py:80-162 hands to the collate function: a 2.5 cm
("fds", patch support) and a 3.5 cm ("sds", + unit normals oriented to the
sensor at the origin) voxel cloud per fragment, randomly permuted, plus the
ground-truth pose src -> tgt.

Host-side numpy only: this is input generation, not part of the hot path.
"""
import numpy as np


def voxel_down_sample(pts, voxel):
    """Voxel-centroid downsample (stand-in for open3d's voxel_down_sample)."""
    if pts.shape[0] == 0:
        return pts
    mn = pts.min(0)
    key = np.floor((pts - mn) / voxel).astype(np.int64)
    dims = key.max(0) + 1
    flat = key[:, 0] + dims[0] * (key[:, 1] + dims[1] * key[:, 2])
    uniq, inv, cnt = np.unique(flat, return_inverse=True, return_counts=True)
    out = np.zeros((uniq.shape[0], pts.shape[1]), np.float64)
    np.add.at(out, inv, pts)
    return out / cnt[:, None]


def random_rotation(rng, max_angle=np.pi):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _rect(origin, eu, ev, normal):
    return dict(o=np.asarray(origin, float), u=np.asarray(eu, float), v=np.asarray(ev, float),
                n=np.asarray(normal, float))


def make_scene(rng, size=(3.0, 3.0, 2.5), n_boxes=6):
    """Room corner (floor + two walls) plus a few boxes: a list of rectangles."""
    sx, sy, sz = size
    rects = [
        _rect([0, 0, 0], [sx, 0, 0], [0, sy, 0], [0, 0, 1]),      # floor
        _rect([0, 0, 0], [sx, 0, 0], [0, 0, sz], [0, 1, 0]),      # wall y=0
        _rect([0, 0, 0], [0, sy, 0], [0, 0, sz], [1, 0, 0]),      # wall x=0
    ]
    for _ in range(n_boxes):
        w, d, h = rng.uniform(0.25, 0.9, 3)
        x0 = rng.uniform(0.05, sx - w - 0.05)
        y0 = rng.uniform(0.05, sy - d - 0.05)
        z0 = 0.0 if rng.random() < 0.7 else rng.uniform(0.3, 1.2)
        rects += [
            _rect([x0, y0, z0 + h], [w, 0, 0], [0, d, 0], [0, 0, 1]),
            _rect([x0, y0, z0], [w, 0, 0], [0, 0, h], [0, -1, 0]),
            _rect([x0, y0 + d, z0], [w, 0, 0], [0, 0, h], [0, 1, 0]),
            _rect([x0, y0, z0], [0, d, 0], [0, 0, h], [-1, 0, 0]),
            _rect([x0 + w, y0, z0], [0, d, 0], [0, 0, h], [1, 0, 0]),
        ]
    return rects


def sample_scene(rng, rects, n, jitter=0.003):
    area = np.array([np.linalg.norm(np.cross(r['u'], r['v'])) for r in rects])
    which = rng.choice(len(rects), size=n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    o = np.stack([rects[i]['o'] for i in which])
    u = np.stack([rects[i]['u'] for i in which])
    v = np.stack([rects[i]['v'] for i in which])
    nrm = np.stack([rects[i]['n'] for i in which])
    pts = o + a[:, None] * u + b[:, None] * v + rng.normal(scale=jitter, size=(n, 3))
    return pts, nrm


def _with_normals(rng, pts, nrm, sensor):
    """Unit normals oriented towards the sensor (+ small jitter), like
    estimate_normals + orient_normals_towards_camera_location (dataset.py:142-153)."""
    nrm = nrm + rng.normal(scale=0.02, size=nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    flip = np.sum(nrm * (sensor[None] - pts), axis=1) < 0
    nrm[flip] *= -1
    return nrm


def make_pair(seed, n_raw=250_000, fds_voxel=0.025, sds_voxel=0.035, overlap=0.7, size=(1.9, 1.9, 1.7),
              n_boxes=5, max_num_pts=30000):
    """One fragment pair in the sample-dict format of ThreeDMatch/dataset.py:155-161.

    Returns dict(src_fds_pts f64[Nf,3], tgt_fds_pts, src_sds_pts f64[n,6], tgt_sds_pts, relt_pose f64[4,4]).
    Both fragments are expressed in their own sensor frame (sensor at the origin).
    """
    rng = np.random.default_rng(seed)
    rects = make_scene(rng, size, n_boxes)
    out = {}
    sx = size[0]
    # the two fragments see overlapping slabs of the room along x
    width = sx / (2 - overlap)
    windows = [(0.0, width), (sx - width, sx)]
    sensors = [np.array([0.55 * width, 0.6 * size[1], 0.5 * size[2]]),
               np.array([sx - 0.55 * width, 0.55 * size[1], 0.55 * size[2]])]
    poses = []
    for name, (lo, hi), sensor in zip(('src', 'tgt'), windows, sensors):
        pts, nrm = sample_scene(rng, rects, n_raw)
        keep = (pts[:, 0] >= lo) & (pts[:, 0] <= hi)
        pts, nrm = pts[keep], nrm[keep]
        # world -> sensor frame
        R = random_rotation(rng, np.pi if name == 'tgt' else 0.3)
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ sensor
        poses.append(T)
        both = np.concatenate([pts, nrm], 1)
        fds = voxel_down_sample(both, fds_voxel)
        sds = voxel_down_sample(fds, sds_voxel)
        fds_p = fds[:, :3] @ R.T + T[:3, 3]
        sds_p = sds[:, :3] @ R.T + T[:3, 3]
        sds_n = _with_normals(rng, sds_p, sds[:, 3:] @ R.T, np.zeros(3))
        rng.shuffle(fds_p)
        perm = rng.permutation(sds_p.shape[0])
        sds_p, sds_n = sds_p[perm], sds_n[perm]
        if sds_p.shape[0] > max_num_pts:
            sds_p, sds_n = sds_p[:max_num_pts], sds_n[:max_num_pts]
        out[f'{name}_fds_pts'] = fds_p
        out[f'{name}_sds_pts'] = np.concatenate([sds_p, sds_n], 1)
    out['relt_pose'] = poses[1] @ np.linalg.inv(poses[0])
    out['src_id'] = f'synth/{seed}_0'
    out['tgt_id'] = f'synth/{seed}_1'
    return out


def make_config1_pair(seed=7, n=5000):
    """BASELINE config #1: two clouds of exactly n points on three
    mutually orthogonal faces, sigma = 3 mm jitter, all coordinates > 0.4 m;
    tgt = rigid transform of an independent sample (||t|| <= 1 m)."""
    rng = np.random.default_rng(seed)
    rects = make_scene(rng, (2.0, 2.0, 2.0), n_boxes=0)

    def cloud():
        p, nrm = sample_scene(rng, rects, n)
        return p + 0.45, nrm

    src, src_n = cloud()
    tgt, tgt_n = cloud()
    R = random_rotation(rng, 0.5)
    t = rng.normal(size=3)
    t *= rng.uniform(0, 1) / np.linalg.norm(t)
    c = tgt.mean(0)
    tgt = (tgt - c) @ R.T + c + t
    tgt_n = tgt_n @ R.T
    tgt = tgt - np.minimum(tgt.min(0) - 0.45, 0)
    pose = np.eye(4)
    pose[:3, :3] = R
    pose[:3, 3] = c + t - R @ c
    return dict(src_fds_pts=src.copy(), tgt_fds_pts=tgt.copy(),
                src_sds_pts=np.concatenate([src, _with_normals(rng, src, src_n, np.zeros(3))], 1),
                tgt_sds_pts=np.concatenate([tgt, _with_normals(rng, tgt, tgt_n, np.zeros(3))], 1),
                relt_pose=pose, src_id='config1/src', tgt_id='config1/tgt')


def make_kitti_pair(seed, beams=64, az_steps=1900, fds_voxel=0.05, sds_voxel=0.30, raw=False):
    """Ring-pattern LiDAR scans (~120k returns) over a ground plane with boxes.  raw=True adds the scans
    before voxelisation as src_raw / tgt_raw (f64[n,3], each in its own sensor frame); the other entries are unchanged."""
    rng = np.random.default_rng(seed)
    boxes = [(rng.uniform(-60, 60), rng.uniform(-60, 60), rng.uniform(2, 10), rng.uniform(2, 10),
              rng.uniform(1.5, 6)) for _ in range(40)]
    out = {}
    poses = []
    for name, pos in (('src', np.zeros(3)), ('tgt', np.array([rng.uniform(5, 10), rng.uniform(-1, 1), 0.0]))):
        el = np.deg2rad(np.linspace(-24.8, 2.0, beams))
        az = np.linspace(0, 2 * np.pi, az_steps, endpoint=False)
        E, A = np.meshgrid(el, az, indexing='ij')
        d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
        h = 1.73
        o = pos + np.array([0, 0, h])
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(d[:, 2] < 0, -o[2] / d[:, 2], np.inf)
        for (bx, by, w, l, hh) in boxes:
            lo = np.array([bx - w / 2, by - l / 2, 0.0])
            hi = np.array([bx + w / 2, by + l / 2, hh])
            with np.errstate(divide='ignore', invalid='ignore'):
                t1 = (lo - o) / d
                t2 = (hi - o) / d
            tn = np.nanmax(np.minimum(t1, t2), 1)
            tf = np.nanmin(np.maximum(t1, t2), 1)
            hit = (tn < tf) & (tn > 0)
            t = np.where(hit & (tn < t), tn, t)
        ok = (t > 3) & (t < 80)
        pts = o + d[ok] * t[ok, None] + rng.normal(scale=0.01, size=(ok.sum(), 3))
        yaw = rng.uniform(-0.1, 0.1) if name == 'tgt' else 0.0
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ o
        poses.append(T)
        p = pts @ R.T + T[:3, 3]
        if raw:
            out[f'{name}_raw'] = p
        fds = voxel_down_sample(p, fds_voxel)
        sds = voxel_down_sample(fds, sds_voxel)
        nrm = np.tile(np.array([[0, 0, 1.0]]), (sds.shape[0], 1))
        rng.shuffle(fds)
        sds = sds[rng.permutation(sds.shape[0])]
        out[f'{name}_fds_pts'] = fds
        out[f'{name}_sds_pts'] = np.concatenate([sds, _with_normals(rng, sds, nrm, np.zeros(3))], 1)
    out['relt_pose'] = poses[1] @ np.linalg.inv(poses[0])
    out['src_id'] = f'kitti_synth/{seed}_0'
    out['tgt_id'] = f'kitti_synth/{seed}_1'
    return out


def make_raw_pair_device(seed, overlap, device, n_raw=250_000, size=(1.9, 1.9, 1.7), n_boxes=5, jitter=0.003):
    """A fragment pair as RAW (un-voxelised) clouds in device memory: what a 3DMatch .ply holds before
    ThreeDMatch/dataset.py:91-153 voxelises it.  Same room / window / sensor construction as make_pair(); the scene
    comes from the seeded numpy generator, the ~n_raw surface samples per fragment from a seeded torch generator on the
    device (a 1623-pair stream is a few seconds of generation instead of minutes).
    -> dict(src_raw f32[n,3], tgt_raw f32[m,3] (device, each in its own sensor frame), relt_pose f64[4,4] numpy src->tgt,
            overlap_pts f32[k,3] (device): tgt-frame points of the shared slab, for the RMSE-proxy information matrix)."""
    import torch
    rng = np.random.default_rng(seed)
    rects = make_scene(rng, size, n_boxes)
    g = torch.Generator(device=device).manual_seed(int(seed))
    o = torch.tensor(np.stack([r['o'] for r in rects]), dtype=torch.float32, device=device)
    u = torch.tensor(np.stack([r['u'] for r in rects]), dtype=torch.float32, device=device)
    v = torch.tensor(np.stack([r['v'] for r in rects]), dtype=torch.float32, device=device)
    area = torch.linalg.norm(torch.linalg.cross(u, v), dim=1)
    sx = size[0]
    width = sx / (2 - overlap)
    windows = [(0.0, width), (sx - width, sx)]
    sensors = [np.array([0.55 * width, 0.6 * size[1], 0.5 * size[2]]), np.array([sx - 0.55 * width, 0.55 * size[1], 0.55 * size[2]])]
    out, poses = {}, []
    for name, (lo, hi), sensor in zip(('src', 'tgt'), windows, sensors):
        which = torch.multinomial(area / area.sum(), n_raw, replacement=True, generator=g)
        ab = torch.rand((n_raw, 2), generator=g, device=device)
        pts = o[which] + ab[:, :1] * u[which] + ab[:, 1:] * v[which] + jitter * torch.randn((n_raw, 3), generator=g, device=device)
        pts = pts[(pts[:, 0] >= lo) & (pts[:, 0] <= hi)]
        R = random_rotation(rng, np.pi if name == 'tgt' else 0.3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, -R @ sensor
        poses.append(T)
        Rt = torch.tensor(R, dtype=torch.float32, device=device)
        tt = torch.tensor(T[:3, 3], dtype=torch.float32, device=device)
        if name == 'tgt':
            shared = pts[(pts[:, 0] >= windows[1][0]) & (pts[:, 0] <= windows[0][1])]
            out['overlap_pts'] = (shared[:: max(1, shared.shape[0] // 4096)] @ Rt.T + tt).contiguous()
        out[f'{name}_raw'] = (pts @ Rt.T + tt).contiguous()
    out['relt_pose'] = poses[1] @ np.linalg.inv(poses[0])
    return out


def _eth_primitives(rng, kind, half):
    """The surfaces of one outdoor scene: (ground height function, list of (area weight, sampler(rng, n) -> f64[n,3]))."""
    gx, gy = rng.uniform(-0.08, 0.08, 2)
    p1, p2 = rng.uniform(0, 2 * np.pi, 2)

    def h(x, y):                                                     # sloped, gently rolling ground
        return gx * x + gy * y + 0.25 * np.sin(0.21 * x + p1) * np.cos(0.17 * y + p2)

    def ground(rng, n):
        x, y = rng.uniform(-half, half, (2, n))
        return np.stack([x, y, h(x, y)], 1)

    def cylinder(cx, cy, r, height):                                 # trunk or post
        z0 = h(cx, cy)

        def f(rng, n):
            a, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, height, n)
            return np.stack([cx + r * np.cos(a), cy + r * np.sin(a), z0 + z], 1)
        return 2 * np.pi * r * height, f

    def blob(c, radii):                                              # canopy / shrub: points filling an ellipsoid, denser outside
        def f(rng, n):
            d = rng.normal(size=(n, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            return c + d * radii * rng.uniform(0, 1, (n, 1)) ** 0.25
        return 4 * np.pi * float(np.mean(radii)) ** 2, f

    def wall(x0, y0, ang, length, height):
        d = np.array([np.cos(ang), np.sin(ang)])

        def f(rng, n):
            s, t = rng.uniform(0, length, n), rng.uniform(0, height, n)
            x, y = x0 + s * d[0], y0 + s * d[1]
            return np.stack([x, y, h(x, y) + t], 1)
        return length * height, f

    prims = [((2 * half) ** 2, ground)]
    if kind == 'wood':
        for _ in range(70):
            cx, cy = rng.uniform(-half, half, 2)
            r, H = rng.uniform(0.12, 0.45), rng.uniform(6, 12)
            prims.append(cylinder(cx, cy, r, H))
            prims.append(blob(np.array([cx, cy, h(cx, cy) + H + rng.uniform(-1, 1)]), rng.uniform(1.5, 3.5, 3)))
        for _ in range(40):
            cx, cy = rng.uniform(-half, half, 2)
            prims.append(blob(np.array([cx, cy, h(cx, cy) + 0.4]), rng.uniform(0.4, 1.2, 3)))
    else:
        for _ in range(3):                                           # gazebos: posts on a ring under a sloped roof
            cx, cy = rng.uniform(-0.6 * half, 0.6 * half, 2)
            R, H = rng.uniform(2.5, 4.5), rng.uniform(2.5, 3.2)
            for a in np.linspace(0, 2 * np.pi, 8, endpoint=False):
                prims.append(cylinder(cx + R * np.cos(a), cy + R * np.sin(a), 0.12, H))
            z = h(cx, cy) + H
            for sgn in (-1, 1):
                o, u, v = np.array([cx - R, cy, z + 1.2]), np.array([2 * R, 0, 0]), np.array([0, sgn * (R + 0.5), -1.2])

                def roof(rng, n, o=o, u=u, v=v):
                    a, b = rng.uniform(0, 1, (2, n))
                    return o + a[:, None] * u + b[:, None] * v
                prims.append((float(np.linalg.norm(np.cross(u, v))), roof))
        for _ in range(12):
            x0, y0 = rng.uniform(-half, half, 2)
            prims.append(wall(x0, y0, rng.uniform(0, np.pi), rng.uniform(4, 15), rng.uniform(1.5, 4)))
        for _ in range(15):
            cx, cy = rng.uniform(-half, half, 2)
            prims.append(cylinder(cx, cy, rng.uniform(0.1, 0.3), rng.uniform(4, 9)))
    return h, prims


def make_eth_root(root, scenes=('gazebo_summer', 'wood_autmn'), stations=3, seed=0, n_raw=120_000, max_range=30.0, half=35.0,
                  spacing=9.0, non_finite_rows=0):
    """A mini ETH test set in the reference's layout (generalization/ThreeD2ETH/dataset.py:34-52): per scene `stations` terrestrial
    scans written as <root>/<scene>/Hokuyo_<k>.ply (f32, each in its own scanner frame) and a tab-separated gt.log (the format
    plyio.load_gt_log parses) with every pair i < j: T_i @ inv(T_j), T_k = world -> scan k, so that inv(gt) maps scan i
    (source) into scan j (target).  Outdoor geometry: sloped ground over a 2*half m square; trunks with canopy clusters and shrubs for
    `wood_*` scenes, gazebo posts and roofs, walls and poles otherwise.  Scanners stand `spacing` m apart on a line, 1.6 m above the
    ground, yaw uniform, tilt <= 2 degrees; each sees up to `max_range` m with a point density falling off as 1/r (overlap is
    partial), about n_raw returns, 1 cm range noise.  non_finite_rows > 0 appends that many NaN / inf rows to every scan (open3d's
    reader drops them; so must ETHTestSet).  -> {scene: [T_k f64[4,4]]}.  Host-side numpy only."""
    import os

    from .plyio import write_ply
    rng = np.random.default_rng(seed)
    out = {}
    for scene in scenes:
        h, prims = _eth_primitives(rng, 'wood' if scene.startswith('wood') else 'gazebo', half)
        area = np.array([a for a, _ in prims])
        a0 = rng.uniform(0, 2 * np.pi)
        c0 = rng.uniform(-5, 5, 2) - 0.5 * (stations - 1) * spacing * np.array([np.cos(a0), np.sin(a0)])
        poses = []
        for k in range(stations):
            sxy = c0 + k * spacing * np.array([np.cos(a0), np.sin(a0)]) + rng.uniform(-1.5, 1.5, 2)
            s = np.array([sxy[0], sxy[1], h(sxy[0], sxy[1]) + 1.6])
            counts = rng.multinomial(5 * n_raw, area / area.sum())
            pts = np.concatenate([f(rng, int(c)) for (_, f), c in zip(prims, counts) if c])
            d = pts - s
            r = np.linalg.norm(d, axis=1)
            keep = (r > 1.0) & (r < max_range) & (rng.uniform(0, 1, r.shape[0]) < np.minimum(1.0, 6.0 / np.maximum(r, 1e-9)))
            pts, d, r = pts[keep], d[keep], r[keep]
            pts = pts + d / r[:, None] * rng.normal(scale=0.01, size=(r.shape[0], 1))      # range noise along the beam
            if pts.shape[0] > n_raw:
                pts = pts[np.sort(rng.choice(pts.shape[0], n_raw, replace=False))]
            tilt = random_rotation(rng, np.deg2rad(2.0))
            yaw = rng.uniform(-np.pi, np.pi)
            R = tilt @ np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, -R @ s
            poses.append(T)
            scan = (pts @ R.T + T[:3, 3]).astype(np.float32)
            if non_finite_rows:
                bad = np.tile(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32), (non_finite_rows // 3 + 1, 1))
                at = np.sort(rng.choice(scan.shape[0], non_finite_rows, replace=False))
                scan = np.insert(scan, at, bad[:non_finite_rows], axis=0)
            write_ply(os.path.join(root, scene, f'Hokuyo_{k}.ply'), scan)
        with open(os.path.join(root, scene, 'gt.log'), 'w') as f:
            for i in range(stations):
                for j in range(i + 1, stations):
                    G = poses[i] @ np.linalg.inv(poses[j])
                    f.write(f'{i}\t{j}\t{stations}\n')
                    for row in G:
                        f.write('\t'.join(repr(float(x)) for x in row) + '\n')
        out[scene] = poses
    return out


def information_matrix(points):
    """6x6 information matrix of a set of overlap points p (fragment-j frame), in the convention of the 3DMatch
    gt.info files that ThreeDMatch/test.py:92-111 consumes: for er = [t, q_xyz] (translation and quaternion vector part of
    a small residual transform) the displacement of p is t + 2 q x p = [I, -2[p]x] er, so  er^T (sum J^T J) er / info[0,0]
    is the mean squared displacement over the overlap -- the RMSE proxy thresholded at 0.2^2 by the RR metric."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    J = np.zeros((p.shape[0], 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    J[:, 0, 4], J[:, 0, 5] = 2 * p[:, 2], -2 * p[:, 1]
    J[:, 1, 3], J[:, 1, 5] = -2 * p[:, 2], 2 * p[:, 0]
    J[:, 2, 3], J[:, 2, 4] = 2 * p[:, 1], -2 * p[:, 0]
    return np.einsum('nij,nik->jk', J, J)
