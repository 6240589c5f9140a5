"""Pair statistics on the device: overlap ratio, inlier RMSE and the 6x6 information matrix of fragment pairs under given poses, and
the tool that makes a 3DMatch-layout ground truth (gt.log, gt.info) from fragments and poses.

    pair_statistics     P pairs over C shared clouds in one call (csrc/pairstats.hip, buf_pair_stats: one cell grid per call)
    information_matrix  the 6x6 matrix from a pair's moments, in the gt.info or the open3d convention (host, fp64)
    scene_pairs         all pairs of a scene's fragments picked by overlap, with pose and information matrix
    write_gt            gt.log / gt.info / gt_overlap.json in the layout ThreeDMatchTestSet reads
    dataset_overlaps    the overlap of the pairs of any of the three test sets; overlap_report: the drivers' --by-overlap

Overlap of a pair = the smaller of the two directional ratios "points of one voxelised fragment that have a point of the other
within `radius` under the ground-truth pose" (voxel = the configuration's `downsample`, radius = 1.5 voxel by default).  This is the
definition in common use for the 3DMatch / 3DLoMatch bands (>= 30 %, 10-30 %), restated from memory: unpinned.

    python -m buffer_amd.pairs --root R --scene S [--poses FILE] [--dataset 3DMatch|3DLoMatch] [--min-overlap 0.3] [--max-overlap 1.0]
                               [--voxel V] [--radius r] [--force]
"""
import json
import os

import numpy as np
import torch

from . import _lib, ops

BANDS = ((0.0, 0.1), (0.1, 0.3), (0.3, 0.6), (0.6, 1.0))      # [lo, hi), the last one closed
DATASET_BANDS = {'3DMatch': (0.3, 1.0), '3DLoMatch': (0.1, 0.3)}
TABLE_CELLS = 1 << 28                                          # cell-table budget of one call (int32 cells: 1 GiB)
ROWS_PER_CALL = 1 << 30                                        # source rows of one call (int32 indices in the library)


def _needed_cells(boxes, radius):
    """cells of the dense table a cloud's box needs at cell edge = radius (buf_grid_build's own rule) -> int64[C]"""
    ext = np.maximum(boxes[:, 1] - boxes[:, 0], 0.0)
    return np.prod(np.floor(ext / (radius * 1.00001)) + 1.0, axis=1).astype(np.int64)


def bounding_boxes(clouds):
    """finite-row bounding boxes of device clouds -> f64[C,2,3] (min, max) on the host, one readback; an empty cloud gives zeros"""
    out = []
    for c in clouds:
        c = c.reshape(-1, 3)
        c = c[torch.isfinite(c).all(1)]
        out.append(torch.stack([c.amin(0), c.amax(0)]).double() if c.shape[0] else torch.zeros((2, 3), dtype=torch.float64, device=c.device))
    return torch.stack(out).cpu().numpy() if out else np.zeros((0, 2, 3))


def boxes_within(box_a, box_b, T, radius):
    """May a point of box_b (f64[2,3] min / max), moved by T into the frame of box_a, lie within `radius` of a point of box_a?
    The 8 corners of box_b are transformed and their axis-aligned hull compared with box_a: a gap wider than the radius along any
    axis means no match is possible.  Conservative (a small slack covers the fp32 rounding of the search point): False only for
    pairs that certainly have no match."""
    box_a, box_b, T = np.asarray(box_a, np.float64), np.asarray(box_b, np.float64), np.asarray(T, np.float64)
    corners = np.array([[box_b[(k >> 0) & 1, 0], box_b[(k >> 1) & 1, 1], box_b[(k >> 2) & 1, 2]] for k in range(8)])
    moved = corners @ T[:3, :3].T + T[:3, 3]
    lo, hi = moved.min(0), moved.max(0)
    slack = radius * 1.001 + 1e-5 * (1.0 + np.abs(np.concatenate([lo, hi, box_a.ravel()])).max())
    return bool(np.all(lo - box_a[1] <= slack) and np.all(box_a[0] - hi <= slack))


def _chunks(pairs, lengths, max_clouds):
    """pair indices split so that one call holds at most max_clouds distinct clouds and ROWS_PER_CALL source rows"""
    out, cur, clouds, rows = [], [], set(), 0
    for k, (a, b) in enumerate(pairs):
        new = clouds | {a, b}
        if cur and (len(new) > max_clouds or rows + lengths[a] > ROWS_PER_CALL):
            out.append(cur)
            cur, new, rows = [], {a, b}, 0
        cur.append(k)
        clouds = new
        rows += lengths[a]
    if cur:
        out.append(cur)
    return out


def pair_statistics(clouds, pairs, transforms, radius, symmetric=False, correspondences=False, table_cells=TABLE_CELLS):
    """Statistics of P pairs under given transforms.  clouds: list of f32[n_c,3] device tensors; pairs: P (a, b) cloud indices;
    transforms f64[P,4,4]: T_k maps cloud a_k into the frame of cloud b_k.  For every source row the nearest row of the target
    cloud within `radius` (buf_pair_stats: the arithmetic of the ICP correspondence search).
    -> dict of numpy arrays over the pairs: n_src, matched, overlap = matched / n_src (0 for an empty source), inlier_rmse =
    sqrt(sum_d2 / matched) (0 without matches), sum_d2, sum_u f64[P,3], sum_uu f64[P,6] (xx, xy, xz, yy, yz, zz) -- the moments
    of the matched TARGET points in the target cloud's frame -- and, with correspondences, nn: a list of int32[n_src] (row inside
    the target cloud, -1 = none).  symmetric=True also evaluates every pair in the other direction with inv(T) in the same call
    (2P pairs, one grid) and returns it under 'reverse' (same keys).
    All clouds named by the pairs share one cell grid per call, sized from the largest box; a job whose clouds do not fit one
    table (table_cells) is split into several calls, which does not change any result."""
    P = len(pairs)
    T = np.asarray(transforms, np.float64).reshape(P, 4, 4)
    pairs = [(int(a), int(b)) for a, b in pairs]
    if not (radius > 0 and np.isfinite(radius)):
        raise ValueError(f"pair_statistics: radius={radius} (must be finite and > 0)")
    for a, b in pairs:
        if not (0 <= a < len(clouds) and 0 <= b < len(clouds)):
            raise ValueError(f"pair_statistics: pair ({a}, {b}) names a cloud outside [0, {len(clouds)})")
    if not all(isinstance(c, torch.Tensor) and c.is_cuda for c in clouds):
        raise _lib.BufferHipError("pair_statistics: expected tensors in device memory (buffer_amd has no CPU path)")
    if symmetric:
        both = pair_statistics(clouds, pairs + [(b, a) for a, b in pairs], np.concatenate([T, np.linalg.inv(T)]) if P else T, radius,
                               correspondences=correspondences, table_cells=table_cells)
        fwd = {k: v[:P] for k, v in both.items()}
        fwd['reverse'] = {k: v[P:] for k, v in both.items()}
        return fwd
    clouds = [c.reshape(-1, 3).float() for c in clouds]
    lengths = [int(c.shape[0]) for c in clouds]
    n_src = np.array([lengths[a] for a, _ in pairs], np.int64)
    matched, moments, nn = np.zeros(P, np.int64), np.zeros((P, 10)), [None] * P
    if P:
        used = sorted({c for p in pairs for c in p})
        boxes = np.zeros((len(clouds), 2, 3))
        boxes[used] = bounding_boxes([clouds[c] for c in used])
        needed = _needed_cells(boxes, float(radius))
        need_max = int(max(needed[used].max(), 1))
        max_clouds = max(2, int(min(table_cells // need_max, len(used))))
        res = []
        for ch in _chunks(pairs, lengths, max_clouds):
            loc = sorted({c for k in ch for c in pairs[k]})
            idx = {c: i for i, c in enumerate(loc)}
            pts = torch.cat([clouds[c] for c in loc])
            default = int(_lib.lib().buf_grid_default_cells(int(pts.shape[0]), len(loc)))
            cells = min(max(default, int(needed[loc].max())), max(table_cells // len(loc), 1))     # the largest box where it fits
            dev = pts.device
            res.append((ch, ops.pair_stats(pts, [lengths[c] for c in loc], [idx[pairs[k][0]] for k in ch], [idx[pairs[k][1]] for k in ch],
                                           torch.from_numpy(T[ch]).to(dev), radius, correspondences, cells)))
        for ch, (m, mo, n) in res:                              # (read back after every call is queued)
            matched[ch], moments[ch] = m.cpu().numpy(), mo.cpu().numpy()
            if correspondences:
                n = n.cpu().numpy()
                off = np.concatenate([[0], np.cumsum(n_src[ch])])
                for i, k in enumerate(ch):
                    nn[k] = n[off[i]:off[i + 1]]
    out = dict(n_src=n_src, matched=matched,
               overlap=np.divide(matched, n_src, out=np.zeros(P), where=n_src > 0),
               inlier_rmse=np.sqrt(np.divide(moments[:, 0], matched, out=np.zeros(P), where=matched > 0)),
               sum_d2=moments[:, 0].copy(), sum_u=moments[:, 1:4].copy(), sum_uu=moments[:, 4:10].copy())
    if correspondences:
        out['nn'] = np.empty(P, dtype=object)
        for k in range(P):
            out['nn'][k] = nn[k]
    return out


def _cross(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def information_matrix(matched, sum_u, sum_uu, convention='3dmatch'):
    """The 6x6 information matrix of a pair from its moments alone (host, fp64): n = matched, s = sum u, S = sum u u^T over the
    matched target points u (sum_uu = xx, xy, xz, yy, yz, zz), [v]x the cross-product matrix.
      '3dmatch'  the gt.info convention of synth.information_matrix / evaluate.transformation_error, order [t, q_xyz]:
                 [[n I, -2 [s]x], [(-2 [s]x)^T, 4 (tr(S) I - S)]], so info[0,0] = n;
      'open3d'   get_information_matrix_from_point_clouds, order [rotation, translation] (restated from the upstream source as
                 recalled, unpinned): [[tr(S) I - S, [s]x], [[s]x^T, n I]]."""
    s = np.asarray(sum_u, np.float64).reshape(3)
    xx, xy, xz, yy, yz, zz = np.asarray(sum_uu, np.float64).reshape(6)
    S = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
    n, I = float(matched), np.eye(3)
    rot = np.array([[yy + zz, -xy, -xz], [-xy, xx + zz, -yz], [-xz, -yz, xx + yy]])      # tr(S) I - S, the diagonal without cancellation
    out = np.zeros((6, 6))
    if convention == '3dmatch':
        out[:3, :3], out[:3, 3:], out[3:, :3], out[3:, 3:] = n * I, -2.0 * _cross(s), (-2.0 * _cross(s)).T, 4.0 * rot
    elif convention == 'open3d':
        out[:3, :3], out[:3, 3:], out[3:, :3], out[3:, 3:] = rot, _cross(s), _cross(s).T, n * I
    else:
        raise ValueError(f"information_matrix: unknown convention {convention!r} ('3dmatch' or 'open3d')")
    return out


def downsample_clouds(clouds, voxel, device):
    """numpy or device clouds -> list of f32[m,3] device tensors: preprocess.voxel_down_sample_batch of all of them in one call"""
    from . import preprocess
    cl = [(c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, np.float32))).to(device).reshape(-1, 3).float()
          for c in clouds]
    if not cl:
        return []
    down, lens = preprocess.voxel_down_sample_batch(torch.cat(cl), [c.shape[0] for c in cl], voxel)
    return list(torch.split(down.float(), [int(x) for x in lens]))


def scene_pairs(fragments, world_poses, voxel=None, radius=None, min_overlap=0.3, max_overlap=1.0, device=None):
    """The pairs of a scene picked by overlap.  fragments: list of [n,3] clouds, each in its own frame; world_poses: W_k f64[4,4]
    fragment k -> world.  The fragments are voxel-down-sampled on the device (voxel: default the 3DMatch configuration's
    `downsample`; radius: default 1.5 voxel); every i < j whose bounding boxes come within `radius` under T_ij = inv(W_i) W_j is
    evaluated in both directions in ONE call; the pair's overlap is the smaller direction (module docstring: unpinned); pairs with
    min_overlap <= overlap < max_overlap are kept (max_overlap >= 1 keeps overlap 1).
    -> dict(n_fragments, voxel, radius, candidates, pairs=[dict(i, j, T = T_ij (fragment j -> fragment i, the gt.log convention),
    info = the '3dmatch' information matrix over the matched points of fragment j in j's frame (source i moved by inv(T_ij): the
    frame evaluate.evaluate_registration applies it in), overlap, overlap_i / overlap_j = the share of fragment i / j that is
    matched, matched_i, matched_j, inlier_rmse)] ascending by (i, j))."""
    from .config import THREEDMATCH
    voxel = float(THREEDMATCH.downsample if voxel is None else voxel)
    radius = float(1.5 * voxel if radius is None else radius)
    n = len(fragments)
    if len(world_poses) != n:
        raise ValueError(f"scene_pairs: {n} fragments but {len(world_poses)} poses")
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    W = [np.asarray(w, np.float64).reshape(4, 4) for w in world_poses]
    down = downsample_clouds(fragments, voxel, device)
    boxes = bounding_boxes(down)
    cand, Ts = [], []
    for i in range(n):
        Wi = np.linalg.inv(W[i])
        for j in range(i + 1, n):
            Tij = Wi @ W[j]
            if down[i].shape[0] and down[j].shape[0] and boxes_within(boxes[i], boxes[j], Tij, radius):
                cand.append((i, j))
                Ts.append(Tij)
    # forward: source j -> target i under T_ij; reverse: source i -> target j under inv(T_ij) (its matched points are fragment j's)
    st = pair_statistics(down, [(j, i) for i, j in cand], np.array(Ts).reshape(-1, 4, 4), radius, symmetric=True)
    rv = st.get('reverse', st)
    kept = []
    for k, (i, j) in enumerate(cand):
        oj, oi = float(st['overlap'][k]), float(rv['overlap'][k])
        ov = min(oi, oj)
        if ov >= min_overlap and (ov < max_overlap or max_overlap >= 1.0):
            kept.append(dict(i=i, j=j, T=Ts[k], info=information_matrix(rv['matched'][k], rv['sum_u'][k], rv['sum_uu'][k], '3dmatch'),
                             overlap=ov, overlap_i=oi, overlap_j=oj, matched_i=int(rv['matched'][k]), matched_j=int(st['matched'][k]),
                             inlier_rmse=float(rv['inlier_rmse'][k])))
    return dict(n_fragments=n, voxel=voxel, radius=radius, candidates=len(cand), pairs=kept)


def write_gt(gt_dir, pairs, n_fragments, force=False, voxel=None, radius=None):
    """gt.log and gt.info in the formats plyio.load_gt_log, evaluate.read_trajectory and evaluate.read_trajectory_info read
    (tab-separated, repr(float)), pairs (dicts of scene_pairs: i, j, T, info) ascending by (i, j), plus gt_overlap.json (per pair
    both directional overlaps, matched counts, inlier RMSE; the voxel / radius used).  Refuses to replace an existing gt.log
    unless force."""
    log = os.path.join(gt_dir, 'gt.log')
    if os.path.exists(log) and not force:
        raise FileExistsError(f'{log} exists (pass force=True / --force to replace it)')
    pairs = sorted(pairs, key=lambda p: (int(p['i']), int(p['j'])))
    os.makedirs(gt_dir, exist_ok=True)
    with open(log, 'w') as fl, open(os.path.join(gt_dir, 'gt.info'), 'w') as fi:
        for p in pairs:
            head = f"{int(p['i'])}\t{int(p['j'])}\t{int(n_fragments)}\n"
            fl.write(head)
            for row in np.asarray(p['T'], np.float64).reshape(4, 4):
                fl.write('\t'.join(repr(float(x)) for x in row) + '\n')
            fi.write(head)
            for row in np.asarray(p['info'], np.float64).reshape(6, 6):
                fi.write('\t'.join(repr(float(x)) for x in row) + '\n')
    extra = ('overlap', 'overlap_i', 'overlap_j', 'matched_i', 'matched_j', 'inlier_rmse')
    with open(os.path.join(gt_dir, 'gt_overlap.json'), 'w') as f:
        json.dump(dict(voxel=voxel, radius=radius, n_fragments=int(n_fragments),
                       pairs=[dict(i=int(p['i']), j=int(p['j']), **{k: p[k] for k in extra if k in p}) for p in pairs]), f, indent=1)


def dataset_overlaps(dataset, indices, device, voxel=None, radius=None, batch=64):
    """The overlap (module docstring) of pairs of a test set through the drivers' common duck type: raw_pair(i) -> two clouds,
    meta(i) -> src_id, tgt_id, relt_pose (source -> target), dataset.downsample.  `batch` pairs per call; every distinct fragment
    of a call is voxelised and uploaded once.  -> f64[len(indices)]"""
    voxel = float(dataset.downsample if voxel is None else voxel)
    radius = float(1.5 * voxel if radius is None else radius)
    idx = list(indices)
    out = np.zeros(len(idx))
    for lo in range(0, len(idx), batch):
        slot, raws, prs, Ts = {}, [], [], []
        for i in idx[lo:lo + batch]:
            m, raw = dataset.meta(i, device), None
            for side, key in enumerate((m['src_id'], m['tgt_id'])):
                if key not in slot:
                    raw = dataset.raw_pair(i) if raw is None else raw
                    slot[key] = len(raws)
                    raws.append(raw[side])
            prs.append((slot[m['src_id']], slot[m['tgt_id']]))
            Ts.append(np.asarray(m['relt_pose'], np.float64))
        st = pair_statistics(downsample_clouds(raws, voxel, device), prs, np.array(Ts), radius, symmetric=True)
        out[lo:lo + len(prs)] = np.minimum(st['overlap'], st['reverse']['overlap'])
    return out


def band_of(overlap):
    """index into BANDS of an overlap ratio in [0, 1]"""
    for b, (lo, hi) in enumerate(BANDS):
        if lo <= overlap < hi:
            return b
    return len(BANDS) - 1 if overlap >= BANDS[-1][0] else 0


def overlap_report(dataset, poses, device, rte_thresh, rre_thresh, counts=None, num_keypts=None):
    """The drivers' --by-overlap: dataset_overlaps of all pairs, then per band of BANDS the pair count, the DGR recall (RTE / RRE
    under the driver's thresholds against meta(i)['relt_pose']) and, with the --stage-metrics count rows, evaluate.stage_summary
    of the band's rows.  -> (by_overlap dict keyed '[lo, hi)', overlaps f64[n])"""
    from . import evaluate
    n = len(dataset)
    ov = dataset_overlaps(dataset, range(n), device)
    ok = np.array([evaluate.dgr_success(poses[i], dataset.meta(i, device)['relt_pose'], rte_thresh, rre_thresh)[0] for i in range(n)], bool)
    band = np.array([band_of(o) for o in ov], np.int64)
    rep = {}
    for b, (lo, hi) in enumerate(BANDS):
        sel = band == b
        row = dict(pairs=int(sel.sum()), dgr_recall=float(ok[sel].mean()) if sel.any() else 0.0)
        if counts is not None:
            row['stage'] = evaluate.stage_summary(np.asarray(counts).reshape(-1, 7)[sel], num_keypts)
        rep[f'[{lo}, {hi}' + (']' if b == len(BANDS) - 1 else ')')] = row
    return rep, ov


def read_poses(path, n_fragments, frag_dir):
    """fragment -> world poses: a trajectory .log (5 lines per fragment: a header, then the 4x4) or, with path None,
    cloud_bin_<k>.pose.npy beside the fragments"""
    if path is None:
        files = [os.path.join(frag_dir, f'cloud_bin_{k}.pose.npy') for k in range(n_fragments)]
        missing = [f for f in files if not os.path.exists(f)]
        if missing:
            raise FileNotFoundError(f'no --poses given and {missing[0]} is missing')
        return [np.load(f).astype(np.float64).reshape(4, 4) for f in files]
    if not os.path.exists(path):
        raise FileNotFoundError(f'{path}: no such poses file')
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    if len(lines) % 5:
        raise ValueError(f'{path}: {len(lines)} lines, not 5 per pose')
    poses = [np.array([[float(x) for x in ln.split()[:4]] for ln in lines[k + 1:k + 5]], np.float64) for k in range(0, len(lines), 5)]
    if len(poses) != n_fragments:
        raise ValueError(f'{path}: {len(poses)} poses for {n_fragments} fragments')
    return poses


def main(argv=None):
    """python -m buffer_amd.pairs --root R --scene S [--poses FILE]: the pairs of one scene by overlap -> gt.log, gt.info,
    gt_overlap.json where ThreeDMatchTestSet reads them.  Prints one JSON line."""
    import argparse
    import time

    from .plyio import read_ply
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument('--root', required=True)
    ap.add_argument('--scene', required=True)
    ap.add_argument('--poses', default=None, help='trajectory .log of fragment -> world poses (default: cloud_bin_<k>.pose.npy beside the fragments)')
    ap.add_argument('--dataset', default='3DMatch', help='3DMatch (overlap >= 0.3) or 3DLoMatch ([0.1, 0.3))')
    ap.add_argument('--min-overlap', type=float, default=None)
    ap.add_argument('--max-overlap', type=float, default=None)
    ap.add_argument('--voxel', type=float, default=None)
    ap.add_argument('--radius', type=float, default=None)
    ap.add_argument('--force', action='store_true', help='replace an existing gt.log')
    a = ap.parse_args(argv)
    if a.dataset not in DATASET_BANDS:
        ap.error(f'unknown data set {a.dataset!r}; one of ' + ', '.join(DATASET_BANDS))
    lo = DATASET_BANDS[a.dataset][0] if a.min_overlap is None else a.min_overlap
    hi = DATASET_BANDS[a.dataset][1] if a.max_overlap is None else a.max_overlap
    frag_dir = os.path.join(a.root, 'test', '3DMatch', 'fragments', a.scene)
    n = 0
    while os.path.exists(os.path.join(frag_dir, f'cloud_bin_{n}.ply')):
        n += 1
    if n == 0:
        ap.error(f'no cloud_bin_0.ply under {frag_dir}')
    try:
        poses = read_poses(a.poses, n, frag_dir)
    except (FileNotFoundError, ValueError) as e:
        ap.error(str(e))
    gt_dir = os.path.join(a.root, 'test', '3DMatch', 'gt_result', a.scene) if a.dataset == '3DMatch' else os.path.join(a.root, 'test', a.dataset, a.scene)
    if os.path.exists(os.path.join(gt_dir, 'gt.log')) and not a.force:
        ap.error(f'{gt_dir}/gt.log exists (--force replaces it)')
    t0 = time.perf_counter()
    frags = [read_ply(os.path.join(frag_dir, f'cloud_bin_{k}.ply'), drop_non_finite=True) for k in range(n)]
    res = scene_pairs(frags, poses, a.voxel, a.radius, lo, hi)
    write_gt(gt_dir, res['pairs'], n, force=a.force, voxel=res['voxel'], radius=res['radius'])
    hist = np.bincount([band_of(p['overlap']) for p in res['pairs']], minlength=len(BANDS))
    out = dict(scene=a.scene, dataset=a.dataset, fragments=n, candidates=res['candidates'], pairs=len(res['pairs']),
               min_overlap=lo, max_overlap=hi, voxel=res['voxel'], radius=res['radius'],
               overlap_histogram={f'{b[0]}-{b[1]}': int(h) for b, h in zip(BANDS, hist)}, seconds=time.perf_counter() - t0)
    print(json.dumps(out))
    return res


if __name__ == '__main__':
    main()
