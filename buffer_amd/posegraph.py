"""Multiway registration: the fragments of a scene placed in one frame by a pose graph with line processes (Choi, Zhou, Koltun
2015), optimised on the device (csrc/posegraph.hip, buf_pose_graph_optimize: every graph of a call in one launch; the mathematics is
the contract comment in include/buffer_hip.h).  Host code here is fp64 numpy bookkeeping around that one call.

    optimize             G graphs -> optimised poses, status, costs, line-process weights, in one device call
    optimize_two_pass    optimise, prune the switched-off edges, optimise the kept ones from the first pass's poses
    initial_poses        composition along the maximum spanning tree (by matched count)
    line_process_weight  mu from the uncertain edges' information matrices
    scene_edges          registered pairs + clouds -> edges with 'open3d'-convention information matrices (one pair_statistics call)
    info_from_3dmatch, project_rigid, prune, trajectory_error, write_trajectory

Conventions: a node pose W_k maps fragment k into the world; an edge (i, j, T) holds T = inv(W_i) W_j, fragment j -> fragment i (the
gt.log convention); info is 6x6 in the order [rotation, translation] over the matched points of fragment j in j's frame."""
import numpy as np

STATUS = ('NOTHING', 'CONVERGED_STEP', 'CONVERGED_COST', 'MAX_ITER', 'STALLED', 'FAILED')      # ops.PG_STATUS
MAX_NODES = 128                                                                                 # BUF_PG_MAX_NODES


def project_rigid(T):
    """the nearest rigid transform of a 4x4 (fp32 poses of the pipeline): rotation by SVD with det +1, last row 0 0 0 1 -> f64[4,4]"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    U, _, Vt = np.linalg.svd(T[:3, :3])
    out = np.eye(4)
    out[:3, :3] = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    out[:3, 3] = T[:3, 3]
    return out


def rigid_inverse(T):
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def info_from_3dmatch(info):
    """gt.info order [t, q_xyz] -> the order [rotation, translation] of the optimiser: the qq block divided by 4, the tq blocks by 2,
    the two halves swapped (the inverse of what pairs.information_matrix documents: q = half the rotation vector)."""
    a = np.asarray(info, np.float64).reshape(6, 6)
    out = np.zeros((6, 6))
    out[:3, :3] = a[3:, 3:] / 4.0
    out[3:, 3:] = a[:3, :3]
    out[:3, 3:] = a[3:, :3] / 2.0
    out[3:, :3] = a[:3, 3:] / 2.0
    return out


def _check_graph(gi, g):
    n = int(g['n'])
    if n < 0:
        raise ValueError(f"graph {gi}: n={n}")
    if n > MAX_NODES:
        raise ValueError(f"graph {gi}: {n} nodes (capacity {MAX_NODES})")
    fixed = int(g.get('fixed', 0))
    if n and not 0 <= fixed < n:
        raise ValueError(f"graph {gi}: fixed node {fixed} outside [0, {n})")
    mu = float(g.get('mu', 0.0))
    if not (mu >= 0.0 and np.isfinite(mu)):
        raise ValueError(f"graph {gi}: mu={mu} (must be finite and >= 0)")
    for k, e in enumerate(g['edges']):
        i, j = int(e['i']), int(e['j'])
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError(f"graph {gi}: edge {k} names nodes ({i}, {j}), outside [0, {n})")
        if i == j:
            raise ValueError(f"graph {gi}: edge {k} joins node {i} to itself")
        if np.asarray(e['T']).shape != (4, 4) or np.asarray(e['info']).shape != (6, 6):
            raise ValueError(f"graph {gi}: edge {k} needs T [4,4] and info [6,6]")
    init = np.asarray(g['init'], np.float64)
    if init.shape != (n, 4, 4):
        raise ValueError(f"graph {gi}: init {init.shape} is not [{n},4,4]")
    return n, fixed, mu, init


def optimize(graphs, max_iterations=100, eps_step=1e-9, eps_cost=1e-10, tau0=1e-5, device=None):
    """graphs: list of dicts (n, edges=[dict(i, j, T, info, uncertain)], init f64[n,4,4], fixed=0, mu=0) -> list of dicts (poses
    f64[n,4,4], status (a name of STATUS), solves, accepted, cost_initial, cost_final, weights f64[E] = l_e, residuals f64[E] = q_e),
    from ONE device call.  Arguments are checked here, before any device use (ValueError)."""
    if max_iterations < 0:
        raise ValueError(f"optimize: max_iterations={max_iterations}")
    for name, v in (('eps_step', eps_step), ('eps_cost', eps_cost), ('tau0', tau0)):
        if not (v > 0 and np.isfinite(v)):
            raise ValueError(f"optimize: {name}={v} (must be finite and > 0)")
    checked = [_check_graph(gi, g) for gi, g in enumerate(graphs)]
    if not graphs:
        return []
    import torch

    from . import ops
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    nodes = [c[0] for c in checked]
    edges = [len(g['edges']) for g in graphs]
    allE = [e for g in graphs for e in g['edges']]
    Z = np.array([np.asarray(e['T'], np.float64) for e in allE]).reshape(-1, 4, 4)
    info = np.array([np.asarray(e['info'], np.float64) for e in allE]).reshape(-1, 6, 6)
    X0 = np.concatenate([c[3] for c in checked]).reshape(-1, 4, 4)
    X, status, cost, edge = ops.pose_graph_optimize(
        nodes, edges, [int(e['i']) for e in allE], [int(e['j']) for e in allE], torch.from_numpy(Z).to(device), torch.from_numpy(info).to(device),
        [1 if e.get('uncertain', False) else 0 for e in allE], [c[1] for c in checked], [c[2] for c in checked],
        torch.from_numpy(X0).to(device), max_iterations, eps_step, eps_cost, tau0)
    X, status, cost, edge = X.cpu().numpy(), status.cpu().numpy(), cost.cpu().numpy(), edge.cpu().numpy()
    out, n0, e0 = [], 0, 0
    for gi, (n, ne) in enumerate(zip(nodes, edges)):
        out.append(dict(poses=X[n0:n0 + n].copy(), status=STATUS[int(status[gi, 0])], solves=int(status[gi, 1]), accepted=int(status[gi, 2]),
                        cost_initial=float(cost[gi, 0]), cost_final=float(cost[gi, 1]), weights=edge[e0:e0 + ne, 0].copy(),
                        residuals=edge[e0:e0 + ne, 1].copy()))
        n0, e0 = n0 + n, e0 + ne
    return out


def initial_poses(n, edges, fixed=0):
    """Poses by composition along the maximum spanning tree of the edges weighted by info[3,3] (the matched count in the
    [rotation, translation] order), grown from `fixed` (Prim; ties go to the lower edge index) -> (f64[n,4,4], the nodes not connected
    to `fixed`, which stay at the identity)."""
    if n and not 0 <= fixed < n:
        raise ValueError(f"initial_poses: fixed node {fixed} outside [0, {n})")
    W = np.tile(np.eye(4), (n, 1, 1))
    if n == 0:
        return W, []
    done = np.zeros(n, bool)
    done[fixed] = True
    wts = [float(np.asarray(e['info'])[3, 3]) for e in edges]
    while True:
        best = -1
        for k, e in enumerate(edges):
            if done[int(e['i'])] != done[int(e['j'])] and (best < 0 or wts[k] > wts[best]):
                best = k
        if best < 0:
            break
        e = edges[best]
        i, j, T = int(e['i']), int(e['j']), np.asarray(e['T'], np.float64)
        if done[i]:
            W[j] = W[i] @ T                                    # T = inv(W_i) W_j
            done[j] = True
        else:
            W[i] = W[j] @ rigid_inverse(T)
            done[i] = True
    return W, [int(k) for k in np.flatnonzero(~done)]


def line_process_weight(edges, max_dist, preference=1.0):
    """mu = preference * max_dist^2 * the mean over the uncertain edges of trace(info[3:,3:]) / 3 (the matched count): the cost an
    edge pays to be switched off = what its matches would cost at the correspondence distance.  0 without an uncertain edge."""
    tr = [np.trace(np.asarray(e['info'], np.float64)[3:, 3:]) / 3.0 for e in edges if e.get('uncertain', False)]
    return float(preference * max_dist * max_dist * np.mean(tr)) if tr else 0.0


def prune(result, threshold=0.25, uncertain=None):
    """mask over a result's edges: line-process weight l < threshold (certain edges have l = 1 and are never pruned; with
    `uncertain`, a bool per edge, only those are considered)"""
    m = np.asarray(result['weights'], np.float64) < threshold
    return m if uncertain is None else m & np.asarray(uncertain, bool)


def optimize_two_pass(graphs, threshold=0.25, **kw):
    """optimize; drop every uncertain edge whose weight fell under `threshold`; optimize the kept edges from the first pass's poses
    (one device call per pass for all graphs) -> list of dicts: the second pass's result + pruned (bool per edge of the input graph),
    first (the first pass's result); weights / residuals of the second pass cover the kept edges, in their input order."""
    first = optimize(graphs, **kw)
    second_in, masks = [], []
    for g, r in zip(graphs, first):
        m = prune(r, threshold, [bool(e.get('uncertain', False)) for e in g['edges']]) if r['status'] != 'FAILED' else np.zeros(len(g['edges']), bool)
        masks.append(m)
        second_in.append(dict(g, edges=[e for e, drop in zip(g['edges'], m) if not drop], init=r['poses']))
    second = optimize(second_in, **kw)
    return [dict(s, pruned=m, first=r) for s, m, r in zip(second, masks, first)]


def scene_edges(clouds, pairs, poses, radius, min_matched=30):
    """Pose-graph edges of registered pairs.  clouds: list of f32[n,3] device tensors (voxelised fragments, each in its own frame);
    pairs: (i, j) registered as source i -> target j with pose P (poses [P,4,4], any float type).  The edge is (i, j, Z =
    inv(project_rigid(P)), info) with info the 'open3d' information matrix from ONE pairs.pair_statistics call over all pairs: the
    matched target points are fragment j's, in j's frame.  All edges uncertain.
    -> (edges, dropped): edges under `min_matched` matches go to dropped (dicts with i, j, matched): their information is ~0, so
    q = 0 and l = 1 whatever the poses, and the line process could never switch them off."""
    from . import pairs as bpairs
    pairs = [(int(a), int(b)) for a, b in pairs]
    P = np.array([project_rigid(p) for p in np.asarray(poses, np.float64).reshape(-1, 4, 4)]).reshape(-1, 4, 4)
    if len(pairs) != P.shape[0]:
        raise ValueError(f"scene_edges: {len(pairs)} pairs but {P.shape[0]} poses")
    st = bpairs.pair_statistics(clouds, pairs, P, radius)
    edges, dropped = [], []
    for k, (i, j) in enumerate(pairs):
        m = int(st['matched'][k])
        if m < min_matched:
            dropped.append(dict(i=i, j=j, matched=m, index=k))
            continue
        edges.append(dict(i=i, j=j, T=rigid_inverse(P[k]), uncertain=True, matched=m, index=k,
                          info=bpairs.information_matrix(m, st['sum_u'][k], st['sum_uu'][k], 'open3d')))
    return edges, dropped


def trajectory_error(W_est, W_gt, fixed=0):
    """Per-fragment errors after aligning the two trajectories at `fixed` (each pose taken relative to its trajectory's own fixed
    node) -> dict(rte f64[n] metres, rre f64[n] degrees, rte_rmse, rre_rmse)"""
    W_est, W_gt = np.asarray(W_est, np.float64).reshape(-1, 4, 4), np.asarray(W_gt, np.float64).reshape(-1, 4, 4)
    if W_est.shape != W_gt.shape:
        raise ValueError(f"trajectory_error: {W_est.shape[0]} estimated poses, {W_gt.shape[0]} true ones")
    n = W_est.shape[0]
    rte, rre = np.zeros(n), np.zeros(n)
    if n:
        Ae, Ag = rigid_inverse(W_est[fixed]), rigid_inverse(W_gt[fixed])
        for k in range(n):
            D = rigid_inverse(Ag @ W_gt[k]) @ (Ae @ W_est[k])
            rte[k] = np.linalg.norm(D[:3, 3])
            s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
            rre[k] = np.degrees(np.arctan2(s, 0.5 * (np.trace(D[:3, :3]) - 1.0)))
    return dict(rte=rte, rre=rre, rte_rmse=float(np.sqrt(np.mean(rte ** 2))) if n else 0.0,
                rre_rmse=float(np.sqrt(np.mean(rre ** 2))) if n else 0.0)


def write_trajectory(path, poses):
    """fragment -> world poses in the five-lines-per-pose format pairs.read_poses reads (header 'k k k+1', then the 4x4, repr floats)"""
    import os
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
        for k, W in enumerate(np.asarray(poses, np.float64).reshape(-1, 4, 4)):
            f.write(f'{k}\t{k}\t{k + 1}\n')
            for row in W:
                f.write('\t'.join(repr(float(x)) for x in row) + '\n')
