"""float64 numpy restatement of buf_pose_graph_optimize, written from its contract comment in include/buffer_hip.h (no library's
conventions are used), with a per-solve trace, and the generators of the scenes the pose-graph tests share.

A graph is the dict buffer_amd.posegraph.optimize takes: n, edges=[dict(i, j, T, info, uncertain)], init f64[n,4,4], fixed, mu."""
import functools

import numpy as np

STATUS = ('NOTHING', 'CONVERGED_STEP', 'CONVERGED_COST', 'MAX_ITER', 'STALLED', 'FAILED')
THREADS = 256                                                   # the shape of the kernel's sums


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(a):
    a = np.asarray(a, np.float64)
    t = np.sqrt(a @ a)
    A, B = 1.0, 0.5
    if t > 0.0:
        h = np.sin(0.5 * t) / (0.5 * t)
        A, B = np.sin(t) / t, 0.5 * (h * h)
    P = hat(a)
    return np.eye(3) + A * P + B * (P @ P)


def so3_log(R):
    """through the quaternion (Shepperd's branch on the largest of w, x, y, z; w >= 0) and atan2"""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0)
        w, x, y, z = 0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        w, x, y, z = (R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        w, x, y, z = (R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        w, x, y, z = (R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s
    v = np.array([x, y, z])
    if w < 0.0:
        w, v = -w, -v
    nv = np.sqrt(v @ v)
    return (2.0 * np.arctan2(nv, w) / nv if nv > 0.0 else 2.0) * v


def pose(R, p):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, p
    return T


def inv(T):
    return pose(T[:3, :3].T, -T[:3, :3].T @ T[:3, 3])


def retract(X, a, b):
    """X (Exp(a), b): R <- R Exp(a), p <- p + R b"""
    return pose(X[:3, :3] @ so3_exp(a), X[:3, 3] + X[:3, :3] @ np.asarray(b, np.float64))


def residual(Xi, Xj, Z):
    """-> r = [Log(R_E); t_E] of E = Z^-1 X_i^-1 X_j, R_E, and M = X_j^-1 X_i"""
    E = inv(Z) @ inv(Xi) @ Xj
    return np.concatenate([so3_log(E[:3, :3]), E[:3, 3]]), E[:3, :3], inv(Xj) @ Xi


def jacobians(Xi, Xj, Z):
    r, RE, M = residual(Xi, Xj, Z)
    RM, pM = M[:3, :3], M[:3, 3]
    P = hat(r[:3])
    Jri = np.eye(3) + P / 2.0 + (P @ P) / 12.0
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Ji[:3, :3], Ji[3:, :3], Ji[3:, 3:] = -Jri @ RM, -RE @ hat(pM) @ RM, -RE @ RM
    Jj[:3, :3], Jj[3:, 3:] = Jri, RE
    return r, Ji, Jj


def weight(q, mu, robust):
    return (mu / (mu + q)) ** 2 if robust else 1.0


def cost_term(q, mu, robust):
    return mu * q / (mu + q) if robust else q


def tree_sum(v):
    """the kernel's sum: per-thread partials over i, i + THREADS, ... in ascending order, then a binary tree over the partials"""
    v = np.asarray(v, np.float64)
    part = np.zeros(THREADS)
    for lo in range(0, len(v), THREADS):
        c = v[lo:lo + THREADS]
        part[:len(c)] += c
    st = THREADS // 2
    while st:
        part[:st] += part[st:2 * st]
        st //= 2
    return part[0]


def _edges_eval(g, X):
    mu = float(g.get('mu', 0.0))
    q = np.zeros(len(g['edges']))
    rb = np.zeros(len(g['edges']), bool)
    for k, e in enumerate(g['edges']):
        r = residual(X[e['i']], X[e['j']], np.asarray(e['T'], np.float64))[0]
        q[k] = r @ (np.asarray(e['info'], np.float64) @ r)
        rb[k] = bool(e.get('uncertain', False)) and mu > 0.0
    l = np.array([weight(q[k], mu, rb[k]) for k in range(len(q))])
    F = tree_sum([cost_term(q[k], mu, rb[k]) for k in range(len(q))])
    return F, l, q


def _normal_equations(g, X):
    n, fixed, mu = g['n'], int(g.get('fixed', 0)), float(g.get('mu', 0.0))
    free = [k for k in range(n) if k != fixed]
    slot = {k: 6 * s for s, k in enumerate(free)}
    D = 6 * len(free)
    H, grad = np.zeros((D, D)), np.zeros(D)
    for e in g['edges']:
        i, j, L = e['i'], e['j'], np.asarray(e['info'], np.float64)
        r, Ji, Jj = jacobians(X[i], X[j], np.asarray(e['T'], np.float64))
        l = weight(r @ (L @ r), mu, bool(e.get('uncertain', False)) and mu > 0.0)
        for a, Ja in ((i, Ji), (j, Jj)):
            if a == fixed:
                continue
            grad[slot[a]:slot[a] + 6] += l * (Ja.T @ (L @ r))
            for b, Jb in ((i, Ji), (j, Jj)):
                if b != fixed:
                    H[slot[a]:slot[a] + 6, slot[b]:slot[b] + 6] += l * (Ja.T @ (L @ Jb))
    return H, grad, free


def optimize(g, max_iterations=100, eps_step=1e-9, eps_cost=1e-10, tau0=1e-5):
    """-> dict(poses, status, solves, accepted, cost_initial, cost_final, weights, residuals, trace); trace: one dict per solve with
    factored, rho, max_delta, cost_ratio = (F - F') / F, lam (the damping the solve used), accepted"""
    n, fixed = g['n'], int(g.get('fixed', 0))
    X0 = np.asarray(g['init'], np.float64).reshape(n, 4, 4)
    E = g['edges']
    finite = np.isfinite(X0).all() and all(np.isfinite(np.asarray(e['T'], np.float64)).all() and np.isfinite(np.asarray(e['info'], np.float64)).all() for e in E)
    if not finite:
        nan = np.full(len(E), np.nan)
        return dict(poses=X0.copy(), status='FAILED', solves=0, accepted=0, cost_initial=np.nan, cost_final=np.nan, weights=nan, residuals=nan, trace=[])
    X = X0.copy()
    F = _edges_eval(g, X)[0]
    F0, status, solves, accepted, trace = F, 'NOTHING', 0, 0, []
    if n > 1 and len(E) > 0:
        H, grad, free = _normal_equations(g, X)
        lam0 = tau0 * np.max(np.diag(H))
        if lam0 > 0.0:
            lam, nu, status = lam0, 2.0, 'MAX_ITER'
            for _ in range(max_iterations):
                solves += 1
                row = dict(factored=False, rho=np.nan, max_delta=np.nan, cost_ratio=np.nan, lam=lam, accepted=False)
                trace.append(row)
                ok = True
                try:
                    Lc = np.linalg.cholesky(H + lam * np.eye(len(grad)))
                    ok = bool(np.isfinite(Lc).all())
                except np.linalg.LinAlgError:
                    ok = False
                if ok:
                    row['factored'] = True
                    delta = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, grad))
                    row['max_delta'] = float(np.abs(delta).max())
                    if row['max_delta'] <= eps_step:
                        status = 'CONVERGED_STEP'
                        break
                    Xc = X.copy()
                    for s, k in enumerate(free):
                        Xc[k] = retract(X[k], delta[6 * s:6 * s + 3], delta[6 * s + 3:6 * s + 6])
                    Fp = _edges_eval(g, Xc)[0]
                    rho = (F - Fp) / tree_sum(delta * (lam * delta - grad))
                    row['rho'], row['cost_ratio'] = float(rho), float((F - Fp) / F) if F != 0 else np.nan
                    if rho > 0.0 and np.isfinite(Fp):
                        row['accepted'] = True
                        accepted += 1
                        dF, Fold, X, F = F - Fp, F, Xc, Fp
                        lam, nu = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0
                        if dF <= eps_cost * Fold:
                            status = 'CONVERGED_COST'
                            break
                        H, grad, free = _normal_equations(g, X)
                        continue
                lam, nu = lam * nu, 2.0 * nu
                if lam > 1e30 * lam0:
                    status = 'STALLED'
                    break
    _, l, q = _edges_eval(g, X)
    return dict(poses=X, status=status, solves=solves, accepted=accepted, cost_initial=F0, cost_final=F, weights=l, residuals=q, trace=trace)


def margins(trace, eps_step=1e-9, eps_cost=1e-10):
    """the smallest ratio by which any decision of a trace clears its threshold (rho against 0 is a sign: |rho| against the
    smallest |rho| a test accepts, see the tests); -> dict(rho = min |rho|, step = min over solves of max(d / eps, eps / d),
    cost = the same for accepted solves' cost ratios)"""
    rho = [abs(t['rho']) for t in trace if t['factored'] and np.isfinite(t['rho'])]
    step = [max(t['max_delta'] / eps_step, eps_step / t['max_delta']) if t['max_delta'] > 0 else np.inf for t in trace if t['factored']]
    cost = [max(abs(t['cost_ratio']) / eps_cost, eps_cost / abs(t['cost_ratio'])) if t['cost_ratio'] != 0 else np.inf
            for t in trace if t['accepted'] and np.isfinite(t['cost_ratio'])]
    return dict(rho=min(rho) if rho else np.inf, step=min(step) if step else np.inf, cost=min(cost) if cost else np.inf)


# ---------------------------------------------------------------------------------------------------- scenes
def random_rotvec(rng, angle):
    v = rng.standard_normal(3)
    return angle * v / np.linalg.norm(v)


def random_motion(rng, angle, dist):
    return pose(so3_exp(random_rotvec(rng, angle)), random_rotvec(rng, dist))


def points_info(rng, count):
    """the 'open3d' information matrix of `count` random points of a 2 m room: sum G^T G, G = [-[u]x, I]"""
    u = rng.uniform(-1.0, 1.0, (count, 3))
    out = np.zeros((6, 6))
    for p in u:
        G = np.hstack([-hat(p), np.eye(3)])
        out += G.T @ G
    return out


def chain_world(rng, n, angle=0.3, dist=0.5):
    W = [np.eye(4)]
    for _ in range(n - 1):
        W.append(W[-1] @ random_motion(rng, angle, dist))
    return np.array(W)


def make_scene(seed, n=12, chords=10, false_edges=4, noise=(0.002, 0.003), false_error=(0.6, 0.7), fixed=0, mu=None, swap=False,
               uncertain=True):
    """The generator of the issue: a chain of n planted poses (0.3 rad / 0.5 m steps), n - 1 chain edges + `chords` random chords
    as true edges, each times a 2 mrad / 3 mm error, `false_edges` chords with a 0.6 rad / 0.7 m error; info from 300-400 random
    points; mu = line_process_weight(edges, 0.05) (None) or the given value; init = the composition of the chain edges from node 0
    re-based so that `fixed` sits at its planted pose.  swap: every second edge is given as (j, i) with the inverse measurement.
    -> (graph, planted world poses, bool per edge: false)"""
    from buffer_amd import posegraph
    rng = np.random.default_rng(seed)
    W = chain_world(rng, n)
    pairs = [(k, k + 1) for k in range(n - 1)]
    free = [(i, j) for i in range(n) for j in range(i + 2, n)]
    chord = [free[k] for k in rng.permutation(len(free))[:chords + false_edges]] if free else []
    n_true = max(len(chord) - false_edges, 0)                   # the last `false_edges` chords are the false ones
    edges, false = [], []
    for k, (i, j) in enumerate(pairs + chord):
        is_false = k >= len(pairs) + n_true
        err = random_motion(rng, *(false_error if is_false else noise))
        T = inv(W[i]) @ W[j] @ err
        info = points_info(rng, int(rng.integers(300, 401)))
        if swap and k % 2 == 1:
            i, j, T = j, i, inv(T)
        edges.append(dict(i=i, j=j, T=T, info=info, uncertain=bool(uncertain)))
        false.append(is_false)
    init = [np.eye(4)]
    for k in range(n - 1):
        e = edges[k]
        init.append(init[-1] @ (e['T'] if e['i'] == k else inv(e['T'])))
    init = np.array(init)
    init = np.array([W[fixed] @ inv(init[fixed]) @ x for x in init])
    g = dict(n=n, edges=edges, init=init, fixed=fixed, mu=posegraph.line_process_weight(edges, 0.05) if mu is None else mu)
    return g, W, np.array(false, bool)


def perturb_init(g, W, seed, angle, dist):
    """free nodes start at their planted poses times a random motion of `angle` rad / `dist` m"""
    rng = np.random.default_rng(seed)
    g['init'] = np.array([W[k] if k == g['fixed'] else W[k] @ random_motion(rng, angle, dist) for k in range(g['n'])])
    return g


@functools.lru_cache(maxsize=None)
def scenes():
    """Every scene the GPU tests run, by name -> (graph, planted poses or None).  The seeds are chosen so that every decision of
    the restatement's trace keeps a margin (test_posegraph_cpu.py::test_gpu_scenes_keep_their_margins): a condition on the inputs."""
    out = {}
    out['outlier'] = make_scene(0)[:2]                                                  # n = 12, 4 false chords, all edges uncertain
    out['outlier_fixed5'] = make_scene(0, fixed=5)[:2]
    out['outlier_fixed11'] = make_scene(0, fixed=11)[:2]
    g, W, _ = make_scene(3, 12, 6, 0, mu=0.0)
    out['rejected'] = (perturb_init(g, W, 2003, 1.5, 1.5), W)                           # 3 rejected solves of 12
    g, W, _ = make_scene(3, 8, 6, 0, noise=(0.0, 0.0), mu=0.0)
    out['zero_residual'] = (perturb_init(g, W, 1003, 0.05, 0.05), W)
    for n, chords, seed in ((2, 0, 0), (3, 1, 20), (23, 10, 0), (44, 20, 2), (128, 100, 2)):   # 6 (n - 1) = 6, 12, 132, 258, 762
        g, W, _ = make_scene(seed, n, chords, 0, mu=0.0)
        out[f'n{n}'] = (perturb_init(g, W, seed + 1000, 0.05, 0.05), W)
    g, W, _ = make_scene(0, swap=True)                                                  # (j, i) edges, and two node pairs with two edges
    rng = np.random.default_rng(77)
    for k in (2, 13):
        e = g['edges'][k]
        g['edges'].append(dict(i=e['j'], j=e['i'], T=inv(inv(W[e['i']]) @ W[e['j']] @ random_motion(rng, 0.002, 0.003)),
                               info=points_info(rng, 350), uncertain=True))
    out['swap_duplicates'] = (g, W)
    g, W, _ = make_scene(9, 15, 10, 0, mu=0.0)                                          # node 15 has no edge and keeps its pose
    g = perturb_init(g, W, 1009, 0.05, 0.05)
    lone = random_motion(np.random.default_rng(5), 0.7, 1.0)
    out['isolated'] = (dict(g, n=16, init=np.concatenate([g['init'], lone[None]])), np.concatenate([W, lone[None]]))
    g, W, false = make_scene(0)                                                         # one false edge 179.9 degrees off
    k = int(np.flatnonzero(false)[0])
    e = g['edges'][k]
    rng = np.random.default_rng(179)
    e['T'] = inv(W[e['i']]) @ W[e['j']] @ pose(so3_exp(random_rotvec(rng, np.radians(179.9))), random_rotvec(rng, 0.7))
    out['rot179'] = (g, W)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, max_iterations=100):
    """the restatement's result on a scene of scenes(), computed once per process and shared: do not modify"""
    return optimize(scenes()[name][0], max_iterations=max_iterations)


def negative_definite_scene():
    """Nodes 2 and 3 are joined by an edge with a negative-definite information matrix; node 1 hangs on the fixed node 0 by an edge
    of 1e-30 times a usual matrix, so lambda0 = tau0 max diag H is positive but tiny and no lambda up to 1e30 lambda0 makes
    H + lambda I positive definite: every solve is rejected at its factorisation and the loop ends STALLED after 14 solves
    (lambda0 2^(k (k + 1) / 2) > 1e30 lambda0 at k = 14).  (A graph whose edges are ALL negative definite has max diag H < 0 and
    returns NOTHING by the lambda0 rule of the contract.)"""
    rng = np.random.default_rng(11)
    W = chain_world(rng, 4)
    edges = [dict(i=0, j=1, T=inv(W[0]) @ W[1] @ random_motion(rng, 0.01, 0.01), info=1e-30 * points_info(rng, 300), uncertain=False),
             dict(i=2, j=3, T=inv(W[2]) @ W[3] @ random_motion(rng, 0.01, 0.01), info=-points_info(rng, 300), uncertain=False)]
    return dict(n=4, edges=edges, init=W.copy(), fixed=0, mu=0.0)


# ---------------------------------------------------------------------------------------------------- the C ABI's argument errors
def abi_base():
    """a valid two-edge, three-node call of buf_pose_graph_optimize as keyword arguments of host values (device arrays left out)"""
    return dict(nodes=[3], edges=[2], edge_i=[0, 1], edge_j=[1, 2], uncertain=[1, 0], fixed=[0], mu=[1.0], max_iterations=10,
                eps_step=1e-9, eps_cost=1e-10, tau0=1e-5)


def einval_cases():
    """name -> the keyword arguments of abi_base() replaced: every BUF_EINVAL case of the header that host values can make"""
    nan, inf = float('nan'), float('inf')
    c = {'negative_nodes': dict(nodes=[-1]), 'negative_edges': dict(edges=[-2]), 'edge_i_outside': dict(edge_i=[3, 1]),
         'edge_j_negative': dict(edge_j=[1, -1]), 'self_edge': dict(edge_i=[0, 2]), 'fixed_outside': dict(fixed=[3]),
         'fixed_negative': dict(fixed=[-1]), 'mu_negative': dict(mu=[-1.0]), 'mu_nan': dict(mu=[nan]), 'mu_inf': dict(mu=[inf]),
         'max_iterations_negative': dict(max_iterations=-1)}
    for k in ('eps_step', 'eps_cost', 'tau0'):
        c[f'{k}_zero'], c[f'{k}_negative'], c[f'{k}_nan'], c[f'{k}_inf'] = {k: 0.0}, {k: -1e-9}, {k: nan}, {k: inf}
    return c
