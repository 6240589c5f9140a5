"""float64 references of the pose-recovery kernels (csrc/registration.hip) for tests/test_pose_recovery_gpu.py: hypotheses and all-vs-all
scoring, one hypothesis of the seeded 3-point RANSAC, and the weighted-Kabsch refinement loop.  Plain numpy; float32 inputs are widened
to float64, so every decision (a distance against a threshold) is taken on the unrounded value.  Where fp32 may decide the other way the
functions say so: `delta` is the width of the band around a threshold inside which a comparison is reported as undecided.  It excludes
cases from an exact comparison; it is not a tolerance on a result.  1e-5 suits the metre scale of fixture match_tiny.npz (keypoint norms
0.17-1.15; about 40 times the fp32 rounding of a distance near 1 m); scale it with the largest coordinate magnitude elsewhere."""
import numpy as np

from oracle.pipeline_ref import _splitmix64

_MASK = (1 << 64) - 1
EDGE, DIST, SCORED, FEW = 'edge', 'dist', 'scored', 'few'      # ransac_hypothesis status


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def hypotheses(ind, ss, tt, ssR, ttR, azi_n):
    """R = ttR Rz(angle) ssR^T, t = tt - R ss with angle = ind * 2 pi / azi_n + 1e-6 (models/BUFFER.py:295-301) -> R f64[m,3,3], t f64[m,3]"""
    ind, ss, tt = _f64(ind).reshape(-1), _f64(ss).reshape(-1, 3), _f64(tt).reshape(-1, 3)
    ssR, ttR = _f64(ssR).reshape(-1, 3, 3), _f64(ttR).reshape(-1, 3, 3)
    angle = ind * 2 * np.pi / azi_n + 1e-6
    c, s = np.cos(angle), np.sin(angle)
    Rz = np.zeros((ind.shape[0], 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
    with np.errstate(all='ignore'):
        R = ttR @ Rz @ np.transpose(ssR, (0, 2, 1))
        t = tt - np.einsum('mij,mj->mi', R, ss)
    return R, t


def score_table(R, t, ss, tt, azi_n, inlier_th, delta, chunk=256):
    """every hypothesis h against every row j: diff = ||R_h ss_j + t_h - tt_j||, thr_j = ||ss_j|| pi / azi_n * inlier_th (BUFFER.py:302-309)
    -> (inl bool[m,m]: diff < thr, und bool[m,m]: |diff - thr| < delta, thr f64[m]).  A non-finite diff or threshold is in neither."""
    R, t = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(t, np.float64).reshape(-1, 3)
    ss, tt = _f64(ss).reshape(-1, 3), _f64(tt).reshape(-1, 3)
    m = ss.shape[0]
    inl, und = np.zeros((m, m), bool), np.zeros((m, m), bool)
    with np.errstate(all='ignore'):
        thr = np.sqrt((ss * ss).sum(1)) * np.pi / azi_n * inlier_th
        for lo in range(0, m, chunk):
            d = np.einsum('hij,mj->hmi', R[lo:lo + chunk], ss) + t[lo:lo + chunk, None] - tt[None]
            diff = np.sqrt((d * d).sum(-1))
            inl[lo:lo + chunk] = diff < thr[None]
            und[lo:lo + chunk] = np.abs(diff - thr[None]) < delta
    return inl, und, thr


def kabsch(H):
    """R = V diag(1, 1, det(V U^T)) U^T of H = U S V^T (BUFFER.py:455-461) -> (R f64[3,3], singular values)"""
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    d = np.linalg.det(V @ U.T)
    return V @ np.diag([1.0, 1.0, d]) @ U.T, S


def sample_indices(seed, h, n):
    """the three distinct positions in the candidate list that hypothesis h of a run seeded `seed` draws (n >= 3)"""
    base = (int(seed) + 3 * int(h)) & _MASK
    i0 = _splitmix64(base) % n
    i1 = _splitmix64((base + 1) & _MASK) % (n - 1)
    i2 = _splitmix64((base + 2) & _MASK) % (n - 2)
    if i1 >= i0:
        i1 += 1
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


def ransac_hypothesis(src, tgt, corr, seed, h, max_dist, edge_sim, delta):
    """one hypothesis of our sampler (csrc/registration.hip ransac_hypothesis) -> (status, T f64[4,4], count, mse, undecided).
    status: EDGE (rejected by the edge-length check), DIST (rejected by the distance check on its three points), SCORED, or FEW (fewer
    than three candidates).  T is the identity unless SCORED.  undecided: an edge-check margin within delta of zero, a 3-point or
    candidate distance within delta of max_dist, or a near-collinear sample (second singular value of H below 1e-3 of the first)."""
    src, tgt = _f64(src).reshape(-1, 3), _f64(tgt).reshape(-1, 3)
    corr = np.asarray(corr, np.int64).reshape(-1)
    n = corr.shape[0]
    I = np.eye(4)
    if n < 3:
        return FEW, I, 0, np.inf, False
    ids = corr[list(sample_indices(seed, h, n))]
    a, b = src[ids], tgt[ids]
    und = False
    for p in range(3):
        q = (p + 1) % 3
        ds, dt = np.linalg.norm(a[p] - a[q]), np.linalg.norm(b[p] - b[q])
        m1, m2 = ds - dt * edge_sim, dt - ds * edge_sim
        und = und or abs(m1) < delta or abs(m2) < delta
        if not (m1 >= 0 and m2 >= 0):
            return EDGE, I, 0, np.inf, und
    ca, cb = a.mean(0), b.mean(0)
    R, S = kabsch((a - ca).T @ (b - cb))
    und = und or S[1] < 1e-3 * S[0]
    t = cb - R @ ca
    d3 = np.linalg.norm(a @ R.T + t - b, axis=1)
    und = und or bool((np.abs(d3 - max_dist) < delta).any())
    if (d3 > max_dist).any():
        return DIST, I, 0, np.inf, und
    S_all, G_all = src[corr], tgt[corr]
    dist = np.linalg.norm(S_all @ R.T + t - G_all, axis=1)
    und = und or bool((np.abs(dist - max_dist) < delta).any())
    inl = dist < max_dist
    cnt = int(inl.sum())
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    mse = float((dist[inl] ** 2).sum() / cnt) if cnt else np.inf
    return SCORED, T, cnt, mse, und


def post_refinement(T, src, tgt, thr, iters, delta):
    """the loop of oracle/torch_ref.post_refinement (BUFFER.py:382-464) in float64; rows with a non-finite coordinate are ignored
    -> (T f64[4,4], last_count, rounds, clear): the inlier count of the last round that updated the pose, the number of such rounds, and
    whether no distance lay within delta of thr in any round."""
    T = np.array(np.asarray(T, np.float64).reshape(4, 4))
    T[3] = [0, 0, 0, 1]
    src, tgt = _f64(src).reshape(-1, 3), _f64(tgt).reshape(-1, 3)
    ok = np.isfinite(src).all(1) & np.isfinite(tgt).all(1)
    src, tgt = src[ok], tgt[ok]
    prev, rounds, clear = 0, 0, True
    for _ in range(iters):
        dis = np.linalg.norm(src @ T[:3, :3].T + T[:3, 3] - tgt, axis=1)
        clear = clear and not bool((np.abs(dis - thr) < delta).any())
        inl = dis < thr
        num = int(inl.sum())
        if abs(num - prev) < 1:
            break
        prev = num
        rounds += 1
        w = 1.0 / (1.0 + (dis[inl] / thr) ** 2)
        A, B = src[inl], tgt[inl]
        ca, cb = (A * w[:, None]).sum(0) / (w.sum() + 1e-6), (B * w[:, None]).sum(0) / (w.sum() + 1e-6)
        R, _ = kabsch(((A - ca) * w[:, None]).T @ (B - cb))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, cb - R @ ca
    return T, prev, rounds, clear


# ------------------------------------------------------------------------------------------ synthetic matches
def random_rotations(rng, k):
    """k proper rotations f64[k,3,3]"""
    q = np.linalg.qr(rng.normal(size=(k, 3, 3)))[0]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def small_motion(rng, deg, shift):
    """a rigid motion with rotation angle `deg` about a random axis and a translation of length `shift` -> f64[4,4]"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    d = rng.normal(size=3)
    T[:3, 3] = shift * d / np.linalg.norm(d)
    return T


def make_matches(seed, m, n_out=None, noise=0.01, out_min=0.3, rot_share=0.5, azi_n=20, scale=1.0):
    """m synthetic matches around a planted rigid motion -> dict(ind f32[m], ss, tt f32[m,3], ssR, ttR f32[m,3,3], T f64[4,4] planted,
    bad bool[m]).  ss is uniform in the box [-0.4, 0.4]^2 x [0.2, 1.0] (norms 0.2-1.15, the range of fixture match_tiny.npz), times
    `scale`; tt = T ss + uniform noise in +-noise; n_out rows (default m // 2) are outliers, moved out_min .. out_min + 0.6 (times scale)
    away from their planted partner.  ssR are random rotations; ttR is set so that a share rot_share of the good rows yields the
    planted rotation for its ind (R_hyp = ttR Rz(ind) ssR^T), random otherwise."""
    rng = np.random.default_rng(seed)
    ss = ((rng.random((m, 3)) * [0.8, 0.8, 0.8] + [-0.4, -0.4, 0.2]) * scale).astype(np.float32)
    T = small_motion(rng, rng.uniform(20, 60), 0.25 * scale)
    tt = ss.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.uniform(-noise, noise, size=(m, 3))
    n_out = m // 2 if n_out is None else n_out
    bad = np.zeros(m, bool)
    bad[rng.permutation(m)[:n_out]] = True
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tt[bad] += (d * rng.uniform(out_min, out_min + 0.6, size=(m, 1)) * scale)[bad]
    tt = tt.astype(np.float32)
    ind = (rng.random(m) * azi_n).astype(np.float32)
    ssR = random_rotations(rng, m).astype(np.float32)
    ttR = random_rotations(rng, m)
    angle = ind.astype(np.float64) * 2 * np.pi / azi_n + 1e-6
    Rz = np.zeros((m, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(angle), -np.sin(angle), np.sin(angle), np.cos(angle), 1.0
    good = ~bad & (rng.random(m) < rot_share)
    ttR[good] = T[:3, :3] @ ssR[good].astype(np.float64) @ np.transpose(Rz[good], (0, 2, 1))
    return dict(ind=ind, ss=ss, tt=tt, ssR=ssR, ttR=ttR.astype(np.float32), T=T, bad=bad)
