"""TEST INFRASTRUCTURE: numpy twin of the descriptor-matching contract of include/buffer_hip.h (N12), in FLOAT32.  numpy's float32
subtraction, multiplication and addition are correctly rounded and never fused, and the sum runs dimension by dimension, so every
figure here is the bits the kernel must give: the comparisons of tests/test_match_gpu.py are exact equalities.

    ssd(a, b)                          f32[na,nb]: sum over the dimensions in order of (a_c - b_c)^2
    two_nearest(a, b)                  (nn int32[na,2], ssd f32[na,2]): nearest and second-nearest row of b by the key
                                       (float bits of ssd) << 32 | row, -1 / +inf where there is none; non-finite rows are not ranked
    match(a, b, mutual, ratio)         dict(corr int32[m,2], nn, ssd, forward = the forward matches without any filter)
    match_batch(pairs, mutual, ratio)  the stacked form: dict(corr, counts int32[P], nn, ssd)
    make_pair(seed, na, nb, d)         the seeded inputs of the tests; CASES = their (seed, na, nb, d)
"""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
RATIO = 0.8

# (seed, na, nb, d): 63 / 64 / 65 queries (one lane off a wavefront), 257 references (one past a tile of 256), d = 7 (padded far), 32 (a
# multiple of 4), 33 (one past it: FPFH), 36 (the padded width itself)
CASES = [(1, 130, 257, 33), (2, 64, 65, 33), (3, 257, 130, 32), (5, 200, 200, 7), (6, 65, 64, 36)]
# and the widest kernel (d > 36), with 129 references: one past ITS tile of 128
WIDE_CASES = [(7, 63, 129, 40), (8, 70, 131, 64)]


def make_pair(seed, na, nb, d):
    """b uniform in [0, 1); even rows of a = a random row of b + 0.05 N(0, 1) (a true match), odd rows fresh uniform rows (none)"""
    rng = np.random.default_rng(seed)
    b = rng.random((nb, d)).astype(np.float32)
    a = rng.random((na, d))
    ne = (na + 1) // 2
    a[0::2] = b[rng.integers(nb, size=ne)] + 0.05 * rng.normal(size=(ne, d))
    return a.astype(np.float32), b


def finite_rows(x):
    return np.isfinite(x).all(1) if x.shape[1] else np.ones(len(x), bool)


def ssd(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    s = np.zeros((len(a), len(b)), np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for c in range(a.shape[1]):
            t = a[:, c][:, None] - b[:, c][None, :]
            s = s + t * t
    assert s.dtype == np.float32
    return s


def keys(a, b):
    """uint64[na,nb]: the ranking keys, NONE where either row is non-finite"""
    s = ssd(a, b)
    k = (s.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(b), dtype=np.uint64)[None, :]
    k[~finite_rows(np.asarray(a, np.float32)), :] = NONE
    k[:, ~finite_rows(np.asarray(b, np.float32))] = NONE
    return k


def two_nearest(a, b):
    k = keys(a, b)
    na = len(k)
    k = np.concatenate([np.sort(k, axis=1)[:, :2], np.full((na, 2), NONE, np.uint64)], 1)[:, :2]
    none = k == NONE
    nn = np.where(none, -1, (k & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    sd = np.where(none, np.float32(np.inf), (k >> np.uint64(32)).astype(np.uint32).view(np.float32)).astype(np.float32)
    return nn, sd


def ratio_squared(ratio):
    r = np.float32(ratio)                                        # the C ABI takes a float
    return np.float32(np.float64(r) * np.float64(r))


def match(a, b, mutual=True, ratio=None):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nn, sd = two_nearest(a, b)
    back = two_nearest(b, a)[0][:, 0] if len(b) else np.zeros(0, np.int32)
    i = np.arange(len(a))
    keep = nn[:, 0] >= 0
    forward = np.stack([i[keep], nn[keep, 0]], 1).astype(np.int32)
    if mutual:
        keep &= back[np.maximum(nn[:, 0], 0)] == i if len(b) else False
    if ratio is not None and ratio > 0:
        with np.errstate(invalid='ignore'):
            keep &= (nn[:, 1] < 0) | (sd[:, 0] <= ratio_squared(ratio) * sd[:, 1])
    return dict(corr=np.stack([i[keep], nn[keep, 0]], 1).astype(np.int32), nn=nn, ssd=sd, forward=forward)


def match_batch(pairs, mutual=True, ratio=None):
    rs = [match(a, b, mutual, ratio) for a, b in pairs]
    cat = lambda k, w, t: np.concatenate([r[k] for r in rs] + [np.zeros((0, w), t)])
    return dict(corr=cat('corr', 2, np.int32), counts=np.array([len(r['corr']) for r in rs], np.int32), nn=cat('nn', 2, np.int32),
                ssd=cat('ssd', 2, np.float32))
