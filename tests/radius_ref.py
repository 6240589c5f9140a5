"""The plain reference of the radius search (A2), written from the contract in include/buffer_hip.h: an all-pairs search per batch
element in numpy.  No grid, no cells, no early exit: every query meets every support of its element.

    d2 = (dx*dx + dy*dy) + dz*dz in float32, one rounding per operation; accept d2 < float32(r) * float32(r), strictly;
    rows ascending by (d2, global support index), padded with the total number of supports.
    A comparison with NaN is false: a non-finite support or query matches nothing.

Beside it, a restatement of the documented cell rule (cell_rule, candidate_sets, cell_coords).  It only tells the test-suite which
capacity of the kernels a named case reaches; it is never an expected value for a kernel's output.
"""
import numpy as np


def brute_force(queries, supports, q_lens, s_lens, radius):
    """-> (table int32[nq, max_count] padded with ns, counts int32[nq] untruncated, max_count int)"""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(supports, np.float32).reshape(-1, 3)
    q_lens, s_lens = np.asarray(q_lens, np.int64), np.asarray(s_lens, np.int64)
    assert q_lens.sum() == len(q) and s_lens.sum() == len(s) and len(q_lens) == len(s_lens)
    nq, ns = len(q), len(s)
    r = np.float32(radius)
    r2 = np.float32(r * r)
    counts = np.zeros(nq, np.int32)
    rows = [None] * len(q_lens)
    q0 = s0 = 0
    with np.errstate(invalid='ignore', over='ignore'):
        for b, (nqb, nsb) in enumerate(zip(q_lens, s_lens)):
            Q, S = q[q0:q0 + nqb], s[s0:s0 + nsb]
            dx = Q[:, None, 0] - S[None, :, 0]
            dy = Q[:, None, 1] - S[None, :, 1]
            dz = Q[:, None, 2] - S[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            hit = d2 < r2                                            # false wherever d2 is NaN
            counts[q0:q0 + nqb] = hit.sum(1)
            # stable sort of the row: ascending d2, equal d2 in ascending support index; what is no neighbour goes behind
            rows[b] = (np.argsort(np.where(hit, d2, np.float32(np.inf)), axis=1, kind='stable') + s0).astype(np.int32)
            q0 += nqb
            s0 += nsb
    mc = int(counts.max()) if nq else 0
    table = np.full((nq, mc), ns, np.int32)
    q0 = 0
    for b, nqb in enumerate(q_lens):
        w = min(mc, rows[b].shape[1])
        table[q0:q0 + nqb, :w] = rows[b][:, :w]
        q0 += nqb
    table[np.arange(mc)[None, :] >= counts[:, None]] = ns
    return table, counts, mc


def expected(ref, k, ns):
    """the rows a query with k_out = k returns: the reference table cut at k, or padded with ns up to k"""
    table = ref[0]
    out = np.full((table.shape[0], k), ns, np.int32)
    w = min(k, table.shape[1])
    out[:, :w] = table[:, :w]
    return out


# ---- the documented cell rule (include/buffer_hip.h, buf_grid_cell_dims and buf_grid_build) ------------------------------------------
def finite_box(points):
    """per-axis (min, max) over the finite coordinates only, float32; (0, 0) on an axis without one -> (mn f32[3], ext f64[3])"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    mn, ext = np.zeros(3, np.float32), np.zeros(3, np.float64)
    for c in range(3):
        v = p[:, c][np.isfinite(p[:, c])]
        if len(v):
            mn[c] = v.min()
            ext[c] = float(v.max()) - float(v.min())
    return mn, ext


def cell_rule(ext, radius, cells_per_elem):
    """edge = r * 1.00001 (1.0 for r <= 0), times 1.25 until prod(floor(ext / edge) + 1) <= cells_per_elem
    -> (edge, dims int[3], coarsening steps)"""
    r = float(np.float32(radius))
    edge = r * 1.00001 if r > 0 else 1.0
    steps = 0
    while True:
        dims = [np.floor(float(e) / edge) + 1.0 for e in ext]
        if dims[0] * dims[1] * dims[2] <= float(cells_per_elem):
            return edge, [int(d) for d in dims], steps
        edge *= 1.25
        steps += 1


def default_cells(ns, nb):
    """table slots per element when the caller names none (buf_grid_default_cells)"""
    per = (ns + nb - 1) // nb if nb > 0 else ns
    return min(16 * per + 65536, 0x7fff0000 // max(nb, 1))


def cell_coords(points, mn, edge):
    """unclamped integer cell coordinates (float64 arithmetic) of finite points in a grid of origin mn -> int64[n,3]"""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    return np.floor((p - mn.astype(np.float64)[None, :]) / edge).astype(np.int64)


def candidate_sets(supports, s_lens, radius, cells_per_elem=0):
    """per support: how many supports of its element lie in the 27 cells around its own (supports clamped to [0, dim - 1]); all
    coordinates finite -> (int64[ns], list of per-element dims)"""
    s = np.asarray(supports, np.float32).reshape(-1, 3)
    assert np.isfinite(s).all()
    s_lens = np.asarray(s_lens, np.int64)
    cells = cells_per_elem if cells_per_elem > 0 else default_cells(len(s), len(s_lens))
    out = np.zeros(len(s), np.int64)
    all_dims = []
    s0 = 0
    for n in s_lens:
        S = s[s0:s0 + n]
        mn, ext = finite_box(S)
        edge, dims, _ = cell_rule(ext, radius, cells)
        all_dims.append(dims)
        if n:
            c = np.clip(cell_coords(S, mn, edge), 0, np.array(dims) - 1)
            near = (np.abs(c[:, None, :] - c[None, :, :]) <= 1).all(2)          # all pairs again: no table here either
            out[s0:s0 + n] = near.sum(1)
        s0 += n
    return out, all_dims
