"""Patch selection on the device (buffer_amd/csrc/pointops.hip) against the numpy reference of tests/patches_ref.py.

Every selection case runs four ways -- ops.select_patches cloud by cloud (k_select_patches, the brute scan) and
ops.select_patches_batched (k_select_patches_grid) with BUF_SPB_PATH=grid (the LDS bitmask for every query), =scan (the ordered scan for
every query) and unset (the kernel's own choice) -- and each result must equal the reference bit for bit (compared as uint32: there is
no tolerance in this file).  The permutation is compared with patches_ref.prp_perm, the ball query with patches_ref.ball_query_ref.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import patches_cases
import patches_ref

pytestmark = pytest.mark.gpu

PATHS = ('grid', 'scan', None)


@contextlib.contextmanager
def _spb_path(value):
    old = os.environ.get('BUF_SPB_PATH')
    try:
        if value is None:
            os.environ.pop('BUF_SPB_PATH', None)
        else:
            os.environ['BUF_SPB_PATH'] = value
        yield
    finally:
        if old is None:
            os.environ.pop('BUF_SPB_PATH', None)
        else:
            os.environ['BUF_SPB_PATH'] = old


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    got, want = _bits(got), want.view(np.uint32)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        rows = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(1))
        slots = np.flatnonzero((got[rows[0]] != want[rows[0]]).any(1))
        raise AssertionError(f'{what}: {len(rows)} of {got.shape[0]} patches differ; first patch {rows[0]}, slots {slots[:8].tolist()} '
                             f'got {got[rows[0], slots[0]].view(np.float32)} want {want[rows[0], slots[0]].view(np.float32)}')


def _run_case(c, dev, name=None):
    """the four results of a case at every patch size it names, each against the reference"""
    from buffer_amd import ops
    name = name or c.name
    sup_h, kp_h = c.stacked()
    sup, kp = _t(sup_h, dev), _t(kp_h, dev)
    clouds, kpts = [_t(p, dev) for p in c.clouds], [_t(k, dev) for k in c.kpts]
    m = c.m
    for nsample in c.nsamples:
        want = patches_cases.reference(name, nsample) if name in patches_cases.ALL_NAMES else \
            patches_ref.select_patches_batched_ref(sup_h, c.lengths, kp_h, m, c.radius, nsample)
        for i in range(len(clouds)):
            got = ops.select_patches(clouds[i], kpts[i], c.radius, nsample)
            _same(got, want[i * m:(i + 1) * m], f'{name} / nsample {nsample} / select_patches, cloud {i} (n = {c.lengths[i]})')
        for path in PATHS:
            with _spb_path(path):
                got = ops.select_patches_batched(sup, c.lengths, kp, m, c.radius, nsample)
            _same(got, want, f'{name} / nsample {nsample} / select_patches_batched, BUF_SPB_PATH={path}')


def test_exact_sphere(dev):
    """a. points exactly ON a keypoint's sphere stay out, their lattice neighbours one step inside are in (true in any precision)"""
    _run_case(patches_cases.get('exact_sphere'), dev)


@pytest.mark.parametrize('name', ['seams_all_hits', 'seams_chosen_hits'])
def test_mask_seams(name, dev):
    """b. first / last bit of a word, one -> two words per lane (n = 4096 -> 4097), the keep cut inside a word, nmax != n"""
    _run_case(patches_cases.get(name), dev)


def _grid_rule(case):
    """cell edge and dims of every cloud's grid, by the build's own rule"""
    from buffer_amd import _lib, ops
    cells = _lib.lib().buf_grid_default_cells(sum(case.lengths), len(case.lengths))
    out = [ops.grid_cell_dims([float(hi) - float(lo) for lo, hi in zip(p.min(0), p.max(0))], case.radius, cells) for p in case.clouds]
    return [e for e, _ in out], [d for _, d in out]


def test_keypoints_outside_the_box(dev):
    """c. keypoints beyond each face of the support cloud's box, within and beyond r of the points on that face"""
    edges, _ = _grid_rule(patches_cases.get('outside_box'))
    c = patches_cases.outside_box(edges)
    hits = [patches_ref.in_ball(p, k, c.radius).any(1).reshape(6, 6) for p, k in zip(c.clouds, c.kpts)]
    assert all(h[:, :2].all() and not h[:, 3:].any() for h in hits)
    _run_case(c, dev, 'outside_box (edge from the grid rule)')


def test_keypoints_on_cell_edges(dev):
    """c. keypoints at mn + j * edge rounded to float32 and at its two float32 neighbours, edge from the build's own rule"""
    edges, dims = _grid_rule(patches_cases.get('cell_edges'))
    _run_case(patches_cases.cell_edges(edges, dims), dev, 'cell_edges (edge from the grid rule)')


def test_coarsened_grid_and_nonfinite_data(dev):
    """d. a point 10 km away, a point at 1e30, NaN / inf support points at index 0, n/2, n-1 and NaN / inf keypoints"""
    _run_case(patches_cases.get('coarse_and_nonfinite'), dev)


@pytest.mark.parametrize('name', patches_cases.BATCH_NAMES)
def test_batch_structure(name, dev):
    """e. empty clouds first / middle / last, one cloud, m in {0, 1, 5, 9}, 6 / 8 / 9 / 15 workgroups (the XCD block remap's seams)"""
    from buffer_amd import ops
    c = patches_cases.get(name)
    if c.m == 0:
        sup, kp = c.stacked()
        for path in PATHS:
            with _spb_path(path):
                assert ops.select_patches_batched(_t(sup, dev), c.lengths, _t(kp, dev), 0, c.radius, 32).shape == (0, 32, 3)
        return
    _run_case(c, dev)


@pytest.mark.parametrize('name', patches_cases.LARGE_NAMES)
def test_large_mask(name, dev):
    """f. 98 305 and 131 072 points: the mask of a workgroup takes granted LDS above 48 KB; 131 073: no mask, 'grid' falls back to the scan"""
    _run_case(patches_cases.get(name), dev)


@pytest.mark.parametrize('n', patches_cases.BQ_N)
def test_ball_query_c_abi(n, dev):
    """g. buf_ball_query writes every slot of every row (the output starts as -1): nsample reached inside a 64-block, first hit in a
    later block, padding with the first hit, empty rows zero"""
    from buffer_amd import _lib
    L = _lib.lib()
    xyz, new, r = patches_cases.ball_query_case(n)
    b, m = patches_cases.BQ_B, patches_cases.BQ_M
    assert m % 4 != 0
    tx, tn = _t(xyz, dev), _t(new, dev)
    for nsample in (5, 16):
        out = torch.full((b, m, nsample), -1, dtype=torch.int32, device=dev)
        rc = L.buf_ball_query(C.c_void_p(tx.data_ptr()), C.c_void_p(tn.data_ptr()), b, n, m, C.c_float(r), nsample, C.c_void_p(out.data_ptr()),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        want = patches_ref.ball_query_ref(r, nsample, xyz, new)
        assert np.array_equal(out.cpu().numpy(), want), (n, nsample)


PERM_EXTRA = (1023, 1024, 1025, 65535, 65536, 65537, 262145)


def _perm_lengths():
    """every n in 0..257 and PERM_EXTRA in one call: 63 clouds, three empty ones at positions 63, 64, 65 (either side of the first
    chunk seam), the rest; then two (n, key) of the first chunk again, in a later chunk"""
    ns = list(range(1, 64)) + [0, 0, 0] + list(range(64, 258)) + list(PERM_EXTRA)
    again = [(36, ns[36]), (202, ns[202])]                            # (position whose key is reused, n): chunks 0 and 3, met again in chunk 4
    return ns, again


def test_permute_clouds_equals_the_restated_permutation(dev):
    """h. index-valued clouds (row i = (i, i + 0.25, -i)) across the 64-cloud chunks of buf_permute_clouds"""
    from buffer_amd import ops
    ns, again = _perm_lengths()
    assert len(ns) > 4 * 64 and ns[63:66] == [0, 0, 0] and set(range(258)) | set(PERM_EXTRA) == set(ns)
    keys = [ops.perm_key(17, j) for j in range(len(ns))]
    for pos, n in again:
        ns.append(n)
        keys.append(keys[pos])
    assert again[0][0] // 64 != (len(ns) - 2) // 64 and again[1][0] // 64 != (len(ns) - 1) // 64
    i = torch.arange(max(ns), dtype=torch.float32, device=dev)
    rows = torch.stack([i, i + 0.25, -i], 1).contiguous()
    clouds = [rows[:n] for n in ns]
    out, lens = ops.permute_clouds(clouds, keys)
    assert lens.tolist() == ns and out.shape == (sum(ns), 3)
    got = out.cpu().numpy()
    lo = 0
    perms = []
    for n, key in zip(ns, keys):
        perm = patches_ref.prp_perm(n, key)
        perms.append(perm)
        want = np.stack([perm, perm + 0.25, -perm], 1).astype(np.float32)
        assert np.array_equal(got[lo:lo + n], want), f'cloud at position {len(perms) - 1} (n = {n})'
        lo += n
    for j, (pos, n) in enumerate(again):
        assert np.array_equal(perms[pos], perms[len(ns) - 2 + j])
    hi = len(got) - ns[-1]
    assert np.array_equal(got[hi:, 0].astype(np.int64), perms[again[1][0]])       # (the device rows themselves, not only the restatement)


def test_permute_clouds_moves_bit_patterns(dev):
    """h. NaN payloads and -0.0 come out with their bits intact and their rows unbroken, on both sides of a chunk seam"""
    from buffer_amd import ops
    n = 300
    i = np.arange(n, dtype=np.uint32)
    src = np.stack([np.uint32(0x7fc00000) | i, np.where(i % 2 == 0, np.uint32(0x80000000), np.uint32(0xffc00000) | i), np.uint32(0x7f800001) + i], 1)
    t = torch.from_numpy(src.view(np.float32)).to(dev)
    filler = torch.zeros((3, 3), dtype=torch.float32, device=dev)
    clouds = [filler] * 63 + [t, t]                                   # positions 63 (last of chunk 0) and 64 (first of chunk 1)
    keys = [ops.perm_key(5, j) for j in range(len(clouds))]
    out, _ = ops.permute_clouds(clouds, keys)
    got = out.cpu().numpy().view(np.uint32)
    for j, pos in enumerate((63, 64)):
        lo = 3 * 63 + j * n
        assert np.array_equal(got[lo:lo + n], src[patches_ref.prp_perm(n, keys[pos])]), pos


def test_permutation_then_selection(dev):
    """i. permute_clouds followed by select_patches_batched == the reference on the restated permutation of each cloud"""
    from buffer_amd import ops
    c = patches_cases.get('composition')
    keys = [ops.perm_key(23, j) for j in range(2)]
    sup, lens = ops.permute_clouds([_t(p, dev) for p in c.clouds], keys)
    assert lens.tolist() == c.lengths
    kp = _t(np.concatenate(c.kpts), dev)
    want = np.concatenate([patches_ref.select_patches_ref(p[patches_ref.prp_perm(len(p), key)], k, c.radius, 512)
                           for p, k, key in zip(c.clouds, c.kpts, keys)])
    for path in PATHS:
        with _spb_path(path):
            got = ops.select_patches_batched(sup, lens, kp, c.m, c.radius, 512)
        _same(got, want, f'composition / BUF_SPB_PATH={path}')
    _run_case(c, dev)                                                 # and the unpermuted clouds, the four ways
