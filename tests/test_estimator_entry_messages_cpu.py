"""Return code and FULL buf_last_error() text of a fixed list of bad calls to the batched pose estimators (buf_icp_batched,
buf_gicp_batched, buf_vgicp_batched, buf_fgr_batched, buf_sc2_batched, buf_clique_batched), the values of their *_ws_bytes queries, and
the ValueError texts of the five buffer_amd.ops functions in front of them (mismatched lengths, wrong widths, limits out of range).
Every condition is decided before the first device call, so dummy pointers do; no GPU needed.  buf_vgicp_batched is reached without
a built map (null handle, empty handle) and with a hand-filled handle of two clouds, which its checks read and nothing else does.

EXPECTED and EXPECTED_OPS were recorded by running this list against a build and the ops.py of the commit BEFORE the estimators'
host checks were folded onto shared helpers (`BUF_LIB_PATH=<that build> PYTHONPATH=<that tree> python
tests/test_estimator_entry_messages_cpu.py` prints both tables) and pasted in: the fold moved no code, no text and no order."""
import ctypes as C
import os
import sys

import pytest

if __name__ == '__main__':          # run as a script: this tree's buffer_amd, unless PYTHONPATH names another
    sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

I32_MAX = 0x7fffffff


def ints(*v):
    return (C.c_int * len(v))(*v)


def bad_calls():
    """[(label, entry point, arguments)] and the objects the arguments point into"""
    from buffer_amd._lib import buf_voxel_map_t
    dummy = (C.c_double * 16)()
    x = C.addressof(dummy)
    keep = [dummy]
    one, two, neg, huge = ints(5), ints(5, 7), ints(5, -1), ints(I32_MAX)
    many = (C.c_int * 65536)()
    seeds = (C.c_uint64 * 2)(1, 2)
    keep += [one, two, neg, huge, many, seeds]
    out = []

    def case(fn, order, base, label, **over):
        unknown = set(over) - set(order)
        assert not unknown, unknown
        out.append((f'{fn[4:]}: {label}', fn, tuple({**base, **over}[k] for k in order)))

    # ---- buf_icp_batched / buf_gicp_batched
    icp_order = ('src', 'sl', 'tgt', 'tnrm', 'tl', 'npairs', 'method', 'max_dist', 'T_init', 'max_it', 'rf', 'rr', 'T', 'fit', 'rmse', 'iters',
                 'nn', 'ws', 'ws_bytes', 'stream')
    gicp_order = ('src', 'snrm', 'sl', 'tgt', 'tnrm', 'tl', 'npairs', 'max_dist', 'eps', 'T_init', 'max_it', 'rf', 'rr', 'T', 'fit', 'rmse',
                  'iters', 'nn', 'ws', 'ws_bytes', 'stream')
    base = dict(src=x, snrm=x, sl=two, tgt=x, tnrm=x, tl=two, npairs=2, method=0, max_dist=0.1, eps=1e-3, T_init=x, max_it=30, rf=1e-6,
                rr=1e-6, T=x, fit=x, rmse=x, iters=x, nn=None, ws=x, ws_bytes=0, stream=None)
    for fn, order in (('buf_icp_batched', icp_order), ('buf_gicp_batched', gicp_order)):
        c = lambda label, **over: case(fn, order, base, label, **over)
        if fn == 'buf_icp_batched':
            c('unknown method', method=3)
            c('the generalized method', method=2)
            c('negative method', method=-1)
            c('point-to-plane without normals', method=1, tnrm=None)
        else:
            c('epsilon 0', eps=0.0)
            c('epsilon above 1', eps=1.5)
            c('epsilon nan', eps=float('nan'))
            c('no source normals', snrm=None)
            c('no target normals', tnrm=None)
        c('negative pairs', npairs=-1)
        c('max_dist 0', max_dist=0.0)
        c('max_dist inf', max_dist=float('inf'))
        c('max_dist nan', max_dist=float('nan'))
        c('negative max_iteration', max_it=-1)
        c('null source lengths', sl=None)
        c('null target lengths', tl=None)
        c('negative source length', sl=neg)
        c('negative target length', tl=neg)
        c('too many source points', sl=huge, npairs=1)
        c('too many target points', tl=huge, npairs=1)
        c('null src', src=None)
        c('null tgt', tgt=None)
        c('null T_init', T_init=None)
        c('null T', T=None)
        c('null fitness', fit=None)
        c('null rmse', rmse=None)
        c('null iterations', iters=None)
        c('null workspace', ws=None)
        c('too many pairs', npairs=65536, sl=many, tl=many)
        c('workspace too small', ws_bytes=1000)
        c('bad max_dist before bad lengths', max_dist=-1.0, sl=None)
        c('negative length before the totals', sl=ints(I32_MAX, -1))
    for m in (0, 1, 2):
        out.append((f'icp_ws_bytes: method {m}', 'buf_icp_ws_bytes', (700, 900, 3, m)))
    out += [('icp_ws_bytes: unknown method', 'buf_icp_ws_bytes', (700, 900, 3, 3)), ('icp_ws_bytes: no pairs', 'buf_icp_ws_bytes', (700, 900, 0, 0)),
            ('icp_ws_bytes: negative rows', 'buf_icp_ws_bytes', (-1, 900, 3, 0)), ('icp_ws_bytes: empty clouds', 'buf_icp_ws_bytes', (0, 0, 1, 1))]

    # ---- buf_vgicp_batched
    empty, filled = buf_voxel_map_t(), buf_voxel_map_t()
    filled.buf, filled.buf_bytes, filled.nclouds, filled.nrows, filled.n, filled.max_cells, filled.voxel, filled.epsilon = x, 128, 2, 0, 0, 8, 0.5, 1e-3
    keep += [empty, filled]
    vg_order = ('map', 'src', 'snrm', 'sl', 'pc', 'npairs', 'neighbors', 'T_init', 'max_it', 'rf', 'rr', 'T', 'fit', 'rmse', 'iters', 'row', 'ws',
                'ws_bytes', 'stream')
    vbase = dict(map=C.byref(filled), src=x, snrm=None, sl=two, pc=None, npairs=2, neighbors=7, T_init=x, max_it=30, rf=1e-6, rr=1e-6, T=x, fit=x,
                 rmse=x, iters=x, row=None, ws=x, ws_bytes=0, stream=None)
    c = lambda label, **over: case('buf_vgicp_batched', vg_order, vbase, label, **over)
    c('null map', map=None)
    c('empty map', map=C.byref(empty))
    c('negative pairs', npairs=-1)
    c('too many pairs', npairs=65536, sl=many)
    c('neighbors 0', neighbors=0)
    c('neighbors 9', neighbors=9)
    c('negative max_iteration', max_it=-1)
    c('null lengths', sl=None)
    c('more pairs than clouds', npairs=3, sl=ints(1, 2, 3))
    c('negative length', sl=neg)
    c('pair_cloud below the map', pc=ints(0, -1))
    c('pair_cloud above the map', pc=ints(2, 0))
    c('negative length before pair_cloud', sl=neg, pc=ints(0, 5))
    c('too many points', sl=huge, npairs=1)
    c('null src', src=None)
    c('null T_init', T_init=None)
    c('null T', T=None)
    c('null iterations', iters=None)
    c('null workspace', ws=None)
    c('workspace too small', ws_bytes=1000)
    c('three pairs on two clouds with pair_cloud, workspace too small', npairs=3, sl=ints(1, 2, 3), pc=ints(1, 1, 0), ws_bytes=8)
    out += [('vgicp_ws_bytes: 700 rows of 3 pairs', 'buf_vgicp_ws_bytes', (700, 3)), ('vgicp_ws_bytes: no rows', 'buf_vgicp_ws_bytes', (0, 1)),
            ('vgicp_ws_bytes: no pairs', 'buf_vgicp_ws_bytes', (700, 0)), ('vgicp_ws_bytes: negative rows', 'buf_vgicp_ws_bytes', (-1, 3))]

    # ---- the three estimators on correspondences
    head = ('src', 'sl', 'tgt', 'tl', 'corr', 'cl', 'npairs')
    tail = ('ws', 'ws_bytes', 'stream')
    fgr_order = head + ('seeds', 'tuple_scale', 'max_tuples', 'trial_factor', 'mu', 'delta', 'dabs', 'div', 'every', 'its', 'T', 'info', 'rows',
                        'weights') + tail
    sc2_order = head + ('d_thr', 'inl', 'ratio', 'max_seeds', 'k1', 'nms', 'pit', 'rit', 'T', 'info', 'conf', 'seeds_out', 'hypc', 'counts',
                        'mask') + tail
    clq_order = head + ('d_thr', 'tim', 't_thr', 'inl', 'max_seeds', 'max_members', 'gnc', 'git', 'rit', 'T', 'info', 'deg', 'core', 'rank', 'sizes',
                        'members', 'weights', 'pose0', 'mask') + tail
    cbase = dict(src=x, sl=two, tgt=x, tl=two, corr=x, cl=two, npairs=2, T=x, info=x, ws=x, ws_bytes=0, stream=None)
    fbase = dict(cbase, seeds=seeds, tuple_scale=0.95, max_tuples=100, trial_factor=100, mu=1.0, delta=0.025, dabs=0, div=1.4, every=4, its=64,
                 rows=None, weights=None)
    sbase = dict(cbase, d_thr=0.1, inl=0.1, ratio=0.2, max_seeds=64, k1=30, nms=0.0, pit=10, rit=20, conf=None, seeds_out=None, hypc=None,
                 counts=None, mask=None)
    qbase = dict(cbase, d_thr=0.1, tim=0.1, t_thr=0.05, inl=0.1, max_seeds=64, max_members=256, gnc=1.4, git=100, rit=20, deg=None, core=None,
                 rank=None, sizes=None, members=None, weights=None, pose0=None, mask=None)
    inf, nan = float('inf'), float('nan')
    for fn, order, b in (('buf_fgr_batched', fgr_order, fbase), ('buf_sc2_batched', sc2_order, sbase), ('buf_clique_batched', clq_order, qbase)):
        c = lambda label, **over: case(fn, order, b, label, **over)
        c('negative pairs', npairs=-1)
        if fn == 'buf_fgr_batched':
            c('tuple_scale 0', tuple_scale=0.0)
            c('tuple_scale above 1', tuple_scale=1.01)
            c('max_tuples 0', max_tuples=0)
            c('max_tuples 4097', max_tuples=4097)
            c('trial_factor 0', trial_factor=0)
            c('mu_start 0', mu=0.0)
            c('mu_start inf', mu=inf)
            c('delta nan', delta=nan)
            c('division_factor 1', div=1.0)
            c('decrease_every 0', every=0)
            c('negative iterations', its=-1)
            c('null seeds', seeds=None)
            c('trial_factor overflow', trial_factor=I32_MAX, cl=ints(0, 2))
            c('negative length before the overflow', trial_factor=I32_MAX, cl=ints(-1, 2))
            c('overflow in pair 0 before a negative length in pair 1', trial_factor=I32_MAX, cl=ints(2, -1))
        else:
            c('too many pairs', npairs=65536, sl=many, tl=many, cl=many)
            c('d_thr 0', d_thr=0.0)
            c('d_thr with an infinite square', d_thr=1e200)
            c('inlier_thr nan', inl=nan)
            c('max_seeds 0', max_seeds=0)
            c('max_seeds 1025', max_seeds=1025)
            c('negative refine_iterations', rit=-1)
            c('too many correspondences in a pair', cl=ints(3, 16385))
            c('negative length before the row limit', cl=ints(-1, 16385))
            c('row limit in pair 0 before a negative length in pair 1', cl=ints(16385, -1))
        if fn == 'buf_sc2_batched':
            c('seed_ratio 0', ratio=0.0)
            c('seed_ratio above 1', ratio=1.5)
            c('k1 2', k1=2)
            c('k1 129', k1=129)
            c('nms_radius negative', nms=-1.0)
            c('power_iterations 1001', pit=1001)
        if fn == 'buf_clique_batched':
            c('tim_thr with a zero square', tim=1e-200)
            c('t_thr 0', t_thr=0.0)
            c('max_members 2', max_members=2)
            c('max_members 513', max_members=513)
            c('gnc_factor 1', gnc=1.0)
            c('gnc_iterations 0', git=0)
            c('gnc_iterations 1001', git=1001)
        c('null source lengths', sl=None)
        c('null target lengths', tl=None)
        c('null correspondence lengths', cl=None)
        c('null T', T=None)
        c('null info', info=None)
        c('null lengths before null outputs', sl=None, T=None)
        c('negative source length', sl=neg)
        c('negative target length', tl=neg)
        c('negative correspondence length', cl=neg)
        c('too many source points', sl=huge, npairs=1)
        c('too many target points', tl=huge, npairs=1)
        c('null src', src=None)
        c('null tgt', tgt=None)
        c('null corr', corr=None)
        c('null outputs before null inputs', src=None, info=None)
        c('null workspace', ws=None, ws_bytes=1 << 40)
        c('workspace too small', ws_bytes=1000)
    out += [('fgr_ws_bytes: 300 rows of 3 pairs', 'buf_fgr_ws_bytes', (300, 3, 1000)), ('fgr_ws_bytes: max_tuples 4097', 'buf_fgr_ws_bytes', (300, 3, 4097)),
            ('fgr_ws_bytes: no pairs', 'buf_fgr_ws_bytes', (300, 0, 1000)), ('fgr_ws_bytes: negative rows', 'buf_fgr_ws_bytes', (-1, 3, 1000))]
    six = ints(0, 2, 3, 64, 65, 300)
    keep.append(six)
    out += [('sc2_ws_bytes: six pairs', 'buf_sc2_ws_bytes', (six, 6, 64)), ('sc2_ws_bytes: null lengths', 'buf_sc2_ws_bytes', (None, 6, 64)),
            ('sc2_ws_bytes: max_seeds 1025', 'buf_sc2_ws_bytes', (six, 6, 1025)), ('sc2_ws_bytes: a pair above the row limit', 'buf_sc2_ws_bytes', (ints(3, 16385), 2, 64)),
            ('sc2_ws_bytes: negative length', 'buf_sc2_ws_bytes', (neg, 2, 64)),
            ('clique_ws_bytes: six pairs', 'buf_clique_ws_bytes', (six, 6, 64, 256)), ('clique_ws_bytes: null lengths', 'buf_clique_ws_bytes', (None, 6, 64, 256)),
            ('clique_ws_bytes: max_members 2', 'buf_clique_ws_bytes', (six, 6, 64, 2)), ('clique_ws_bytes: max_seeds 0', 'buf_clique_ws_bytes', (six, 6, 0, 256)),
            ('clique_ws_bytes: a pair above the row limit', 'buf_clique_ws_bytes', (ints(3, 16385), 2, 64, 256))]
    return out, keep


def bad_ops_calls():
    """[(label, function of buffer_amd.ops, args, kwargs)]: each raises ValueError before it reaches the library"""
    import torch
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32)
    corr = lambda n: torch.zeros((n, 2), dtype=torch.int32)
    T2 = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    out = []
    for fn, extra in (('fgr_batched', ()), ('sc2_batched', (0.1, 0.1)), ('clique_batched', (0.1,))):
        c = lambda label, *a, **kw: out.append((f'{fn}: {label}', fn, a + extra, kw))
        c('target lengths of another batch', f32(12, 3), [5, 7], f32(12, 3), [12], corr(4), [2, 2])
        c('correspondence lengths of another batch', f32(12, 3), [5, 7], f32(12, 3), [5, 7], corr(4), [1, 2, 1])
        c('src of width 4', f32(12, 4), [5, 7], f32(12, 3), [5, 7], corr(4), [2, 2])
        c('flat tgt', f32(12, 3), [5, 7], f32(36), [5, 7], corr(4), [2, 2])
        c('corr of width 3', f32(12, 3), [5, 7], f32(12, 3), [5, 7], torch.zeros((4, 3), dtype=torch.int32), [2, 2])
        c('src lengths off the rows', f32(12, 3), [5, 8], f32(12, 3), [5, 7], corr(4), [2, 2])
        c('negative tgt length', f32(12, 3), [5, 7], f32(12, 3), [13, -1], corr(4), [2, 2])
        c('corr lengths off the rows', f32(12, 3), [5, 7], f32(12, 3), [5, 7], corr(4), [2, 3])
        good = (f32(12, 3), [5, 7], f32(12, 3), [5, 7], corr(4), [2, 2])
        if fn == 'fgr_batched':
            c('max_tuples 0', *good, max_tuples=0)
            c('max_tuples 4097', *good, max_tuples=4097)
            c('one seed for two pairs', *good, seeds=[3])
        else:
            c('a pair above the row limit', f32(12, 3), [5, 7], f32(12, 3), [5, 7], corr(16388), [3, 16385])
            c('max_seeds 0', *good, max_seeds=0)
            c('max_seeds 1025', *good, max_seeds=1025)
        if fn == 'sc2_batched':
            c('k1 2', *good, k1=2)
            c('k1 129', *good, k1=129)
        if fn == 'clique_batched':
            c('max_members 2', *good, max_members=2)
            c('max_members 513', *good, max_members=513)
    c = lambda label, *a, **kw: out.append((f'icp_batched: {label}', 'icp_batched', a, kw))
    pair = (f32(12, 3), [5, 7], f32(12, 3), [5, 7], 0.1, T2)
    c('generalized without source normals', *pair, method='generalized', tgt_normals=f32(12, 3))
    c('generalized without target normals', *pair, method='generalized', src_normals=f32(12, 3))
    c('epsilon 0', *pair, method='generalized', src_normals=f32(12, 3), tgt_normals=f32(12, 3), epsilon=0.0)
    c('epsilon above 1', *pair, method='generalized', src_normals=f32(12, 3), tgt_normals=f32(12, 3), epsilon=2)
    c('source normals of another shape', *pair, method='generalized', src_normals=f32(11, 3), tgt_normals=f32(12, 3))
    c('target normals of another shape', *pair, method='generalized', src_normals=f32(12, 3), tgt_normals=f32(4, 9))
    c = lambda label, *a, **kw: out.append((f'vgicp_batched: {label}', 'vgicp_batched', a, kw))
    c('neighbors 9', f32(12, 3), [5, 7], None, T2, neighbors=9)
    c('neighbors 0', f32(12, 3), [5, 7], None, T2, neighbors=0)
    c('source normals of another shape', f32(12, 3), [5, 7], None, T2, src_normals=f32(11, 3))
    c('three pair_cloud entries for two pairs', f32(12, 3), [5, 7], None, T2, pair_cloud=[0, 1, 1])
    return out


EXPECTED = {
    'icp_batched: unknown method': (-1, 'buf_icp_batched: unknown method 3'),
    'icp_batched: the generalized method': (-1, 'buf_icp_batched: unknown method 2'),
    'icp_batched: negative method': (-1, 'buf_icp_batched: unknown method -1'),
    'icp_batched: point-to-plane without normals': (-1, 'buf_icp_batched: point-to-plane needs target normals'),
    'icp_batched: negative pairs': (-1, 'buf_icp_batched: npairs=-1'),
    'icp_batched: max_dist 0': (-1, 'buf_icp_batched: max_dist=0 (must be finite and > 0)'),
    'icp_batched: max_dist inf': (-1, 'buf_icp_batched: max_dist=inf (must be finite and > 0)'),
    'icp_batched: max_dist nan': (-1, 'buf_icp_batched: max_dist=nan (must be finite and > 0)'),
    'icp_batched: negative max_iteration': (-1, 'buf_icp_batched: max_iteration=-1'),
    'icp_batched: null source lengths': (-1, 'buf_icp_batched: null lengths'),
    'icp_batched: null target lengths': (-1, 'buf_icp_batched: null lengths'),
    'icp_batched: negative source length': (-1, 'buf_icp_batched: negative length in pair 1'),
    'icp_batched: negative target length': (-1, 'buf_icp_batched: negative length in pair 1'),
    'icp_batched: too many source points': (-1, 'buf_icp_batched: 2147483647 / 5 points (int32 indices)'),
    'icp_batched: too many target points': (-1, 'buf_icp_batched: 5 / 2147483647 points (int32 indices)'),
    'icp_batched: null src': (-1, 'buf_icp_batched: null src'),
    'icp_batched: null tgt': (-1, 'buf_icp_batched: null tgt'),
    'icp_batched: null T_init': (-1, 'buf_icp_batched: null argument'),
    'icp_batched: null T': (-1, 'buf_icp_batched: null argument'),
    'icp_batched: null fitness': (-1, 'buf_icp_batched: null argument'),
    'icp_batched: null rmse': (-1, 'buf_icp_batched: null argument'),
    'icp_batched: null iterations': (-1, 'buf_icp_batched: null argument'),
    'icp_batched: null workspace': (-1, 'buf_icp_batched: null argument'),
    'icp_batched: too many pairs': (-1, 'buf_icp_batched: 65536 pairs (at most 65535 per call)'),
    'icp_batched: workspace too small': (-3, 'buf_icp_batched: workspace 1000 < 534272 bytes'),
    'icp_batched: bad max_dist before bad lengths': (-1, 'buf_icp_batched: max_dist=-1 (must be finite and > 0)'),
    'icp_batched: negative length before the totals': (-1, 'buf_icp_batched: negative length in pair 1'),
    'gicp_batched: epsilon 0': (-1, 'buf_gicp_batched: epsilon=0 (must be in (0, 1])'),
    'gicp_batched: epsilon above 1': (-1, 'buf_gicp_batched: epsilon=1.5 (must be in (0, 1])'),
    'gicp_batched: epsilon nan': (-1, 'buf_gicp_batched: epsilon=nan (must be in (0, 1])'),
    'gicp_batched: no source normals': (-1, 'buf_gicp_batched: Generalized ICP needs source and target normals'),
    'gicp_batched: no target normals': (-1, 'buf_gicp_batched: Generalized ICP needs source and target normals'),
    'gicp_batched: negative pairs': (-1, 'buf_gicp_batched: npairs=-1'),
    'gicp_batched: max_dist 0': (-1, 'buf_gicp_batched: max_dist=0 (must be finite and > 0)'),
    'gicp_batched: max_dist inf': (-1, 'buf_gicp_batched: max_dist=inf (must be finite and > 0)'),
    'gicp_batched: max_dist nan': (-1, 'buf_gicp_batched: max_dist=nan (must be finite and > 0)'),
    'gicp_batched: negative max_iteration': (-1, 'buf_gicp_batched: max_iteration=-1'),
    'gicp_batched: null source lengths': (-1, 'buf_gicp_batched: null lengths'),
    'gicp_batched: null target lengths': (-1, 'buf_gicp_batched: null lengths'),
    'gicp_batched: negative source length': (-1, 'buf_gicp_batched: negative length in pair 1'),
    'gicp_batched: negative target length': (-1, 'buf_gicp_batched: negative length in pair 1'),
    'gicp_batched: too many source points': (-1, 'buf_gicp_batched: 2147483647 / 5 points (int32 indices)'),
    'gicp_batched: too many target points': (-1, 'buf_gicp_batched: 5 / 2147483647 points (int32 indices)'),
    'gicp_batched: null src': (-1, 'buf_gicp_batched: null src'),
    'gicp_batched: null tgt': (-1, 'buf_gicp_batched: null tgt'),
    'gicp_batched: null T_init': (-1, 'buf_gicp_batched: null argument'),
    'gicp_batched: null T': (-1, 'buf_gicp_batched: null argument'),
    'gicp_batched: null fitness': (-1, 'buf_gicp_batched: null argument'),
    'gicp_batched: null rmse': (-1, 'buf_gicp_batched: null argument'),
    'gicp_batched: null iterations': (-1, 'buf_gicp_batched: null argument'),
    'gicp_batched: null workspace': (-1, 'buf_gicp_batched: null argument'),
    'gicp_batched: too many pairs': (-1, 'buf_gicp_batched: 65536 pairs (at most 65535 per call)'),
    'gicp_batched: workspace too small': (-3, 'buf_gicp_batched: workspace 1000 < 534528 bytes'),
    'gicp_batched: bad max_dist before bad lengths': (-1, 'buf_gicp_batched: max_dist=-1 (must be finite and > 0)'),
    'gicp_batched: negative length before the totals': (-1, 'buf_gicp_batched: negative length in pair 1'),
    'icp_ws_bytes: method 0': (964352, ''),
    'icp_ws_bytes: method 1': (964864, ''),
    'icp_ws_bytes: method 2': (964864, ''),
    'icp_ws_bytes: unknown method': (0, ''),
    'icp_ws_bytes: no pairs': (0, ''),
    'icp_ws_bytes: negative rows': (0, ''),
    'icp_ws_bytes: empty clouds': (270336, ''),
    'vgicp_batched: null map': (-1, 'buf_vgicp_batched: no voxel map'),
    'vgicp_batched: empty map': (-1, 'buf_vgicp_batched: no voxel map'),
    'vgicp_batched: negative pairs': (-1, 'buf_vgicp_batched: npairs=-1 (0..65535)'),
    'vgicp_batched: too many pairs': (-1, 'buf_vgicp_batched: npairs=65536 (0..65535)'),
    'vgicp_batched: neighbors 0': (-1, 'buf_vgicp_batched: neighbors=0 (1, 7 or 27)'),
    'vgicp_batched: neighbors 9': (-1, 'buf_vgicp_batched: neighbors=9 (1, 7 or 27)'),
    'vgicp_batched: negative max_iteration': (-1, 'buf_vgicp_batched: max_iteration=-1'),
    'vgicp_batched: null lengths': (-1, 'buf_vgicp_batched: null lengths'),
    'vgicp_batched: more pairs than clouds': (-1, 'buf_vgicp_batched: 3 pairs but 2 map clouds and no pair_cloud'),
    'vgicp_batched: negative length': (-1, 'buf_vgicp_batched: negative length in pair 1'),
    'vgicp_batched: pair_cloud below the map': (-1, "buf_vgicp_batched: pair_cloud[1]=-1 outside the map's 2 clouds"),
    'vgicp_batched: pair_cloud above the map': (-1, "buf_vgicp_batched: pair_cloud[0]=2 outside the map's 2 clouds"),
    'vgicp_batched: negative length before pair_cloud': (-1, 'buf_vgicp_batched: negative length in pair 1'),
    'vgicp_batched: too many points': (-1, 'buf_vgicp_batched: 2147483647 points (int32 indices)'),
    'vgicp_batched: null src': (-1, 'buf_vgicp_batched: null src'),
    'vgicp_batched: null T_init': (-1, 'buf_vgicp_batched: null argument'),
    'vgicp_batched: null T': (-1, 'buf_vgicp_batched: null argument'),
    'vgicp_batched: null iterations': (-1, 'buf_vgicp_batched: null argument'),
    'vgicp_batched: null workspace': (-1, 'buf_vgicp_batched: null argument'),
    'vgicp_batched: workspace too small': (-3, 'buf_vgicp_batched: workspace 1000 < 2048 bytes'),
    'vgicp_batched: three pairs on two clouds with pair_cloud, workspace too small': (-3, 'buf_vgicp_batched: workspace 8 < 2304 bytes'),
    'vgicp_ws_bytes: 700 rows of 3 pairs': (2816, ''),
    'vgicp_ws_bytes: no rows': (1536, ''),
    'vgicp_ws_bytes: no pairs': (0, ''),
    'vgicp_ws_bytes: negative rows': (0, ''),
    'fgr_batched: negative pairs': (-1, 'buf_fgr_batched: npairs=-1'),
    'fgr_batched: tuple_scale 0': (-1, 'buf_fgr_batched: tuple_scale=0 (must be in (0, 1])'),
    'fgr_batched: tuple_scale above 1': (-1, 'buf_fgr_batched: tuple_scale=1.01 (must be in (0, 1])'),
    'fgr_batched: max_tuples 0': (-1, 'buf_fgr_batched: max_tuples=0 (1..4096)'),
    'fgr_batched: max_tuples 4097': (-1, 'buf_fgr_batched: max_tuples=4097 (1..4096)'),
    'fgr_batched: trial_factor 0': (-1, 'buf_fgr_batched: trial_factor=0'),
    'fgr_batched: mu_start 0': (-1, 'buf_fgr_batched: mu_start=0 (must be finite and > 0)'),
    'fgr_batched: mu_start inf': (-1, 'buf_fgr_batched: mu_start=inf (must be finite and > 0)'),
    'fgr_batched: delta nan': (-1, 'buf_fgr_batched: delta=nan (must be finite and > 0)'),
    'fgr_batched: division_factor 1': (-1, 'buf_fgr_batched: division_factor=1 (must be finite and > 1)'),
    'fgr_batched: decrease_every 0': (-1, 'buf_fgr_batched: decrease_every=0 iterations=64'),
    'fgr_batched: negative iterations': (-1, 'buf_fgr_batched: decrease_every=4 iterations=-1'),
    'fgr_batched: null seeds': (-1, 'buf_fgr_batched: null host array'),
    'fgr_batched: trial_factor overflow': (-1, 'buf_fgr_batched: trial_factor * 2 correspondences of pair 1 overflows int'),
    'fgr_batched: negative length before the overflow': (-1, 'buf_fgr_batched: negative length in pair 0'),
    'fgr_batched: overflow in pair 0 before a negative length in pair 1': (-1, 'buf_fgr_batched: trial_factor * 2 correspondences of pair 0 overflows int'),
    'fgr_batched: null source lengths': (-1, 'buf_fgr_batched: null host array'),
    'fgr_batched: null target lengths': (-1, 'buf_fgr_batched: null host array'),
    'fgr_batched: null correspondence lengths': (-1, 'buf_fgr_batched: null host array'),
    'fgr_batched: null T': (-1, 'buf_fgr_batched: null output'),
    'fgr_batched: null info': (-1, 'buf_fgr_batched: null output'),
    'fgr_batched: null lengths before null outputs': (-1, 'buf_fgr_batched: null host array'),
    'fgr_batched: negative source length': (-1, 'buf_fgr_batched: negative length in pair 1'),
    'fgr_batched: negative target length': (-1, 'buf_fgr_batched: negative length in pair 1'),
    'fgr_batched: negative correspondence length': (-1, 'buf_fgr_batched: negative length in pair 1'),
    'fgr_batched: too many source points': (-1, 'buf_fgr_batched: 2147483647 / 5 points, 5 correspondences (int32 indices)'),
    'fgr_batched: too many target points': (-1, 'buf_fgr_batched: 5 / 2147483647 points, 5 correspondences (int32 indices)'),
    'fgr_batched: null src': (-1, 'buf_fgr_batched: null input'),
    'fgr_batched: null tgt': (-1, 'buf_fgr_batched: null input'),
    'fgr_batched: null corr': (-1, 'buf_fgr_batched: null input'),
    'fgr_batched: null outputs before null inputs': (-1, 'buf_fgr_batched: null output'),
    'fgr_batched: null workspace': (-1, 'buf_fgr_batched: workspace 0 < 34048 bytes'),
    'fgr_batched: workspace too small': (-1, 'buf_fgr_batched: workspace 1000 < 34048 bytes'),
    'sc2_batched: negative pairs': (-1, 'buf_sc2_batched: npairs=-1 (0..65535)'),
    'sc2_batched: too many pairs': (-1, 'buf_sc2_batched: npairs=65536 (0..65535)'),
    'sc2_batched: d_thr 0': (-1, 'buf_sc2_batched: d_thr=0 (must be finite and > 0, and so its square)'),
    'sc2_batched: d_thr with an infinite square': (-1, 'buf_sc2_batched: d_thr=1e+200 (must be finite and > 0, and so its square)'),
    'sc2_batched: inlier_thr nan': (-1, 'buf_sc2_batched: inlier_thr=nan (must be finite and > 0)'),
    'sc2_batched: max_seeds 0': (-1, 'buf_sc2_batched: max_seeds=0 (1..1024)'),
    'sc2_batched: max_seeds 1025': (-1, 'buf_sc2_batched: max_seeds=1025 (1..1024)'),
    'sc2_batched: negative refine_iterations': (-1, 'buf_sc2_batched: power_iterations=10 (0..1000) refine_iterations=-1'),
    'sc2_batched: too many correspondences in a pair': (-1, 'buf_sc2_batched: 16385 correspondences in pair 1 (at most 16384)'),
    'sc2_batched: negative length before the row limit': (-1, 'buf_sc2_batched: negative length in pair 0'),
    'sc2_batched: row limit in pair 0 before a negative length in pair 1': (-1, 'buf_sc2_batched: 16385 correspondences in pair 0 (at most 16384)'),
    'sc2_batched: seed_ratio 0': (-1, 'buf_sc2_batched: seed_ratio=0 (must be in (0, 1])'),
    'sc2_batched: seed_ratio above 1': (-1, 'buf_sc2_batched: seed_ratio=1.5 (must be in (0, 1])'),
    'sc2_batched: k1 2': (-1, 'buf_sc2_batched: k1=2 (3..128)'),
    'sc2_batched: k1 129': (-1, 'buf_sc2_batched: k1=129 (3..128)'),
    'sc2_batched: nms_radius negative': (-1, 'buf_sc2_batched: nms_radius=-1 (must be finite and >= 0)'),
    'sc2_batched: power_iterations 1001': (-1, 'buf_sc2_batched: power_iterations=1001 (0..1000) refine_iterations=20'),
    'sc2_batched: null source lengths': (-1, 'buf_sc2_batched: null host array'),
    'sc2_batched: null target lengths': (-1, 'buf_sc2_batched: null host array'),
    'sc2_batched: null correspondence lengths': (-1, 'buf_sc2_batched: null host array'),
    'sc2_batched: null T': (-1, 'buf_sc2_batched: null output'),
    'sc2_batched: null info': (-1, 'buf_sc2_batched: null output'),
    'sc2_batched: null lengths before null outputs': (-1, 'buf_sc2_batched: null host array'),
    'sc2_batched: negative source length': (-1, 'buf_sc2_batched: negative length in pair 1'),
    'sc2_batched: negative target length': (-1, 'buf_sc2_batched: negative length in pair 1'),
    'sc2_batched: negative correspondence length': (-1, 'buf_sc2_batched: negative length in pair 1'),
    'sc2_batched: too many source points': (-1, 'buf_sc2_batched: 2147483647 / 5 points, 5 correspondences (int32 indices)'),
    'sc2_batched: too many target points': (-1, 'buf_sc2_batched: 5 / 2147483647 points, 5 correspondences (int32 indices)'),
    'sc2_batched: null src': (-1, 'buf_sc2_batched: null input'),
    'sc2_batched: null tgt': (-1, 'buf_sc2_batched: null input'),
    'sc2_batched: null corr': (-1, 'buf_sc2_batched: null input'),
    'sc2_batched: null outputs before null inputs': (-1, 'buf_sc2_batched: null output'),
    'sc2_batched: null workspace': (-1, 'buf_sc2_batched: workspace 0 < 16128 bytes'),
    'sc2_batched: workspace too small': (-1, 'buf_sc2_batched: workspace 1000 < 16128 bytes'),
    'clique_batched: negative pairs': (-1, 'buf_clique_batched: npairs=-1 (0..65535)'),
    'clique_batched: too many pairs': (-1, 'buf_clique_batched: npairs=65536 (0..65535)'),
    'clique_batched: d_thr 0': (-1, 'buf_clique_batched: d_thr=0 (must be finite and > 0)'),
    'clique_batched: d_thr with an infinite square': (-1, 'buf_clique_batched: workspace 0 < 136448 bytes'),
    'clique_batched: inlier_thr nan': (-1, 'buf_clique_batched: inlier_thr=nan (must be finite and > 0)'),
    'clique_batched: max_seeds 0': (-1, 'buf_clique_batched: max_seeds=0 (1..1024)'),
    'clique_batched: max_seeds 1025': (-1, 'buf_clique_batched: max_seeds=1025 (1..1024)'),
    'clique_batched: negative refine_iterations': (-1, 'buf_clique_batched: gnc_iterations=100 (1..1000) refine_iterations=-1'),
    'clique_batched: too many correspondences in a pair': (-1, 'buf_clique_batched: 16385 correspondences in pair 1 (at most 16384)'),
    'clique_batched: negative length before the row limit': (-1, 'buf_clique_batched: negative length in pair 0'),
    'clique_batched: row limit in pair 0 before a negative length in pair 1': (-1, 'buf_clique_batched: 16385 correspondences in pair 0 (at most 16384)'),
    'clique_batched: tim_thr with a zero square': (-1, 'buf_clique_batched: tim_thr=1e-200 (must be finite and > 0, and so its square)'),
    'clique_batched: t_thr 0': (-1, 'buf_clique_batched: t_thr=0 (must be finite and > 0, and so its square)'),
    'clique_batched: max_members 2': (-1, 'buf_clique_batched: max_members=2 (3..512)'),
    'clique_batched: max_members 513': (-1, 'buf_clique_batched: max_members=513 (3..512)'),
    'clique_batched: gnc_factor 1': (-1, 'buf_clique_batched: gnc_factor=1 (must be finite and > 1)'),
    'clique_batched: gnc_iterations 0': (-1, 'buf_clique_batched: gnc_iterations=0 (1..1000) refine_iterations=20'),
    'clique_batched: gnc_iterations 1001': (-1, 'buf_clique_batched: gnc_iterations=1001 (1..1000) refine_iterations=20'),
    'clique_batched: null source lengths': (-1, 'buf_clique_batched: null host array'),
    'clique_batched: null target lengths': (-1, 'buf_clique_batched: null host array'),
    'clique_batched: null correspondence lengths': (-1, 'buf_clique_batched: null host array'),
    'clique_batched: null T': (-1, 'buf_clique_batched: null output'),
    'clique_batched: null info': (-1, 'buf_clique_batched: null output'),
    'clique_batched: null lengths before null outputs': (-1, 'buf_clique_batched: null host array'),
    'clique_batched: negative source length': (-1, 'buf_clique_batched: negative length in pair 1'),
    'clique_batched: negative target length': (-1, 'buf_clique_batched: negative length in pair 1'),
    'clique_batched: negative correspondence length': (-1, 'buf_clique_batched: negative length in pair 1'),
    'clique_batched: too many source points': (-1, 'buf_clique_batched: 2147483647 / 5 points, 5 correspondences (int32 indices)'),
    'clique_batched: too many target points': (-1, 'buf_clique_batched: 5 / 2147483647 points, 5 correspondences (int32 indices)'),
    'clique_batched: null src': (-1, 'buf_clique_batched: null input'),
    'clique_batched: null tgt': (-1, 'buf_clique_batched: null input'),
    'clique_batched: null corr': (-1, 'buf_clique_batched: null input'),
    'clique_batched: null outputs before null inputs': (-1, 'buf_clique_batched: null output'),
    'clique_batched: null workspace': (-1, 'buf_clique_batched: workspace 0 < 136448 bytes'),
    'clique_batched: workspace too small': (-1, 'buf_clique_batched: workspace 1000 < 136448 bytes'),
    'fgr_ws_bytes: 300 rows of 3 pairs': (504576, ''),
    'fgr_ws_bytes: max_tuples 4097': (0, ''),
    'fgr_ws_bytes: no pairs': (0, ''),
    'fgr_ws_bytes: negative rows': (0, ''),
    'sc2_ws_bytes: six pairs': (197888, ''),
    'sc2_ws_bytes: null lengths': (0, ''),
    'sc2_ws_bytes: max_seeds 1025': (0, ''),
    'sc2_ws_bytes: a pair above the row limit': (0, ''),
    'sc2_ws_bytes: negative length': (0, ''),
    'clique_ws_bytes: six pairs': (476672, ''),
    'clique_ws_bytes: null lengths': (0, ''),
    'clique_ws_bytes: max_members 2': (0, ''),
    'clique_ws_bytes: max_seeds 0': (0, ''),
    'clique_ws_bytes: a pair above the row limit': (0, ''),
}

EXPECTED_OPS = {
    'fgr_batched: target lengths of another batch': 'fgr_batched: 2 source lengths but 1 target and 2 correspondence lengths',
    'fgr_batched: correspondence lengths of another batch': 'fgr_batched: 2 source lengths but 2 target and 3 correspondence lengths',
    'fgr_batched: src of width 4': 'fgr_batched: src (12, 4) is not [N,3]',
    'fgr_batched: flat tgt': 'fgr_batched: tgt (36,) is not [N,3]',
    'fgr_batched: corr of width 3': 'fgr_batched: corr (4, 3) is not [N,2]',
    'fgr_batched: src lengths off the rows': 'fgr_batched: src lengths sum to 13, src holds 12 rows',
    'fgr_batched: negative tgt length': 'fgr_batched: tgt lengths sum to 12, tgt holds 12 rows',
    'fgr_batched: corr lengths off the rows': 'fgr_batched: corr lengths sum to 5, corr holds 4 rows',
    'fgr_batched: max_tuples 0': 'fgr_batched: max_tuples=0 (1..4096)',
    'fgr_batched: max_tuples 4097': 'fgr_batched: max_tuples=4097 (1..4096)',
    'fgr_batched: one seed for two pairs': 'fgr_batched: 2 pairs but 1 seeds',
    'sc2_batched: target lengths of another batch': 'sc2_batched: 2 source lengths but 1 target and 2 correspondence lengths',
    'sc2_batched: correspondence lengths of another batch': 'sc2_batched: 2 source lengths but 2 target and 3 correspondence lengths',
    'sc2_batched: src of width 4': 'sc2_batched: src (12, 4) is not [N,3]',
    'sc2_batched: flat tgt': 'sc2_batched: tgt (36,) is not [N,3]',
    'sc2_batched: corr of width 3': 'sc2_batched: corr (4, 3) is not [N,2]',
    'sc2_batched: src lengths off the rows': 'sc2_batched: src lengths sum to 13, src holds 12 rows',
    'sc2_batched: negative tgt length': 'sc2_batched: tgt lengths sum to 12, tgt holds 12 rows',
    'sc2_batched: corr lengths off the rows': 'sc2_batched: corr lengths sum to 5, corr holds 4 rows',
    'sc2_batched: a pair above the row limit': 'sc2_batched: 16385 correspondences in one pair (at most 16384)',
    'sc2_batched: max_seeds 0': 'sc2_batched: max_seeds=0 (1..1024), k1=30 (3..128)',
    'sc2_batched: max_seeds 1025': 'sc2_batched: max_seeds=1025 (1..1024), k1=30 (3..128)',
    'sc2_batched: k1 2': 'sc2_batched: max_seeds=512 (1..1024), k1=2 (3..128)',
    'sc2_batched: k1 129': 'sc2_batched: max_seeds=512 (1..1024), k1=129 (3..128)',
    'clique_batched: target lengths of another batch': 'clique_batched: 2 source lengths but 1 target and 2 correspondence lengths',
    'clique_batched: correspondence lengths of another batch': 'clique_batched: 2 source lengths but 2 target and 3 correspondence lengths',
    'clique_batched: src of width 4': 'clique_batched: src (12, 4) is not [N,3]',
    'clique_batched: flat tgt': 'clique_batched: tgt (36,) is not [N,3]',
    'clique_batched: corr of width 3': 'clique_batched: corr (4, 3) is not [N,2]',
    'clique_batched: src lengths off the rows': 'clique_batched: src lengths sum to 13, src holds 12 rows',
    'clique_batched: negative tgt length': 'clique_batched: tgt lengths sum to 12, tgt holds 12 rows',
    'clique_batched: corr lengths off the rows': 'clique_batched: corr lengths sum to 5, corr holds 4 rows',
    'clique_batched: a pair above the row limit': 'clique_batched: 16385 correspondences in one pair (at most 16384)',
    'clique_batched: max_seeds 0': 'clique_batched: max_seeds=0 (1..1024), max_members=256 (3..512)',
    'clique_batched: max_seeds 1025': 'clique_batched: max_seeds=1025 (1..1024), max_members=256 (3..512)',
    'clique_batched: max_members 2': 'clique_batched: max_seeds=64 (1..1024), max_members=2 (3..512)',
    'clique_batched: max_members 513': 'clique_batched: max_seeds=64 (1..1024), max_members=513 (3..512)',
    'icp_batched: generalized without source normals': "icp_batched: method 'generalized' needs src_normals and tgt_normals",
    'icp_batched: generalized without target normals': "icp_batched: method 'generalized' needs src_normals and tgt_normals",
    'icp_batched: epsilon 0': 'icp_batched: epsilon=0.0 (must be in (0, 1])',
    'icp_batched: epsilon above 1': 'icp_batched: epsilon=2 (must be in (0, 1])',
    'icp_batched: source normals of another shape': 'icp_batched: src_normals / tgt_normals must be shaped like src / tgt',
    'icp_batched: target normals of another shape': 'icp_batched: src_normals / tgt_normals must be shaped like src / tgt',
    'vgicp_batched: neighbors 9': 'vgicp_batched: neighbors=9 (one of (1, 7, 27))',
    'vgicp_batched: neighbors 0': 'vgicp_batched: neighbors=0 (one of (1, 7, 27))',
    'vgicp_batched: source normals of another shape': 'vgicp_batched: src_normals must be shaped like src',
    'vgicp_batched: three pair_cloud entries for two pairs': 'vgicp_batched: 2 pairs but 3 pair_cloud entries',
}


def run(L, fn, args):
    """(return value, message): the message of a *_ws_bytes query is the empty string (it sets none)"""
    if fn.endswith('_ws_bytes'):
        return int(getattr(L, fn)(*args)), ''
    rc = getattr(L, fn)(*args)
    return rc, (L.buf_last_error() or b'').decode()


def run_ops(ops, fn, args, kwargs):
    """the ValueError text of a call on host tensors (the device check of the arguments is stepped over: everything asked for here
    comes before the first allocation on the device or call into the library, or needs host-side queries of the library only)"""
    real = ops._dev
    ops._dev = lambda t, dtype, what: t.to(dtype).contiguous()
    try:
        getattr(ops, fn)(*args, **kwargs)
    except ValueError as e:
        return str(e)
    finally:
        ops._dev = real
    return None


CALLS, _KEEP = bad_calls()
OPS_CALLS = bad_ops_calls()


def test_the_lists_are_the_recorded_ones():
    assert [label for label, _, _ in CALLS] == list(EXPECTED) and len(set(EXPECTED)) == len(CALLS)
    assert [c[0] for c in OPS_CALLS] == list(EXPECTED_OPS) and len(set(EXPECTED_OPS)) == len(OPS_CALLS)
    assert {fn for _, fn, _ in CALLS} == {'buf_icp_batched', 'buf_gicp_batched', 'buf_vgicp_batched', 'buf_fgr_batched', 'buf_sc2_batched',
                                          'buf_clique_batched', 'buf_icp_ws_bytes', 'buf_vgicp_ws_bytes', 'buf_fgr_ws_bytes',
                                          'buf_sc2_ws_bytes', 'buf_clique_ws_bytes'}
    assert {c[1] for c in OPS_CALLS} == {'icp_batched', 'vgicp_batched', 'fgr_batched', 'sc2_batched', 'clique_batched'}
    assert all(rc != 0 and text for label, (rc, text) in EXPECTED.items() if 'ws_bytes:' not in label)
    assert all(EXPECTED_OPS.values())


@pytest.mark.parametrize('label,fn,args', CALLS, ids=[c[0] for c in CALLS])
def test_code_and_message(label, fn, args):
    from buffer_amd import _lib
    assert run(_lib.lib(), fn, args) == EXPECTED[label]


@pytest.mark.parametrize('label,fn,args,kwargs', OPS_CALLS, ids=[c[0] for c in OPS_CALLS])
def test_value_error_text(label, fn, args, kwargs):
    from buffer_amd import ops
    assert run_ops(ops, fn, args, kwargs) == EXPECTED_OPS[label]


if __name__ == '__main__':          # prints both tables of the library BUF_LIB_PATH names and the buffer_amd on the path (default: this tree's)
    from buffer_amd import _lib, ops
    print('EXPECTED = {')
    for label, fn, args in CALLS:
        print(f'    {label!r}: {run(_lib.lib(), fn, args)!r},')
    print('}\n\nEXPECTED_OPS = {')
    for label, fn, args, kwargs in OPS_CALLS:
        print(f'    {label!r}: {run_ops(ops, fn, args, kwargs)!r},')
    print('}')
