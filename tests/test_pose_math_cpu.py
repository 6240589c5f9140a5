"""The scalar fp64 routines of buffer_amd/csrc/pose_math.h (kabsch_rotation, solve6, rot_zyx), compiled for the host into a stand-alone
program (tests/native/pose_math_host.cpp, built into a temporary directory) and held to numpy float64.  The same program is built once
more with -fsanitize=address,undefined and run on the same case file: it is stand-alone, nothing is preloaded.

What each figure is relative to, and the worst value measured with g++ 11.4 -O2 on x86-64 (`python tests/test_pose_math_cpu.py`
prints them); BOUND is one decade above, since another host compiler may order the library calls (sqrt, sin, cos) differently:

  kabsch, against R* = V diag(1, 1, det(V U^T)) U^T of numpy.linalg.svd(H):
    gap      (tr(R* H) - tr(R H)) / ||H||_F, every group (rank 1 has no unique maximiser: there this and `rotation` are the test)
    rotation max(||R^T R - I||_F, |det R - 1|), every group
    R        ||R - R*||_F, the groups with a unique maximiser
                              gap        rotation   R
    full rank (64)            1.19e-15   1.75e-15   6.86e-15
    reflective, det < 0 (64)  1.19e-15   1.69e-15   2.66e-14
    rank 2 (32)               1.38e-15   1.93e-15   1.50e-15
    rank 1 (32)               7.02e-16   1.54e-15   (2.83: another maximiser)
    scale 1e-30 (16)          1.11e-15   1.67e-15   5.54e-15
    scale 1e+30 (16)          6.68e-16   1.22e-15   5.85e-15
  H = 0 (+0 and -0) returns false and leaves R as it was.
  solve6, against numpy.linalg.solve(A, -g) on A = Q diag(1 .. 1/cond) Q^T, cond = 1e0 .. 1e10 (8 systems each):
    ||x - x*|| / (cond(A) eps ||x*||), cond(A) from numpy.linalg.cond: 0.199.  It returns false on two indefinite systems, on a zero
    pivot (the zero matrix; a zero in the fourth place of the diagonal) and on NaN / inf in the matrix or the right-hand side.
  rot_zyx, against Rz(x2) Ry(x1) Rx(x0) multiplied out by numpy (angles in [-pi, pi], 64 cases): max |R - R*| / eps: 0.5
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'native', 'pose_math_host.cpp')
FLAGS = ['-O2', '-std=c++17', '-ffp-contract=off', '-fno-fast-math', '-Wall', '-D__host__=', '-D__device__=']
EPS = np.finfo(np.float64).eps

BOUND = {'kabsch full rank': (1.2e-14, 1.8e-14, 6.9e-14), 'kabsch reflective': (1.2e-14, 1.7e-14, 2.7e-13),
         'kabsch rank 2': (1.4e-14, 2.0e-14, 1.5e-14), 'kabsch rank 1': (7.1e-15, 1.6e-14),
         'kabsch scale 1e-30': (1.2e-14, 1.7e-14, 5.6e-14), 'kabsch scale 1e+30': (6.7e-15, 1.3e-14, 5.9e-14),
         'solve spd': 2.0, 'rot_zyx': 5.0}


def rand_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_cases():
    """(rows f64[n,28] as tests/native/pose_math_host.cpp reads them, groups {name: slice of the rows})"""
    rng = np.random.default_rng(20240607)
    rows, groups = [], {}

    def add(name, kind, payloads):
        start = len(rows)
        for p in payloads:
            r = np.zeros(28)
            r[0] = kind
            r[1:1 + len(p)] = p
            rows.append(r)
        groups[name] = slice(start, len(rows))

    def with_sv(s):          # H = A diag(s) B^T for random proper rotations A, B
        return rand_rotation(rng) @ np.diag(s) @ rand_rotation(rng).T

    full = [rng.standard_normal((3, 3)) for _ in range(64)]
    full = [h if np.linalg.det(h) > 0 else -h for h in full]
    add('kabsch full rank', 0, [h.ravel() for h in full])
    add('kabsch reflective', 0, [(-h).ravel() for h in full])
    add('kabsch rank 2', 0, [with_sv([rng.uniform(1, 2), rng.uniform(0.1, 1), 0.0]).ravel() for _ in range(32)])
    rank1 = [np.outer(rng.standard_normal(3), rng.standard_normal(3)) for _ in range(28)]
    rank1 += [np.outer(e, rng.standard_normal(3)) for e in np.eye(3)] + [np.outer([0.6, 0.8, 0.0], [0.0, 0.0, 1.0])]   # |u_x| at the 0.6 switch
    add('kabsch rank 1', 0, [h.ravel() for h in rank1])
    add('kabsch zero', 0, [np.zeros(9), -np.zeros(9)])
    add('kabsch scale 1e-30', 0, [(1e-30 * h).ravel() for h in full[:16]])
    add('kabsch scale 1e+30', 0, [(1e30 * h).ravel() for h in full[:16]])

    def system(A, g):
        return np.concatenate([A[np.triu_indices(6)], g])

    spd = []
    for e in range(11):
        for _ in range(8):
            q, _r = np.linalg.qr(rng.standard_normal((6, 6)))
            A = q @ np.diag(np.logspace(0, -e, 6)) @ q.T
            spd.append(system((A + A.T) / 2, rng.standard_normal(6)))
    add('solve spd', 1, spd)
    q, _r = np.linalg.qr(rng.standard_normal((6, 6)))
    indef = q @ np.diag([3.0, 2.0, 1.0, 1.0, 0.5, -0.5]) @ q.T
    add('solve indefinite', 1, [system((indef + indef.T) / 2, np.ones(6)), system(-np.eye(6), np.ones(6))])
    zp = np.eye(6)
    zp[3, 3] = 0.0
    add('solve zero pivot', 1, [system(np.zeros((6, 6)), np.ones(6)), system(zp, np.ones(6))])
    nan_a, nan_g = np.eye(6), np.ones(6)
    nan_a[2, 4] = nan_a[4, 2] = np.nan
    nan_g[5] = np.nan
    add('solve nan', 1, [system(nan_a, np.ones(6)), system(np.eye(6), nan_g), system(np.full((6, 6), np.nan), np.ones(6)),
                         system(np.diag(np.full(6, np.inf)), np.ones(6))])
    add('rot_zyx', 2, [np.concatenate([rng.uniform(-np.pi, np.pi, 3), rng.standard_normal(3)]) for _ in range(60)] +
        [np.zeros(6), np.array([np.pi / 2, -np.pi / 2, np.pi, 1, 2, 3]), np.array([1e-9, -1e-9, 1e-300, 0, 0, 0]),
         np.array([-np.pi, np.pi, -np.pi / 2, 0, 0, 0])])
    return np.array(rows), groups


def build(tmp, sanitize=False):
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = os.path.join(tmp, 'pose_math_host_san' if sanitize else 'pose_math_host')
    r = subprocess.run([cxx] + FLAGS + (['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitize else []) +
                       [SRC, '-o', exe], capture_output=True, text=True)
    if r.returncode != 0 and sanitize and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the sanitizer runtime is not installed: ' + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, tmp, rows, tag):
    cases, results = os.path.join(tmp, 'cases.bin'), os.path.join(tmp, f'results_{tag}.bin')
    rows.astype('<f8').tofile(cases)
    r = subprocess.run([exe, cases, results], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(results, dtype='<f8').reshape(-1, 10)


@pytest.fixture(scope='module')
def computed(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('pose_math'))
    rows, groups = make_cases()
    return tmp, rows, groups, run(build(tmp), tmp, rows, 'plain')


def kabsch_reference(H):
    U, s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    return Vt.T @ np.diag([1.0, 1.0, d]) @ U.T


def kabsch_figures(rows, out, sl):
    """worst (gap, rotation, R) over the group"""
    gap = rot = err = 0.0
    for c, r in zip(rows[sl], out[sl]):
        H, R = c[1:10].reshape(3, 3), r[1:10].reshape(3, 3)
        assert r[0] == 1.0
        Rs = kabsch_reference(H)
        gap = max(gap, (np.trace(Rs @ H) - np.trace(R @ H)) / np.linalg.norm(H))
        rot = max(rot, np.linalg.norm(R.T @ R - np.eye(3)), abs(np.linalg.det(R) - 1.0))
        err = max(err, np.linalg.norm(R - Rs))
    return gap, rot, err


def solve_figure(rows, out, sl):
    worst = 0.0
    for c, r in zip(rows[sl], out[sl]):
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = c[1:22]
        A = A + np.triu(A, 1).T
        assert r[0] == 1.0
        xs = np.linalg.solve(A, -c[22:28])
        worst = max(worst, np.linalg.norm(r[1:7] - xs) / (np.linalg.cond(A) * EPS * np.linalg.norm(xs)))
    return worst


def rot_figure(rows, out, sl):
    worst = 0.0
    for c, r in zip(rows[sl], out[sl]):
        a, b, g = c[1:4]
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
        worst = max(worst, np.abs(r[1:10].reshape(3, 3) - Rz @ Ry @ Rx).max() / EPS)
    return worst


UNIQUE = ('kabsch full rank', 'kabsch reflective', 'kabsch rank 2', 'kabsch scale 1e-30', 'kabsch scale 1e+30')


@pytest.mark.parametrize('group', UNIQUE + ('kabsch rank 1',))
def test_kabsch(computed, group):
    _tmp, rows, groups, out = computed
    gap, rot, err = kabsch_figures(rows, out, groups[group])
    print(f'{group}: gap {gap:.3g} rotation {rot:.3g} R {err:.3g}')
    assert gap <= BOUND[group][0] and rot <= BOUND[group][1]
    if group in UNIQUE:
        assert err <= BOUND[group][2]


def test_kabsch_of_zero_is_false_and_leaves_R(computed):
    _tmp, _rows, groups, out = computed
    assert (out[groups['kabsch zero'], 0] == 0.0).all() and (out[groups['kabsch zero'], 1:10] == 7.0).all()


def test_solve(computed):
    _tmp, rows, groups, out = computed
    worst = solve_figure(rows, out, groups['solve spd'])
    print(f'solve spd: {worst:.3g}')
    assert worst <= BOUND['solve spd']


@pytest.mark.parametrize('group', ('solve indefinite', 'solve zero pivot', 'solve nan'))
def test_solve_refuses(computed, group):
    _tmp, _rows, groups, out = computed
    assert (out[groups[group], 0] == 0.0).all()


def test_rot_zyx(computed):
    _tmp, rows, groups, out = computed
    worst = rot_figure(rows, out, groups['rot_zyx'])
    print(f'rot_zyx: {worst:.3g}')
    assert worst <= BOUND['rot_zyx']


def test_under_address_and_undefined_behaviour_sanitizers(computed):
    tmp, rows, _groups, out = computed
    san = run(build(tmp, sanitize=True), tmp, rows, 'san')
    assert san.tobytes() == out.tobytes()          # (the same compiler at the same -O2: the same bits, NaN payloads included)


if __name__ == '__main__':          # prints the measured figures
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rows, groups = make_cases()
        out = run(build(tmp), tmp, rows, 'plain')
        for g in UNIQUE + ('kabsch rank 1',):
            print(g, ' '.join(f'{v:.3g}' for v in kabsch_figures(rows, out, groups[g])))
        print('solve spd', f'{solve_figure(rows, out, groups["solve spd"]):.3g}')
        print('rot_zyx', f'{rot_figure(rows, out, groups["rot_zyx"]):.3g}')
        for g in ('kabsch zero', 'solve indefinite', 'solve zero pivot', 'solve nan'):
            print(g, out[groups[g], 0])
