"""The numpy reference of patch selection (tests/patches_ref.py) is itself checked here, without a device: against the CPU oracle's
select_patches and ball_query, for float32 against float64 membership on the random inputs the GPU tests use, for exactness of the
lattice inputs, and the keyed permutation for being one."""
import numpy as np
import pytest
import torch

import patches_cases
import patches_ref


def _cloud(rng, n, scale=1.0):
    return (rng.random((n, 3)) * scale).astype(np.float32)


# (n, m, radius, nsample, keypoints): 'cloud' = points of the cloud (jittered), 'off' = 25 m off the cloud (empty balls), 'mixed' = both
ORACLE_SHAPES = [
    (1, 4, 0.3, 1, 'cloud'), (1, 4, 0.3, 2, 'mixed'), (1, 3, 0.3, 3, 'off'),
    (65, 7, 0.3, 1, 'mixed'), (65, 7, 0.3, 2, 'mixed'), (65, 7, 0.3, 3, 'mixed'), (65, 9, 2.0, 64, 'cloud'), (65, 9, 2.0, 66, 'cloud'),
    (700, 33, 0.12, 16, 'mixed'), (700, 33, 0.3, 512, 'mixed'), (2000, 20, 0.05, 8, 'off'), (2000, 40, 0.1, 64, 'mixed'),
    (3000, 50, 0.3, 512, 'mixed'),
]


def _oracle_inputs(i, n, m, kind):
    rng = np.random.default_rng(300 + i)
    pts = _cloud(rng, n)
    k = pts[rng.integers(0, n, m)] + rng.normal(0, 0.02, (m, 3)).astype(np.float32)
    if kind == 'off':
        k += np.float32(25.0)
    elif kind == 'mixed':
        k[::3] += np.float32(25.0)
    return pts, np.ascontiguousarray(k, np.float32)


@pytest.mark.parametrize('i', range(len(ORACLE_SHAPES)))
def test_select_patches_ref_is_bit_equal_to_the_oracle(i, oracle):
    from oracle import torch_ref
    n, m, radius, nsample, kind = ORACLE_SHAPES[i]
    pts, k = _oracle_inputs(i, n, m, kind)
    want = torch_ref.select_patches(torch.from_numpy(pts), torch.from_numpy(k), torch.arange(n), radius, nsample).numpy()
    got = patches_ref.select_patches_ref(pts, k, radius, nsample)
    assert got.shape == want.shape == (m, nsample, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ORACLE_SHAPES[i]
    if kind != 'cloud' and nsample > 1:
        empty = ~patches_ref.in_ball(pts, k, radius).any(1)
        assert empty.any() and np.array_equal(got[empty, 0], np.broadcast_to(pts[0], (int(empty.sum()), 3)))
    one = patches_ref.select_patches_batched_ref(np.concatenate([pts, pts[:n // 2]]), [n, n // 2], np.concatenate([k, k]), m, radius, nsample)
    assert np.array_equal(one[:m].view(np.uint32), got.view(np.uint32))
    assert np.array_equal(one[m:].view(np.uint32), patches_ref.select_patches_ref(pts[:n // 2], k, radius, nsample).view(np.uint32))


@pytest.mark.parametrize('i', range(len(ORACLE_SHAPES)))
def test_ball_query_ref_equals_the_oracle(i, oracle):
    n, m, radius, nsample, kind = ORACLE_SHAPES[i]
    xyz = np.stack([_oracle_inputs(i, n, m, kind)[0], _oracle_inputs(i + 50, n, m, kind)[0]])
    new = np.stack([_oracle_inputs(i, n, m, kind)[1], _oracle_inputs(i + 50, n, m, kind)[1]])
    want = oracle.ball_query(radius, nsample, xyz, new)
    got = patches_ref.ball_query_ref(radius, nsample, xyz, new)
    assert got.dtype == np.int32 and np.array_equal(got, want), ORACLE_SHAPES[i]


@pytest.mark.parametrize('n', patches_cases.BQ_N)
def test_ball_query_case_has_the_rows_it_is_named_for(n, oracle):
    xyz, new, r = patches_cases.ball_query_case(n)
    for nsample in (5, 16):
        got = patches_ref.ball_query_ref(r, nsample, xyz, new)
        assert np.array_equal(got, oracle.ball_query(r, nsample, xyz, new))
    hits = [patches_ref.in_ball(xyz[e], new[e], r) for e in range(patches_cases.BQ_B)]
    assert not any(h[6].any() for h in hits)                                         # an empty row
    if n == 129:
        assert all(np.flatnonzero(h[5])[0] >= 64 for h in hits)                      # first hit in the second 64-block
        assert all(h[0].sum() > 5 and np.flatnonzero(h[0])[4] % 64 not in (0, 63) for h in hits)    # nsample = 5 ends inside a block


def test_empty_cloud_and_tiny_patch_rules():
    k = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    out = patches_ref.select_patches_ref(np.zeros((0, 3), np.float32), k, 0.3, 4)
    assert np.array_equal(out, np.broadcast_to(k[:, None], (2, 4, 3)))                # n == 0: every slot is the keypoint
    pts = np.array([[9, 9, 9], [1, 2, 3.1], [1, 2, 3.2]], np.float32)
    assert np.array_equal(patches_ref.select_patches_ref(pts, k, 0.3, 1), k[:, None])  # nsample == 1: the keypoint alone
    out = patches_ref.select_patches_ref(pts, k, 0.3, 2)
    assert np.array_equal(out[0], [pts[1], k[0]]) and np.array_equal(out[1], [pts[0], k[1]])
    out = patches_ref.select_patches_ref(pts, k, 0.3, 4)
    assert np.array_equal(out[0], [pts[1], pts[2], k[0], k[0]]) and np.array_equal(out[1], [pts[0], k[1], k[1], k[1]])
    # bit patterns survive: a NaN payload and -0.0 in a copied row
    odd = np.array([[0x7fc12345, 0x80000000, 0x3f800000]], np.uint32).view(np.float32)
    out = patches_ref.select_patches_ref(odd, np.array([[50, 50, 50]], np.float32), 0.3, 2)
    assert np.array_equal(out[0, 0].view(np.uint32), odd[0].view(np.uint32))


RANDOM_NAMES = [n for n in patches_cases.ALL_NAMES if n not in ('exact_sphere',)]


def test_float32_membership_is_float64_membership_away_from_the_sphere():
    """On every randomly drawn input of the GPU tests: the float32 test and the float64 test of the same float32 coordinates may differ
    only for pairs with |d2_64 - r2| <= 2^-20 r2 (twice the worst-case rounding of three squared differences and two additions), and
    such pairs are at most 1e-4 of all pairs: the bit-equality the GPU tests ask for is a property of the operator, not of one
    rounding order."""
    pairs = near = differ = 0
    for name in RANDOM_NAMES:
        c = patches_cases.get(name)
        assert c.random
        r2 = float(patches_ref.r2_of(c.radius))
        for p, k in zip(c.clouds, c.kpts):
            if len(p) == 0 or len(k) == 0:
                continue
            with np.errstate(all='ignore'):
                d = k.astype(np.float64)[:, None, :] - p.astype(np.float64)[None, :, :]
                d2 = (d * d).sum(-1)
                ok = np.isfinite(d2) & (d2 < 1e30)                     # (beyond: the float32 sum overflows, both tests say "outside")
                m32 = patches_ref.in_ball(p, k, c.radius)
                m64 = d2 < r2
                close = ok & (np.abs(d2 - r2) <= 2.0 ** -20 * r2)
            assert not (m32 & ~ok).any(), name
            bad = ok & (m32 != m64) & ~close
            assert not bad.any(), (name, int(bad.sum()))
            pairs += int(ok.sum())
            near += int(close.sum())
            differ += int((ok & (m32 != m64)).sum())
    print(f'pairs {pairs}, within 2^-20 r2 of the sphere {near} ({near / pairs:.2e}), float32 != float64 {differ}')
    assert pairs > 5_000_000 and near <= 1e-4 * pairs


def test_lattice_distances_are_exact():
    """exact_sphere: float32 d2 == float64 d2 for every pair, the planted points ON a sphere are outside it and their neighbours one
    lattice step inwards are inside"""
    c = patches_cases.get('exact_sphere')
    assert c.lattice and c.radius == 65.0 / 64.0 and float(patches_ref.r2_of(c.radius)) == 4225.0 / 4096.0
    for ci, (p, k) in enumerate(zip(c.clouds, c.kpts)):
        assert np.array_equal(p * 64, np.round(p * 64)) and np.abs(p).max() <= 8 and np.array_equal(k * 64, np.round(k * 64))
        d = k.astype(np.float64)[:, None, :] - p.astype(np.float64)[None, :, :]
        d2 = (d * d).sum(-1)
        d32 = patches_ref.sqdist3(k, p)
        assert np.array_equal(d32.astype(np.float64), d2)
        hits = patches_ref.in_ball(p, k, c.radius)
        assert np.array_equal(hits, d2 < 4225.0 / 4096.0)
        for q, (on, ins) in enumerate(zip(c.notes['on'][ci], c.notes['inside'][ci])):
            assert len(on) == len(ins) == 102
            assert (d2[q, on] == 4225.0 / 4096.0).all() and not hits[q, on].any()
            assert hits[q, ins].all() and (d2[q, ins] >= 4096.0 / 4096.0).all()
    assert len(patches_cases.sphere_offsets()) == 102


def test_seam_cases_hit_what_they_name():
    c = patches_cases.get('seams_all_hits')
    assert tuple(c.lengths) == patches_cases.SEAM_N
    for p, k in zip(c.clouds, c.kpts):
        assert patches_ref.in_ball(p, k, c.radius).all()
    c = patches_cases.get('seams_chosen_hits')
    for p, k in zip(c.clouds, c.kpts):
        want = np.zeros(len(p), bool)
        want[patches_cases.seam_hit_indices(len(p))] = True
        assert (patches_ref.in_ball(p, k, c.radius) == want[None]).all()
    assert patches_cases.seam_hit_indices(8193)[-3:] == [8128, 8191, 8192] and 4032 in patches_cases.seam_hit_indices(4097)


def test_outside_keypoints_are_outside_and_some_reach_in():
    c = patches_cases.get('outside_box')
    for p, k in zip(c.clouds, c.kpts):
        mn, mx = p.min(0), p.max(0)
        assert (((k < mn) | (k > mx)).sum(1) == 1).all()                # beyond exactly one face
        any_hit = patches_ref.in_ball(p, k, c.radius).any(1).reshape(6, 6)
        assert any_hit[:, :2].all() and not any_hit[:, 3:].any()        # 0.5 r and 0.999 r reach the face point; 1.5 edges and beyond nothing


PRP_SEAMS = sorted({4 ** k + d for k in range(10) for d in (-1, 0, 1)})


@pytest.mark.parametrize('key', [0, 1, 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF])
def test_prp_perm_is_a_bijection(key):
    for n in list(range(301)) + PRP_SEAMS:
        perm = patches_ref.prp_perm(n, key)
        assert perm.shape == (n,) and perm.dtype == np.int64
        assert np.array_equal(np.sort(perm), np.arange(n)), n


def test_prp_perm_depends_on_key_and_length_only():
    a, b = patches_ref.prp_perm(1000, 12345), patches_ref.prp_perm(1000, 12346)
    assert np.array_equal(a, patches_ref.prp_perm(1000, 12345)) and (a != b).mean() > 0.9
    assert [patches_ref.prp_half_bits(n) for n in (0, 1, 4, 5, 16, 17, 262144, 262145)] == [1, 1, 1, 2, 2, 3, 9, 10]
