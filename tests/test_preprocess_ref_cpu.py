"""Pin tests/preprocess_ref.py (the float64 references of tests/test_preprocess_edges_gpu.py) against hand-computed cases, measure the
constant K of its angle bound on the CPU oracle, and check that no random input of the suite asks for an undetermined normal.  CPU only."""
import numpy as np
import pytest

import preprocess_ref as ref


def test_knn_sets_by_hand():
    pts = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [2, 0, 0]], np.float32)
    sets = ref.knn_sets(pts, [4], 3)
    assert [s.tolist() for s in sets] == [[0, 1, 2], [1, 0, 3], [2, 0, 1], [3, 1, 0]]          # (d2, index): 1 before 2 at d2 = 1
    sets = ref.knn_sets(pts, [2, 2], 3)                                                        # min(knn, n_cloud), own cloud only
    assert [s.tolist() for s in sets] == [[0, 1], [1, 0], [2, 3], [3, 2]]
    assert ref.knn_sets(pts, [4], 9)[3].tolist() == [3, 1, 0, 2]
    # fp64 d2 of the fp32 coordinates: 1 + 2**-23 and 1 + 2**-24 (not a float32) differ, 1e-30 does not underflow
    pts = np.array([[0, 0, 0], [1 + 2.0 ** -23, 0, 0], [0, 1, 0], [0, 0, 1e-30]], np.float32)
    assert ref.knn_sets(pts, [4], 4)[0].tolist() == [0, 3, 2, 1]
    assert ref.rerank(pts, 0, [1, 2, 3], 2).tolist() == [3, 2]


def test_normal_ref_by_hand():
    # a 3-4-5 lattice plane: i (4,-3,0) + j (0,0,5), i, j in {-1,0,1}: normal (3,4,0)/5, in-plane variances 2/3 * 25 twice
    pts = np.array([[4 * i, -3 * i, 5 * j] for i in (-1, 0, 1) for j in (-1, 0, 1)], np.float32)
    n0, l0, l1, l2, mean = ref.normal_ref(pts, np.arange(9))
    assert ref.angle(n0, [0.6, 0.8, 0.0]) < 1e-15
    np.testing.assert_allclose([l0, l1, l2], [0.0, 50 / 3, 50 / 3], rtol=0, atol=1e-14)
    assert np.all(mean == 0)
    assert ref.det_sign((l0, l1, l2)) < 0                                                       # planar
    # the same plane moved away: the reference centres before it squares, the eigenvalues stay
    far = pts + np.array([1024.0, -2048.0, 512.0], np.float32)
    n0, l0, l1, l2, mean = ref.normal_ref(far, np.arange(9))
    assert ref.angle(n0, [0.6, 0.8, 0.0]) < 1e-15 and abs(l0) < 1e-14 and mean.tolist() == [1024.0, -2048.0, 512.0]
    # a needle along (1,2,2): t in -2..2, and +-(2,-2,1)/64, +-(2,1,-2)/128 across: eigenvalues 10, 1/2048, 1/8192
    pts = np.array([[t, 2 * t, 2 * t] for t in (-2, -1, 0, 1, 2)] + [[2 / 64, -2 / 64, 1 / 64], [-2 / 64, 2 / 64, -1 / 64],
                   [2 / 128, 1 / 128, -2 / 128], [-2 / 128, -1 / 128, 2 / 128]], np.float32)
    n0, l0, l1, l2, mean = ref.normal_ref(pts, np.arange(9))
    eigh_err = 8 * 2.0 ** -53 * 10.0 / (1 / 2048 - 1 / 8192)                                    # eigh is backward stable: eps |A| / gap
    assert ref.angle(n0, np.array([2, 1, -2]) / 3) < eigh_err
    np.testing.assert_allclose([l0, l1, l2], [1 / 8192, 1 / 2048, 10.0], rtol=0, atol=8 * 2.0 ** -53 * 10.0)
    assert ref.det_sign((l0, l1, l2)) > 0                                                       # needle
    assert ref.angle_bound((1 / 8192, 1 / 2048, 10.0), np.array([0.0, 3.0, 4.0])) == 1.5e-7 + ref.K * 2.0 ** -53 * ((25.0 + 10.0) / (1 / 2048 - 1 / 8192) + (10.0 / (1 / 2048 - 1 / 8192)) ** 2)
    # a subset, in any order
    n0, l0, l1, l2, _ = ref.normal_ref(pts, [4, 0, 2, 6, 5])
    assert abs(l0) < 8 * 2.0 ** -53 * l2 and ref.angle(n0, np.array([2, 1, -2]) / 3) < eigh_err
    # the octahedron: isotropic, no normal is determined
    pts = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    _, l0, l1, l2, mean = ref.normal_ref(pts, np.arange(6))
    np.testing.assert_allclose([l0, l1, l2], [1 / 3] * 3, rtol=1e-15)
    assert ref.angle_bound((l0, l0, l2), mean) == np.inf


def test_angle_by_hand():
    assert ref.angle([0, 0, 1], [0, 0, -1]) == 0.0
    assert abs(ref.angle([0, 0, 1], [1e-9, 0, 1]) - 1e-9) < 1e-24
    assert abs(ref.angle([1, 0, 0], [0, 0, 2]) - np.pi / 2) < 1e-15


def test_voxel_means_by_hand():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0.04, 0, 0], [0, 0.26, 0]])
    # o = -0.05; indices (0,0,0) (10,0,0) (0,0,0) (0,3,0); N = (11, 4, 1): keys 0, 10, 0, 33
    np.testing.assert_array_equal(ref.voxel_means(pts, 0.1), [[0.02, 0, 0], [1, 0, 0], [0, 0.26, 0]])
    got, nrm = ref.voxel_means(pts, 0.1, normals=np.array([[0, 0, 1.0], [1, 0, 0], [0, 1.0, 0], [2, 2, 2]]))
    np.testing.assert_array_equal(nrm, [[0, 0.5, 0.5], [1, 0, 0], [2, 2, 2]])                   # mean, not re-normalised
    assert ref.voxel_means(np.zeros((0, 3)), 0.1).shape == (0, 3)
    # input-order sum: (1e16 + 1) + 1 - 1e16 is 0 in that order, 2 in another
    pts = np.array([[1e16, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [-1e16, 0, 0]])
    assert ref.voxel_means(pts, 1e17)[0, 0] == 0.0
    assert ref.voxel_means(pts[[1, 2, 0, 3]], 1e17)[0, 0] == 0.5


def _all_random_inputs():
    for name, spec in ref.PATCH_SETS.items():
        for knn in spec[6]:
            yield ('patch', name, knn), lambda a=(name, knn): ref.patch_reference(*a)
    for kind, n, knn in ref.cloud_cases():
        if not ref.undetermined(kind, n):
            yield (kind, n, knn), lambda a=(kind, n, knn): ref.cloud_reference(*a)


def test_inputs_land_in_their_arms_and_are_determined():
    """the cap is a condition on the INPUTS: a seed that violates it is changed, the cap is not"""
    for what, get in _all_random_inputs():
        pts, sets, n0, lam, mean, bound = get()
        assert np.all(bound <= ref.BOUND_CAP), (what, float(bound.max()))
    for name, sign in (('plane', -1), ('plane_48', -1), ('plane_1e-4', -1), ('plane_1e+3', -1), ('plane_shift', -1), ('plane_nq', -1), ('needle', 1),
                       ('needle_1e-4', 1), ('needle_1e+3', 1), ('needle_shift', 1), ('edge', 1)):
        lam = ref.patch_reference(name)[3]
        assert all(ref.det_sign(l) == sign for l in lam), name
    lam = ref.patch_reference('edge')[3]
    assert np.all(lam[:, 1] < 0.02 * lam[:, 2]) and np.all(lam[:, 1] < 20 * lam[:, 0])         # lambda0 ~ lambda1 << lambda2
    # part (b) meets both arms too
    lam = ref.cloud_reference('mix', 3000, 30)[3]
    signs = np.array([ref.det_sign(l) for l in lam])
    assert (signs < 0).sum() > 1000 and (signs > 0).sum() > 500


def test_measure_K(oracle):
    """The constants of angle_bound are not derivable: they are measured here, on the CPU oracle (the same cumulant form and Eberly solver
    as the kernel, on the host) against the float64 reference, over every random input of the suite, as the worst multiple of t1 (K1)
    and of t1 + t2 (K) that the oracle's angle amounts to; constant = worst x 8 rounded up to a power of two (device fp64 differs by
    acos/cos of a few ulp and by the order of the sums, which the same amplification applies to; a wrong arm or eigenvector is off by
    O(1) rad).  Measured: K1 worst 5.06e4 -> 2**19, K worst 0.614 -> 8.  With K1 alone the needle patches (1 long, 1e-3 thick) would
    get bounds of 0.12 rad and their translated copy > 1 rad: the finding recorded in preprocess_ref and profiles/preprocess_edges.md."""
    worst1, worst, where1, where = 0.0, 0.0, None, None
    for what, get in _all_random_inputs():
        pts, sets, n0, lam, mean, bound = get()
        knn = what[2]
        got = oracle.o3d_estimate_normals(pts, knn=knn, orient=False).astype(np.float64)
        for i in range(len(sets)):
            t1, t2 = ref.bound_terms(lam[i], mean[i])
            excess = ref.angle(got[i], n0[i]) - ref.F32_TERM
            if excess / t1 > worst1:
                worst1, where1 = excess / t1, (what, i)
            if excess / (t1 + t2) > worst:
                worst, where = excess / (t1 + t2), (what, i)
    print(f"worst oracle ratio to t1 {worst1:.4g} at {where1} (K1 = {ref.K1}); to t1 + t2 {worst:.4g} at {where} (K = {ref.K})")
    # the recorded figures are the measured ones (3 digits), and the constants follow from them
    assert 0.999 * ref.K1_MEASURED_WORST <= worst1 <= 1.001 * ref.K1_MEASURED_WORST, (worst1, where1)
    assert 0.999 * ref.K_MEASURED_WORST <= worst <= 1.001 * ref.K_MEASURED_WORST, (worst, where)
    assert ref.K1 == 2.0 ** np.ceil(np.log2(worst1 * 8)) and ref.K == 2.0 ** np.ceil(np.log2(worst * 8))
    # the finding: K1 alone leaves the needle cases of the issue without a usable bound
    lam, mean = ref.patch_reference('needle_shift')[3:5]
    assert max(ref.K1 * ref.bound_terms(l, m)[0] for l, m in zip(lam, mean)) > 1.0
