"""Host side of the F(2x4, 3x3) form of the descriptor CNN's 128-output layers (csrc/convnet_w24.hip): the filter transform
U = G2 g G4^T, its tiling, the identity the kernel evaluates, and the opt-in flag of buf_cylindrical_net_wg.  No GPU needed."""
import ctypes as C

import numpy as np

# F(2,3) down the rows, F(4,3) with the points 0, +-1, +-2, infinity along the azimuth
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)
B2T = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
B4T = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
               np.float64)
A2T = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
A4T = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)


def untile(t, cout, cin):
    """the kernel's tiling [pair][i][k-step][ n2: [lk][li][j = 0, 1, 2, 5] | n2: [lk][li][j = 3, 4] ] -> U [4, 6, Cout, Cin]"""
    t = t.reshape(cout // 32, 4, cin // 4, 768)
    wide = t[..., :512].reshape(cout // 32, 4, cin // 4, 2, 4, 16, 4)            # [pair, i, ks, n2, lk, li, q]
    narrow = t[..., 512:].reshape(cout // 32, 4, cin // 4, 2, 4, 16, 2)
    U = np.empty((cout // 32, 4, cin // 4, 2, 4, 16, 6), t.dtype)
    U[..., [0, 1, 2, 5]] = wide
    U[..., [3, 4]] = narrow
    return np.transpose(U, (1, 6, 0, 3, 5, 2, 4)).reshape(4, 6, cout, cin)      # [i, j, (pair, n2, li), (ks, lk)]


def correlate(x, w):
    """float64 3x3 correlation, circular along the last axis, zero rows above and below: x [Cin, H, 20], w [Cout, Cin, 3, 3]"""
    H = x.shape[1]
    xp = np.zeros((x.shape[0], H + 2, 22))
    xp[:, 1:-1, 1:-1] = x
    xp[:, 1:-1, 0], xp[:, 1:-1, 21] = x[:, :, 19], x[:, :, 0]
    y = np.zeros((w.shape[0], H, 20))
    for a in range(3):
        for b in range(3):
            y += np.einsum('oc,chw->ohw', w[:, :, a, b], xp[:, a:a + H, b:b + 20])
    return y


def winograd_f24(x, U, rows):
    """Y = A2^T [sum_c U[c] (.) (B2^T d[c] B4)] A4 over tiles of 2 x 4 outputs: x [Cin, H, 20] float64 (H even), U [4, 6, Cout, Cin]"""
    H = x.shape[1]
    xp = np.zeros((x.shape[0], H + 2, 22))
    xp[:, 1:-1, 1:-1] = x
    xp[:, 1:-1, 0], xp[:, 1:-1, 21] = x[:, :, 19], x[:, :, 0]
    y = np.zeros((U.shape[2], H, 20))
    for ty in range(H // 2):
        for tx in range(5):
            d = xp[:, 2 * ty:2 * ty + 4, 4 * tx:4 * tx + 6]
            V = np.einsum('ia,cab,jb->ijc', B2T, d, B4T)
            M = np.einsum('ijoc,ijc->ijo', U, V)
            y[:, 2 * ty:2 * ty + 2, 4 * tx:4 * tx + 4] = np.einsum('ui,ijo,vj->ouv', A2T, M, A4T)
    return y[:, :rows]


def test_untiled_set_is_the_filter_transform():
    from buffer_amd import ops
    rng = np.random.default_rng(5)
    for cout, cin in ((32, 8), (128, 32)):
        w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
        t = ops.winograd_f24_tile_weights(w)
        assert t.dtype == np.float32 and t.shape == (24 * cout * cin,)
        want = np.einsum('ia,ocab,jb->ijoc', G2, w.astype(np.float64), G4)
        U = untile(t, cout, cin)
        assert np.array_equal(U, ops.winograd_f24_filters(w).astype(np.float32))          # rounded once from float64
        assert np.abs(U - want).max() <= 2.0 ** -24 * np.abs(want).max() * 1.001


def test_identity_reproduces_the_correlation():
    """A circular 4 x 20 strip, and the 7 x 20 map with zero rows above and below (the eighth output row does not exist: dropped)"""
    from buffer_amd import ops
    rng = np.random.default_rng(6)
    cout, cin = 32, 8
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    U64 = ops.winograd_f24_filters(w)
    U32 = untile(ops.winograd_f24_tile_weights(w), cout, cin).astype(np.float64)
    for H in (4, 7):
        x = rng.standard_normal((cin, H, 20))
        ref = correlate(x, w.astype(np.float64))
        xe = np.concatenate([x, np.zeros((cin, H % 2, 20))], axis=1)              # an even number of rows for the tiles
        scale = np.abs(ref).max()
        e64 = np.abs(winograd_f24(xe, U64, H) - ref).max() / scale
        e32 = np.abs(winograd_f24(xe, U32, H) - ref).max() / scale
        print(f'H = {H}: float64 set {e64:.2e}, fp32-rounded set {e32:.2e}')
        assert e64 < 1e-12
        assert e32 < 1e-6


def test_c_function_equals_numpy_bit_for_bit():
    from buffer_amd import _lib, ops
    L = _lib.lib()
    rng = np.random.default_rng(7)
    for cout, cin in ((32, 16), (128, 64)):
        w = np.ascontiguousarray(rng.standard_normal((cout, cin, 3, 3)).astype(np.float32))
        got = np.full(24 * cout * cin, np.nan, np.float32)
        assert L.buf_winograd_f24_tile_weights(w.ctypes.data_as(C.c_void_p), cout, cin, got.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got, ops.winograd_f24_tile_weights(w))
    w = np.zeros((16, 16, 3, 3), np.float32)
    assert L.buf_winograd_f24_tile_weights(w.ctypes.data_as(C.c_void_p), 16, 16, got.ctypes.data_as(C.c_void_p)) == -1      # pairs of N-tiles
    assert L.buf_winograd_f24_tile_weights(w.ctypes.data_as(C.c_void_p), 32, 6, got.ctypes.data_as(C.c_void_p)) == -1


def test_unflagged_calls_are_accepted_and_rejected_as_before():
    """relu words 0 / 1 (every caller so far: buffers of 16 Cout Cin floats) never reach the F(2x4) kernel; the launcher validates
    before its first device call, so dummy pointers do.  A flagged call must flag exactly the layers with 128 output channels."""
    from buffer_amd import _lib
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    ptrs = (C.c_void_p * 8)(*[x] * 8)
    ints = lambda *v: (C.c_int * 8)(*v)
    ok_in, ok_out = ints(48, 64, 64, 128, 128, 64, 64, 32), ints(64, 64, 128, 128, 64, 64, 32, 32)
    relu = ints(1, 1, 1, 1, 1, 1, 1, 0)
    assert L.buf_cylindrical_net_wg(x, 0, ptrs, ptrs, ok_in, ok_out, relu, x, None) == 0
    assert L.buf_cylindrical_net_wg(x, -1, ptrs, ptrs, ok_in, ok_out, relu, x, None) == -1
    assert L.buf_cylindrical_net_wg(x, 2, ptrs, None, ok_in, ok_out, relu, x, None) == -1 and b"null argument" in L.buf_last_error()
    rc = L.buf_cylindrical_net_wg(x, 2, ptrs, ptrs, ints(48, 64, 32, 64, 128, 128, 64, 32), ints(64, 32, 64, 128, 128, 64, 32, 32), relu, x, None)
    assert rc == -1 and b"may follow a 32-output layer" in L.buf_last_error()
    rc = L.buf_cylindrical_net_wg(x, 2, ptrs, ptrs, ints(48, 64, 64, 128, 128, 64, 64, 64), ints(64, 64, 128, 128, 64, 64, 64, 64), relu, x, None)
    assert rc == -1 and b"last layer" in L.buf_last_error()
    # flagged: the width rules first, then the flags
    rc = L.buf_cylindrical_net_wg(x, 2, ptrs, ptrs, ints(40, 64, 64, 128, 128, 64, 64, 32), ok_out, ints(1, 1, 3, 3, 1, 1, 1, 0), x, None)
    assert rc == -1 and b"unsupported widths" in L.buf_last_error()
    for flags in ((1, 1, 3, 1, 1, 1, 1, 0), (1, 3, 3, 3, 1, 1, 1, 0), (1, 1, 3, 3, 1, 1, 1, 2)):
        rc = L.buf_cylindrical_net_wg(x, 2, ptrs, ptrs, ok_in, ok_out, ints(*flags), x, None)
        assert rc == -1 and b"F(2x4) flag" in L.buf_last_error(), flags
