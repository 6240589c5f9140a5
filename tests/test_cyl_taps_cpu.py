"""Host side and code object of k_cyl_net_w25t / k_cyl_net_w25t_rerun (csrc/convnet_w25t.hip: the fused kernel of every layer form, and
in the layers of 128 output channels the direct round of output row 6 on host-formed taps and in front of the Winograd round): the tap tiler against a numpy
restatement, the argument checks of the new entry points, what the two ops classes run with and without row6=, and what the kernels
compiled to, read off the gfx950 code object of the in-tree library.  No GPU needed."""
import ctypes as C
import re

import numpy as np
import pytest

from test_cyl_code_object_cpu import code_object, kernel_meta, kernel_text, loops  # noqa: F401  (code_object: the module's fixture)
from test_cyl_f24k_cpu import RELEASED_IN, RELEASED_OUT, ints
from test_cyl_f24_code_object_cpu import KERNELS
from test_cyl_f25_cpu import W25_LOOPS, loop_stats, zero_layers

# MFMAs per k-loop of the fused kernel: every form before this file's (tests/test_cyl_f25_cpu.py) and three forms of the 128-output layers,
# each with four Winograd passes and one direct loop of 48
W25T_LOOPS = sorted(W25_LOOPS + [48] * 15)
WORDS = (1, 5, 3, 3, 5, 5, 1, 0)


def restated_taps(w):
    """out[((pair * K4 + ks) * 3 + q) * 256 + (lk * 16 + li) * 4 + e] = w[16 (2 pair + n2) + li][4 ks + lk][a][b], 4 q + e = 6 n2 + 3 a + b"""
    cout, cin = w.shape[:2]
    out = np.full(6 * cout * cin, np.nan, np.float32)
    for o in range(cout):
        for c in range(cin):
            pair, n2, li, ks, lk = o // 32, (o // 16) % 2, o % 16, c // 4, c % 4
            for a in range(2):
                for b in range(3):
                    f = 6 * n2 + 3 * a + b
                    out[((pair * (cin // 4) + ks) * 3 + f // 4) * 256 + (lk * 16 + li) * 4 + f % 4] = w[o, c, a, b]
    return out


@pytest.mark.parametrize('cout,cin', [(128, 64), (128, 128), (32, 64), (32, 32)])
def test_tile_taps_against_numpy(cout, cin):
    """buf_cyl_row6_tile_taps: the filter rows 0 and 1 as they are (bit for bit), each once, in the kernel's tiling; ops.cyl_row6_tile_taps
    the same; filter row 2 is not looked at"""
    from buffer_amd import _lib, ops
    rng = np.random.default_rng(cout + cin)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    out = np.full(6 * cout * cin, np.nan, np.float32)
    assert _lib.lib().buf_cyl_row6_tile_taps(w.ctypes.data, cout, cin, out.ctypes.data) == 0
    want = restated_taps(w)
    assert not np.isnan(want).any() and np.array_equal(out.view(np.int32), want.view(np.int32))
    assert np.array_equal(np.sort(out), np.sort(w[:, :, :2].reshape(-1)))
    mine = ops.cyl_row6_tile_taps(w)
    assert mine.dtype == np.float32 and np.array_equal(mine.view(np.int32), out.view(np.int32))
    w2 = w.copy()
    w2[:, :, 2] = 7.0
    assert np.array_equal(ops.cyl_row6_tile_taps(w2).view(np.int32), out.view(np.int32))
    w2[:, :, :2] = 0.0
    assert not ops.cyl_row6_tile_taps(w2).view(np.int32).any()


def test_tile_taps_arguments():
    from buffer_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 1024)()
    x = C.addressof(buf)
    assert L.buf_cyl_row6_tile_taps(None, 32, 4, x) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cyl_row6_tile_taps(x, 32, 4, None) == -1 and b'null argument' in L.buf_last_error()
    assert L.buf_cyl_row6_tile_taps(x, 16, 4, x) == -1 and b'widths' in L.buf_last_error()
    assert L.buf_cyl_row6_tile_taps(x, 32, 6, x) == -1 and b'widths' in L.buf_last_error()
    assert L.buf_cyl_row6_tile_taps(x, 0, 4, x) == -1 and b'widths' in L.buf_last_error()


def test_argument_checks():
    """Both entry points validate before their first device call, so dummy pointers do."""
    from buffer_amd import _lib
    L = _lib.lib()
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    ptrs = (C.c_void_p * 8)(*[x] * 8)
    none = (C.c_void_p * 8)()
    own25 = (C.c_void_p * 8)(x, x, None, None, x, x, None, None)
    taps = (C.c_void_p * 8)(None, None, x, x, None, None, None, None)
    ok_in, ok_out, words = ints(*RELEASED_IN), ints(*RELEASED_OUT), ints(*WORDS)

    def both(ci, co, re_, w24, w25, tp, order, n=2):
        out = []
        rc = L.buf_cylindrical_net_w25t(x, n, ptrs, ptrs, ci, co, re_, w24, w25, tp, order, x, None)
        out.append((rc, L.buf_last_error()))
        rc = L.buf_cylindrical_net_split_safe_w25t(x, n, ptrs, ptrs, ptrs, ci, co, re_, w24, w25, tp, order, None, x, None, None, x, None)
        out.append((rc, L.buf_last_error()))
        return out

    for w24, w25, tp in ((None, own25, taps), (none, None, taps), (none, own25, None)):
        for rc, msg in both(ok_in, ok_out, words, w24, w25, tp, 1):
            assert rc == -1 and b"null argument" in msg
    # a tap set goes on layers with 128 outputs only
    for bad in (0, 1, 4, 7):
        tp = (C.c_void_p * 8)(*[x if l == bad else None for l in range(8)])
        for rc, msg in both(ok_in, ok_out, words, none, own25, tp, 0):
            assert rc == -1 and b"takes no row-6 tap set" in msg and b"layer %d " % bad in msg, msg
    for order in (-1, 2, 3):
        for rc, msg in both(ok_in, ok_out, words, none, own25, taps, order):
            assert rc == -1 and b"order=" in msg, msg
    # the relu words, the widths and the other sets keep the rules of buf_cylindrical_net_w25
    for rc, msg in both(ok_in, ok_out, ints(1, 5, 3, 3, 5, 8, 1, 0), none, own25, taps, 1):
        assert rc == -1 and b"relu word" in msg
    for rc, msg in both(ok_in, ok_out, ints(1, 5, 1, 3, 5, 5, 1, 0), none, own25, taps, 1):
        assert rc == -1 and b"every layer with 128 output channels" in msg
    for rc, msg in both(ok_in, ok_out, words, none, (C.c_void_p * 8)(None, None, x, None, None, None, None, None), taps, 1):
        assert rc == -1 and b"takes no F(2x5) set" in msg
    for rc, msg in both(ints(48, 72, 64, 128, 128, 64, 64, 32), ints(72, 64, 128, 128, 64, 64, 32, 32), words, none, none, none, 0):
        assert rc == -1 and b"unsupported widths" in msg
    for rc, msg in both(ok_in, ok_out, words, none, own25, taps, 1, n=-1):
        assert rc == -1 and b"npatch" in msg
    for rc, msg in both(ok_in, ok_out, words, none, own25, taps, 1, n=0):                # no patches: nothing else is looked at
        assert rc == 0
    assert L.buf_cylindrical_net_split_safe_w25t(x, 2, ptrs, ptrs, ptrs, ok_in, ok_out, words, none, own25, taps, 1, x, x, None, None, x, None) == -1
    assert b"head without desc" in L.buf_last_error()


def test_ops_defaults_and_explicit_arguments():
    """row6 picks the parts; 'off' leaves every attribute of the net what it was; the other buffers do not change"""
    from buffer_amd import ops
    layers = zero_layers()
    assert ops.ROW6_DEFAULT in ops.ROW6_PARTS
    want = {'both': ([2, 3], True), 'taps': ([2, 3], False), 'order': ([], True), 'off': ([], False)}
    net = ops.CylindricalNet(layers, 'cpu')
    assert (net.taps_layers, net.row6_first) == want[ops.ROW6_DEFAULT]
    base = ops.CylindricalNet(layers, 'cpu', row6='off')
    assert base.fn == 'buf_cylindrical_net_w25' and base.fn_split_safe == 'buf_cylindrical_net_split_safe_w25' and len(base._extra) == 2
    for part, (ls, first) in want.items():
        net = ops.CylindricalNet(layers, 'cpu', row6=part)
        assert (net.taps_layers, net.row6_first) == (ls, first) and list(net._re) == list(WORDS)
        assert [t is not None for t in net.taps] == [l in ls for l in range(8)] and [bool(p) for p in net._tapsp] == [l in ls for l in range(8)]
        assert all(t.numel() == 6 * layers[l][0].shape[0] * layers[l][0].shape[1] for l, t in enumerate(net.taps) if t is not None)
        assert net.f25_layers == base.f25_layers and net.f24_layers == base.f24_layers
        assert [t.numel() for t in net.wt] == [t.numel() for t in base.wt]
        if part != 'off':
            assert net.fn == 'buf_cylindrical_net_w25t' and net.fn_split_safe == 'buf_cylindrical_net_split_safe_w25t'
            assert net._extra[3] == (1 if first else 0)
        else:
            assert net.fn == base.fn
        split = ops.CylindricalNetSplit(layers, 'cpu', row6=part)
        assert not split.safe or (split.taps_layers, split.row6_first) == (ls, first)
    assert ops.CylindricalNet(layers, 'cpu', row6=True).taps_layers == [2, 3] and ops.CylindricalNet(layers, 'cpu', row6=False).fn == base.fn
    assert ops.CylindricalNet(layers, 'cpu', f25='off', row6='both').fn == 'buf_cylindrical_net_w25t'
    # a stack without a 128-output layer has nothing to switch
    narrow = zero_layers((48, 64, 64, 64, 64, 64, 64, 32), (64, 64, 64, 64, 64, 64, 32, 32))
    net = ops.CylindricalNet(narrow, 'cpu', row6='both')
    assert net.taps_layers == [] and not net.row6_first and net.fn == 'buf_cylindrical_net_w25'
    # any other explicit form argument: neither part unless asked for, and then only with the default forms
    for kw in (dict(f24p=True), dict(f24k=True), dict(f24=True), dict(f24a='all'), dict(f25='out64'), dict(f25='off')):
        net = ops.CylindricalNet(layers, 'cpu', **kw)
        assert net.taps_layers == [] and not net.row6_first and net.fn != 'buf_cylindrical_net_w25t'
        if 'f24' not in kw:                          # (CylindricalNetSplit takes no f24)
            assert ops.CylindricalNetSplit(layers, 'cpu', **kw).taps_layers == []
    assert ops.CylindricalNet(layers, 'cpu', f24p=True, row6='taps').taps_layers == [2, 3]
    for kw in (dict(f24p=False), dict(f24k=False), dict(f24=False)):
        with pytest.raises(ValueError):
            ops.CylindricalNet(layers, 'cpu', row6='both', **kw)
    with pytest.raises(ValueError):
        ops.CylindricalNet(layers, 'cpu', row6='some')


@pytest.mark.parametrize('name', KERNELS)
def test_resources(code_object, name):
    """No scratch, no spills, and at most 128 + 128 registers: two workgroups share a CU.  (The one copy for the fused kernel and every
    layer form in it; k_cyl_net_wg and k_cyl_net_w24k have theirs in tests/test_cyl_code_object_cpu.py and tests/test_cyl_f24k_cpu.py.)"""
    asm, notes = code_object
    m = kernel_meta(notes, name)
    print(name, m)
    assert m['private_segment_fixed_size'] == 0, 'scratch memory'
    assert m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0
    assert m['vgpr_count'] <= 256 and m['agpr_count'] <= 128          # .vgpr_count of the unified file counts both kinds
    assert m['vgpr_count'] - m['agpr_count'] <= 128
    assert m['group_segment_fixed_size'] == 0, 'static LDS beside the dynamic 80 KB buffer'
    text = kernel_text(asm, name)
    assert not [op for _, op, _ in text if re.match(r'v_pk_\w+_f32', op)]
    assert not [op for _, op, _ in text if op.startswith('scratch_')]
    ls = loops(text)
    assert ls, 'no loop found: the disassembly format changed?'
    for a, b in ls:
        assert 'ds_read2_b64' not in [op for _, op, _ in text[a:b + 1]]


def is_new_direct(s):
    """a k-loop of w25t_round_direct: 48 MFMAs behind three 16-byte loads per k-step"""
    return s['mfma'] == 48 and s['vmem'] == 12


@pytest.mark.parametrize('name', KERNELS)
def test_matrix_instruction_count(code_object, name):
    """The whole list of the fused kernel, exactly.  Every k-loop of W25_LOOPS is here with its count (the layers without a part run
    them); the forms of the 128-output layers add loops of 48 only: per form four Winograd passes and one direct loop."""
    asm, _ = code_object
    stats = loop_stats(kernel_text(asm, name))
    counts = sorted(s['mfma'] for s in stats)
    print(f'MFMAs per k-loop of {name}:', counts)
    assert sorted(W25_LOOPS) == [24] * 6 + [32] * 12 + [48] * 7 + [56] * 2 + [96] + [112]
    assert W25T_LOOPS == [24] * 6 + [32] * 12 + [48] * 22 + [56] * 2 + [96] + [112]      # three forms x (4 passes + 1 direct loop) more
    assert counts == W25T_LOOPS, counts
    assert sum(1 for s in stats if is_new_direct(s)) == 2            # taps and order | taps only


@pytest.mark.parametrize('name', KERNELS)
def test_the_new_direct_loops(code_object, name):
    """Per iteration four k-steps: 48 MFMAs, the window words of two rows as six paired 4-byte LDS reads per two k-steps, three 16-byte
    buffer loads per k-step -- and no tap arithmetic: no float addition, subtraction or multiplication at all, no copies between the
    register files.  The last iteration stands behind the loop: 48 more MFMAs per direct round outside the k-loops, and no other layer
    form has a matrix instruction outside its k-loops."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    new = []
    for a, b in loops(text):
        ops = [op for _, op, _ in text[a:b + 1]]
        if sum(o.startswith('v_mfma') for o in ops) == 48 and sum(o.startswith('buffer_load') for o in ops) == 12:
            new.append(ops)
    assert len(new) == 2
    for ops in new:
        valu = [o for o in ops if o.startswith('v_') and not o.startswith('v_mfma')]
        print(name, 'vector instructions beside the MFMAs:', valu)
        assert ops.count('buffer_load_dwordx4') == 12
        assert not [o for o in valu if re.match(r'v_(add|sub|subrev|mul|fma|fmac|mac|mad)_f32', o)], valu
        assert not [o for o in valu if o.startswith('v_accvgpr')]
        assert len(valu) <= 8
        assert sum(o.startswith('ds_read') for o in ops) == 12 and 'ds_read_b64' not in ops
    stats = loop_stats(text)
    assert sum(1 for _, op, _ in text if op.startswith('v_mfma')) == sum(s['mfma'] for s in stats) + 2 * 48


@pytest.mark.parametrize('name', KERNELS)
def test_no_parking_behind_the_winograd_round(code_object, name):
    """The two forms with the direct round first: between one workgroup barrier and the next stand the direct loop and then the four
    Winograd passes, and from the end of the last pass to the barrier nothing is written to an accumulation register (w24_layer_pair
    parks 72 values per lane there; these forms park 8 behind the direct round)."""
    asm, _ = code_object
    text = kernel_text(asm, name)
    bars = [i for i, (_, op, _) in enumerate(text) if op == 's_barrier']
    found = []
    for lo, hi in zip(bars, bars[1:]):
        inside = [(a, b) for a, b in loops(text) if lo < a and b < hi]
        st = [dict(mfma=sum(op.startswith('v_mfma') for _, op, _ in text[a:b + 1]), vmem=sum(op.startswith('buffer_load') for _, op, _ in text[a:b + 1]))
              for a, b in inside]
        st = [(s, ab) for s, ab in zip(st, inside) if s['mfma']]
        if len(st) != 5 or any(s['mfma'] != 48 for s, _ in st):
            continue
        direct = [k for k, (s, _) in enumerate(st) if s['vmem'] in (12, 24)]          # 12: host taps, 24: w24_round_direct
        assert len(direct) == 1
        if direct[0] != 0:
            continue                                                                 # the Winograd round first
        tail = [op for _, op, _ in text[st[-1][1][1] + 1:hi]]
        writes = sum(op.startswith('v_accvgpr_write') for op in tail)
        between = [op for _, op, _ in text[st[0][1][1] + 1:st[1][1][0]]]
        print(name, 'direct loop with', st[0][0]['vmem'], 'loads: accumulation-register writes behind the last pass', writes,
              '| behind the direct round', sum(op.startswith('v_accvgpr_write') for op in between))
        assert writes == 0
        found.append(st[0][0]['vmem'])
    assert sorted(found) == [12, 24], found
