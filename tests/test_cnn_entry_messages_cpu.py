"""Return code and FULL buf_last_error() text of a fixed list of bad calls to the fp32 CNN entry points: the four descriptor-net calls
(buf_cylindrical_net_wg, _wg_form, _wg_all, _w25), their four split-safe forms, the six dense / gathered cost-net calls and their three
split-safe forms, and the query functions (buf_cylindrical_net_wg_supports, _wg_flags, _wg_all_flags, _w25_flags).  Everything is validated
before the first device call, so dummy pointers do; no GPU needed.

EXPECTED was recorded by running this list against a build of the commit BEFORE the host launch code of these kernels was folded onto
one path per family (`BUF_LIB_PATH=<that build> python tests/test_cnn_entry_messages_cpu.py` prints the table) and pasted in: the fold
moved no message.  Five cases could not be recorded on a machine without a GPU and are written out from that commit's format strings
(LATE below): null fp32 weights handed to buf_cylindrical_net_split_safe[_form] and to the three cost-net split-safe calls, which that
commit found only in the launcher of the fp32 re-run, BEHIND its memset and its split kernel.  They are found before the first device
call now; code and text are the ones that launcher gave."""
import ctypes as C

import pytest

from test_cyl_f24k_cpu import RELEASED_IN, RELEASED_OUT, ints

WORDS = (1, 5, 3, 3, 5, 5, 1, 0)
LATE = ('split_safe: null weights', 'split_safe_form: null weights', 'cost_split_safe: null weights', 'cost_split_safe_w24: null weights',
        'cost_split_safe_w24b: null weights')


def bad_calls():
    """[(label, entry point, arguments)]"""
    dummy = (C.c_float * 4)()
    x = C.addressof(dummy)
    keep = [dummy]

    def arr(n, *holes):
        a = (C.c_void_p * n)(*[None if i in holes else x for i in range(n)])
        keep.append(a)
        return a

    p8, none8, own = arr(8), arr(8, *range(8)), arr(8, 1, 2, 3, 4, 5)          # own: a set for layer 0 and the two 32-output layers
    ci, co, re_ = ints(*RELEASED_IN), ints(*RELEASED_OUT), ints(*WORDS)
    plain = ints(1, 1, 1, 1, 1, 1, 1, 0)
    a_in, a_out, a_words = ints(48, 64, 32, 32, 64, 64, 64, 32), ints(64, 32, 32, 64, 64, 64, 32, 32), ints(1, 1, 1, 1, 5, 5, 1, 0)
    bad_in = ints(40, 64, 64, 128, 128, 64, 64, 32)
    wrong_flag = ints(1, 5, 1, 3, 5, 5, 1, 0)                               # a 128-output layer without bit 1
    ten, eleven, s3, s5 = arr(10), arr(11), arr(3), arr(5)
    out = []

    # the descriptor net: (x, npatch, wt, bias, cin, cout, relu, [form | wt24 [, wt25]], y, stream)
    def wg(tail, npatch=2, x_=x, wt=p8, ci_=ci, co_=co, re__=re_):
        return (x_, npatch, wt, p8, ci_, co_, re__) + tail + (x, None)

    for name, tail in (('wg', ()), ('wg_form', (1,)), ('wg_all', (own,)), ('w25', (own, none8))):
        f = 'buf_cylindrical_net_' + name
        out += [(f'{name}: negative count', f, wg(tail, npatch=-1)), (f'{name}: null argument', f, wg(tail, x_=None)),
                (f'{name}: null weights', f, wg(tail, wt=arr(8, 3))), (f'{name}: bad widths', f, wg(tail, ci_=bad_in)),
                (f'{name}: flag on the wrong layer', f, wg(tail, re__=wrong_flag)),
                (f'{name}: relu word of 8', f, wg(tail, re__=ints(1, 5, 3, 3, 5, 8, 1, 0)))]
    out += [('wg_form: bad form', 'buf_cylindrical_net_wg_form', wg((2,))),
            ('wg: a wider layer behind a 32-output layer', 'buf_cylindrical_net_wg', wg((), ci_=a_in, co_=a_out, re__=a_words)),
            ('wg_all: null sets', 'buf_cylindrical_net_wg_all', wg((None,))),
            ('w25: null F(2x5) sets', 'buf_cylindrical_net_w25', wg((own, None))),
            ('wg_all: only 32-output layers may follow', 'buf_cylindrical_net_wg_all', wg((none8,), ci_=a_in, co_=a_out, re__=a_words)),
            ('w25: only 32-output layers may follow', 'buf_cylindrical_net_w25', wg((none8, none8), ci_=a_in, co_=a_out, re__=a_words)),
            ('wg_all: a set on a layer that takes none', 'buf_cylindrical_net_wg_all', wg((arr(8, 0, 2, 3, 4, 5, 6, 7),))),
            ('w25: an F(2x4) set on a layer that takes none', 'buf_cylindrical_net_w25', wg((arr(8, 0, 1, 3, 4, 5, 6, 7), none8))),
            ('w25: an F(2x5) set on a layer that takes none', 'buf_cylindrical_net_w25', wg((own, arr(8, 0, 1, 2, 4, 5, 6, 7))))]

    # its split-safe forms: (x, npatch, wt_split, wt_wg, bias, cin, cout, relu, [form | wt24 [, wt25]], head, y, desc, status, flags, stream)
    def safe(mid, npatch=2, x_=x, wt=p8, ci_=ci, co_=co, re__=re_, head=None):
        return (x_, npatch, p8, wt, p8, ci_, co_, re__) + mid + (head, x, None, None, x, None)

    for name, mid in (('split_safe', ()), ('split_safe_form', (1,)), ('split_safe_all', (own,)), ('split_safe_w25', (own, none8))):
        f = 'buf_cylindrical_net_' + name
        out += [(f'{name}: negative count', f, safe(mid, npatch=-1)), (f'{name}: null argument', f, safe(mid, x_=None)),
                (f'{name}: null weights', f, safe(mid, wt=arr(8, 3))), (f'{name}: head without desc', f, safe(mid, head=x)),
                (f'{name}: bad widths', f, safe(mid, ci_=bad_in)), (f'{name}: flag on the wrong layer', f, safe(mid, re__=wrong_flag))]
    out += [('split_safe_form: bad form', 'buf_cylindrical_net_split_safe_form', safe((-2,))),
            ('split_safe: no relu words', 'buf_cylindrical_net_split_safe', safe((), re__=None)),
            ('split_safe_all: null sets', 'buf_cylindrical_net_split_safe_all', safe((None,))),
            ('split_safe_w25: null F(2x5) sets', 'buf_cylindrical_net_split_safe_w25', safe((own, None))),
            ('split_safe_all: only 32-output layers may follow', 'buf_cylindrical_net_split_safe_all',
             safe((none8,), ci_=a_in, co_=a_out, re__=a_words)),
            ('split_safe_w25: only 32-output layers may follow', 'buf_cylindrical_net_split_safe_w25',
             safe((none8, none8), ci_=a_in, co_=a_out, re__=a_words)),
            ('split_safe_all: a set on a layer that takes none', 'buf_cylindrical_net_split_safe_all', safe((arr(8, 0, 2, 3, 4, 5, 6, 7),))),
            ('split_safe_w25: an F(2x5) set on a layer that takes none', 'buf_cylindrical_net_split_safe_w25',
             safe((own, arr(8, 0, 1, 2, 4, 5, 6, 7))))]

    # the queries
    out += [('wg_supports: null argument', 'buf_cylindrical_net_wg_supports', (ci, None)),
            ('wg_supports: bad widths', 'buf_cylindrical_net_wg_supports', (bad_in, co)),
            ('wg_supports: a wider layer behind a 32-output layer', 'buf_cylindrical_net_wg_supports', (a_in, a_out)),
            ('wg_flags: null argument', 'buf_cylindrical_net_wg_flags', (ci, co, None)),
            ('wg_flags: flag on the wrong layer', 'buf_cylindrical_net_wg_flags', (ci, co, wrong_flag)),
            ('wg_flags: bit 2 on layer 0', 'buf_cylindrical_net_wg_flags', (ci, co, ints(5, 5, 3, 3, 5, 5, 1, 0))),
            ('wg_flags: a wider layer behind a 32-output layer', 'buf_cylindrical_net_wg_flags', (a_in, a_out, a_words)),
            ('wg_all_flags: null argument', 'buf_cylindrical_net_wg_all_flags', (ci, co, re_, None)),
            ('wg_all_flags: only 32-output layers may follow', 'buf_cylindrical_net_wg_all_flags', (a_in, a_out, a_words, none8)),
            ('wg_all_flags: a set on a layer that takes none', 'buf_cylindrical_net_wg_all_flags', (ci, co, re_, arr(8, 0, 2, 3, 4, 5, 6, 7))),
            ('wg_all_flags: relu word of 8', 'buf_cylindrical_net_wg_all_flags', (ci, co, ints(1, 5, 3, 3, 5, 8, 1, 0), own)),
            ('w25_flags: null argument', 'buf_cylindrical_net_w25_flags', (ci, co, re_, own, None)),
            ('w25_flags: only 32-output layers may follow', 'buf_cylindrical_net_w25_flags', (a_in, a_out, a_words, none8, none8)),
            ('w25_flags: an F(2x5) set on a layer that takes none', 'buf_cylindrical_net_w25_flags', (ci, co, plain, none8, arr(8, 0, 1, 2, 4, 5, 6, 7))),
            ('w25_flags: bad widths', 'buf_cylindrical_net_w25_flags', (bad_in, co, re_, own, none8))]

    # the cost net: dense (s_eq, t_eq, m, wt, bias, [sets], ind, stream), gathered (equi, ele_n, s_rows, t_rows, m, wt, bias, [sets], ind, stream)
    for name, sets in (('', None), ('_w24', s3), ('_w24b', s5)):
        f, tail = 'buf_cost_volume_net' + name, (() if sets is None else (sets,))
        out += [(f'cost{name}: negative count', f, (x, x, -1, ten, ten) + tail + (x, None)),
                (f'cost{name}: null argument', f, (x, None, 2, ten, ten) + tail + (x, None)),
                (f'cost{name}: null weights', f, (x, x, 2, arr(10, 4), ten) + tail + (x, None)),
                (f'cost{name}: null bias', f, (x, x, 2, ten, arr(10, 9)) + tail + (x, None)),
                (f'cost{name}_gather: negative count', f + '_gather', (x, 7, x, x, -3, ten, ten) + tail + (x, None)),
                (f'cost{name}_gather: ele_n=6', f + '_gather', (x, 6, x, x, 2, ten, ten) + tail + (x, None)),
                (f'cost{name}_gather: null argument', f + '_gather', (x, 7, x, None, 2, ten, ten) + tail + (x, None)),
                (f'cost{name}_gather: null weights', f + '_gather', (x, 7, x, x, 2, arr(10, 0), ten) + tail + (x, None))]
        if sets is not None:
            out += [(f'cost{name}: null sets', f, (x, x, 2, ten, ten, None, x, None)),
                    (f'cost{name}_gather: null sets', f + '_gather', (x, 7, x, x, 2, ten, ten, None, x, None))]

        # (s_eq, t_eq, ele_n, s_rows, t_rows, m, wt_split, bias_split, wt_f32, bias_f32, [sets], ind, status, flags, stream)
        def cs(m=2, t=x, ele_n=7, s_rows=None, t_rows=None, wt=ten, flags=x):
            return (x, t, ele_n, s_rows, t_rows, m, eleven, ten, wt, ten) + tail + (x, None, flags, None)

        f = 'buf_cost_volume_net_split_safe' + name
        out += [(f'cost_split_safe{name}: negative count', f, cs(m=-1)), (f'cost_split_safe{name}: null argument', f, cs(t=None)),
                (f'cost_split_safe{name}: no flags', f, cs(flags=None)),
                (f'cost_split_safe{name}: one row list without the other', f, cs(s_rows=x)),
                (f'cost_split_safe{name}: ele_n=6', f, cs(ele_n=6, s_rows=x, t_rows=x)),
                (f'cost_split_safe{name}: null weights', f, cs(wt=arr(10, 4)))]
    out.append(('cost_split_safe_w24: null sets', 'buf_cost_volume_net_split_safe_w24', (x, x, 7, None, None, 2, eleven, ten, ten, ten, None, x, None, x, None)))
    return out, keep


EXPECTED = {
    'wg: negative count': (-1, 'buf_cylindrical_net_wg: npatch=-1'),
    'wg: null argument': (-1, 'buf_cylindrical_net_wg: null argument'),
    'wg: null weights': (-1, 'buf_cylindrical_net_wg: null weights for layer 3'),
    'wg: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'wg: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'wg: relu word of 8': (-1, 'buf_cylindrical_net_wg: layer 5 has the relu word 8 (bit 0: ReLU, bits 1 and 2: the F(2x4) flags, nothing above)'),
    'wg_form: negative count': (-1, 'buf_cylindrical_net_wg: npatch=-1'),
    'wg_form: null argument': (-1, 'buf_cylindrical_net_wg: null argument'),
    'wg_form: null weights': (-1, 'buf_cylindrical_net_wg: null weights for layer 3'),
    'wg_form: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'wg_form: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'wg_form: relu word of 8': (-1, 'buf_cylindrical_net_wg: layer 5 has the relu word 8 (bit 0: ReLU, bits 1 and 2: the F(2x4) flags, nothing above)'),
    'wg_all: negative count': (-1, 'buf_cylindrical_net_wg_all: npatch=-1'),
    'wg_all: null argument': (-1, 'buf_cylindrical_net_wg_all: null argument'),
    'wg_all: null weights': (-1, 'buf_cylindrical_net_wg_all: null weights for layer 3'),
    'wg_all: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'wg_all: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'wg_all: relu word of 8': (-1, 'buf_cylindrical_net_wg: layer 5 has the relu word 8 (bit 0: ReLU, bits 1 and 2: the F(2x4) flags, nothing above)'),
    'w25: negative count': (-1, 'buf_cylindrical_net_w25: npatch=-1'),
    'w25: null argument': (-1, 'buf_cylindrical_net_w25: null argument'),
    'w25: null weights': (-1, 'buf_cylindrical_net_w25: null weights for layer 3'),
    'w25: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'w25: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'w25: relu word of 8': (-1, 'buf_cylindrical_net_wg: layer 5 has the relu word 8 (bit 0: ReLU, bits 1 and 2: the F(2x4) flags, nothing above)'),
    'wg_form: bad form': (-1, "buf_cylindrical_net_wg: form=2 (-1: the library's default, 0: K split, 1: pass split)"),
    'wg: a wider layer behind a 32-output layer': (-1, 'buf_cylindrical_net_wg: layer 3 has unsupported widths 32 -> 64 (only 32-output layers may follow a 32-output layer)'),
    'wg_all: null sets': (-1, 'buf_cylindrical_net_wg_all: null argument'),
    'w25: null F(2x5) sets': (-1, 'buf_cylindrical_net_w25: null argument'),
    'wg_all: only 32-output layers may follow': (-1, 'buf_cylindrical_net_wg_all: layer 3 has unsupported widths 32 -> 64 (once a 32-output layer in the F(2x2) form has run, layer 1 here, only 32-output layers may follow)'),
    'w25: only 32-output layers may follow': (-1, 'buf_cylindrical_net_w25: layer 3 has unsupported widths 32 -> 64 (once a 32-output layer in the F(2x2) form has run, layer 1 here, only 32-output layers may follow)'),
    'wg_all: a set on a layer that takes none': (-1, 'buf_cylindrical_net_wg_all: layer 1 (64 -> 64, flags 5) takes no F(2x4) set of its own (64 or 32 output channels, no F(2x4) flag)'),
    'w25: an F(2x4) set on a layer that takes none': (-1, 'buf_cylindrical_net_w25: layer 2 (64 -> 128, flags 3) takes no F(2x4) set of its own (64 or 32 output channels, no F(2x4) flag)'),
    'w25: an F(2x5) set on a layer that takes none': (-1, 'buf_cylindrical_net_w25: layer 3 (128 -> 128) takes no F(2x5) set (64 or 32 output channels, Cin % 16 == 0)'),
    'split_safe: negative count': (-1, 'buf_cylindrical_net_split_safe: npatch=-1'),
    'split_safe: null argument': (-1, 'buf_cylindrical_net_split_safe: null argument'),
    'split_safe: null weights': (-1, 'buf_cylindrical_net_wg: null weights for layer 3'),
    'split_safe: head without desc': (-1, 'buf_cylindrical_net_split_safe: head without desc'),
    'split_safe: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'split_safe: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'split_safe_form: negative count': (-1, 'buf_cylindrical_net_split_safe: npatch=-1'),
    'split_safe_form: null argument': (-1, 'buf_cylindrical_net_split_safe: null argument'),
    'split_safe_form: null weights': (-1, 'buf_cylindrical_net_wg: null weights for layer 3'),
    'split_safe_form: head without desc': (-1, 'buf_cylindrical_net_split_safe: head without desc'),
    'split_safe_form: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'split_safe_form: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'split_safe_all: negative count': (-1, 'buf_cylindrical_net_split_safe_all: npatch=-1'),
    'split_safe_all: null argument': (-1, 'buf_cylindrical_net_split_safe_all: null argument'),
    'split_safe_all: null weights': (-1, 'buf_cylindrical_net_wg_all: null weights for layer 3'),
    'split_safe_all: head without desc': (-1, 'buf_cylindrical_net_split_safe_all: head without desc'),
    'split_safe_all: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'split_safe_all: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'split_safe_w25: negative count': (-1, 'buf_cylindrical_net_split_safe_w25: npatch=-1'),
    'split_safe_w25: null argument': (-1, 'buf_cylindrical_net_split_safe_w25: null argument'),
    'split_safe_w25: null weights': (-1, 'buf_cylindrical_net_w25: null weights for layer 3'),
    'split_safe_w25: head without desc': (-1, 'buf_cylindrical_net_split_safe_w25: head without desc'),
    'split_safe_w25: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'split_safe_w25: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'split_safe_form: bad form': (-1, "buf_cylindrical_net_split_safe: form=-2 (-1: the library's default, 0: K split, 1: pass split)"),
    'split_safe: no relu words': (-1, 'buf_cylindrical_net_split_safe: null argument'),
    'split_safe_all: null sets': (-1, 'buf_cylindrical_net_wg_all: null argument'),
    'split_safe_w25: null F(2x5) sets': (-1, 'buf_cylindrical_net_w25: null argument'),
    'split_safe_all: only 32-output layers may follow': (-1, 'buf_cylindrical_net_wg_all: layer 3 has unsupported widths 32 -> 64 (once a 32-output layer in the F(2x2) form has run, layer 1 here, only 32-output layers may follow)'),
    'split_safe_w25: only 32-output layers may follow': (-1, 'buf_cylindrical_net_w25: layer 3 has unsupported widths 32 -> 64 (once a 32-output layer in the F(2x2) form has run, layer 1 here, only 32-output layers may follow)'),
    'split_safe_all: a set on a layer that takes none': (-1, 'buf_cylindrical_net_wg_all: layer 1 (64 -> 64, flags 5) takes no F(2x4) set of its own (64 or 32 output channels, no F(2x4) flag)'),
    'split_safe_w25: an F(2x5) set on a layer that takes none': (-1, 'buf_cylindrical_net_w25: layer 3 (128 -> 128) takes no F(2x5) set (64 or 32 output channels, Cin % 16 == 0)'),
    'wg_supports: null argument': (-1, 'buf_cylindrical_net_wg_supports: null argument'),
    'wg_supports: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'wg_supports: a wider layer behind a 32-output layer': (-1, 'buf_cylindrical_net_wg: layer 3 has unsupported widths 32 -> 64 (only 32-output layers may follow a 32-output layer)'),
    'wg_flags: null argument': (-1, 'buf_cylindrical_net_wg_flags: null argument'),
    'wg_flags: flag on the wrong layer': (-1, 'buf_cylindrical_net_wg: the F(2x4) flag goes on every layer with 128 output channels and on no other (layer 2: 64 -> 128, flags 1)'),
    'wg_flags: bit 2 on layer 0': (-1, 'buf_cylindrical_net_wg: the K-split F(2x4) flag (bit 2) goes only on layers with 64 output channels and Cin % 64 == 0 (layer 0: 48 -> 64, flags 5)'),
    'wg_flags: a wider layer behind a 32-output layer': (-1, 'buf_cylindrical_net_wg: layer 3 has unsupported widths 32 -> 64 (only 32-output layers may follow a 32-output layer)'),
    'wg_all_flags: null argument': (-1, 'buf_cylindrical_net_wg_all_flags: null argument'),
    'wg_all_flags: only 32-output layers may follow': (-1, 'buf_cylindrical_net_wg_all: layer 3 has unsupported widths 32 -> 64 (once a 32-output layer in the F(2x2) form has run, layer 1 here, only 32-output layers may follow)'),
    'wg_all_flags: a set on a layer that takes none': (-1, 'buf_cylindrical_net_wg_all: layer 1 (64 -> 64, flags 5) takes no F(2x4) set of its own (64 or 32 output channels, no F(2x4) flag)'),
    'wg_all_flags: relu word of 8': (-1, 'buf_cylindrical_net_wg: layer 5 has the relu word 8 (bit 0: ReLU, bits 1 and 2: the F(2x4) flags, nothing above)'),
    'w25_flags: null argument': (-1, 'buf_cylindrical_net_w25_flags: null argument'),
    'w25_flags: only 32-output layers may follow': (-1, 'buf_cylindrical_net_w25: layer 3 has unsupported widths 32 -> 64 (once a 32-output layer in the F(2x2) form has run, layer 1 here, only 32-output layers may follow)'),
    'w25_flags: an F(2x5) set on a layer that takes none': (-1, 'buf_cylindrical_net_w25: layer 3 (128 -> 128) takes no F(2x5) set (64 or 32 output channels, Cin % 16 == 0)'),
    'w25_flags: bad widths': (-1, 'buf_cylindrical_net_wg: layer 0 has unsupported widths 40 -> 64'),
    'cost: negative count': (-1, 'buf_cost_volume_net: m=-1'),
    'cost: null argument': (-1, 'buf_cost_volume_net: null argument'),
    'cost: null weights': (-1, 'buf_cost_volume_net: null weights for layer 4'),
    'cost: null bias': (-1, 'buf_cost_volume_net: null weights for layer 9'),
    'cost_gather: negative count': (-1, 'buf_cost_volume_net_gather: m=-3 ele_n=7 (the kernel is built for ele_n = 7)'),
    'cost_gather: ele_n=6': (-1, 'buf_cost_volume_net_gather: m=2 ele_n=6 (the kernel is built for ele_n = 7)'),
    'cost_gather: null argument': (-1, 'buf_cost_volume_net_gather: null argument'),
    'cost_gather: null weights': (-1, 'buf_cost_volume_net_gather: null weights for layer 0'),
    'cost_split_safe: negative count': (-1, 'buf_cost_volume_net_split_safe: m=-1'),
    'cost_split_safe: null argument': (-1, 'buf_cost_volume_net_split_safe: null argument'),
    'cost_split_safe: no flags': (-1, 'buf_cost_volume_net_split_safe: null argument'),
    'cost_split_safe: one row list without the other': (-1, 'buf_cost_volume_net_split_safe: one row list without the other'),
    'cost_split_safe: ele_n=6': (-1, 'buf_cost_volume_net_split_safe: ele_n=6 (the kernels are built for ele_n = 7)'),
    'cost_split_safe: null weights': (-1, 'buf_cost_volume_net_split_safe: null weights for layer 4'),
    'cost_w24: negative count': (-1, 'buf_cost_volume_net_w24: m=-1'),
    'cost_w24: null argument': (-1, 'buf_cost_volume_net_w24: null argument'),
    'cost_w24: null weights': (-1, 'buf_cost_volume_net_w24: null weights for layer 4'),
    'cost_w24: null bias': (-1, 'buf_cost_volume_net_w24: null weights for layer 9'),
    'cost_w24_gather: negative count': (-1, 'buf_cost_volume_net_w24_gather: m=-3 ele_n=7 (the kernel is built for ele_n = 7)'),
    'cost_w24_gather: ele_n=6': (-1, 'buf_cost_volume_net_w24_gather: m=2 ele_n=6 (the kernel is built for ele_n = 7)'),
    'cost_w24_gather: null argument': (-1, 'buf_cost_volume_net_w24_gather: null argument'),
    'cost_w24_gather: null weights': (-1, 'buf_cost_volume_net_w24_gather: null weights for layer 0'),
    'cost_w24: null sets': (-1, 'buf_cost_volume_net_w24: null argument'),
    'cost_w24_gather: null sets': (-1, 'buf_cost_volume_net_w24_gather: null argument'),
    'cost_split_safe_w24: negative count': (-1, 'buf_cost_volume_net_split_safe_w24: m=-1'),
    'cost_split_safe_w24: null argument': (-1, 'buf_cost_volume_net_split_safe_w24: null argument'),
    'cost_split_safe_w24: no flags': (-1, 'buf_cost_volume_net_split_safe_w24: null argument'),
    'cost_split_safe_w24: one row list without the other': (-1, 'buf_cost_volume_net_split_safe_w24: one row list without the other'),
    'cost_split_safe_w24: ele_n=6': (-1, 'buf_cost_volume_net_split_safe_w24: ele_n=6 (the kernels are built for ele_n = 7)'),
    'cost_split_safe_w24: null weights': (-1, 'buf_cost_volume_net_split_safe_w24: null weights for layer 4'),
    'cost_w24b: negative count': (-1, 'buf_cost_volume_net_w24b: m=-1'),
    'cost_w24b: null argument': (-1, 'buf_cost_volume_net_w24b: null argument'),
    'cost_w24b: null weights': (-1, 'buf_cost_volume_net_w24b: null weights for layer 4'),
    'cost_w24b: null bias': (-1, 'buf_cost_volume_net_w24b: null weights for layer 9'),
    'cost_w24b_gather: negative count': (-1, 'buf_cost_volume_net_w24b_gather: m=-3 ele_n=7 (the kernel is built for ele_n = 7)'),
    'cost_w24b_gather: ele_n=6': (-1, 'buf_cost_volume_net_w24b_gather: m=2 ele_n=6 (the kernel is built for ele_n = 7)'),
    'cost_w24b_gather: null argument': (-1, 'buf_cost_volume_net_w24b_gather: null argument'),
    'cost_w24b_gather: null weights': (-1, 'buf_cost_volume_net_w24b_gather: null weights for layer 0'),
    'cost_w24b: null sets': (-1, 'buf_cost_volume_net_w24b: null argument'),
    'cost_w24b_gather: null sets': (-1, 'buf_cost_volume_net_w24b_gather: null argument'),
    'cost_split_safe_w24b: negative count': (-1, 'buf_cost_volume_net_split_safe_w24b: m=-1'),
    'cost_split_safe_w24b: null argument': (-1, 'buf_cost_volume_net_split_safe_w24b: null argument'),
    'cost_split_safe_w24b: no flags': (-1, 'buf_cost_volume_net_split_safe_w24b: null argument'),
    'cost_split_safe_w24b: one row list without the other': (-1, 'buf_cost_volume_net_split_safe_w24b: one row list without the other'),
    'cost_split_safe_w24b: ele_n=6': (-1, 'buf_cost_volume_net_split_safe_w24b: ele_n=6 (the kernels are built for ele_n = 7)'),
    'cost_split_safe_w24b: null weights': (-1, 'buf_cost_volume_net_split_safe_w24b: null weights for layer 4'),
    'cost_split_safe_w24: null sets': (-1, 'buf_cost_volume_net_split_safe_w24: null argument'),
}


def run(L, fn, args):
    rc = getattr(L, fn)(*args)
    return rc, (L.buf_last_error() or b'').decode()


CALLS, _KEEP = bad_calls()


def test_the_list_is_the_recorded_one():
    assert [label for label, _, _ in CALLS] == list(EXPECTED) and len(set(EXPECTED)) == len(CALLS) and set(LATE) <= set(EXPECTED)
    entries = {fn for _, fn, _ in CALLS}
    assert len(entries) == 17 + 4, sorted(entries)


@pytest.mark.parametrize('label,fn,args', CALLS, ids=[c[0] for c in CALLS])
def test_code_and_message(label, fn, args):
    from buffer_amd import _lib
    assert run(_lib.lib(), fn, args) == EXPECTED[label]


if __name__ == '__main__':          # prints the table of the library BUF_LIB_PATH names (default: the in-tree build)
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from buffer_amd import _lib
    for label, fn, args in CALLS:
        print(f'    {label!r}: {run(_lib.lib(), fn, args)!r},')
