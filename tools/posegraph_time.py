"""Time buf_pose_graph_optimize (csrc/posegraph.hip): HIP-event ms per call and per solve, the kernel's own split of its time
(factorisation / substitution / linearisation + assembly, from its 100 MHz tick counters in the workspace), and the float64 numpy
restatement's host time on the same graphs -- the only yardstick there is.

    python tools/posegraph_time.py [--repeat 5]

Cases: (N = 60, E = 300) at G = 1 and G = 8, (N = 128, E = 1000) at G = 1; the generator of tests/posegraph_ref.py, all edges
uncertain, 5 % of the chords false.  Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import posegraph_ref as R                                    # noqa: E402
from buffer_amd import ops                                   # noqa: E402


def flatten(graphs, dev):
    allE = [e for g in graphs for e in g['edges']]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)        # noqa: E731
    return dict(nodes=[g['n'] for g in graphs], edges=[len(g['edges']) for g in graphs], edge_i=[e['i'] for e in allE],
                edge_j=[e['j'] for e in allE], Z=t(np.array([e['T'] for e in allE])), info=t(np.array([e['info'] for e in allE])),
                uncertain=[1 if e['uncertain'] else 0 for e in allE], fixed=[g['fixed'] for g in graphs], mu=[g['mu'] for g in graphs],
                X_init=t(np.concatenate([g['init'] for g in graphs])))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--repeat', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    for n, e, G in ((60, 300, 1), (60, 300, 8), (128, 1000, 1)):
        chords = e - (n - 1)
        false = chords // 20
        graphs = [R.make_scene(100 + k, n, chords - false, false)[0] for k in range(G)]
        assert all(len(g['edges']) == e for g in graphs)
        args = flatten(graphs, dev)
        ops.pose_graph_optimize(**args)                      # warm-up: module load, workspace allocation
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeat):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            X, status, cost, edge, ticks = ops.pose_graph_optimize(**args, want_ticks=True)
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        status, ticks = status.cpu().numpy(), ticks.cpu().numpy().astype(np.float64)
        h0 = time.perf_counter()
        ref = [R.optimize(g) for g in graphs]
        host_ms = 1e3 * (time.perf_counter() - h0)
        same = all((ops.PG_STATUS[int(s[0])], int(s[1]), int(s[2])) == (r['status'], r['solves'], r['accepted']) for s, r in zip(status, ref))
        tot = ticks[:, 0].sum()
        print(json.dumps(dict(nodes=n, edges=e, graphs=G, ms_per_call=float(np.median(ms)), ms_all=[round(x, 3) for x in ms],
                              solves=[int(s[1]) for s in status], status=[ops.PG_STATUS[int(s[0])] for s in status],
                              ms_per_solve=float(np.median(ms) / max(int(status[:, 1].max()), 1)),
                              kernel_ms_longest_graph=float(ticks[:, 0].max() / ops.PG_TICK_HZ * 1e3),
                              share_factorisation=float(ticks[:, 1].sum() / tot), share_substitution=float(ticks[:, 2].sum() / tot),
                              share_linearise_assemble=float(ticks[:, 3].sum() / tot),
                              restatement_host_ms=host_ms, restatement_agrees_on_counts=bool(same))))


if __name__ == '__main__':
    main()
