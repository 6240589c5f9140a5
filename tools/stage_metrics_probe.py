#!/usr/bin/env python3
"""Development aid for the per-stage metrics (BufferPipeline.register_batch(metrics_gt=), buf_match_metrics): the figures of DESIGN §5a.

  cost    register_batch at the benchmark configuration (5000 keypoints, 32 pairs per call) with and without metrics_gt, alternating
          in one process, HIP events around warmed-up calls; --reps 2 under `rocprofv3 --kernel-trace --stats` gives the kernel's
          own time (k_match_metrics) beside the 1-NN kernels (k_nn1f_*).
  stream  the synthetic 3DMatch stream (buffer_amd/stream.py) with metrics on: stage summary overall and per overlap class.
  eth     a synthetic ETH root (synth.make_eth_root: 4 scenes x 4 stations, seed 11, the root of tests/test_eth_gpu.py) through
          eth.main --stage-metrics for both presets."""
import argparse
import json
import os
import sys
import time
from dataclasses import replace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buffer_amd import evaluate, synth                     # noqa: E402
from buffer_amd.config import THREEDMATCH                   # noqa: E402
from buffer_amd.pipeline import BufferPipeline              # noqa: E402


def cost(a):
    dev = torch.device('cuda:0')
    pipe = BufferPipeline(replace(THREEDMATCH, num_keypts=a.keypts), dev)
    samples = [synth.make_pair(2000 + i) for i in range(a.distinct)]
    pipe.calibrate([synth.make_pair(1000)])
    inps = [pipe.upload(samples[i % a.distinct]) for i in range(a.pairs)]
    gts = np.stack([samples[i % a.distinct]['relt_pose'] for i in range(a.pairs)])
    seeds = list(range(a.pairs))

    def call(on):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipe.register_batch(inps, seeds=seeds, metrics_gt=gts if on else None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for on in (False, True, False, True):                   # warm-up of both forms
        call(on)
    ms = {False: [], True: []}
    ref = None
    for _ in range(a.reps):
        for on in (False, True):                            # alternating: drift of the shared host hits both alike
            t, out = call(on)
            ms[on].append(t)
            poses = torch.stack(out[0] if on else out)
            ref = poses if ref is None else ref
            assert torch.equal(poses, ref), 'poses moved'
    off, on = np.array(ms[False]), np.array(ms[True])
    print(json.dumps(dict(what='register_batch, HIP events', keypts=a.keypts, pairs=a.pairs, reps=a.reps,
                          off_ms=dict(median=float(np.median(off)), min=float(off.min()), max=float(off.max())),
                          on_ms=dict(median=float(np.median(on)), min=float(on.min()), max=float(on.max())),
                          delta_ms_median=float(np.median(on) - np.median(off)))))


def stream_table(a):
    from buffer_amd import stream
    from buffer_amd.driver import register_chunks
    dev = torch.device('cuda:0')
    cfg = replace(THREEDMATCH, num_keypts=1500)
    pipe = BufferPipeline(cfg, dev)
    raws = stream.generate(a.pairs, dev)
    first = stream.prepare(raws[0], cfg, 0)
    pipe.calibrate([{k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in first.items()}])
    chunks = [list(range(lo, min(lo + 32, a.pairs))) for lo in range(0, a.pairs, 32)]
    poses, counts = (x.cpu().numpy() for x in register_chunks(
        pipe, chunks, lambda ids: stream.prepare_batch([raws[i] for i in ids], cfg, ids), lambda ids: [raws[i]['relt_pose'] for i in ids]))
    ok = np.array([evaluate.dgr_success(poses[k], raws[k]['relt_pose'])[0] for k in range(a.pairs)])
    rows = {'all': np.arange(a.pairs)}
    for j, ov in enumerate(stream.OVERLAPS):
        rows[f'overlap {ov}'] = np.arange(j, a.pairs, len(stream.OVERLAPS))
    for name, idx in rows.items():
        print(json.dumps(dict(what='stream', rows=name, dgr_recall=float(ok[idx].mean()), **evaluate.stage_summary(counts[idx], 1500))))
    bad = np.nonzero(~ok)[0]
    print(json.dumps(dict(what='stream, the pairs that fail the DGR criterion', n=int(bad.size), **evaluate.stage_summary(counts[bad], 1500))))


def eth_table(a):
    from buffer_amd import eth
    root = os.path.join(a.out, 'eth_root')
    synth.make_eth_root(root, scenes=eth.SCENES, stations=4, seed=11, non_finite_rows=3)
    for name in ('3DMatch->ETH', 'KITTI->ETH'):
        poses = eth.main(['--root', root, '--preset', name, '--batch', '4', '--stage-metrics', '--log-root',
                          os.path.join(a.out, 'eth_' + name.split('-')[0])])
        rec = json.load(open(os.path.join(a.out, 'eth_' + name.split('-')[0], 'stage_metrics.json')))
        counts = np.array([r['counts'] for r in rec['pairs']])
        ds = eth.ETHTestSet(root)
        ok = np.array([evaluate.dgr_success(poses[i], ds.meta(i)['relt_pose'], 0.3, 2.0)[0] for i in range(len(ds))])
        for flag, label in ((True, 'DGR success'), (False, 'DGR failure')):
            print(json.dumps(dict(what='eth ' + name, rows=label, n=int((ok == flag).sum()), **evaluate.stage_summary(counts[ok == flag], 1500))))
        print(json.dumps(dict(what='eth ' + name, rows='per pair', ok=ok.astype(int).tolist(), counts=counts.tolist())))


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['cost', 'stream', 'eth'])
    ap.add_argument('--keypts', type=int, default=5000)
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--distinct', type=int, default=8, help='cost: distinct synthetic pairs, repeated to fill the batch')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default='stage_probe_out', help='eth: where the synthetic root and the logs go')
    a = ap.parse_args()
    t0 = time.perf_counter()
    {'cost': cost, 'stream': stream_table, 'eth': eth_table}[a.what](a)
    print(f'({a.what}: {time.perf_counter() - t0:.1f} s)')
