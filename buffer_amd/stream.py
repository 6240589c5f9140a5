"""BASELINE config #3 on synthetic data: a stream of fragment pairs from RAW clouds through the test-split
pre-processing (ThreeDMatch/dataset.py:91-153 on device: two voxel levels, shuffles, 30-NN normals) and the batched
registration path, evaluated with the 3DMatch protocol (ThreeDMatch/test.py:114-173,263-308: DGR criterion per pair,
Registration Recall = mean over 8 scenes of the per-scene recall on non-consecutive fragment pairs through the
gt.info RMSE proxy).  The real test set (1623 pairs over 8 scenes) is not available offline: pair k of the stream goes to
scene k mod 8 as fragments (3q, 3q+2) with q = k div 8, and its gt.info matrix comes from the shared slab of the room."""
import time

import numpy as np
import torch

from . import evaluate, synth
from .driver import dgr_summary, pack_pair, pack_pairs, register_chunks

OVERLAPS = (0.75, 0.6, 0.45, 0.3)            # a quarter of the stream at 0.3 (3DLoMatch territory)
N_SCENES = 8


def generate(n_pairs, device, seed0=20000, overlaps=OVERLAPS, n_raw=250_000):
    """-> list of make_raw_pair_device dicts, device resident (the untimed part: 'files already read')."""
    return [synth.make_raw_pair_device(seed0 + k, overlaps[k % len(overlaps)], device, n_raw=n_raw) for k in range(n_pairs)]


def prepare(raw, cfg, index):
    """one raw pair -> the reference's sample dict (device tensors), seeds as PairTestSet.item"""
    return pack_pair((raw['src_raw'], raw['tgt_raw']), (2 * index, 2 * index + 1), {'relt_pose': raw['relt_pose']}, cfg)


def prepare_batch(raws, cfg, indices):
    """prepare() for several raw pairs with the normals of all 2B fragments estimated in one stacked pass (same result)"""
    return pack_pairs([r[f'{side}_raw'] for r in raws for side in ('src', 'tgt')], [2 * i + j for i in indices for j in range(2)],
                      [{'relt_pose': r['relt_pose']} for r in raws], cfg)


def run(pipe, raws, batch=32, first_index=0):
    """Timed part: pre-processing + registration of every pair, `batch` pairs per set of stacked launches, batches
    software-pipelined (driver.register_chunks).  Pair k of `raws` is pair first_index + k of the stream.
    -> (poses f32[n,4,4] device, seconds)."""
    dev = pipe.device
    ids = range(first_index, first_index + len(raws))
    chunks = [list(ids[lo:lo + batch]) for lo in range(0, len(raws), batch)]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    res = register_chunks(pipe, chunks, lambda ch: prepare_batch([raws[i - first_index] for i in ch], pipe.cfg, ch))
    torch.cuda.synchronize(dev)
    return res, time.perf_counter() - t0


def evaluate_stream(raws, poses, first_index=0):
    """3DMatch protocol over the synthetic stream -> dict(dgr_recall, registration_recall, per_scene, te, re, per-overlap)."""
    poses = np.asarray(poses, np.float64)
    n = len(raws)
    stats = [evaluate.dgr_success(poses[k], raws[k]['relt_pose']) for k in range(n)]
    scenes = [dict(pairs=[], gt=[], info=[], est=[]) for _ in range(N_SCENES)]
    for k in range(n):
        g = first_index + k
        sc, q = scenes[g % N_SCENES], g // N_SCENES
        # one leading consecutive pair per scene so that list index 0 is never a counted pair (test.py:119-123 skips it)
        if not sc['pairs']:
            sc['pairs'].append((0, 1)); sc['gt'].append(np.eye(4)); sc['info'].append(np.eye(6)); sc['est'].append(np.eye(4))
        sc['pairs'].append((3 * q + 2, 3 * q + 4))
        sc['gt'].append(np.linalg.inv(raws[k]['relt_pose']))              # gt.log: fragment j -> fragment i
        sc['info'].append(np.asarray(raws[k]['info'], np.float64) if 'info' in raws[k]
                          else synth.information_matrix(raws[k]['overlap_pts'].cpu().numpy()))
        sc['est'].append(np.linalg.inv(poses[k]))                          # the .log holds the inverse estimate (test.py:255)
    per_scene = []
    for sc in scenes:
        if len(sc['pairs']) <= 1:
            continue
        pr = np.array(sc['pairs'])
        nfrag = int(pr.max()) + 1
        _, recall, _, _ = evaluate.evaluate_registration(nfrag, np.array(sc['est']), pr, pr, np.array(sc['gt']), np.array(sc['info']))
        per_scene.append(float(recall))
    return dict(dgr_summary(stats, 'dgr_recall'), registration_recall=float(np.mean(per_scene)) if per_scene else 0.0, per_scene=per_scene)
