"""TEST INFRASTRUCTURE: runs the CPU oracle (oracle/pipeline_ref.register_pair) on prepared ETH-shape samples in a process of
its own, with the device hidden -- tests/test_eth_gpu.py writes the host samples the GPU path consumed (pre-processed on the
device by the ETH driver), the preset, the limits and the support permutations to an .npz and compares pair by pair.

    python tests/eth_oracle_worker.py --inp /tmp/eth_in_0.npz --out /tmp/eth_out_0.npz --threads 4
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inp', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--threads', type=int, default=0)
    a = ap.parse_args()
    if a.threads:
        os.environ['OMP_NUM_THREADS'] = str(a.threads)
    os.environ['CUDA_VISIBLE_DEVICES'] = ''
    os.environ['HIP_VISIBLE_DEVICES'] = ''
    from dataclasses import replace
    import numpy as np
    import torch
    if a.threads:
        torch.set_num_threads(a.threads)
    from buffer_amd.config import preset
    from buffer_amd.weights import load_weights
    from oracle import cpu, pipeline_ref
    z = np.load(a.inp)
    cfg = replace(preset(str(z['preset'])), num_keypts=int(z['keypts']))
    cpu.build(ref=False)
    W = {k: torch.from_numpy(v) for k, v in load_weights(cfg.weights).items()}
    sample = {k: z[k] for k in ('src_fds_pts', 'tgt_fds_pts', 'src_sds_pts', 'tgt_sds_pts', 'relt_pose')}
    seed = int(z['seed'])
    pose, d = pipeline_ref.register_pair(sample, W, [int(x) for x in z['limits']], cfg, seed, [z['perm0'], z['perm1']],
                                         use_ref=cpu.have_ref())
    np.savez(a.out, pose=np.asarray(pose, np.float64), kp0=d['kpts'][0].numpy(), kp1=d['kpts'][1].numpy(),
             smids=np.asarray(d['s_mids']), tmids=np.asarray(d['t_mids']))
    print('oracle pair', seed, 'done', flush=True)


if __name__ == '__main__':
    main()
