"""FID cost on the GPU: ms per image of metrics.FID.features_u8 (256 x 256, B = 16 and 64) with the fraction of the 157 TF
fp32 MFMA peak (11.42 GFLOP per image, every input resized to 299), and the val loop's rate with and without --fid on the same
box (--batch 16 f16x3; --batch 64 --precision f16 --rng engine), A B A B.  The val pass with FID also spends host time on the
fp64 statistics and two 2048 x 2048 sqrtm (res['host_seconds']['fid_statistics']): the loop-only rate without it is printed too.

    python tools/fid_timing.py [--images 128] > profiles/fid_timing.txt

Synthetic weights (synth.synth_inception_fid); the cost does not depend on the weight values."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GFLOP_PER_IMAGE = 11.42
PEAK_TF = 157.3


def kernel_ms(fid, b, reps=10):
    g = torch.Generator(device='cuda').manual_seed(b)
    x = torch.randint(0, 256, (b, 256, 256, 3), dtype=torch.uint8, device='cuda', generator=g)
    for _ in range(2):
        fid.features_u8(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fid.features_u8(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=128)
    a = ap.parse_args()
    from fastdiffsr_amd import val
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.metrics import FID
    from fastdiffsr_amd.synth import synth_inception_fid
    from test_gpu_val import _config_plain
    from test_val_host import make_dataset
    fid = FID(synth_inception_fid(0))
    print('# gpu: %s' % torch.cuda.get_device_name())
    for b in (16, 64):
        ms = kernel_ms(fid, b)
        tf = b * GFLOP_PER_IMAGE / ms
        print('FID.features_u8  B=%-3d 256x256: %7.2f ms per call, %.3f ms per image  (%.1f TF/s, %.1f %% of the fp32 MFMA peak)' % (
            b, ms, ms / b, tf, 100 * tf / PEAK_TF))
    tmp = tempfile.mkdtemp()
    root = make_dataset(os.path.join(tmp, 'data'), n=a.images, l=64, r=256, seed=1)
    cfg = _config_plain(root)
    cpath = os.path.join(tmp, 'cfg.json')
    with open(cpath, 'w') as f:
        json.dump(cfg, f)
    for name, kw in (('--batch 16 f16x3', dict(batch=16, precision='f16x3')),
                     ('--batch 64 --precision f16 --rng engine', dict(batch=64, precision='f16', rng='engine'))):
        from fastdiffsr_amd.model import create_model
        opt = load_config(cpath, phase='val')
        diffusion = create_model(opt)
        val.run(opt, diffusion=diffusion, save_images=False, log=lambda m: None, **kw)          # warm-up (graph capture)
        rates = {False: [], True: []}
        loop = []
        stats = []
        for use in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = val.run(opt, diffusion=diffusion, save_images=False, log=lambda m: None, fid=fid if use else None, **kw)
            dt = time.perf_counter() - t0
            rates[use].append(res['images'] / dt)
            if use:
                st = res['host_seconds']['fid_statistics']
                stats.append(st)
                loop.append(res['images'] / (dt - st))
        off, on, on_loop = np.mean(rates[False]), np.mean(rates[True]), np.mean(loop)
        print('val %-40s images/s without FID %7.2f  with %7.2f  ratio %.3f  | with FID minus its host statistics (%.2f s per pass) '
              '%7.2f  ratio %.3f  (runs %s / %s, %d images)' % (
                  name, off, on, on / off, np.mean(stats), on_loop, on_loop / off, ['%.2f' % r for r in rates[False]],
                  ['%.2f' % r for r in rates[True]], a.images))


if __name__ == '__main__':
    main()
