"""LPIPS cost on the GPU: ms per fdsr_lpips_u8 call (256 x 256, two test images per truth, B = 16 and 64) and the val loop's
rate with and without LPIPS on the same box (--batch 16 f16x3; --batch 64 --precision f16 --rng engine), A B A B.

    python tools/lpips_timing.py [--images 128] > profiles/lpips_timing.txt

Synthetic backbone (synth.synth_alexnet_features) and heads; LPIPS' cost does not depend on the weight values."""
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


def kernel_ms(lp, b, reps=20):
    g = torch.Generator(device='cuda').manual_seed(b)
    t, a, c = (torch.randint(0, 256, (b, 256, 256, 3), dtype=torch.uint8, device='cuda', generator=g) for _ in range(3))
    for _ in range(3):
        lp.lpips_u8(t, a, c)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        lp.lpips_u8(t, a, c)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=128)
    a = ap.parse_args()
    from fastdiffsr_amd import val
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.metrics import LPIPS, LPIPS_CHANNELS
    from fastdiffsr_amd.synth import synth_alexnet_features
    from test_gpu_val import _config_plain
    from test_val_host import make_dataset
    rng = np.random.default_rng(0)
    lin = {'lin%d.model.1.weight' % k: np.abs(rng.normal(0, 0.1, (1, c, 1, 1))).astype(np.float32) for k, c in enumerate(LPIPS_CHANNELS)}
    lp = LPIPS(synth_alexnet_features(0), lin)
    print('# gpu: %s' % torch.cuda.get_device_name())
    flop = 0
    for b in (16, 64):
        ms = kernel_ms(lp, b)
        gflop = 3 * b * 1.7367                       # 1.74 GFLOP per AlexNet forward at 256^2 (five convs), three per image
        print('fdsr_lpips_u8  B=%-3d 256x256 two tests: %7.2f ms per call  (%.1f TF/s on the convolutions)' % (b, ms, gflop / ms))
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
        for use in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = val.run(opt, diffusion=diffusion, save_images=False, log=lambda m: None, lpips=lp if use else None, **kw)
            rates[use].append(res['images'] / (time.perf_counter() - t0))
        off, on = np.mean(rates[False]), np.mean(rates[True])
        print('val %-40s images/s without LPIPS %7.2f  with %7.2f  ratio %.3f  (runs %s / %s, %d images)' % (
            name, off, on, on / off, ['%.2f' % r for r in rates[False]], ['%.2f' % r for r in rates[True]], a.images))


if __name__ == '__main__':
    main()
