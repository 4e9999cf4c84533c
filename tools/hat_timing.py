"""HAT forward times on one GPU -> profiles/hat_timing.txt.

    python tools/hat_timing.py [--baseline] [--append] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/hat_timing.py --profile-run      # the per-kernel split

The reference's configuration (embed_dim 180, 6 groups of 6 HABs and one OCAB, 6 heads, window 16, mlp_ratio 4, x4), synthetic
weights, exact fp32: ms per image at 64x64 -> 256x256, B = 1 and 16, eager and graph replay; the median of --repeats timed
calls after one warm-up call, hipEvents around the call.  --baseline runs the same network through stock PyTorch on the same
GPU, fp32: the plain-torch restatement of tests/hat_restatement.py, a baseline only, never the product path.  --append adds to
the file instead of replacing it.  --profile-run makes five eager forwards at 64x64, B = 16 and writes nothing: the run to
put under rocprofv3."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'profiles', 'hat_timing.txt')
SETTING = dict(img_size=64, upscale=4)      # every other argument at the reference's default


def forward_flops(h, w):
    """2 M K N over every Linear and convolution of one forward plus the attention products (256 keys in a HAB, 576 in an OCAB);
    h, w multiples of 16."""
    c, hid, m = 180, 720, h * w
    lin = 2 * m * (c * 3 * c + c * c + 2 * c * hid)
    hab = lin + 2 * 2 * m * 256 * c + 2 * m * 9 * 2 * c * (c // 3)
    ocab = lin + 2 * 2 * m * 576 * c
    tail = 2 * m * 9 * (3 * c + c * 64 + 64 * 256) + 2 * 4 * m * 9 * 64 * 256 + 2 * 16 * m * 9 * 64 * 3
    return 36 * hab + 6 * ocab + 7 * 2 * m * 9 * c * c + tail


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--baseline', action='store_true')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[64])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--profile-run', action='store_true')
    a = ap.parse_args()
    from fastdiffsr_amd.hat import HAT, load_synthetic
    from fastdiffsr_amd.synth import synth_hat
    dev = torch.device('cuda')
    net = load_synthetic(HAT(**SETTING), 0).to(dev).eval()
    if a.profile_run:
        x = torch.rand(16, 3, 64, 64, device=dev)
        for _ in range(5):
            net(x)
        torch.cuda.synchronize()
        return
    lines = ['HAT timing: %s, embed_dim 180, 6 x (6 HABs + 1 OCAB), 6 heads, window 16, mlp_ratio 4, x4, exact fp32, synthetic weights'
             % torch.cuda.get_device_name(0),
             'command: python tools/hat_timing.py' + ' --baseline' * a.baseline + ' --repeats %d' % a.repeats
             + ' --sizes %s --batches %s' % (' '.join(map(str, a.sizes)), ' '.join(map(str, a.batches))),
             'ms per image, median of %d calls after a warm-up call (min, max); TF = the forward\'s %.1f GFLOP per 64x64 image over the time'
             % (a.repeats, forward_flops(64, 64) / 1e9)]
    if a.baseline:
        import hat_restatement as R
        wdev = {k: torch.from_numpy(v).to(dev) for k, v in synth_hat(net.cfg, 0).items()}
    for size in a.sizes:
        fl = forward_flops(size, size)
        for b in a.batches:
            x = torch.rand(b, 3, size, size, generator=torch.Generator().manual_seed(b)).to(dev)
            row = {}
            for mode in ('eager', 'graph'):
                med, lo, hi = timed(lambda: net(x, graph=mode == 'graph'), a.repeats)
                row[mode] = med / b
                lines.append('engine    %4dx%-4d B=%-2d %-6s %9.3f ms/image (min %.3f max %.3f)  %5.1f TF'
                             % (size, size, b, mode, med / b, lo / b, hi / b, fl * b / med / 1e9))
            if a.baseline:
                with torch.no_grad():
                    med, lo, hi = timed(lambda: R.hat_forward(wdev, net.cfg, x, torch.float32)['out'], a.repeats)
                lines.append('baseline  %4dx%-4d B=%-2d eager  %9.3f ms/image (min %.3f max %.3f)  stock PyTorch fp32; engine eager is %.2f x, '
                             'graph %.2f x as fast' % (size, size, b, med / b, lo / b, hi / b, med / b / row['eager'], med / b / row['graph']))
            net._static.clear()      # the graph path's kept input / output / workspace of this shape
            net._ws.clear()
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
