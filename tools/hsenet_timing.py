"""HSENet forward times on one GPU -> profiles/hsenet_timing.txt.

    python tools/hsenet_timing.py [--baseline] [--append] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/hsenet_timing.py --profile-run [--batch B]     # the per-kernel split

The configuration the reference tests with (n_feats 64, ten BasicModules, x4), synthetic weights, exact fp32: ms per image at
64x64 -> 256x256, B = 1 and 16, eager and graph replay; the median of --repeats timed calls after one warm-up call, hipEvents
around the call.  --baseline runs the same network through stock PyTorch on the same GPU, fp32: the plain-torch restatement of
tests/hsenet_restatement.py (a 4096 x 4096 score matrix per image and block), a baseline only, never the product path.
--append adds to the file instead of replacing it.  --profile-run makes five eager forwards at 64x64, B = --batch (16) and
writes nothing: the run to put under rocprofv3."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'profiles', 'hsenet_timing.txt')
SETTING = dict(n_feats=64, scale=4, n_basic_modules=10)


def attention_flops(h, w, nf=64, modules=10):
    """The useful 2 N_q N_k d of q k^T and of p v, summed over the three non-local blocks of every module (the kernel itself
    forms q k^T twice)."""
    n, nd = h * w, (h // 2) * (w // 2)
    return modules * 4 * (nf // 2) * (2 * n * n + nd * nd)


def conv3_flops(h, w, nf=64, modules=10):
    """The 13 n_feats -> n_feats 3x3 convolutions of a module: nine at the base scale, four at half scale."""
    n, nd = h * w, (h // 2) * (w // 2)
    return modules * 2 * 9 * nf * nf * (9 * n + 4 * nd)


def forward_flops(h, w, nf=64, scale=4, modules=10):
    """2 M K N over every convolution of one forward plus the attention products; scale a power of two."""
    n, nd = h * w, (h // 2) * (w // 2)
    one = modules * 2 * nf * (nf // 2) * (4 * (2 * n + nd)) + modules * 2 * nf * nf * (n + nd)      # theta, phi, g, W; AB.1
    tail, k = 2 * n * 27 * nf, 1
    while k < scale:
        tail += 2 * n * k * k * 9 * nf * 4 * nf
        k *= 2
    tail += 2 * n * scale * scale * 9 * nf * 3
    return conv3_flops(h, w, nf, modules) + one + tail + attention_flops(h, w, nf, modules)


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
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--batch', type=int, default=16, help='of --profile-run')
    a = ap.parse_args()
    from fastdiffsr_amd.hsenet import HSENet, load_synthetic
    from fastdiffsr_amd.synth import synth_hsenet
    dev = torch.device('cuda')
    net = load_synthetic(HSENet(**SETTING), 0).to(dev).eval()
    if a.profile_run:
        x = torch.rand(a.batch, 3, 64, 64, device=dev)
        for _ in range(5):
            net(x)
        torch.cuda.synchronize()
        return
    fl = forward_flops(64, 64)
    lines = ['HSENet timing: %s, n_feats 64, 10 BasicModules, x4, exact fp32, synthetic weights' % torch.cuda.get_device_name(0),
             'command: python tools/hsenet_timing.py' + ' --baseline' * a.baseline + ' --repeats %d' % a.repeats
             + ' --batches %s' % ' '.join(map(str, a.batches)),
             'ms per image, median of %d calls after a warm-up call (min, max); TF = the forward\'s %.1f GFLOP per 64x64 image '
             '(%.1f of them the attention products, %.1f the 130 3x3 convolutions of the body) over the time'
             % (a.repeats, fl / 1e9, attention_flops(64, 64) / 1e9, conv3_flops(64, 64) / 1e9)]
    if a.baseline:
        import hsenet_restatement as R
        wdev = {k: torch.from_numpy(v).to(dev) for k, v in synth_hsenet(net.cfg, 0).items()}
    for b in a.batches:
        x = torch.rand(b, 3, 64, 64, generator=torch.Generator().manual_seed(b)).to(dev)
        row = {}
        for mode in ('eager', 'graph'):
            med, lo, hi = timed(lambda: net(x, graph=mode == 'graph'), a.repeats)
            row[mode] = med / b
            lines.append('engine      64x64   B=%-2d %-6s %9.3f ms/image (min %.3f max %.3f)  %5.1f TF'
                         % (b, mode, med / b, lo / b, hi / b, fl * b / med / 1e9))
        if a.baseline:
            with torch.no_grad():
                med, lo, hi = timed(lambda: R.hsenet_forward(wdev, net.cfg, x, torch.float32)['out'], a.repeats)
            lines.append('baseline    64x64   B=%-2d eager  %9.3f ms/image (min %.3f max %.3f)  stock PyTorch fp32; engine eager is %.2f x, '
                         'graph %.2f x as fast' % (b, med / b, lo / b, hi / b, med / b / row['eager'], med / b / row['graph']))
        net._static.clear()      # the graph path's kept input / output / workspace of this shape
        net._ws.clear()
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
