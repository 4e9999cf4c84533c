"""TransENet forward times on one GPU -> profiles/transenet_timing.txt.

    python tools/transenet_timing.py [--baseline] [--append] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/transenet_timing.py --profile-run      # the per-kernel split

The reference's configuration (n_feats 64, four encoders of 8 layers, three decoders of 1, 6 heads of 32, dim 512, x4,
hr_patch_size 256), synthetic weights, exact fp32: ms per image at 64x64 -> 256x256, B = 1 and 16, eager and graph replay; the
median of --repeats timed calls after one warm-up call, hipEvents around the call.  --baseline runs the same network through
stock PyTorch on the same GPU, fp32: the plain-torch restatement of tests/transenet_restatement.py, a baseline only, never the
product path.  --append adds to the file instead of replacing it.  --profile-run makes five eager forwards at 64x64, B = 16 and
writes nothing: the run to put under rocprofv3."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'profiles', 'transenet_timing.txt')
SETTING = dict(scale=4, hr_patch_size=256)      # every other argument at the reference's default


def attention_flops(h, w, scale=4, en_depth=8, de_depth=1):
    """The useful 2 N_q N_k d of q k^T and of p v over the six heads, summed over every attention of one forward (the kernel
    itself forms q k^T twice)."""
    nl, nh = h * w // 64, h * w * scale * scale // 64
    return 4 * 192 * (3 * en_depth * nl * nl + (en_depth + 3 * de_depth) * nh * nh + 3 * de_depth * nh * nl)


def forward_flops(h, w, nf=64, scale=4, en_depth=8, de_depth=1):
    """2 M K N over every Linear and convolution of one forward plus the attention products; h, w multiples of 8, scale a power
    of two."""
    m, ch, d, inner = h * w, nf // 4, 512, 192
    nl, nh, mh = m // 64, m * scale * scale // 64, m * scale * scale
    conv = 2 * m * 27 * nf + 30 * 2 * m * 9 * nf * nf + 3 * 2 * m * nf * ch
    k = 1
    while k < scale:
        conv += 2 * m * k * k * 9 * nf * 4 * nf
        k *= 2
    conv += 2 * mh * nf * ch + 2 * mh * ch * nf + 2 * mh * 9 * nf * 3
    embed = 2 * (3 * nl + 2 * nh) * 64 * ch * d

    def self_ff(n):
        return 2 * n * d * 3 * inner + 2 * n * inner * d + 2 * 2 * n * d * d

    cross = 2 * nh * d * inner + 2 * 2 * nl * d * inner + 2 * nh * inner * d
    lin = en_depth * (3 * self_ff(nl) + self_ff(nh)) + 3 * de_depth * (self_ff(nh) + cross)
    return conv + embed + lin + attention_flops(h, w, scale, en_depth, de_depth)


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
    a = ap.parse_args()
    from fastdiffsr_amd.synth import synth_transenet
    from fastdiffsr_amd.transenet import TransENet, load_synthetic
    dev = torch.device('cuda')
    net = load_synthetic(TransENet(**SETTING), 0).to(dev).eval()
    if a.profile_run:
        x = torch.rand(16, 3, 64, 64, device=dev)
        for _ in range(5):
            net(x)
        torch.cuda.synchronize()
        return
    fl = forward_flops(64, 64)
    lines = ['TransENet timing: %s, n_feats 64, 4 encoders x 8 layers, 3 decoders x 1, dim 512, 6 heads of 32, x4, exact fp32, synthetic weights'
             % torch.cuda.get_device_name(0),
             'command: python tools/transenet_timing.py' + ' --baseline' * a.baseline + ' --repeats %d' % a.repeats
             + ' --batches %s' % ' '.join(map(str, a.batches)),
             'ms per image, median of %d calls after a warm-up call (min, max); TF = the forward\'s %.1f GFLOP per 64x64 image '
             '(%.1f of them the attention products) over the time' % (a.repeats, fl / 1e9, attention_flops(64, 64) / 1e9)]
    if a.baseline:
        import transenet_restatement as R
        wdev = {k: torch.from_numpy(v).to(dev) for k, v in synth_transenet(net.cfg, 0).items()}
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
                med, lo, hi = timed(lambda: R.transenet_forward(wdev, net.cfg, x, torch.float32)['out'], a.repeats)
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
