"""EDiffSR sampling times on one GPU -> profiles/ediffsr_timing.txt (or --out).

    python tools/ediffsr_timing.py [--out FILE] [--size 256] [--steps 100] [--baseline] [--precision f32|f16x3|f16]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ediffsr_timing.py --forward-only     # per-kernel split of forwards

Shipped setting (width 64, enc [14,1,1,1]), synthetic weights, T = --steps, B = 1 and B = 16, eager and graph: ms per image,
median of --repeats timed runs after one warm-up run (hipEvents around the whole sampler call).  Forward: median of 20.
The achieved fraction of the exact-fp32 MFMA peak (157.3 TF) counts the 1x1-convolution FLOPs of a forward only, over the time
of the WHOLE forward, so it is a lower bound for the GEMM family.  --baseline adds the plain-torch restatement of the same
forward (tests/ediffsr_restatement.py) through stock PyTorch on the same GPU, fp32: a baseline only, never the product path."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
PEAK_TF = 157.3


def conv1x1_flops(setting, h, w):
    """2 * M * K * N over every 1x1 convolution of one forward (conv1, conv3, conv4, conv5, ups) at H x W"""
    total, c, m = 0, setting['width'], h * w
    per_block = lambda c: 2 * (c * 2 * c + c * c + c * 2 * c + c * c)
    for n in setting['enc_blk_nums']:
        total += n * per_block(c) * m
        c, m = 2 * c, m // 4
    total += setting['middle_blk_num'] * per_block(c) * m
    for n in setting['dec_blk_nums']:
        total += 2 * c * 2 * c * m
        c, m = c // 2, m * 4
        total += n * per_block(c) * m
    return total


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
    ap.add_argument('--out', default=None)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--baseline', action='store_true')
    ap.add_argument('--forward-only', action='store_true')
    ap.add_argument('--precision', choices=('f32', 'f16x3', 'f16'), default='f32')
    a = ap.parse_args()
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet, IRSDE
    from fastdiffsr_amd.synth import synth_nafnet
    dev = torch.device('cuda')
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **SETTING).items()}
    net = ConditionalNAFNet(**SETTING)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    net.set_precision(a.precision)
    sde = IRSDE(max_sigma=50, T=a.steps, schedule='cosine', eps=0.005, device=dev, rng='engine')
    sde.set_model(net)
    lines = ['EDiffSR timing: %s, width 64 enc [14,1,1,1], %dx%d, T = %d, %s, engine-drawn noise'
             % (torch.cuda.get_device_name(0), a.size, a.size, a.steps,
                {'f32': 'fp32 (exact-fp32 MFMA)', 'f16x3': 'f16x3 (three f16 MFMAs per product, fp32 accumulate)',
                 'f16': 'f16 (f16 activations in memory, one f16 MFMA per product, fp32 accumulate)'}[a.precision])]
    fl = conv1x1_flops(SETTING, a.size, a.size)
    for b in a.batches:
        g = torch.Generator().manual_seed(b)
        cond = torch.rand(b, 3, a.size, a.size, generator=g).to(dev)
        state = cond + 0.2 * torch.randn(b, 3, a.size, a.size, generator=g).to(dev)
        med, lo, hi = timed(lambda: net(state, cond, 50), 20)
        line = 'forward   B=%-2d         %8.3f ms/image (median of 20; min %.3f max %.3f per call / B)' % (b, med / b, lo / b, hi / b)
        if a.precision == 'f32':   # a share of the exact-fp32 MFMA peak: no such figure for three f16 MFMAs per product
            line += '  1x1 GEMMs >= %.1f TF = %.3f of %.1f' % (fl * b / med / 1e9, fl * b / med / 1e9 / PEAK_TF, PEAK_TF)
        lines.append(line)
        if a.forward_only:
            continue
        sde.set_mu(cond)
        for graph in (False, True):
            sde.graph = graph
            med, lo, hi = timed(lambda: sde.reverse_sde(state), a.repeats)
            lines.append('sample    B=%-2d %-6s  %8.1f ms/image (median of %d; min %.1f max %.1f)' % (b, 'graph' if graph else 'eager', med / b, a.repeats, lo / b, hi / b))
        if a.baseline:
            import ediffsr_restatement as R
            dsd = {k: v.to(dev) for k, v in sd.items()}
            with torch.no_grad():
                med, lo, hi = timed(lambda: R.forward(dsd, state, cond, torch.full((1,), 50.0, device=dev)), 10)
            lines.append('baseline  B=%-2d forward  %8.3f ms/image (stock PyTorch, fp32, the restatement; x %d steps = %.1f ms/image)'
                         % (b, med / b, a.steps, med / b * a.steps))
    if a.precision != 'f32':
        net.check_saturation()   # raises if any timed call left the f16 range
        lines.append('range guard: clear')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
