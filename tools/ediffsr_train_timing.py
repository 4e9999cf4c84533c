"""EDiffSR training-step times on one GPU -> profiles/ediffsr_train_timing.txt (or --out).

    python tools/ediffsr_train_timing.py [--out FILE] [--append] [--size 256] [--repeats 5] [--baseline] [--bridge] [--precision f32|f16]

Shipped setting (width 64, enc [14,1,1,1]), synthetic weights, l1 loss, AdamW (lr 4e-5, betas 0.9 / 0.99), B = 2 (the
reference's batch_size) and B = 16: one step = fdsr_nafnet_train_grads + fdsr_nafnet_optim_step with the parameter copy-back, ms
per step and images/s as the median of --repeats timed steps after two warm-up steps (hipEvents around the step), and the step's
workspace bytes.  --baseline adds the same step of tests/ediffsr_train_restatement.py through stock PyTorch autograd and
torch.optim.AdamW on the same GPU, fp32: a baseline only, never the product path.  --bridge adds the step through torch autograd
on the engine (model.requires_grad_(True): fdsr_nafnet_forward_train, IRSDE's loss terms in torch, fdsr_nafnet_backward,
torch.optim.AdamW, the weights back through fdsr_nafnet_set_weights_flat), and the same without the optimizer.  --precision f16 times
the engine (and the bridge) with f16 activation storage for training (set_train_precision('f16'): fp32 gradients); the baseline
stays fp32.  --append adds to the file instead of replacing it.  The file records what was seen."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ediffsr_train_timing.txt'))
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--baseline', action='store_true')
    ap.add_argument('--bridge', action='store_true')
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--precision', choices=('f32', 'f16'), default='f32')
    a = ap.parse_args()
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet, IRSDE
    from fastdiffsr_amd.synth import synth_nafnet
    import ediffsr_train_restatement as TR
    dev = torch.device('cuda', torch.cuda.current_device())
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **SETTING).items()}
    sde = IRSDE(max_sigma=50, T=100, schedule='cosine', eps=0.005, device='cpu')
    lines = ['EDiffSR training timing: %s, width 64 enc [14,1,1,1], %dx%d, %s, l1, AdamW' % (
        torch.cuda.get_device_name(dev), a.size, a.size,
        'fp32 (exact-fp32 MFMA)' if a.precision == 'f32' else 'f16 activation storage for training (f16 MFMA forward, fp32 gradients)'), 'command: python tools/ediffsr_train_timing.py ' + ' '.join(sys.argv[1:])]
    for b in (2, 16):
        g = torch.Generator().manual_seed(b)
        gt = torch.rand(b, 3, a.size, a.size, generator=g)
        mu = (gt + 0.1 * torch.randn(b, 3, a.size, a.size, generator=g)).clamp(0, 1)
        ts = torch.randint(1, 101, (b, 1, 1, 1), generator=g)
        sde.set_mu(mu)
        state = (torch.randn(b, 3, a.size, a.size, generator=g) * sde.sigma_bar(ts) + sde.mu_bar(gt, ts)).float()
        x, c, y = state.to(dev), mu.to(dev), gt.to(dev)
        m = ConditionalNAFNet(**SETTING)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        m.set_train_precision(a.precision)
        sde.set_model(m)

        def step():
            m.train_grads(x, c, y, ts)
            m.optim_step('AdamW', 4e-5, (0.9, 0.99), 1e-8, 0.0)
        med, lo, hi = timed(step, a.repeats)
        lines.append('step      B=%-2d %-10s%9.2f ms/step  %7.2f images/s  (median of %d; min %.2f max %.2f)  workspace %.2f GiB' % (
            b, 'engine' if a.precision == 'f32' else 'engine-f16', med, b * 1000 / med, a.repeats, lo, hi,
            m.train_workspace_bytes(b, a.size, a.size) / 2 ** 30))
        print(lines[-1], flush=True)
        del m
        torch.cuda.empty_cache()
        if a.bridge:
            m = ConditionalNAFNet(**SETTING)
            m.load_state_dict(sd, strict=True)
            m = m.to(dev).train().requires_grad_(True)
            m.set_train_precision(a.precision)
            dsde = IRSDE(max_sigma=50, T=100, schedule='cosine', eps=0.005, device=dev)
            dsde.set_model(m)
            dsde.set_mu(c)
            opt = torch.optim.AdamW(m.parameters(), lr=4e-5, betas=(0.9, 0.99), weight_decay=0.0)
            tsd = ts.to(dev)

            def fwd_bwd():
                opt.zero_grad(set_to_none=True)
                score = dsde.get_score_from_noise(dsde.noise_fn(x, tsd.squeeze()), tsd)
                diff = dsde.reverse_sde_step_mean(x, score, tsd) - dsde.reverse_optimum_step(x, y, tsd)
                diff.abs().flatten(1).mean(dim=1).mean().backward()

            def bridged():
                fwd_bwd()
                opt.step()
            for name, fn in (('fwd+bwd', fwd_bwd), ('step', bridged)):
                med, lo, hi = timed(fn, a.repeats)
                lines.append('bridge    B=%-2d %-9s %9.2f ms/step  %7.2f images/s  (torch autograd on the engine, loss in torch%s; median of %d; min %.2f max %.2f)' % (
                    b, name, med, b * 1000 / med, ', torch.optim.AdamW' if name == 'step' else ', no optimizer', a.repeats, lo, hi))
                print(lines[-1], flush=True)
            del m, opt, dsde
            torch.cuda.empty_cache()
        if a.baseline:
            w = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
            tb = tuple(t.to(dev) for t in TR.cast_tables(sde, torch.float32))
            opt = torch.optim.AdamW(list(w.values()), lr=4e-5, betas=(0.9, 0.99), weight_decay=0.0)
            tsd = ts.to(dev)

            def base():
                opt.zero_grad(set_to_none=True)
                TR.loss(w, tb, x, c, y, tsd)[0].backward()
                opt.step()
            med, lo, hi = timed(base, a.repeats)
            lines.append('baseline  B=%-2d autograd  %9.2f ms/step  %7.2f images/s  (stock PyTorch, fp32, the restatement; median of %d; min %.2f max %.2f)' % (
                b, med, b * 1000 / med, a.repeats, lo, hi))
            print(lines[-1], flush=True)
            del w, opt
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
