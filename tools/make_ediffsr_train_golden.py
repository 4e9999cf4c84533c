"""tests/golden/ediffsr_train_step.npz from the reference's OWN modules (EDiffSR/codes: ConditionalNAFNet, IRSDE, MatchingLoss,
models/optimizer.Lion) and torch.optim.Adam / AdamW, fp32 on the CPU: one DenoisingModel.optimize_parameters step, restated from
its lines because denoising_model.py itself imports ema_pytorch and torchvision.  It pins tests/ediffsr_train_restatement.py and
fastdiffsr_amd/ediffsr/sde.py; it runs only where a checkout of the reference exists (REFERENCE_ROOT, as make_ediffsr_golden.py).

    REFERENCE_ROOT=/path/to/FastDiffSR python tools/make_ediffsr_train_golden.py

Test setting, synth_nafnet(0), B = 2, 36x44.  Contents: gt / mu; generate_random_states' timesteps and states under
torch.manual_seed(SEED); for t = [1, 100] with a stored noise: the state, xt_1_expection, xt_1_optimum, the l1 and l2 losses;
for all 208 tensors the l1 gradient's max-abs and fp64 sum; the full l1 gradient of the FULL tensors and those tensors after one
Adam, AdamW and Lion step (lr 1e-3, betas (0.9, 0.99), weight decay 0.01)."""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_ediffsr_golden as G   # noqa: E402

OUT = os.path.join(G.ROOT, 'tests', 'golden', 'ediffsr_train_step.npz')
SEED = 20
LR, BETAS, WD = 1e-3, (0.9, 0.99), 0.01
FULL = ['encoders.0.0.conv1.weight', 'encoders.0.0.conv1.bias', 'encoders.0.0.conv2.weight', 'encoders.0.0.conv2.bias',
        'encoders.0.0.conv3.weight', 'encoders.0.0.conv4.weight', 'encoders.0.0.conv5.weight', 'encoders.0.0.sca.1.weight',
        'encoders.0.0.sca.1.bias', 'encoders.0.0.mlp.1.weight', 'encoders.0.0.mlp.1.bias', 'encoders.0.0.norm1.g', 'encoders.0.0.norm2.g',
        'encoders.0.0.beta', 'encoders.0.0.gamma', 'middle_blks.0.norm1.g', 'downs.0.weight', 'downs.0.bias', 'ups.3.0.weight', 'intro.weight',
        'ending.weight', 'ending.bias', 'enhance.rcab.0.weight', 'enhance.rcab.3.attention.1.weight', 'enhance.rcab.3.attention.3.weight',
        'enhance.rcab.3.attention.3.bias', 'time_mlp.1.weight', 'time_mlp.3.weight', 'time_mlp.3.bias']


def main():
    from fastdiffsr_amd.synth import synth_nafnet
    arch, sde_utils = G.import_reference()
    loss_mod = importlib.import_module('ediffsr_ref_modules.loss')
    spec = importlib.util.spec_from_file_location('ediffsr_ref_optimizer', os.path.join(G.CODES, 'config', 'sisr', 'models', 'optimizer.py'))
    opt_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(opt_mod)
    torch.set_num_threads(8)
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **G.TEST_SETTING).items()}

    def fresh():
        net = arch.ConditionalNAFNet(img_channel=3, upscale=1, **G.TEST_SETTING)
        net.load_state_dict(sd, strict=True)
        return net.train()

    g = torch.Generator().manual_seed(SEED)
    gt = torch.rand(2, 3, 36, 44, generator=g)
    mu = (gt + 0.1 * torch.randn(2, 3, 36, 44, generator=g)).clamp(0, 1)
    noise = torch.randn(2, 3, 36, 44, generator=g)
    sde = sde_utils.IRSDE(max_sigma=50, T=100, schedule='cosine', eps=0.005, device='cpu')
    out = dict(gt=gt.numpy(), mu=mu.numpy(), noise=noise.numpy(), seed=np.array(SEED), full=np.array(FULL),
               hyper=np.array([LR, BETAS[0], BETAS[1], 1e-8, WD]))
    torch.manual_seed(SEED)
    ts, states = sde.generate_random_states(x0=gt, mu=mu)
    out.update(gen_timesteps=ts.numpy(), gen_states=states.numpy())

    t = torch.tensor([1, 100]).reshape(2, 1, 1, 1)
    sde.set_mu(mu)
    state = (noise * sde.sigma_bar(t) + sde.mu_bar(gt, t)).to(torch.float32)
    out.update(timesteps=t.numpy(), state=state.numpy())

    def step(net, loss_type):      # denoising_model.py:127-141
        sde.set_model(net)
        sde.set_mu(mu)
        eps = sde.noise_fn(state, t.squeeze())
        score = sde.get_score_from_noise(eps, t)
        expect = sde.reverse_sde_step_mean(state, score, t)
        optimum = sde.reverse_optimum_step(state, gt, t)
        return 1.0 * loss_mod.MatchingLoss(loss_type, False)(expect, optimum), expect, optimum

    net = fresh()
    l2, _, _ = step(net, 'l2')
    l1, expect, optimum = step(net, 'l1')
    l1.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for k, p in net.named_parameters()}
    assert list(grads) == list(sd) and len(grads) == 208
    out.update(loss_l1=l1.detach().numpy(), loss_l2=l2.detach().numpy(), expect=expect.detach().numpy(), optimum=optimum.detach().numpy(),
               keys=np.array(list(grads)), grad_maxabs=np.array([float(v.abs().max()) for v in grads.values()]),
               grad_sum=np.array([float(v.double().sum()) for v in grads.values()]))
    for k in FULL:
        out['grad_' + k] = grads[k].numpy()
    for kind, make in (('Adam', lambda p: torch.optim.Adam(p, lr=LR, betas=BETAS, weight_decay=WD)),
                       ('AdamW', lambda p: torch.optim.AdamW(p, lr=LR, betas=BETAS, weight_decay=WD)),
                       ('Lion', lambda p: opt_mod.Lion(p, lr=LR, betas=BETAS, weight_decay=WD))):
        net = fresh()
        o = make([p for p in net.parameters() if p.requires_grad])
        o.zero_grad()
        step(net, 'l1')[0].backward()
        o.step()
        after = dict(net.named_parameters())
        for k in FULL:
            out['%s_%s' % (kind, k)] = after[k].detach().numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
