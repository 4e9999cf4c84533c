"""The siblings at their own schedule lengths (SR3 / GDP T = 1000, TESR T = 2000) through fdsr_sample_stepwise: bitwise equal to
fdsr_sample where both run, strided trajectories, parity with the oracle at the real T, graph replay equal to eager, the engine's
noise through the facade, and bounded memory."""
import math

import numpy as np
import pytest
import torch

from fastdiffsr_amd.arch import UNetConfig
from fastdiffsr_amd.schedule import schedule_buffers, sampling_scalars
from fastdiffsr_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

SMALL = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2, 4), attn_res=(8,), res_blocks=1,
             dropout=0.2, image_size=32)
CFGS = {
    'fastdiffsr': dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 4, 4), attn_res=(),
                       res_blocks=1, dropout=0.0, image_size=32),
    'ddpm': dict(SMALL, variant='ddpm'),
    'tesr': dict(SMALL, variant='tesr'),
    'gdp': dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 2), attn_res=(2, 4), res_blocks=1,
                dropout=0.1, image_size=32, variant='gdp'),
}
LONG = {   # the reference's own lengths (sr_ddpm_* / sr_gdp_*: 1000, sr_tesr_*: 2000)
    'ddpm': dict(schedule='linear', n_timestep=1000, linear_start=1e-4, linear_end=2e-2),
    'gdp': dict(schedule='linear', n_timestep=1000, linear_start=1e-4, linear_end=2e-2),
    'tesr': dict(schedule='linear', n_timestep=2000, linear_start=1e-6, linear_end=1e-2),
}


def _engine(name, T, seed=5):
    from fastdiffsr_amd.engine import Engine
    cfg = UNetConfig(**CFGS[name])
    eng = Engine(cfg)
    eng.load_state_dict(synth_state_dict(cfg, seed))
    bufs, sp = schedule_buffers(dict(schedule='linear', n_timestep=T, linear_start=1e-4, linear_end=2e-2))
    eng.set_schedule(sampling_scalars(bufs, sp))
    return eng


def _planes(eng):
    return eng.T + (1 if eng.cfg.variant in ('ddpm', 'gdp') else 0)


@pytest.mark.parametrize('name,T,chunks', [('fastdiffsr', 20, (5, 7)), ('ddpm', 12, (4, 5)), ('tesr', 12, (4, 5)), ('gdp', 12, (4, 5))])
def test_stepwise_equals_fdsr_sample_bitwise(name, T, chunks):
    """out and the full trajectory (traj_every = 1) of fdsr_sample_stepwise equal fdsr_sample's, bitwise, in every precision, with
    explicit noise and with the engine's own draws, eager and graph (a chunk that divides T and one that does not); a strided
    trajectory is the matching rows of the full one."""
    eng = _engine(name, T)
    B, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(11)
    cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    noise = torch.randn((_planes(eng), B, 3, H, W), generator=g).cuda()
    for prec in ('f32', 'f16x3', 'bf16', 'f16'):
        eng.set_precision(prec)
        for nz in (noise, None):
            eng.set_seed(3)
            ref_out, ref_traj = eng.sample(cond, nz, want_traj=True)
            runs = [dict(graph=False, chunk=0)] + [dict(graph=True, chunk=c) for c in chunks]
            for kw in runs:
                eng.set_seed(3)
                out, traj = eng.sample(cond, nz, want_traj=True, stepwise=True, **kw)
                tag = (name, prec, nz is None, kw)
                assert torch.equal(out, ref_out), tag
                assert torch.equal(traj, ref_traj), tag
            for every in (3, 7):
                eng.set_seed(3)
                out, frames = eng.sample(cond, nz, want_traj=True, stepwise=True, graph=True, traj_every=every, chunk=chunks[1])
                ks = [k for k, t in enumerate(reversed(range(T))) if t % every == 0]
                assert frames.shape[0] == len(ks) == eng.traj_slots(every)
                assert torch.equal(frames, ref_traj[ks]), (name, prec, every)
                assert torch.equal(out, ref_out)
    # no trajectory at all, and the refusal of a step-dependent precision probe
    eng.set_precision('f32')
    out = eng.sample(cond, noise, stepwise=True, graph=True)
    assert torch.equal(out, eng.sample(cond, noise))
    from fastdiffsr_amd import _lib
    _lib.debug_option('bf16_f16x3_steps', 2)
    try:
        with pytest.raises(_lib.FdsrError):
            eng.sample(cond, noise, stepwise=True)
    finally:
        _lib.debug_option('bf16_f16x3_steps', 0)


_FACADES = {}


def _facade(variant):
    """The facade of a sibling at its own T, 16x16 synth weights (cached for the module)."""
    if variant not in _FACADES:
        _FACADES[variant] = _new_facade(variant, LONG[variant])
    return _FACADES[variant]


def _new_facade(variant, sched):
    from fastdiffsr_amd import networks
    dev = torch.device('cuda')
    kw = CFGS[variant]
    if variant == 'gdp':
        from fastdiffsr_amd.gdp import diffusion, unet
        net = unet.UNet(image_size=16, in_channel=6, model_channels=64, out_channel=3, res_blocks=1, attention_resolutions=(2, 4),
                        dropout=0.1, channel_mults=(1, 2, 2), inner_channel=64, norm_groups=32, attn_res=(16,))
        netG = diffusion.GaussianDiffusion(net, image_size=16, channels=3, loss_type='l1', conditional=True, schedule_opt=sched).to(dev)
    else:
        opt = {'phase': 'val', 'gpu_ids': [0], 'distributed': False, 'datasets': {'train': {'l_resolution': 16}},
               'model': {'which_model_G': variant, 'finetune_norm': False,
                         'unet': {'in_channel': 6, 'out_channel': 3, 'inner_channel': kw['inner_channel'], 'norm_groups': 32,
                                  'channel_multiplier': list(kw['channel_mults']), 'attn_res': list(kw['attn_res']),
                                  'res_blocks': kw['res_blocks'], 'dropout': kw['dropout']},
                         'beta_schedule': {'train': dict(sched), 'val': dict(sched)},
                         'diffusion': {'image_size': 16, 'channels': 3, 'conditional': True}}}
        netG = networks.define_G(opt).to(dev)
    netG.set_loss(dev)
    netG.set_new_noise_schedule(sched, dev)
    cfg = UNetConfig(**dict(kw, image_size=16))
    sd = synth_state_dict(cfg, 17)
    ck = {'denoise_fn.' + k: torch.from_numpy(v) for k, v in sd.items()}
    ck.update({k: v.cpu() for k, v in netG.state_dict().items() if not k.startswith('denoise_fn.')})
    netG.load_state_dict(ck, strict=True)
    netG.eval()
    assert netG.num_timesteps == sched['n_timestep']
    T = netG.num_timesteps
    g = torch.Generator().manual_seed(23)
    cond = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    noise = torch.randn((T + (0 if variant == 'tesr' else 1), 2, 3, 16, 16), generator=g)
    return netG, cfg, sd, cond, noise


_ORACLE = {}


def _oracle_frames(variant):
    """The oracle's p_sample_loop(return_trajectory=True) at the frames continous=True keeps: [x_in] + kept x_t."""
    if variant in _ORACLE:
        return _ORACLE[variant]
    from oracle import fdsr_oracle as O, gdp_oracle as G, sr3_oracle as S, tesr_oracle as TO
    from fastdiffsr_amd.long_schedule import kept_steps
    netG, cfg, sd, cond, noise = _facade(variant)
    mod = {'ddpm': S, 'tesr': TO, 'gdp': G}[variant]
    nthr = torch.get_num_threads()
    torch.set_num_threads(4)            # tiny tensors: more threads only add overhead
    try:
        _, traj = mod.p_sample_loop(O.to_torch_sd(sd), cfg, O.schedule_tables(LONG[variant]), cond, noise, return_trajectory=True)
    finally:
        torch.set_num_threads(nthr)
    T = netG.num_timesteps
    frames = torch.cat([cond] + [traj[T - 1 - t] for t in kept_steps(T)], dim=0)
    _ORACLE[variant] = frames
    return frames


@pytest.mark.parametrize('variant', ['ddpm', 'gdp', 'tesr'])
def test_parity_with_oracle_at_the_reference_T(variant):
    """Through the facade's p_sample_loop(continous=True) at T = 1000 (SR3, GDP) / 2000 (TESR): f32 and f16x3 within 1e-3 of the
    oracle on every kept frame; f16 / bf16 judged on the final image's PSNR (the bar the T = 12 bf16 tests use)."""
    from oracle import fdsr_oracle as O
    netG, cfg, sd, cond, noise = _facade(variant)
    ref = _oracle_frames(variant)
    for prec in ('f32', 'f16x3', 'bf16', 'f16'):
        netG.precision = prec
        got = netG.p_sample_loop(cond.cuda(), continous=True, noise=noise.cuda()).cpu()
        assert got.shape == ref.shape
        d = (got - ref).abs().max().item()
        final = min(O.psnr_u8(O.tensor2img_u8(got[i]), O.tensor2img_u8(ref[i])) for i in (-2, -1))
        print(f'long schedule {variant} T={netG.num_timesteps} [{prec}]: max|d| over kept frames {d:.2e}, final-image PSNR {final:.1f} dB')
        if prec in ('f32', 'f16x3'):
            assert d <= 1e-3, (variant, prec, d)
        else:
            assert final >= 40.0, (variant, prec, final)
    netG.precision = 'f16x3'


@pytest.mark.parametrize('variant', ['tesr', 'ddpm'])
def test_graph_equals_eager_at_the_reference_T(variant):
    """The chunked graph replay (T / chunk replays of one captured chunk) equals the eager stepwise loop bitwise; a second graph call
    on the same buffers replays the cached graphs and equals the first."""
    netG, cfg, sd, cond, noise = _facade(variant)
    netG.precision = 'f16x3'
    x, nz = cond.cuda(), noise.cuda()
    netG.graph = 'off'
    eager = netG.p_sample_loop(x, continous=True, noise=nz)
    netG.graph = 'on'
    g1 = netG.p_sample_loop(x, continous=True, noise=nz)
    g2 = netG.p_sample_loop(x, continous=True, noise=nz)
    netG.graph = 'auto'
    assert torch.equal(g1, eager)
    assert torch.equal(g2, g1)


def test_engine_rng_through_the_sr3_facade():
    """rng = 'engine' (SR3, T = 1000): the result equals a call given, as explicit noise, the T+1 planes fdsr_randn returns under that
    call's counter; two calls after the same set_seed repeat bitwise."""
    netG, cfg, sd, cond, noise = _facade('ddpm')
    netG.precision = 'f16x3'
    eng = netG.denoise_fn.engine
    x = cond.cuda()
    netG.rng = 'engine'
    try:
        eng.set_seed(1234)
        a = netG.p_sample_loop(x, continous=True)
        planes = torch.stack([eng.randn(2, 16, 16, k) for k in range(netG.num_timesteps + 1)])
        b = netG.p_sample_loop(x, continous=True, noise=planes)
        eng.set_seed(1234)
        c = netG.p_sample_loop(x, continous=True)
    finally:
        netG.rng = 'torch'
    assert torch.equal(a, b)
    assert torch.equal(a, c)


def test_memory_is_bounded_at_256():
    """SR3's small config at 256^2, B = 1, T = 1000, rng = 'engine', continous=True: the call's peak allocation stays below one
    [T,1,3,256,256] tensor (the pre-stepwise path pre-drew T+1 noise planes and kept T trajectory frames: about twice that)."""
    from fastdiffsr_amd import networks
    from fastdiffsr_amd.long_schedule import kept_steps
    sched = LONG['ddpm']
    kw = CFGS['ddpm']
    opt = {'phase': 'val', 'gpu_ids': [0], 'distributed': False, 'datasets': {'train': {'l_resolution': 64}},
           'model': {'which_model_G': 'ddpm', 'finetune_norm': False,
                     'unet': {'in_channel': 6, 'out_channel': 3, 'inner_channel': kw['inner_channel'], 'norm_groups': 32,
                              'channel_multiplier': list(kw['channel_mults']), 'attn_res': list(kw['attn_res']),
                              'res_blocks': kw['res_blocks'], 'dropout': kw['dropout']},
                     'beta_schedule': {'train': dict(sched), 'val': dict(sched)},
                     'diffusion': {'image_size': 256, 'channels': 3, 'conditional': True}}}
    dev = torch.device('cuda')
    netG = networks.define_G(opt).to(dev)
    netG.set_new_noise_schedule(sched, dev)
    sd = synth_state_dict(UNetConfig(**dict(kw, image_size=256)), 17)
    ck = {'denoise_fn.' + k: torch.from_numpy(v) for k, v in sd.items()}
    ck.update({k: v.cpu() for k, v in netG.state_dict().items() if not k.startswith('denoise_fn.')})
    netG.load_state_dict(ck, strict=True)
    netG.eval()
    netG.rng = 'engine'
    netG.precision = 'bf16'
    x = torch.rand(1, 3, 256, 256, device=dev) * 2 - 1
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    frames = netG.p_sample_loop(x, continous=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    one = 1000 * 3 * 256 * 256 * 4
    print(f'long schedule memory: SR3 256^2 B=1 T=1000 continous: peak rise {rise / 2**20:.0f} MiB (one [T,1,3,256,256]: {one / 2**20:.0f} MiB)')
    assert frames.shape == (1 + len(kept_steps(1000)), 3, 256, 256)
    assert torch.isfinite(frames).all()
    assert rise < one


@pytest.mark.parametrize('n_timestep', [12, 60])
@pytest.mark.parametrize('variant', ['ddpm', 'tesr', 'gdp'])
def test_validation_after_a_training_step(variant, n_timestep):
    """train.py's flow on both sampling paths (T = 12: fdsr_sample, T = 60: stepwise): an optimisation step (dropout live: it leaves
    the engine in train mode), netG.eval(), then two val samples with graph = 'auto' -- at T > 50 the second replays the chunked
    graph.  Both run, and they equal each other and an eager call bitwise.  The engine's dropout is off (as after the reference's
    netG.eval()): the same dropout seed would give all three calls the same masks, so a fourth call after switching the engine's
    train mode off by hand is what shows it -- it equals the first."""
    sched = dict(LONG[variant], n_timestep=n_timestep)
    netG, cfg, sd, cond, noise = _new_facade(variant, sched)
    assert cfg.dropout > 0
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(31)
    hr = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev)
    sr = (torch.rand(2, 3, 16, 16, generator=g) * 2 - 1).to(dev)
    netG.train()
    netG.optimize_step({'HR': hr, 'SR': sr}, lr=1e-5)
    netG.eval()
    netG.graph = 'auto'
    x, nz = cond.to(dev), noise.to(dev)
    a = netG.p_sample_loop(x, continous=True, noise=nz)
    b = netG.p_sample_loop(x, continous=True, noise=nz)
    netG.graph = 'off'
    c = netG.p_sample_loop(x, continous=True, noise=nz)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c)
    netG.denoise_fn.engine.set_training(False)
    d = netG.p_sample_loop(x, continous=True, noise=nz)
    assert torch.equal(a, d)
