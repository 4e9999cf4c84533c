"""Sampling of the sibling denoisers (SR3 / TESR / GDP) at their own schedule lengths (T = 1000, TESR 2000) through
fdsr_sample_stepwise (include/fdsr.h): the per-step inputs live on the device, a graph replays a chunk of steps, and
`continous=True` keeps only the frames the reference keeps instead of all T of them."""
import torch

# schedules longer than this go through the stepwise entry point; up to it the facades call fdsr_sample as before
STEPWISE_ABOVE = 50


def frame_every(T):
    """The reference's `sample_inter = (1 | (T // 10))` (ddpm_modules/diffusion.py:200 and its siblings)."""
    return 1 | (int(T) // 10)


def kept_steps(T):
    """The t whose x_t `continous=True` returns, in loop order (t descending): `t % sample_inter == 0`."""
    every = frame_every(T)
    return [t for t in reversed(range(int(T))) if t % every == 0]


def use_stepwise(T):
    return int(T) > STEPWISE_ABOVE


def sample_stepwise(facade, eng, x, continous, draw_noise=None, noise=None):
    """One p_sample_loop of a sibling facade on the stepwise entry point.

    noise: an explicit [planes,B,3,H,W] tensor, or None with draw_noise(dst) filling dst in the reference's order (torch
    stream), or None with draw_noise None (the engine's own Philox draws, rng = 'engine').  facade.graph has the flagship's
    meaning ('auto' captures on the second call of a shape, 'on' on the first, 'off' never); graph replays need stable
    addresses, so cond / noise / out / frames live in per-shape buffers of the facade and the results are cloned out.
    Those buffers stay allocated between calls: with noise (explicit or rng = 'torch') that includes the [planes,B,3,H,W]
    noise buffer, 12.6 GB at B = 16, 256^2, T = 1000.  graph = 'off' keeps nothing; release_buffers(facade) frees them.
    Like the reference's netG.eval() / .train(), the engine's Dropout follows denoise_fn.training (a training step leaves the
    engine in train mode); with live dropout the loop runs eagerly, since a replayed chunk would repeat its masks.
    Returns out, or (out, frames [S,B,3,H,W]) with continous."""
    unet = facade.denoise_fn
    live_dropout = bool(unet.training and unet.cfg.dropout > 0)
    eng.set_training(live_dropout, seed_from_torch=True)
    T = eng.T
    every = frame_every(T)
    planes = T + (1 if eng.cfg.variant in ('ddpm', 'gdp') else 0)
    shape = (planes,) + tuple(x.shape)
    mode = getattr(facade, 'graph', 'auto')
    gbuf = facade.__dict__.setdefault('_gbuf', {})
    key = ('stepwise', tuple(x.shape), bool(continous), str(x.device), T)
    seen = gbuf.get(key)
    use_graph = mode != 'off' and not live_dropout and (mode == 'on' or seen is not None)
    if mode == 'auto' and seen is None:
        gbuf[key] = {}                    # this shape has been sampled once: the next call captures
    if not use_graph:
        if noise is None and draw_noise is not None:
            noise = torch.empty(shape, device=x.device, dtype=torch.float32)
            draw_noise(noise)
        return eng.sample(x, noise, want_traj=bool(continous), stepwise=True, traj_every=every)
    buf = gbuf.setdefault(key, {})
    if 'cond' not in buf:
        if len(gbuf) > 4:                 # shapes come and go: keep the buffers of the last few
            for old in [k_ for k_ in gbuf if k_ != key][:len(gbuf) - 4]:
                del gbuf[old]
        buf['cond'] = torch.empty_like(x)
        buf['out'] = torch.empty_like(x)
        buf['traj'] = torch.empty((eng.traj_slots(every),) + tuple(x.shape), device=x.device, dtype=torch.float32) if continous else None
    buf['cond'].copy_(x)
    nb = None
    if noise is not None or draw_noise is not None:
        if buf.get('noise') is None:
            buf['noise'] = torch.empty(shape, device=x.device, dtype=torch.float32)
        nb = buf['noise']
        if noise is not None:
            nb.copy_(noise)
        else:
            draw_noise(nb)
    res = eng.sample(buf['cond'], nb, want_traj=bool(continous), graph=True, out=buf['out'], traj=buf['traj'], stepwise=True,
                     traj_every=every)
    return (res[0].clone(), res[1].clone()) if continous else res.clone()


def release_buffers(facade):
    """Free the per-shape graph buffers sample_stepwise keeps on a facade (the next graph call of a shape captures again)."""
    gbuf = facade.__dict__.get('_gbuf', {})
    for k in [k_ for k_ in gbuf if k_[0] == 'stepwise']:
        del gbuf[k]


def frames_of(x, frames):
    """`continous=True`: ret_img = x_in followed by the kept x_t, concatenated along the batch dimension."""
    return torch.cat([x, frames.reshape((-1,) + tuple(x.shape[1:]))], dim=0)
