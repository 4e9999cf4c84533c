"""Whole-scene sampling rate on the GPU: a synthetic 2048 x 2048 scene through scene.super_resolve_scene (tile 256, overlap 32,
batch 16: 81 tiles = 5 groups of 16 and a last group of 1) against Engine.sample with explicit noise at B = 16 on the same tile
shape (the scene's first group of tiles as its input), in one process, f16x3 and f16, in alternating windows.  The ratio is
tiles/s of the scene over tiles/s of the bare sampler; the parts of a scene run (the noise field, one group's gather and blend, the facade call of a full group and of the last 1-tile group) are
timed on their own so that a ratio below 1 can be attributed.

Two more sets of rows (--rows picks; --append adds to the file under a header of its own):
  stream   noise='stream' (drawn in the sampler's kernels, no field) beside noise='scene' (the field drawn once, cropped, passed as
           explicit noise), both under rng='engine', same scene and process, alternating windows; peak device memory of each
  ediffsr  EDiffSR (the shipped ConditionalNAFNet setting, IRSDE T = 100, --precision f16, noise='stream'): tiles/s of the same
           2048 x 2048 scene at batch 16 against the bare ConditionalNAFNet.sample at B = 16 on the scene's first group

    python tools/scene_timing.py [--out profiles/scene_timing.txt] [--rows base stream ediffsr] [--append]

Synthetic weights (synth.synth_state_dict, the flagship UNet; synth.synth_nafnet); the cost does not depend on the weight values."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENE, TILE, OVERLAP, BATCH = 2048, 256, 32, 16
WINDOWS = 6        # per side; a window with a range-guard re-run in it is left out of the mean, so take a few more than three


def facade():
    from fastdiffsr_amd import networks
    from fastdiffsr_amd.arch import FASTDIFFSR_SCHEDULE_VAL, FASTDIFFSR_UNET, UNetConfig
    from fastdiffsr_amd.synth import synth_state_dict
    u = FASTDIFFSR_UNET
    dev = torch.device('cuda')
    opt = {'phase': 'val', 'gpu_ids': [0], 'distributed': False, 'datasets': {'train': {'l_resolution': 64}},
           'model': {'which_model_G': 'fastdiffsr', 'finetune_norm': False,
                     'unet': {'in_channel': 6, 'out_channel': 3, 'inner_channel': u['inner_channel'], 'norm_groups': u['norm_groups'],
                              'channel_multiplier': list(u['channel_mults']), 'attn_res': list(u['attn_res']),
                              'res_blocks': u['res_blocks'], 'dropout': u['dropout']},
                     'beta_schedule': {'train': dict(FASTDIFFSR_SCHEDULE_VAL), 'val': dict(FASTDIFFSR_SCHEDULE_VAL)},
                     'diffusion': {'image_size': TILE, 'channels': 3, 'conditional': True}}}
    netG = networks.define_G(opt).to(dev)
    netG.set_loss(dev)
    netG.set_new_noise_schedule(FASTDIFFSR_SCHEDULE_VAL, dev)
    sd = synth_state_dict(UNetConfig(**dict(u, image_size=TILE)), 0)
    ck = {'denoise_fn.' + k: torch.from_numpy(v) for k, v in sd.items()}
    ck.update({k: v.cpu() for k, v in netG.state_dict().items() if not k.startswith('denoise_fn.')})
    netG.load_state_dict(ck, strict=True)
    netG.eval()
    return netG


def timed(fn, reps):
    """Mean seconds of fn() over `reps` calls: host clock around work that ends in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def peak_mib(fn):
    """Peak device memory over one fn(), MiB: everything resident counts (weights, workspaces, graph buffers, the scene)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20


def stream_rows(netG, scene, lines):
    """noise='stream' beside noise='scene' under rng='engine': A B A B windows of two scenes each, then the peak memory of one run."""
    from fastdiffsr_amd import scene as S
    from fastdiffsr_amd.engine import Engine
    n = len(S.plan_tiles(SCENE, SCENE, TILE, OVERLAP).origins)
    netG.rng = 'engine'
    try:
        for prec in ('f16x3', 'f16'):
            netG.precision = prec
            runs = {m: (lambda m=m: S.super_resolve_scene(netG, scene, tile=TILE, overlap=OVERLAP, batch=BATCH, seed=0, noise=m))
                    for m in ('scene', 'stream')}
            for m in runs:
                for _ in range(3):
                    runs[m]()
            # the two modes compute the same scene (tests/test_gpu_scene_stream.py): checked here on the eager loop, and the warmed-up
            # graph replays of either mode are compared with that result
            netG.graph = 'off'
            eager = {m: runs[m]() for m in runs}
            netG.graph = 'auto'
            same = '%s; graph replays equal the eager scene: noise=scene %s, noise=stream %s' % (
                torch.equal(eager['scene'], eager['stream']), torch.equal(runs['scene'](), eager['scene']),
                torch.equal(runs['stream'](), eager['stream']))
            del eager
            ts = {m: [] for m in runs}
            for _ in range(WINDOWS):
                for m in runs:
                    fb0 = Engine.saturation_fallbacks
                    dt = timed(runs[m], 2)
                    ts[m].append((dt, Engine.saturation_fallbacks - fb0))
            mean = {m: (lambda c: sum(c) / len(c))([t for t, fb in ts[m] if fb == 0] or [t for t, _ in ts[m]]) for m in runs}
            peaks = {m: peak_mib(runs[m]) for m in runs}
            show = lambda v: ' '.join('%.3f%s' % (t, '*' * fb) for t, fb in v)   # noqa: E731
            lines.append('%-5s rng=engine  noise=scene %7.3f s, %7.2f tiles/s, peak %6.0f MiB | noise=stream %7.3f s, %7.2f tiles/s, peak %6.0f MiB | '
                         'stream / scene rate %.3f; uint8 scenes equal: %s  (windows: %s s / %s s; *: a range-guard re-run inside, left out of the means)' % (
                             prec, mean['scene'], n / mean['scene'], peaks['scene'], mean['stream'], n / mean['stream'], peaks['stream'],
                             mean['scene'] / mean['stream'], same, show(ts['scene']), show(ts['stream'])))
    finally:
        netG.rng = 'torch'


EDIFFSR_SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])   # the shipped options
EDIFFSR_SDE = dict(max_sigma=50, T=100, schedule='cosine', eps=0.005)
EDIFFSR_WINDOWS = 2      # a scene is 81 tiles x 100 forwards


def ediffsr_row(lines):
    from fastdiffsr_amd import scene as S
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    from fastdiffsr_amd.ediffsr import scene as ES
    from fastdiffsr_amd.ediffsr.model import upscale
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    from fastdiffsr_amd.synth import synth_nafnet
    net = ConditionalNAFNet(**EDIFFSR_SETTING)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_nafnet(0, **EDIFFSR_SETTING).items()}, strict=True)
    net = net.to('cuda').eval()
    net.set_precision('f16')
    sde = IRSDE(device='cuda', rng='engine', **EDIFFSR_SDE)
    sde.set_model(net)
    scale = 4
    lq = torch.rand(3, SCENE // scale, SCENE // scale, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    plan = S.plan_tiles(SCENE, SCENE, TILE, OVERLAP)
    n = len(plan.origins)
    origins, _ = S.plan_tables(plan, 'cuda')
    run = lambda: ES.super_resolve_scene(net, sde, lq, scale, tile=TILE, overlap=OVERLAP, batch=BATCH, seed=0)   # noqa: E731
    mu = ES.gather_f32(upscale(lq[None], scale)[0], origins[:BATCH], TILE)
    state = mu + net.randn(BATCH, TILE, TILE, EDIFFSR_SDE['T'], 0) * sde.max_sigma
    bare = lambda: net.sample(state, mu, noise=None, seed=0)   # noqa: E731
    peak = peak_mib(run)          # the warm-up too
    bare()
    t_scene, t_bare = [], []
    for _ in range(EDIFFSR_WINDOWS):
        t_scene.append(timed(run, 1))
        t_bare.append(timed(bare, 2))
    m_scene, m_bare = sum(t_scene) / len(t_scene), sum(t_bare) / len(t_bare)
    r_scene, r_bare = n / m_scene, BATCH / m_bare
    lines.append('ediffsr f16 (width 64, enc 14-1-1-1, T = %d) noise=stream scene %7.3f s, %6.2f tiles/s, peak %6.0f MiB (a field would take %.2f GiB) | '
                 'ConditionalNAFNet.sample B=%d engine-drawn noise, eager %8.1f ms per call, %6.2f tiles/s | ratio %.3f  (windows: %s s / %s ms)' % (
                     EDIFFSR_SDE['T'], m_scene, r_scene, peak, S.noise_field_bytes(EDIFFSR_SDE['T'] + 1, SCENE, SCENE) / 2 ** 30, BATCH,
                     1e3 * m_bare, r_bare, r_scene / r_bare, ' '.join('%.3f' % t for t in t_scene), ' '.join('%.1f' % (1e3 * t) for t in t_bare)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'scene_timing.txt'))
    ap.add_argument('--rows', nargs='+', default=['base', 'stream', 'ediffsr'], choices=['base', 'stream', 'ediffsr'])
    ap.add_argument('--append', action='store_true', help='add to --out under this run\'s own header, keeping what is there')
    a = ap.parse_args()
    from fastdiffsr_amd import scene as S
    from fastdiffsr_amd.engine import Engine
    netG = facade()
    eng = netG.denoise_fn.engine
    g = torch.Generator(device='cuda').manual_seed(1)
    scene = torch.randint(0, 256, (SCENE, SCENE, 3), dtype=torch.uint8, device='cuda', generator=g)
    plan = S.plan_tiles(SCENE, SCENE, TILE, OVERLAP)
    n = len(plan.origins)
    origins, ramps = S.plan_tables(plan, 'cuda')
    T = netG.num_timesteps
    props = torch.cuda.get_device_properties(0)
    lines = ['# python tools/scene_timing.py --rows %s   (synthetic weights, synth.synth_state_dict(FASTDIFFSR_UNET, 0); T = %d)' % (' '.join(a.rows), T),
             '# gpu, as the runtime names it: %s, %s, %d CUs, %.0f GiB' % (props.name, getattr(props, 'gcnArchName', '?'),
                                                                         props.multi_processor_count, props.total_memory / 2 ** 30),
             '# scene %dx%d, tile %d, overlap %d, batch %d: %d tiles = %d groups of %d and a last group of %d; noise field %.2f GiB' % (
                 SCENE, SCENE, TILE, OVERLAP, BATCH, n, n // BATCH, BATCH, n % BATCH, S.noise_field_bytes(T, SCENE, SCENE) / 2 ** 30)]
    for prec in ('f16x3', 'f16') if 'base' in a.rows else ():
        netG.precision = prec
        run = lambda: S.super_resolve_scene(netG, scene, tile=TILE, overlap=OVERLAP, batch=BATCH, seed=0)   # noqa: E731
        for _ in range(3):       # warm-up: 'auto' captures a shape's graph on its second call, the 1-tile group's on the second scene
            run()
        eng.set_precision(prec)
        field = S.scene_noise_field(netG, SCENE, SCENE, 0)
        cond, noise = S.gather(scene, field, origins[:BATCH], TILE)      # the bare sampler's inputs: the scene's first group
        out = torch.empty_like(cond)
        bare = lambda: eng.sample(cond, noise, graph=True, out=out)   # noqa: E731
        for _ in range(3):
            bare()
        t_scene, t_bare = [], []       # (seconds per call, f16x3 range-guard re-runs in the window)
        for _ in range(WINDOWS):       # A B A B ...
            for fn, reps, dst in ((run, 2, t_scene), (bare, 10, t_bare)):
                fb0 = Engine.saturation_fallbacks
                dt = timed(fn, reps)
                dst.append((dt, Engine.saturation_fallbacks - fb0))
        # a window in which the range guard re-ran a call on the fp32 kernels (Engine.on_saturation) timed that re-run too: the rates
        # compare the windows without one (all of them if there is none)
        clean = [[t for t, fb in ts if fb == 0] or [t for t, _ in ts] for ts in (t_scene, t_bare)]
        m_scene, m_bare = sum(clean[0]) / len(clean[0]), sum(clean[1]) / len(clean[1])
        r_scene, r_bare = n / m_scene, BATCH / m_bare
        show = lambda ts, k: ' '.join('%.*f%s' % (3 if k == 1 else 2, k * t, '*' * fb) for t, fb in ts)   # noqa: E731
        lines.append('%-5s scene %7.3f s, %7.2f tiles/s | Engine.sample B=%d explicit noise, graph %7.2f ms per call, %7.2f tiles/s | ratio %.3f  '
                     '(windows: %s s / %s ms; *: a range-guard re-run inside, left out of the means)' % (
                         prec, m_scene, r_scene, BATCH, 1e3 * m_bare, r_bare, r_scene / r_bare, show(t_scene, 1), show(t_bare, 1e3)))
        if prec == 'f16x3':
            # the blend does not depend on the grouping; the sampler's own bits per image may (the launcher picks kernel forms by grid size)
            fb0 = Engine.saturation_fallbacks
            a16 = run()
            a9 = S.super_resolve_scene(netG, scene, tile=TILE, overlap=OVERLAP, batch=9, seed=0)
            d = (a16.int() - a9.int()).abs()
            lines.append('%-5s   batch 16 against batch 9 (same seed): %d of %d uint8 samples differ, max |difference| %d (range-guard re-runs '
                         'in the two runs: %d)' % (prec, int((d != 0).sum()), d.numel(), int(d.max()), Engine.saturation_fallbacks - fb0))
            del a16, a9, d
        # the parts of one scene run
        t_field = timed(lambda: S.scene_noise_field(netG, SCENE, SCENE, 0), 3)
        acc = torch.zeros(3, SCENE, SCENE, device='cuda')
        wsum = torch.zeros(SCENE, SCENE, device='cuda')
        c16, n16 = S.gather(scene, field, origins[:BATCH], TILE)
        c1, n1 = S.gather(scene, field, origins[:1], TILE)
        t_gather = timed(lambda: S.gather(scene, field, origins[:BATCH], TILE), 10)
        t_blend = timed(lambda: S.blend(c16, origins[:BATCH], ramps[:BATCH], acc, wsum), 10)
        t_finish = timed(lambda: S.finish(acc + 1, wsum + 1), 5)
        for _ in range(2):
            netG.p_sample_loop(c16, noise=n16), netG.p_sample_loop(c1, noise=n1)
        t_full = timed(lambda: netG.p_sample_loop(c16, noise=n16), 5)
        t_last = timed(lambda: netG.p_sample_loop(c1, noise=n1), 5)
        full_groups, rest = n // BATCH, n % BATCH
        parts = t_field + (full_groups + (1 if rest else 0)) * (t_gather + t_blend) + full_groups * t_full + (t_last if rest == 1 else 0) + t_finish
        lines.append('%-5s   parts: noise field %.1f ms; per group of %d: gather %.2f ms, blend %.2f ms, p_sample_loop (explicit noise, graph '
                     'replay) %.2f ms; the last 1-tile group %.2f ms; finish (with two scene-sized adds) %.2f ms; sum of parts %.3f s' % (
                         prec, 1e3 * t_field, BATCH, 1e3 * t_gather, 1e3 * t_blend, 1e3 * t_full, 1e3 * t_last, 1e3 * t_finish, parts))
        del field, acc, wsum, c16, n16, c1, n1, cond, noise, out
        torch.cuda.empty_cache()
    if 'stream' in a.rows:
        stream_rows(netG, scene, lines)
    del netG, eng, scene
    torch.cuda.empty_cache()
    if 'ediffsr' in a.rows:
        ediffsr_row(lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
