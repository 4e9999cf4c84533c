"""Whole-scene super-resolution with EDiffSR (ConditionalNAFNet + IR-SDE): the scene is walked as overlapping square tiles.

    python -m fastdiffsr_amd.ediffsr.scene -opt setting_mfe_Test_x4.yml --lr IN -o OUT [--tile 256] [--overlap 32] [--batch 16]
                                           [--precision f32|f16x3|f16] [--seed 0] [--noise stream|scene|tile] [--graph]

Reads the YAML sections ediffsr/test.py reads (`network_G.setting`, `path.pretrain_model_G`, `sde`, `degradation.scale`).  The plan,
the blend and the budget check are fastdiffsr_amd/scene.py's; what differs is the model's side:

  input     LR uint8 -> [0,1] fp32 -> bicubic upscale of the WHOLE scene on the device (tile borders see their neighbours) -> mu
            tiles by fdsr_scene_gather_f32
  state     mu + randn(plane T) * max_sigma; the steps use planes 0 .. T-1 (what test.py does under --rng engine)
  noise     always the engine's Philox stream (there is no torch-generator variant):
              'stream' (default)  drawn in the sampler's kernels from each pixel's place in the scene
                                  (ConditionalNAFNet.set_noise_tiles): no array of the scene's size, at any T
              'scene'             the same numbers as a field [T+1,3,SH,SW] drawn with randn(1, SH, SW, plane, seed), cropped and
                                  passed as explicit noise -- what 'stream' is proven against, and the way to supply a field
              'tile'              per tile its own stream: seed = the key of (seed, tile index), origin (0, 0)
  output    fdsr_scene_blend, fdsr_scene_finish to fp32, tensor2img with min_max (0, 1) -> uint8 [SH,SW,3]

'stream' equals 'scene' bit for bit, and both are bitwise independent of --batch: the NAFNet's result for an image depends neither
on the batch size nor on the image's position in it.  A tiled result is not the untiled one (the SCA statistics are per tile).
Under f16x3 / f16 the range guard is read once per group, and a group that raised it is run again in f32 with a warning."""
import argparse
import ctypes as C
import time

from ..scene import NOISE_BUDGET, _tile_key, blend, check_noise_budget, finish, plan_tables, plan_tiles

NOISES = ('stream', 'scene', 'tile')


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def gather_f32(scene, origins, tile, out=None):
    """fdsr_scene_gather_f32: scene [3,SH,SW] fp32, origins [n,2] int32 (on the device) -> tiles [n,3,t,t]."""
    import torch
    from .. import _lib
    if not (scene.is_cuda and scene.dtype == torch.float32 and scene.dim() == 3 and scene.shape[0] == 3 and scene.is_contiguous()):
        raise ValueError('scene must be a contiguous CUDA fp32 tensor [3,SH,SW]')
    if not origins.is_cuda or origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or origins.shape[0] < 1:
        raise ValueError(f'origins must be a CUDA int32 tensor [n,2] with n >= 1 (got {origins.dtype} {tuple(origins.shape)})')
    _, sh, sw = scene.shape
    n = int(origins.shape[0])
    if out is None:
        out = torch.empty(n, 3, tile, tile, device=scene.device, dtype=torch.float32)
    elif tuple(out.shape) != (n, 3, tile, tile) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != scene.device:
        raise ValueError(f'out must be a contiguous fp32 tensor [{n},3,{tile},{tile}] on the scene\'s device')
    st = torch.cuda.current_stream(scene.device).cuda_stream
    _lib.check(None, _lib.load().fdsr_scene_gather_f32(None, _ptr(scene), sh, sw, _ptr(origins.contiguous()), n, tile, _ptr(out), C.c_void_p(st)))
    return out


def scene_noise_field(net, T, scene_h, scene_w, seed, device):
    """The field noise='scene' samples with: [T+1,3,SH,SW], plane k = the eps of step t = T - k, plane T = x_T's."""
    import torch
    return torch.cat([net.randn(1, scene_h, scene_w, p, seed, device=device) for p in range(T + 1)])


def super_resolve_scene(net, sde, lq, scale, tile=256, overlap=32, batch=16, noise='stream', seed=0, precision=None, log=None,
                        noise_budget=NOISE_BUDGET):
    """lq: the low-resolution scene, [3,h,w] fp32 in [0,1] on the device.  net: a ConditionalNAFNet; sde: an IRSDE with set_model(net)
    done.  -> the super-resolved scene, [SH,SW,3] uint8 on the device, SH = h * scale.

    Tiles go through sde.reverse_sde in groups of `batch` in plan order (the last group is smaller); sde.graph applies.  The sde's
    rng, seed and first_image are set for the call ('engine', `seed`, 0) and put back; precision: the network's for this call
    (None: as it is set)."""
    import torch
    from .. import metrics as M
    from .model import upscale
    from .test import reverse_sde_guarded
    if not lq.is_cuda or lq.dim() != 3 or lq.shape[0] != 3:
        raise ValueError('lq must be a CUDA tensor of shape [3,h,w]')
    if noise not in NOISES:
        raise ValueError(f"noise must be one of {NOISES} (got {noise!r})")
    if int(batch) < 1:
        raise ValueError('batch must be at least 1')
    dev = lq.device
    T, batch = int(sde.T), int(batch)
    mu_scene = upscale(lq[None], scale)[0]
    _, sh, sw = mu_scene.shape
    plan = plan_tiles(sh, sw, tile, overlap)
    n = len(plan.origins)
    if noise == 'scene':
        check_noise_budget(T + 1, sh, sw, noise_budget)
    old = (sde.rng, sde.seed, sde.first_image, net.precision)
    if precision is not None and precision != net.precision:
        if precision == 'f16' and net.precision == 'f16x3':
            net.set_precision('f32')
        net.set_precision(precision)
    sde.rng, sde.seed, sde.first_image = 'engine', int(seed), 0
    try:
        field = scene_noise_field(net, T, sh, sw, seed, dev) if noise == 'scene' else None
        origins, ramps = plan_tables(plan, dev)
        acc = torch.zeros(3, sh, sw, device=dev, dtype=torch.float32)
        wsum = torch.zeros(sh, sw, device=dev, dtype=torch.float32)
        # noise='stream': group size -> the device buffer its calls read their origins from; kept with the network, so that a later
        # scene finds the graph this one captured (it keys on the buffer's address)
        tables = net.__dict__.setdefault('_scene_tables', {})
        for k0 in range(0, n, batch):
            k1 = min(k0 + batch, n)
            b = k1 - k0
            mu = gather_f32(mu_scene, origins[k0:k1], tile)
            nz = None
            if noise == 'stream':
                if (b, str(dev)) not in tables:
                    tables[b, str(dev)] = torch.empty(b, 2, dtype=torch.int32, device=dev)
                table = tables[b, str(dev)]
                table.copy_(origins[k0:k1])
                net.set_noise_tiles(table, sw)
                x_t = net.randn(b, tile, tile, T, seed, device=dev)
            else:
                nz = torch.empty(T + 1, b, 3, tile, tile, device=dev, dtype=torch.float32)
                for p in range(T + 1):
                    if noise == 'scene':
                        gather_f32(field[p], origins[k0:k1], tile, out=nz[p])
                    else:
                        for j in range(b):
                            nz[p, j].copy_(net.randn(1, tile, tile, p, _tile_key(seed, k0 + j), device=dev)[0])
                x_t, nz = nz[T], nz[:T]
            state = mu + x_t * sde.max_sigma
            sde.set_mu(mu)
            out = reverse_sde_guarded(net, sde, state, 'tiles %d..%d' % (k0, k1 - 1), noise=nz)
            blend(out.contiguous(), origins[k0:k1], ramps[k0:k1], acc, wsum)
            if log is not None:
                log(f'scene: tiles {k0 + 1}..{k1} of {n}')
        return M.tensor2img_batch(finish(acc, wsum, want_u8=False, want_f32=True)[None], min_max=(0, 1))[0]
    finally:
        if noise == 'stream':
            net.clear_noise_tiles()
        sde.rng, sde.seed, sde.first_image = old[:3]
        if net.precision != old[3]:
            if old[3] == 'f16' and net.precision == 'f16x3':
                net.set_precision('f32')
            net.set_precision(old[3])


# -- CLI ------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m fastdiffsr_amd.ediffsr.scene', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-opt', required=True, help="the reference's YAML test options")
    ap.add_argument('--lr', required=True, metavar='IN', help='the low-resolution scene; upscaled once, whole, on the device')
    ap.add_argument('-o', '--out', required=True, metavar='OUT', help='output image; the format follows the extension')
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--overlap', type=int, default=32)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--precision', default='f32', choices=['f32', 'f16x3', 'f16'])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--noise', default='stream', choices=list(NOISES))
    ap.add_argument('--graph', action='store_true', help='replay one captured step')
    a = ap.parse_args(argv)
    if a.tile < 1:
        ap.error('--tile must be positive')
    if not 0 <= a.overlap <= a.tile // 2:
        ap.error('--overlap must lie in [0, tile // 2]')
    if a.batch < 1:
        ap.error('--batch must be at least 1')
    return a


def read_options(path):
    """The sections of the reference's YAML this driver needs (test.py's, without the datasets)."""
    import yaml
    with open(path) as f:
        opt = yaml.safe_load(f)
    for need in ('sde', 'degradation', 'network_G', 'path'):
        if need not in opt:
            raise KeyError('%s: missing section %r' % (path, need))
    opt['scale'] = opt['degradation']['scale']
    return opt


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    from .. import metrics as M
    from .sde import IRSDE
    from .test import build_model
    opt = read_options(a.opt)
    device = torch.device('cuda', torch.cuda.current_device())
    net = build_model(opt, device)
    net.set_precision(a.precision)
    s = opt['sde']
    sde = IRSDE(max_sigma=s['max_sigma'], T=s['T'], schedule=s['schedule'], eps=s['eps'], device=device, rng='engine', graph=a.graph,
                seed=a.seed)
    sde.set_model(net)
    img = torch.from_numpy(np.array(Image.open(a.lr).convert('RGB'))).to(device)
    lq = M.u8_to_tensor(img[None], min_max=(0, 1))[0]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = super_resolve_scene(net, sde, lq, opt['scale'], tile=a.tile, overlap=a.overlap, batch=a.batch, noise=a.noise, seed=a.seed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sh, sw, _ = out.shape
    tiles = len(plan_tiles(sh, sw, a.tile, a.overlap).origins)
    Image.fromarray(out.cpu().numpy()).save(a.out)
    peak = torch.cuda.max_memory_allocated() / 2 ** 20
    print(f'scene {sh}x{sw}: {tiles} tiles of {a.tile} (overlap {a.overlap}, batch {a.batch}, noise {a.noise}) in {dt:.3f} s, '
          f'{tiles / dt:.2f} tiles/s, peak device memory {peak:.0f} MiB -> {a.out}')
    return dict(tiles=tiles, seconds=dt, tiles_per_second=tiles / dt, peak_mib=peak, out=a.out, shape=(sh, sw))


if __name__ == '__main__':
    main()
