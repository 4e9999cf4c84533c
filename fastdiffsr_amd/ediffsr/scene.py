"""Whole-scene super-resolution with EDiffSR (ConditionalNAFNet + IR-SDE): the scene is walked as overlapping square tiles.

    python -m fastdiffsr_amd.ediffsr.scene -opt setting_mfe_Test_x4.yml --lr IN -o OUT [--tile 256] [--overlap 32] [--batch 16]
                                           [--precision f32|f16x3|f16] [--seed 0] [--noise stream|scene|tile] [--graph]

Reads the YAML sections ediffsr/test.py reads (`network_G.setting`, `path.pretrain_model_G`, `sde`, `degradation.scale`).  The plan,
the walk over it, the gathers, the refusals and the CLI's tail are fastdiffsr_amd/scene.py's; this file holds the model's side:

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

# the shared side, imported, not copied: also what only the walk calls (tables, blend, stream table) stays reachable from here
from ..scene import (NOISE_BUDGET, _tile_key, blend, check_noise_budget, check_origins, check_request, finish, gather_f32,
                     plan_tables, plan_tiles, stream_table, timed_scene, walk)

NOISES = ('stream', 'scene', 'tile')


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
    check_request(noise, batch, NOISES)
    dev = lq.device
    T = int(sde.T)
    mu_scene = upscale(lq[None], scale)[0]
    _, sh, sw = mu_scene.shape
    plan = plan_tiles(sh, sw, tile, overlap)
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

        def sample_group(k0, k1, origins):
            b = k1 - k0
            mu = gather_f32(mu_scene, origins, tile)
            nz = None
            if noise == 'stream':             # the walk has set the group's table: randn and the sampler draw the scene's crops
                x_t = net.randn(b, tile, tile, T, seed, device=dev)
            else:
                nz = torch.empty(T + 1, b, 3, tile, tile, device=dev, dtype=torch.float32)
                for p in range(T + 1):
                    if noise == 'scene':
                        gather_f32(field[p], origins, tile, out=nz[p])
                    else:
                        for j in range(b):
                            nz[p, j].copy_(net.randn(1, tile, tile, p, _tile_key(seed, k0 + j), device=dev)[0])
                x_t, nz = nz[T], nz[:T]
            state = mu + x_t * sde.max_sigma
            sde.set_mu(mu)
            return reverse_sde_guarded(net, sde, state, 'tiles %d..%d' % (k0, k1 - 1), noise=nz)

        acc, wsum = walk(plan, dev, int(batch), sample_group, stream=net if noise == 'stream' else None, log=log)
        return M.tensor2img_batch(finish(acc, wsum, want_u8=False, want_f32=True)[None], min_max=(0, 1))[0]
    finally:
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
    return timed_scene(a, lambda: super_resolve_scene(net, sde, lq, opt['scale'], tile=a.tile, overlap=a.overlap, batch=a.batch,
                                                      noise=a.noise, seed=a.seed))


if __name__ == '__main__':
    main()
