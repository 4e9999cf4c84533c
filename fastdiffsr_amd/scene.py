"""Whole-scene super-resolution: a scene larger than one sampling call is walked as overlapping square tiles.

    python -m fastdiffsr_amd.scene -c CONFIG (--lr IN --scale S | --sr IN) -o OUT
        [--tile 256] [--overlap 32] [--batch 16] [--precision ...] [--rng ...] [--seed 0] [--noise scene|tile|stream]

The reference has no such driver (its data are pre-cut patches); this is the layer above `p_sample_loop(x_in, noise=...)`:

  plan      `plan_tiles`: tile origins in row-major order and, per tile, over how many pixels its weight ramps up from each side
  noise     `noise='scene'`: ONE field [P,3,SH,SW] for the whole scene; a tile gets its crop, so two overlapping tiles start from
            the same x_T and see the same per-step noise in the pixels they share.  `noise='tile'`: [P,1,3,t,t] per tile from a
            generator keyed by (seed, tile index), for scenes whose field does not fit.  `noise='stream'` (rng='engine'): the
            field of noise='scene' without the array -- the sampler draws each tile pixel's numbers in its kernels from the
            pixel's place in the scene (Engine.set_noise_tiles), bit for bit what the crop would hold, at any T and any scene size.
  device    fdsr_scene_gather (scene -> cond / noise tiles), the sampler, fdsr_scene_blend (tiles -> acc, wsum), fdsr_scene_finish
            (acc / wsum -> uint8), csrc/fdsr_scene.hip; nothing of a scene's size crosses PCIe but the input and the result
  shared    with ediffsr/scene.py, which imports them: `walk`, `stream_table`, `check_request`, `check_origins`, both gathers and
            `timed_scene`; a driver keeps its model's side -- what a group's cond / state / noise are, and the sampling call

Every tile is its own sampling chain: GroupNorm statistics are per tile, so a tiled result is NOT the result of one untiled call
(DESIGN, "Whole-scene sampling").  What holds exactly: reruns are bitwise equal, with a single tile the result is the untiled path
bit for bit, and the blend does not depend on `batch` -- the whole result then depends on it only as far as the sampler's own image
depends on its batch size (not at all at the tested shapes; in a few last-bit uint8 roundings at 256x256 tiles, DESIGN)."""
import argparse
import ctypes as C
import time
from typing import List, NamedTuple, Tuple

NOISE_BUDGET = 16 << 30        # bytes the noise field of noise='scene' may take by default
# The least sum of weights over a scene pixel, in exact arithmetic (`plan_tiles`): along an axis at most three tiles meet (the
# stride is at least tile / 2, so tiles k and k + 2 only meet where the shifted last tile is involved), and with A < B < C the
# tiles over a pixel, a = A's trailing factor and b = B's trailing factor there, the sum is a + (1 - a) b + (1 - b) = 1 + a (1 - b)
# >= 1; with two tiles it is exactly 1.  The 2-D sum is the product of the two axes' sums.
WSUM_MIN = 1.0


class TilePlan(NamedTuple):
    origins: List[Tuple[int, int]]            # (y0, x0) per tile, row-major
    ramps: List[Tuple[int, int, int, int]]    # (top, left, bottom, right) per tile
    tile: int
    scene_h: int
    scene_w: int


def _axis(length, tile, overlap):
    """Origins along one axis and (leading, trailing) ramp lengths per tile: stride tile - overlap, the last tile shifted back to
    end at the border; a ramp is as long as the actual overlap with the neighbour on that side (0 at a scene border)."""
    stride = tile - overlap
    n = -(-(length - tile) // stride)
    org = [min(k * stride, length - tile) for k in range(n + 1)]
    lead = [0] + [org[k - 1] + tile - org[k] for k in range(1, n + 1)]
    trail = [org[k] + tile - org[k + 1] for k in range(n)] + [0]
    return org, lead, trail


def plan_tiles(scene_h, scene_w, tile, overlap, multiple=1):
    """The tiles of a scene_h x scene_w scene: square, `tile` pixels a side, neighbours `overlap` pixels apart from touching.

    Along an axis of length L with stride s = tile - overlap the origins are min(k s, L - tile), k = 0 .. ceil((L - tile) / s): the
    last tile is shifted back to end at the border, never padded.  A side has a ramp only where a neighbour exists; its length r
    is the overlap with that neighbour (larger than `overlap` for the shifted last tile).  The 1-D weight of pixel i = 0 .. r - 1
    of a leading ramp is (i + 1) / (r + 1) and (r - i) / (r + 1) on the neighbour's matching trailing ramp, 1 elsewhere; where a
    tile's two ramps meet (a short step before the shifted tile) the two factors multiply.  The 2-D weight is the product of the
    axes'.  Two tiles over a pixel sum to 1, three to at least 1 (WSUM_MIN); the blend divides by the accumulated weight.
    `multiple`: what the network needs a side to be a multiple of -- only to name a usable tile in the refusal; whether `tile`
    itself suits the network is the engine's to say (super_resolve_scene asks it)."""
    scene_h, scene_w, tile, overlap = int(scene_h), int(scene_w), int(tile), int(overlap)
    if tile < 1:
        raise ValueError(f'tile must be positive (got {tile})')
    if scene_h < tile or scene_w < tile:
        m = max(int(multiple), 1)
        best = min(scene_h, scene_w) // m * m
        usable = f'the largest usable tile is {best}' if best >= 1 else f'no tile fits (sides are multiples of {m})'
        raise ValueError(f'a {scene_h}x{scene_w} scene is smaller than tile {tile}: {usable}')
    if not 0 <= overlap <= tile // 2:
        raise ValueError(f'overlap must lie in [0, tile // 2] = [0, {tile // 2}] (got {overlap})')
    ys, top, bottom = _axis(scene_h, tile, overlap)
    xs, left, right = _axis(scene_w, tile, overlap)
    origins = [(y, x) for y in ys for x in xs]
    ramps = [(top[j], left[i], bottom[j], right[i]) for j in range(len(ys)) for i in range(len(xs))]
    return TilePlan(origins, ramps, tile, scene_h, scene_w)


def noise_field_bytes(planes, scene_h, scene_w):
    return int(planes) * 3 * int(scene_h) * int(scene_w) * 4


def check_noise_budget(planes, scene_h, scene_w, budget=NOISE_BUDGET):
    """noise='scene' keeps [planes,3,SH,SW] fp32 on the device for the whole run: refuse what does not fit the budget."""
    need = noise_field_bytes(planes, scene_h, scene_w)
    if need > budget:
        raise ValueError(f"the noise field of a {scene_h}x{scene_w} scene with {planes} planes takes {need / 2 ** 30:.2f} GiB "
                         f"({need} bytes), over the budget of {budget / 2 ** 30:.2f} GiB: use noise='tile' (or raise noise_budget)")
    return need


def _tile_key(seed, index):
    """A 63-bit generator seed for (seed, tile index): splitmix64's finaliser over the pair."""
    z = (int(seed) * 0x9E3779B97F4A7C15 + int(index) + 1) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return (z ^ (z >> 31)) & (2 ** 63 - 1)


def _planes(diffusion):
    return int(diffusion.num_timesteps) + (1 if diffusion.noise_at_t0 else 0)


def _draw(diffusion, seed, h, w, device):
    """[P,3,h,w] N(0,1) under the facade's rng: torch.randn from a device generator seeded by `seed`, or the engine's Philox planes
    (Engine.randn(1, h, w, plane)) after set_seed(seed).  The second re-seeds the facade's OWN engine and zeroes its call counter
    (the engine has no getter to put them back from): see super_resolve_scene."""
    import torch
    planes = _planes(diffusion)
    out = torch.empty(planes, 3, h, w, device=device, dtype=torch.float32)
    if diffusion.rng == 'engine':
        eng = diffusion.denoise_fn.engine
        eng.set_seed(seed)
        for p in range(planes):
            out[p].copy_(eng.randn(1, h, w, p, device=device)[0])
    else:
        g = torch.Generator(device=device)
        g.manual_seed(int(seed))
        for p in range(planes):
            torch.randn((3, h, w), generator=g, out=out[p])
    return out


def scene_noise_field(diffusion, scene_h, scene_w, seed, device='cuda'):
    """The field noise='scene' samples a scene_h x scene_w scene with: [P,3,SH,SW], P = T + noise_at_t0 as p_sample_loop counts."""
    return _draw(diffusion, seed, scene_h, scene_w, device)


def tile_noise(diffusion, tile, seed, index, device='cuda'):
    """The [P,1,3,t,t] noise of tile `index` under noise='tile'."""
    return _draw(diffusion, _tile_key(seed, index), tile, tile, device)[:, None]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def check_origins(origins):
    """What every reader of a tile table requires of it (the kernels read n pairs of int32 at its address); -> n."""
    import torch
    if not (origins.is_cuda and origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 2 and origins.shape[0] >= 1
            and origins.is_contiguous()):
        raise ValueError('origins must be a contiguous CUDA int32 tensor [n,2] with n >= 1')
    return int(origins.shape[0])


def gather(scene_u8, field, origins, tile):
    """fdsr_scene_gather: scene_u8 [SH,SW,3] uint8, field [P,3,SH,SW] fp32 or None, origins [n,2] int32 (all on the device) ->
    (cond [n,3,t,t], noise [P,n,3,t,t] or None)."""
    import torch
    from . import _lib
    sh, sw, _ = scene_u8.shape
    n = check_origins(origins)
    dev = scene_u8.device
    cond = torch.empty(n, 3, tile, tile, device=dev, dtype=torch.float32)
    planes = int(field.shape[0]) if field is not None else 0
    noise = torch.empty(planes, n, 3, tile, tile, device=dev, dtype=torch.float32) if field is not None else None
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(None, _lib.load().fdsr_scene_gather(None, _ptr(scene_u8), _ptr(field), planes, sh, sw, _ptr(origins), n, tile,
                                                   _ptr(cond), _ptr(noise), C.c_void_p(st)))
    return cond, noise


def gather_f32(scene, origins, tile, out=None):
    """fdsr_scene_gather_f32: scene [3,SH,SW] fp32, origins [n,2] int32 (on the device) -> tiles [n,3,t,t]."""
    import torch
    from . import _lib
    if not (scene.is_cuda and scene.dtype == torch.float32 and scene.dim() == 3 and scene.shape[0] == 3 and scene.is_contiguous()):
        raise ValueError('scene must be a contiguous CUDA fp32 tensor [3,SH,SW]')
    n = check_origins(origins)
    _, sh, sw = scene.shape
    if out is None:
        out = torch.empty(n, 3, tile, tile, device=scene.device, dtype=torch.float32)
    elif tuple(out.shape) != (n, 3, tile, tile) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != scene.device:
        raise ValueError(f'out must be a contiguous fp32 tensor [{n},3,{tile},{tile}] on the scene\'s device')
    st = torch.cuda.current_stream(scene.device).cuda_stream
    _lib.check(None, _lib.load().fdsr_scene_gather_f32(None, _ptr(scene), sh, sw, _ptr(origins), n, tile, _ptr(out), C.c_void_p(st)))
    return out


def blend(tiles, origins, ramps, acc, wsum):
    """fdsr_scene_blend: tiles [n,3,t,t] fp32 into acc [3,SH,SW] / wsum [SH,SW], tile by tile in ascending index."""
    import torch
    from . import _lib
    n, _, tile, _ = tiles.shape
    if tuple(origins.shape) != (n, 2) or tuple(ramps.shape) != (n, 4):      # the kernels index both tables by the tile's number
        raise ValueError(f'{n} tiles need origins [{n},2] and ramps [{n},4] (got {tuple(origins.shape)} and {tuple(ramps.shape)})')
    sh, sw = wsum.shape
    st = torch.cuda.current_stream(tiles.device).cuda_stream
    _lib.check(None, _lib.load().fdsr_scene_blend(None, _ptr(tiles), _ptr(origins), _ptr(ramps), n, tile, _ptr(acc), _ptr(wsum), sh, sw,
                                                  C.c_void_p(st)))


def finish(acc, wsum, want_u8=True, want_f32=False):
    """fdsr_scene_finish: acc / wsum -> the uint8 [SH,SW,3] scene and / or the fp32 [3,SH,SW] quotient."""
    import torch
    from . import _lib
    sh, sw = wsum.shape
    u8 = torch.empty(sh, sw, 3, device=acc.device, dtype=torch.uint8) if want_u8 else None
    f32 = torch.empty(3, sh, sw, device=acc.device, dtype=torch.float32) if want_f32 else None
    st = torch.cuda.current_stream(acc.device).cuda_stream
    _lib.check(None, _lib.load().fdsr_scene_finish(None, _ptr(acc), _ptr(wsum), sh, sw, _ptr(u8), _ptr(f32), C.c_void_p(st)))
    return (u8, f32) if want_u8 and want_f32 else (u8 if want_u8 else f32)


def plan_tables(plan, device):
    """The plan as the two int32 device tables the kernels read: origins [n,2], ramps [n,4]."""
    import torch
    return (torch.tensor(plan.origins, dtype=torch.int32, device=device).reshape(-1, 2).contiguous(),
            torch.tensor(plan.ramps, dtype=torch.int32, device=device).reshape(-1, 4).contiguous())


def check_request(noise, batch, modes):
    """The refusals both drivers make of their `noise` and `batch` arguments; modes: the driver's noise modes, its default first."""
    if noise not in modes:
        raise ValueError(f'noise must be one of {tuple(modes)} (got {noise!r})')
    if int(batch) < 1:
        raise ValueError('batch must be at least 1')


def stream_table(owner, origins, scene_w):
    """noise='stream': `origins` [b,2] copied into the owner's int32 buffer for groups of b and handed to owner.set_noise_tiles.  One
    buffer per (b, device), kept with the owner (an Engine or a ConditionalNAFNet) from its first use: the samplers' graph caches key
    on its address, so full groups replay one graph and a later scene finds the graphs an earlier one captured."""
    import torch
    tables = owner.__dict__.setdefault('_scene_tables', {})
    key = (int(origins.shape[0]), str(origins.device))
    if key not in tables:
        tables[key] = torch.empty(key[0], 2, dtype=torch.int32, device=origins.device)
    tables[key].copy_(origins)
    owner.set_noise_tiles(tables[key], scene_w)
    return tables[key]


def walk(plan, device, group, sample_group, stream=None, log=None):
    """The scene walk of both drivers: the plan's tiles in groups of `group` in plan order (the last group smaller, never padded),
    each sampled by sample_group(k0, k1, origins[k0:k1]) -> [k1-k0,3,t,t] fp32 and blended.  -> (acc [3,SH,SW], wsum [SH,SW]).
    stream: under noise='stream' the engine or network that draws -- each group's origins go into its `stream_table` before
    sample_group runs, and its table is cleared on the way out, whatever happened.  log: called with one line per group."""
    import torch
    n = len(plan.origins)
    origins, ramps = plan_tables(plan, device)
    acc = torch.zeros(3, plan.scene_h, plan.scene_w, device=device, dtype=torch.float32)
    wsum = torch.zeros(plan.scene_h, plan.scene_w, device=device, dtype=torch.float32)
    try:
        for k0 in range(0, n, group):
            k1 = min(k0 + group, n)
            if stream is not None:
                stream_table(stream, origins[k0:k1], plan.scene_w)
            out = sample_group(k0, k1, origins[k0:k1])
            if out.dim() == 3:                # a call of ONE image comes back without its batch axis from the ddpm / tesr / gdp siblings
                out = out[None]
            if out.shape[0] != k1 - k0:
                raise RuntimeError(f'p_sample_loop returned {out.shape[0]} image(s) for {k1 - k0} tiles')
            blend(out.contiguous(), origins[k0:k1], ramps[k0:k1], acc, wsum)
            if log is not None:
                log(f'scene: tiles {k0 + 1}..{k1} of {n}')
    finally:
        if stream is not None:
            stream.clear_noise_tiles()
    return acc, wsum


def tiles_per_call(diffusion, batch):
    """How many tiles one p_sample_loop call of this facade can sample: `batch`, but 1 for the tesr and gdp siblings, whose
    p_sample_loop returns ret_img[-1] -- the LAST image of its batch -- as the reference's does (their `_result`; val.py refuses
    their batches for the same reason).  Asked of the facade itself, with an empty batch of two."""
    import torch
    whole = diffusion._result(torch.empty(2, 1, 1, 1)).dim() == 4
    return int(batch) if whole else 1


def super_resolve_scene(diffusion, scene_u8, tile=256, overlap=32, batch=16, noise='scene', seed=0, precision=None, log=None,
                        noise_budget=NOISE_BUDGET):
    """scene_u8: the UPSCALED scene (the conditioning image, e.g. data.lr_to_sr of the whole LR scene), [SH,SW,3] uint8 on the
    device.  diffusion: any of the four GaussianDiffusion facades, schedule set.  -> the super-resolved scene, [SH,SW,3] uint8 on
    the device.

    Tiles go through diffusion.p_sample_loop(cond, noise=...) in groups of `batch` in plan order (the last group is smaller, not
    padded); the facade's `graph` setting applies, so the full groups -- one shape -- replay a captured graph.  The tesr and gdp
    siblings return one image per call, so their tiles go one per call whatever `batch` says (`tiles_per_call`).  Tiles are blended
    in ascending index with one fp32 add each (include/fdsr.h: fdsr_scene_blend), so the blend is bitwise independent of `batch`.
    precision: the facade's precision for this call (None: as it is set).  log: called with one line per group.

    Side effect under rng='engine': the noise is drawn with the facade's own engine after Engine.set_seed -- once with `seed`
    (noise='scene'), or per tile with the key of (seed, tile index) (noise='tile').  The engine's seed and its per-call counter
    stay as the last of these left them: a later p_sample_loop that draws its own noise continues from there, not from where the
    caller's earlier set_seed had it.  Call set_seed again before such a call.  rng='torch' uses a generator of its own and leaves
    torch's global stream alone.

    noise='stream' (rng='engine' only; ValueError under rng='torch'): no field is drawn and noise_budget is not consulted.
    set_seed(seed) once, then per group the walk points the sampler at the group's origins (`stream_table`) and p_sample_loop(cond)
    draws its own noise: for the tile at (y0, x0) the crop of the field noise='scene' would have drawn, so the result equals
    noise='scene' bit for bit.  Such calls leave the engine's call counter at 0, where set_seed put it; the table is cleared on the
    way out.  The f16x3 range guard's re-run of a call (Engine.on_saturation) therefore redraws the SAME noise here: the counter
    does not move, and the numbers depend on nothing else."""
    import torch
    if not scene_u8.is_cuda or scene_u8.dtype != torch.uint8 or scene_u8.dim() != 3 or scene_u8.shape[-1] != 3:
        raise ValueError('scene_u8 must be a CUDA uint8 tensor of shape [SH,SW,3]')
    check_request(noise, batch, ('scene', 'tile', 'stream'))
    if noise == 'stream' and diffusion.rng != 'engine':
        raise ValueError(f"noise='stream' draws in the engine's kernels and requires rng='engine' (the facade's rng is {diffusion.rng!r})")
    scene_u8 = scene_u8.contiguous()
    dev = scene_u8.device
    sh, sw, _ = scene_u8.shape
    unet = diffusion.denoise_fn
    eng = unet.engine
    eng.workspace_bytes(1, tile, tile)        # a tile the network does not take is refused here, in the engine's own words
    plan = plan_tiles(sh, sw, tile, overlap, multiple=1 << (len(unet.cfg.channel_mults) - 1))
    if noise == 'scene':
        check_noise_budget(_planes(diffusion), sh, sw, noise_budget)
    old_precision, was_training = diffusion.precision, unet.training
    if precision is not None:
        diffusion.precision = precision
    unet.train(False)                         # as DDPM.test does around a sampling call: no live Dropout
    try:
        field = scene_noise_field(diffusion, sh, sw, seed, dev) if noise == 'scene' else None
        if noise == 'stream':
            eng.set_seed(seed)

        def sample_group(k0, k1, origins):
            cond, nz = gather(scene_u8, field, origins, tile)
            if noise == 'tile':
                nz = torch.cat([tile_noise(diffusion, tile, seed, k, dev) for k in range(k0, k1)], dim=1)
            return diffusion.p_sample_loop(cond, noise=nz)    # under 'stream' nz is None: the sampler draws, by the walk's table

        group = tiles_per_call(diffusion, batch)
        return finish(*walk(plan, dev, group, sample_group, stream=eng if noise == 'stream' else None, log=log))
    finally:
        diffusion.precision = old_precision
        unet.train(was_training)


# -- CLI ------------------------------------------------------------------------------------------------------------------
def timed_scene(a, run):
    """The tail of both CLIs: time run() -> the [SH,SW,3] uint8 scene, save it to a.out, print the summary line, return it as a dict."""
    import torch
    from PIL import Image
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sh, sw, _ = out.shape
    tiles = len(plan_tiles(sh, sw, a.tile, a.overlap).origins)
    Image.fromarray(out.cpu().numpy()).save(a.out)
    peak = torch.cuda.max_memory_allocated() / 2 ** 20
    print(f'scene {sh}x{sw}: {tiles} tiles of {a.tile} (overlap {a.overlap}, batch {a.batch}, noise {a.noise}) in {dt:.3f} s, '
          f'{tiles / dt:.2f} tiles/s, peak device memory {peak:.0f} MiB -> {a.out}')
    return dict(tiles=tiles, seconds=dt, tiles_per_second=tiles / dt, peak_mib=peak, out=a.out, shape=(sh, sw))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m fastdiffsr_amd.scene', description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('-c', '--config', required=True, help="JSON file for configuration (the reference's own, as val.py reads it)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--lr', metavar='IN', help='the low-resolution scene; upscaled once, whole, on the device (PIL-exact bicubic)')
    src.add_argument('--sr', metavar='IN', help='the scene already upscaled to the output size (the conditioning image)')
    ap.add_argument('--scale', type=int, default=None, metavar='S', help='upscaling factor of --lr')
    ap.add_argument('-o', '--out', required=True, metavar='OUT', help='output image; the format follows the extension')
    ap.add_argument('-gpu', '--gpu_ids', default=None)
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--overlap', type=int, default=32)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--precision', default='f16x3', choices=['f32', 'f16x3', 'bf16', 'f16'])
    ap.add_argument('--rng', default=None, choices=['torch', 'engine'])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--noise', default='scene', choices=['scene', 'tile', 'stream'],
                    help="'stream': the field of 'scene' drawn in the sampler's kernels, no array of the scene's size (needs --rng engine)")
    a = ap.parse_args(argv)
    if a.lr is not None and a.scale is None:
        ap.error('--lr requires --scale')
    if a.sr is not None and a.scale is not None:
        ap.error('--scale applies to --lr only')
    if a.scale is not None and a.scale < 1:
        ap.error('--scale must be at least 1')
    if a.noise == 'stream' and a.rng == 'torch':
        ap.error('--noise stream requires --rng engine')
    return a


def main(argv=None):
    """The model, its checkpoint and the val schedule come from the config exactly as val.py builds them."""
    a = parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    from .config import load_config
    from .data import lr_to_sr
    from .model import create_model
    opt = load_config(a.config, phase='val', gpu_ids=a.gpu_ids)
    diffusion = create_model(opt)
    if a.rng is not None:
        diffusion.netG.rng = a.rng
    diffusion.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    img = torch.from_numpy(np.array(Image.open(a.lr or a.sr).convert('RGB'))).to(diffusion.device)
    if a.lr is not None:
        h, w, _ = img.shape
        _, up = lr_to_sr(img[None], h * a.scale, w * a.scale, want_u8=True)     # the scene, not the tiles: borders see their neighbours
        img = up[0]
    return timed_scene(a, lambda: super_resolve_scene(diffusion.netG, img, tile=a.tile, overlap=a.overlap, batch=a.batch, noise=a.noise,
                                                      seed=a.seed, precision=a.precision))


if __name__ == '__main__':
    main()
