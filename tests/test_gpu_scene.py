"""Whole-scene sampling on the GPU (fastdiffsr_amd/scene.py, csrc/fdsr_scene.hip): gather / blend / finish against a numpy fp64
restatement, the single tile and the zero-overlap scene against the untiled path, independence of the batching, the CLI."""
import json

import numpy as np
import pytest
import torch

from fastdiffsr_amd import metrics as M
from fastdiffsr_amd import scene as S
from fastdiffsr_amd.arch import UNetConfig
from fastdiffsr_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

# the small fastdiffsr network of tests/test_gpu_long_schedule.py, a 4-step schedule, tile 32
CFG = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 4, 4), attn_res=(), res_blocks=1,
           dropout=0.0, image_size=32)
SCHED = dict(schedule='linear', n_timestep=4, linear_start=1e-4, linear_end=2e-2)
TILE = 32
_FACADE = []


def _facade():
    if _FACADE:
        return _FACADE[0]
    from fastdiffsr_amd import networks
    dev = torch.device('cuda')
    opt = {'phase': 'val', 'gpu_ids': [0], 'distributed': False, 'datasets': {'train': {'l_resolution': 64}},
           'model': {'which_model_G': 'fastdiffsr', 'finetune_norm': False,
                     'unet': {'in_channel': 6, 'out_channel': 3, 'inner_channel': CFG['inner_channel'], 'norm_groups': 32,
                              'channel_multiplier': list(CFG['channel_mults']), 'attn_res': [], 'res_blocks': CFG['res_blocks'],
                              'dropout': CFG['dropout']},
                     'beta_schedule': {'train': dict(SCHED), 'val': dict(SCHED)},
                     'diffusion': {'image_size': TILE, 'channels': 3, 'conditional': True}}}
    netG = networks.define_G(opt).to(dev)
    netG.set_loss(dev)
    netG.set_new_noise_schedule(SCHED, dev)
    sd = synth_state_dict(UNetConfig(**CFG), 17)
    ck = {'denoise_fn.' + k: torch.from_numpy(v) for k, v in sd.items()}
    ck.update({k: v.cpu() for k, v in netG.state_dict().items() if not k.startswith('denoise_fn.')})
    netG.load_state_dict(ck, strict=True)
    netG.eval()
    assert netG.num_timesteps == 4
    _FACADE.append(netG)
    return netG


def _scene(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()


def _w1(tile, lead, trail):
    w = np.ones(tile, dtype=np.float64)
    for i in range(lead):
        w[i] *= (i + 1) / (lead + 1)
    for i in range(trail):
        w[tile - trail + i] *= (trail - i) / (trail + 1)
    return w


# 60x76, tile 32, overlap 8 (the issue's case: origins 0, 24, 28 along y / 0, 24, 44 along x -- shifted last tiles on both axes;
# rows 28..31 lie under all three tiles of a column, along x no more than two tiles meet (tile 0 ends at 31, tile 2 begins at 44);
# every origin and the width are multiples of 4, so every access is a wide one) and 61x75 with overlap 7 (origins 0, 25, 29 / 0,
# 25, 43 and an odd width: the element-by-element paths)
@pytest.mark.parametrize('sh,sw,overlap', [(60, 76, 8), (61, 75, 7)])
def test_gather_blend_finish_against_fp64(sh, sw, overlap):
    """No sampler: random uint8 scene, random fp32 field and tiles.  cond and the gathered noise are bit for bit the restatement's;
    the fp32 quotient is within 16 * 2^-24 * max|tile value| of it; the uint8 scene differs only where the fp64 value * 255 lies
    within that distance of a rounding boundary.

    The bound is the issue's, which counts the four tiles of a two-per-axis overlap.  Here up to SIX tiles meet over a pixel (three
    along y, two along x), and the bound still covers them: with u = 2^-24, S the pixel's sum of weights and m = max|tile value|,
    each term w v carries 2u (w rounded to fp32, the product), the five adds of the numerator at most u S m each, so acc is within
    7u S m; wsum is within 6u S (w rounded, five adds); the division adds u: |quotient - exact| <= (7 + 6 + 1) u m = 14u m, to
    first order."""
    rng = np.random.default_rng(sh * 100 + sw)
    plan = S.plan_tiles(sh, sw, TILE, overlap)
    n, planes = len(plan.origins), 5
    assert n == 9
    scene = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    field = rng.standard_normal((planes, 3, sh, sw)).astype(np.float32)
    tiles = (rng.standard_normal((n, 3, TILE, TILE)) * 0.8).astype(np.float32)      # a good part beyond [-1, 1]: the clamp works
    origins, ramps = S.plan_tables(plan, 'cuda')
    d_scene, d_field, d_tiles = torch.from_numpy(scene).cuda(), torch.from_numpy(field).cuda(), torch.from_numpy(tiles).cuda()
    # gather: ToTensor() * 2 - 1 in fp32 (one division, one product, one sum) and plain copies
    full = (scene.astype(np.float32) / np.float32(255.0)) * np.float32(2.0) + np.float32(-1.0)
    assert full.dtype == np.float32
    want_cond = np.stack([full[y:y + TILE, x:x + TILE].transpose(2, 0, 1) for y, x in plan.origins])
    want_noise = np.stack([field[:, :, y:y + TILE, x:x + TILE] for y, x in plan.origins], axis=1)
    cond, noise = S.gather(d_scene, d_field, origins, TILE)
    assert noise.shape == (planes, n, 3, TILE, TILE)
    assert np.array_equal(cond.cpu().numpy().view(np.uint32), want_cond.view(np.uint32))
    assert np.array_equal(noise.cpu().numpy().view(np.uint32), np.ascontiguousarray(want_noise).view(np.uint32))
    assert torch.equal(cond, M.u8_to_tensor(torch.stack([d_scene[y:y + TILE, x:x + TILE] for y, x in plan.origins])))
    cond2, none = S.gather(d_scene, None, origins[3:7], TILE)                        # a slice of the table, no field
    assert none is None and torch.equal(cond2, cond[3:7])
    # blend + finish, in two calls (tiles 0..3, then 4..8) and in one: the same bits
    acc64, wsum64 = np.zeros((3, sh, sw)), np.zeros((sh, sw))
    for (y, x), (top, left, bottom, right), v in zip(plan.origins, plan.ramps, tiles):
        w = np.outer(_w1(TILE, top, bottom), _w1(TILE, left, right))
        acc64[:, y:y + TILE, x:x + TILE] += w * v.astype(np.float64)
        wsum64[y:y + TILE, x:x + TILE] += w
    q64 = acc64 / wsum64
    results = []
    for cuts in ([0, 4, n], [0, n]):
        acc = torch.zeros(3, sh, sw, device='cuda')
        wsum = torch.zeros(sh, sw, device='cuda')
        for a, b in zip(cuts[:-1], cuts[1:]):
            S.blend(d_tiles[a:b].contiguous(), origins[a:b], ramps[a:b], acc, wsum)
        results.append(S.finish(acc, wsum, want_u8=True, want_f32=True))
        assert torch.equal(S.finish(acc, wsum, want_u8=True, want_f32=False), results[-1][0])
        assert torch.equal(S.finish(acc, wsum, want_u8=False, want_f32=True), results[-1][1])
        assert np.abs(wsum.cpu().numpy() - wsum64).max() <= 8 * 2.0 ** -24 * wsum64.max()
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    u8, f32 = results[0][0].cpu().numpy(), results[0][1].cpu().numpy().astype(np.float64)
    bound = 16 * 2.0 ** -24 * float(np.abs(tiles).max())
    err = np.abs(f32 - q64).max()
    x255 = (np.clip(q64, -1.0, 1.0) + 1.0) / 2.0 * 255.0
    want_u8 = np.rint(x255).astype(np.uint8).transpose(1, 2, 0)
    near = (np.abs(x255 - (np.floor(x255) + 0.5)) <= bound).transpose(1, 2, 0)
    differ = u8 != want_u8
    print(f'scene blend {sh}x{sw}: max |fp32 quotient - fp64| {err:.3e} (bound {bound:.3e}); uint8: {int(differ.sum())} pixels differ, '
          f'{int(near.sum())} lie within the bound of a rounding boundary, {int((differ & ~near).sum())} differ elsewhere')
    assert err <= bound
    assert not (differ & ~near).any()
    assert (np.abs(u8.astype(int) - want_u8.astype(int)) <= 1).all()


def _untiled(netG, scene_u8, field):
    """The existing path for ONE tile-sized scene: u8 -> tensor, p_sample_loop with the given planes, tensor2img."""
    cond = M.u8_to_tensor(scene_u8[None].contiguous())
    return M.tensor2img_batch(netG.p_sample_loop(cond, noise=field[:, None].contiguous()))[0]


@pytest.mark.parametrize('rng', ['torch', 'engine'])
def test_one_tile_is_the_existing_path(rng):
    netG = _facade()
    netG.rng = rng
    try:
        scene = _scene(TILE, TILE, 1)
        out = S.super_resolve_scene(netG, scene, tile=TILE, overlap=8, seed=3)
        field = S.scene_noise_field(netG, TILE, TILE, 3)
        assert field.shape == (4, 3, TILE, TILE)
        assert out.shape == (TILE, TILE, 3) and out.dtype == torch.uint8
        assert torch.equal(out, _untiled(netG, scene, field))
        assert len(torch.unique(out)) > 16                   # an image, not a constant
    finally:
        netG.rng = 'torch'


def test_zero_overlap_halves_are_their_own_samples():
    netG = _facade()
    scene = _scene(2 * TILE, TILE, 2)
    out = S.super_resolve_scene(netG, scene, tile=TILE, overlap=0, seed=4)
    field = S.scene_noise_field(netG, 2 * TILE, TILE, 4)
    for k in range(2):
        rows = slice(k * TILE, (k + 1) * TILE)
        assert torch.equal(out[rows], _untiled(netG, scene[rows], field[:, :, rows])), k


@pytest.mark.parametrize('noise', ['scene', 'tile'])
def test_batch_independence_and_seeds(noise):
    """60x76: 9 tiles (3 x 3).  batch = 1, 4, 6 and 9 (every tile in one call) give the same bytes; so does a rerun; another seed
    does not."""
    netG = _facade()
    scene = _scene(60, 76, 3)
    outs = [S.super_resolve_scene(netG, scene, tile=TILE, overlap=8, batch=b, noise=noise, seed=11) for b in (1, 4, 6, 9, 4)]
    assert outs[0].shape == (60, 76, 3)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    other = S.super_resolve_scene(netG, scene, tile=TILE, overlap=8, batch=4, noise=noise, seed=12)
    assert not torch.equal(other, outs[0])
    if noise == 'scene':
        with pytest.raises(ValueError, match="noise='tile'"):
            S.super_resolve_scene(netG, scene, tile=TILE, overlap=8, noise_budget=4 * 3 * 60 * 76 * 4 - 1)


# the siblings' small network of tests/test_gpu_long_schedule.py (attention at 8x8), without dropout
SIBLING = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2, 4), attn_res=(8,), res_blocks=1,
               dropout=0.0, image_size=TILE)
_SIBLINGS = {}


def _sibling(which):
    if which in _SIBLINGS:
        return _SIBLINGS[which]
    from fastdiffsr_amd import networks
    dev = torch.device('cuda')
    opt = {'phase': 'val', 'gpu_ids': [0], 'distributed': False, 'datasets': {'train': {'l_resolution': 64}},
           'model': {'which_model_G': which, 'finetune_norm': False,
                     'unet': {'in_channel': 6, 'out_channel': 3, 'inner_channel': SIBLING['inner_channel'], 'norm_groups': 32,
                              'channel_multiplier': list(SIBLING['channel_mults']), 'attn_res': list(SIBLING['attn_res']),
                              'res_blocks': SIBLING['res_blocks'], 'dropout': SIBLING['dropout']},
                     'beta_schedule': {'train': dict(SCHED), 'val': dict(SCHED)},
                     'diffusion': {'image_size': TILE, 'channels': 3, 'conditional': True}}}
    netG = networks.define_G(opt).to(dev)
    netG.set_loss(dev)
    netG.set_new_noise_schedule(SCHED, dev)
    sd = synth_state_dict(UNetConfig(**dict(SIBLING, variant=which)), 17)
    ck = {'denoise_fn.' + k: torch.from_numpy(v) for k, v in sd.items()}
    ck.update({k: v.cpu() for k, v in netG.state_dict().items() if not k.startswith('denoise_fn.')})
    netG.load_state_dict(ck, strict=True)
    netG.eval()
    _SIBLINGS[which] = netG
    return netG


@pytest.mark.parametrize('which,per_call', [('tesr', 1), ('ddpm', 4)])
def test_sibling_facades_at_batch_above_one(which, per_call):
    """tesr returns the LAST image of a batch (gdp shares that `_result`: tests/test_scene_host.py), so its tiles go one per call
    whatever `batch` says; ddpm (SR3) returns the batch whole.  Either way every tile lands at its own place: with overlap 0 each
    half of a 64x32 scene is that crop sampled alone, and on the 60x76 scene batch 4 gives the bytes of batch 1."""
    netG = _sibling(which)
    assert S.tiles_per_call(netG, 4) == per_call
    planes = 4 + (1 if which == 'ddpm' else 0)
    scene = _scene(2 * TILE, TILE, 5)
    out = S.super_resolve_scene(netG, scene, tile=TILE, overlap=0, batch=2, seed=6)
    field = S.scene_noise_field(netG, 2 * TILE, TILE, 6)
    assert field.shape == (planes, 3, 2 * TILE, TILE)
    for k in range(2):
        rows = slice(k * TILE, (k + 1) * TILE)
        alone = netG.p_sample_loop(M.u8_to_tensor(scene[rows][None].contiguous()), noise=field[:, None, :, rows].contiguous())
        assert alone.shape == (3, TILE, TILE)               # one image: without its batch axis
        assert torch.equal(out[rows], M.tensor2img_batch(alone[None])[0]), k
        assert len(torch.unique(out[rows])) > 16
    assert not torch.equal(out[:TILE], out[TILE:])
    big = _scene(60, 76, 3)
    for noise in ('scene', 'tile'):
        a, b = (S.super_resolve_scene(netG, big, tile=TILE, overlap=8, batch=bt, noise=noise, seed=11) for bt in (4, 1))
        assert torch.equal(a, b), noise


def test_blend_refuses_tables_of_another_length():
    plan = S.plan_tiles(60, 76, TILE, 8)
    origins, ramps = S.plan_tables(plan, 'cuda')
    acc, wsum = torch.zeros(3, 60, 76, device='cuda'), torch.zeros(60, 76, device='cuda')
    one = torch.zeros(1, 3, TILE, TILE, device='cuda')
    with pytest.raises(ValueError, match=r'1 tiles need origins \[1,2\]'):
        S.blend(one, origins[:4], ramps[:4], acc, wsum)
    with pytest.raises(ValueError, match='ramps'):
        S.blend(one, origins[:1], ramps[:2], acc, wsum)
    assert not acc.any() and not wsum.any()


def test_refusals_on_the_device():
    from fastdiffsr_amd import _lib
    netG = _facade()
    with pytest.raises(_lib.FdsrError, match='multiples of 8'):          # the engine's own message for a size the network rejects
        S.super_resolve_scene(netG, _scene(60, 76, 3), tile=36, overlap=8)
    with pytest.raises(ValueError, match='largest usable tile is 24'):
        S.super_resolve_scene(netG, _scene(30, 76, 3), tile=TILE, overlap=8)
    with pytest.raises(ValueError, match='CUDA uint8'):
        S.super_resolve_scene(netG, _scene(60, 76, 3).cpu(), tile=TILE)


def test_cli_end_to_end(tmp_path):
    """15x19 LR png, --scale 4 -> a 60x76 file whose pixels are the Python entry's; --sr on the PIL-upscaled file gives the same
    (the device bicubic is PIL's, bit for bit)."""
    from PIL import Image
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.data import lr_to_sr
    from fastdiffsr_amd.model import create_model
    from test_gpu_val import _config_plain
    cfg = _config_plain(str(tmp_path / 'data'))
    cfg['model']['unet'].update(inner_channel=32, channel_multiplier=[1, 2, 4, 4], attn_res=[], res_blocks=1)
    cfg['model']['beta_schedule'] = {'train': dict(SCHED), 'val': dict(SCHED)}
    cfg['model']['diffusion']['image_size'] = TILE
    cpath = tmp_path / 'cfg.json'
    cpath.write_text(json.dumps(cfg, indent=1).replace('"phase": "val",', '"phase": "val", // a comment'))
    lr = np.random.default_rng(9).integers(0, 256, (15, 19, 3), dtype=np.uint8)
    Image.fromarray(lr).save(tmp_path / 'lr.png')
    common = ['-c', str(cpath), '--tile', str(TILE), '--overlap', '8', '--seed', '5']
    torch.manual_seed(7)                                       # no checkpoint: the weights are torch's default draws
    r = S.main(common + ['--lr', str(tmp_path / 'lr.png'), '--scale', '4', '-o', str(tmp_path / 'out_lr.png'), '--batch', '4'])
    assert r['tiles'] == 9 and r['shape'] == (60, 76)
    got = np.asarray(Image.open(tmp_path / 'out_lr.png'))
    assert got.shape == (60, 76, 3) and got.dtype == np.uint8
    # the Python entry on the same weights, seed and (device-upscaled) scene
    torch.manual_seed(7)
    model = create_model(load_config(str(cpath), phase='val'))
    model.set_new_noise_schedule(cfg['model']['beta_schedule']['val'], schedule_phase='val')
    _, up = lr_to_sr(torch.from_numpy(lr).cuda()[None], 60, 76, want_u8=True)
    want = S.super_resolve_scene(model.netG, up[0], tile=TILE, overlap=8, batch=9, seed=5, precision='f16x3')
    assert np.array_equal(got, want.cpu().numpy())
    assert len(np.unique(got)) > 16
    # --sr: the scene upscaled by PIL itself; tif output
    Image.open(tmp_path / 'lr.png').resize((76, 60), Image.BICUBIC).save(tmp_path / 'sr.png')
    torch.manual_seed(7)
    S.main(common + ['--sr', str(tmp_path / 'sr.png'), '-o', str(tmp_path / 'out_sr.tif')])
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'out_sr.tif')), got)
