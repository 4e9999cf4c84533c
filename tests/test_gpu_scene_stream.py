"""Scene sampling without a noise field (noise='stream': Engine.set_noise_tiles, fdsr_set_noise_tiles): the sampler draws a tile
pixel's numbers from the pixel's place in the scene.  Every comparison is bitwise: the stream is the field, so a 'stream' scene is the
'scene' scene -- through fdsr_sample, through fdsr_sample_stepwise, eagerly and as graphs -- and the call counter does not move."""
import numpy as np
import pytest
import torch

from fastdiffsr_amd import metrics as M
from fastdiffsr_amd import scene as S
from fastdiffsr_amd.arch import UNetConfig
from fastdiffsr_amd.long_schedule import STEPWISE_ABOVE, use_stepwise
from fastdiffsr_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

# the synthetic facades of tests/test_gpu_scene.py
CFG = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 4, 4), attn_res=(), res_blocks=1,
           dropout=0.0, image_size=32)
SCHED = dict(schedule='linear', n_timestep=4, linear_start=1e-4, linear_end=2e-2)
TILE = 32
SIBLING = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2, 4), attn_res=(8,), res_blocks=1,
               dropout=0.0, image_size=TILE)
_FACADES = {}


def _build(which, unet, sched, variant=None):
    from fastdiffsr_amd import networks
    dev = torch.device('cuda')
    opt = {'phase': 'val', 'gpu_ids': [0], 'distributed': False, 'datasets': {'train': {'l_resolution': 64}},
           'model': {'which_model_G': which, 'finetune_norm': False,
                     'unet': {'in_channel': 6, 'out_channel': 3, 'inner_channel': unet['inner_channel'], 'norm_groups': 32,
                              'channel_multiplier': list(unet['channel_mults']), 'attn_res': list(unet['attn_res']),
                              'res_blocks': unet['res_blocks'], 'dropout': unet['dropout']},
                     'beta_schedule': {'train': dict(sched), 'val': dict(sched)},
                     'diffusion': {'image_size': TILE, 'channels': 3, 'conditional': True}}}
    netG = networks.define_G(opt).to(dev)
    netG.set_loss(dev)
    netG.set_new_noise_schedule(sched, dev)
    sd = synth_state_dict(UNetConfig(**(dict(unet, variant=variant) if variant else unet)), 17)
    ck = {'denoise_fn.' + k: torch.from_numpy(v) for k, v in sd.items()}
    ck.update({k: v.cpu() for k, v in netG.state_dict().items() if not k.startswith('denoise_fn.')})
    netG.load_state_dict(ck, strict=True)
    netG.eval()
    netG.rng = 'engine'
    return netG


def _facade():
    if 'fastdiffsr' not in _FACADES:
        _FACADES['fastdiffsr'] = _build('fastdiffsr', CFG, SCHED)
        assert _FACADES['fastdiffsr'].num_timesteps == 4
    return _FACADES['fastdiffsr']


def _sibling(which, T=4):
    if (which, T) not in _FACADES:
        _FACADES[which, T] = _build(which, SIBLING, dict(SCHED, n_timestep=T), variant=which)
    return _FACADES[which, T]


def _scene(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()


def _run(netG, scene, graph='off', **kw):
    netG.graph = graph
    try:
        return S.super_resolve_scene(netG, scene, tile=TILE, **kw)
    finally:
        netG.graph = 'auto'


def test_the_stream_is_the_field():
    eng = _facade().denoise_fn.engine
    origins = [(0, 0), (28, 44), (5, 3)]
    table = torch.tensor(origins, dtype=torch.int32, device='cuda')
    eng.set_seed(21)
    before = eng.randn(3, TILE, TILE, 1)
    for p in (0, 1, 19):
        field = eng.randn(1, 60, 76, p)[0]
        eng.set_noise_tiles(table, 76)
        try:
            tiles = eng.randn(3, TILE, TILE, p)
        finally:
            eng.clear_noise_tiles()
        for k, (y, x) in enumerate(origins):
            assert torch.equal(tiles[k], field[:, y:y + TILE, x:x + TILE]), (p, k)
        assert len(torch.unique(tiles)) > 1000
    assert torch.equal(eng.randn(3, TILE, TILE, 1), before)           # table cleared: what it was before
    assert not torch.equal(before[1], before[0])
    # more images than the table has origins: refused on the host, nothing is launched
    from fastdiffsr_amd import _lib
    eng.set_noise_tiles(table, 76)
    try:
        with pytest.raises(_lib.FdsrError, match='noise-tile table of 3'):
            eng.randn(4, TILE, TILE, 0)
    finally:
        eng.clear_noise_tiles()
    with pytest.raises(ValueError, match='int32'):
        eng.set_noise_tiles(table.long(), 76)


_WANT = {}


def _want(sh, sw, overlap):
    """noise='scene' on the flagship facade, batch 4, eager: the reference of the comparisons below, computed once."""
    if (sh, sw) not in _WANT:
        _WANT[sh, sw] = _run(_facade(), _scene(sh, sw, 3), overlap=overlap, batch=4, noise='scene', seed=11)
    return _WANT[sh, sw]


@pytest.mark.parametrize('graph', ['off', 'on'])
@pytest.mark.parametrize('batch', [4, 3])
@pytest.mark.parametrize('sh,sw,overlap', [(60, 76, 8), (61, 75, 7)])
def test_stream_equals_scene(sh, sw, overlap, batch, graph):
    """9 tiles: batch 4 is two full groups and a last group of one (a replayed graph reads a rewritten table), batch 3 another grouping."""
    want = _want(sh, sw, overlap)
    got = _run(_facade(), _scene(sh, sw, 3), graph=graph, overlap=overlap, batch=batch, noise='stream', seed=11)
    assert got.shape == (sh, sw, 3) and got.dtype == torch.uint8
    assert torch.equal(got, want)
    assert len(torch.unique(got)) > 16
    if (batch, graph) == (4, 'off'):
        assert not torch.equal(_run(_facade(), _scene(sh, sw, 3), overlap=overlap, batch=4, noise='stream', seed=12), want)


def test_a_second_scene_finds_the_first_one_s_tables():
    """The per-group-size origins buffers stay with the engine (S.stream_table): a second scene writes into the same memory -- the
    address the sampler's graphs key on -- and gives the same bytes.  Eagerly: what is checked is the driver's buffer, not a replay."""
    netG = _facade()
    eng = netG.denoise_fn.engine
    scene = _scene(60, 76, 3)
    first = _run(netG, scene, overlap=8, batch=4, noise='stream', seed=11)
    ptrs = {k: t.data_ptr() for k, t in eng._scene_tables.items()}
    assert {k[0] for k in ptrs} >= {4, 1}                     # nine tiles: groups of 4, 4 and 1
    second = _run(netG, scene, overlap=8, batch=4, noise='stream', seed=11)
    assert {k: t.data_ptr() for k, t in eng._scene_tables.items()} == ptrs
    assert torch.equal(second, first) and torch.equal(first, _want(60, 76, 8))


def test_stepwise_sibling():
    """ddpm at the smallest T that takes fdsr_sample_stepwise: posterior_step_kernel draws, eagerly and as replayed chunks; 40x56 is
    four tiles, batch 3 a group of three and one of one."""
    T = STEPWISE_ABOVE + 1
    assert use_stepwise(T) and not use_stepwise(T - 1)
    netG = _sibling('ddpm', T)
    assert netG.long_schedules and netG.num_timesteps == T
    scene = _scene(40, 56, 5)
    want = _run(netG, scene, overlap=8, batch=3, noise='scene', seed=6)
    for graph in ('off', 'on'):
        assert torch.equal(_run(netG, scene, graph=graph, overlap=8, batch=3, noise='stream', seed=6), want), graph
    assert len(torch.unique(want)) > 16


def test_tesr_one_tile_per_call():
    netG = _sibling('tesr')
    assert S.tiles_per_call(netG, 4) == 1
    scene = _scene(60, 76, 3)
    want = _run(netG, scene, overlap=8, batch=4, noise='scene', seed=11)
    assert torch.equal(_run(netG, scene, overlap=8, batch=4, noise='stream', seed=11), want)
    assert len(torch.unique(want)) > 16


def test_the_call_counter_is_frozen():
    netG = _facade()
    eng = netG.denoise_fn.engine
    eng.set_seed(31)
    fresh = eng.randn(1, 8, 8, 0)
    _run(netG, _scene(60, 76, 3), overlap=8, batch=4, noise='stream', seed=31)       # set_seed(31), then three calls that draw
    assert torch.equal(eng.randn(1, 8, 8, 0), fresh)
    # the control: a call that draws its own noise WITHOUT a table moves the counter
    netG.p_sample_loop(M.u8_to_tensor(_scene(TILE, TILE, 1)[None].contiguous()))
    assert not torch.equal(eng.randn(1, 8, 8, 0), fresh)


def test_no_field():
    netG = _facade()
    scene = _scene(60, 76, 3)
    field = S.noise_field_bytes(4, 60, 76)
    with pytest.raises(ValueError, match="noise='tile'"):
        _run(netG, scene, overlap=8, batch=4, noise='scene', seed=11, noise_budget=field - 1)
    peaks = {}
    for noise in ('tile', 'stream'):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = _run(netG, scene, overlap=8, batch=4, noise=noise, seed=11, noise_budget=field - 1)
        torch.cuda.synchronize()
        peaks[noise] = torch.cuda.max_memory_allocated() - base
        del out
    print('peak device memory over the call: tile %d bytes, stream %d bytes; the field would take %d' % (peaks['tile'], peaks['stream'], field))
    assert peaks['stream'] < field + peaks['tile']
    assert torch.equal(_run(netG, scene, overlap=8, batch=4, noise='stream', seed=11, noise_budget=field - 1), _want(60, 76, 8))


def test_refusals():
    netG = _facade()
    eng = netG.denoise_fn.engine
    netG.rng = 'torch'
    try:
        with pytest.raises(ValueError, match="requires rng='engine'"):
            _run(netG, _scene(60, 76, 3), overlap=8, noise='stream')
    finally:
        netG.rng = 'engine'
    # explicit noise does not look at the table
    cond = M.u8_to_tensor(torch.stack([_scene(TILE, TILE, k) for k in (1, 2)]))
    noise = torch.randn(4, 2, 3, TILE, TILE, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    netG.graph = 'off'
    try:
        want = netG.p_sample_loop(cond, noise=noise)
        eng.set_noise_tiles(torch.tensor([(7, 9), (100, 3)], dtype=torch.int32, device='cuda'), 76)
        try:
            assert torch.equal(netG.p_sample_loop(cond, noise=noise), want)
        finally:
            eng.clear_noise_tiles()
    finally:
        netG.graph = 'auto'
