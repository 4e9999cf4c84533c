"""Whole scenes for EDiffSR (fastdiffsr_amd/ediffsr/scene.py): the fp32 gather, the single tile against test.py's flow, field-free
noise ('stream') against the cropped field ('scene'), independence of the batching, the precisions and the CLI.  The small synthetic
NAFNet of tests/test_gpu_ediffsr.py, IRSDE(T = 10, eps = 0.5).  Every comparison is bitwise."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TEST_SETTING = dict(width=16, enc_blk_nums=[2, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
SDE = dict(max_sigma=50, T=10, schedule='cosine', eps=0.5)
DEV = 'cuda'
TILE, SCALE = 32, 4


@pytest.fixture(scope='module')
def pair():
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    from fastdiffsr_amd.synth import synth_nafnet
    net = ConditionalNAFNet(**TEST_SETTING)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}, strict=True)
    net = net.to(DEV).eval()
    sde = IRSDE(device=DEV, rng='engine', **SDE)
    sde.set_model(net)
    return net, sde


def _lq(h, w, seed):
    return torch.rand(3, h, w, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _scene(pair, lq, **kw):
    from fastdiffsr_amd.ediffsr import scene as ES
    net, sde = pair
    kw.setdefault('overlap', 8)
    return ES.super_resolve_scene(net, sde, lq, SCALE, tile=TILE, **kw)


@pytest.mark.parametrize('sh,sw,overlap', [(60, 76, 8), (61, 75, 7)])
def test_gather_f32_is_slicing(sh, sw, overlap):
    from fastdiffsr_amd import scene as S
    from fastdiffsr_amd.ediffsr import scene as ES
    scene = torch.randn(3, sh, sw, generator=torch.Generator().manual_seed(sh)).to(DEV)
    plan = S.plan_tiles(sh, sw, TILE, overlap)
    origins, _ = S.plan_tables(plan, DEV)
    tiles = ES.gather_f32(scene, origins, TILE)
    assert tiles.shape == (9, 3, TILE, TILE)
    for k, (y, x) in enumerate(plan.origins):
        assert torch.equal(tiles[k], scene[:, y:y + TILE, x:x + TILE]), k
    assert torch.equal(ES.gather_f32(scene, origins[3:7], TILE), tiles[3:7])
    with pytest.raises(ValueError, match='fp32'):
        ES.gather_f32(scene.double(), origins, TILE)


def test_one_tile_is_the_existing_path(pair):
    from fastdiffsr_amd import metrics as M
    from fastdiffsr_amd.ediffsr.model import upscale
    net, sde = pair
    lq = _lq(8, 8, 1)
    got = _scene(pair, lq, seed=7)
    assert got.shape == (TILE, TILE, 3) and got.dtype == torch.uint8
    # test.py's flow for that image under --rng engine, first_image = 0
    mu = upscale(lq[None], SCALE)
    state = mu + net.randn(1, TILE, TILE, SDE['T'], 7, first_image=0, device=DEV) * sde.max_sigma
    sde.seed, sde.first_image = 7, 0
    sde.set_mu(mu)
    want = M.tensor2img_batch(sde.reverse_sde(state), min_max=(0, 1))[0]
    assert torch.equal(got, want)
    assert len(torch.unique(got)) > 16
    for noise in ('scene', 'tile'):      # one tile at (0, 0): the field is the tile's plane; 'tile' is another stream
        other = _scene(pair, lq, seed=7, noise=noise)
        assert torch.equal(other, want) == (noise == 'scene'), noise


def test_stream_equals_scene_whatever_the_batch(pair):
    net, sde = pair
    lq = _lq(15, 19, 2)                                   # 60 x 76: nine tiles
    want = _scene(pair, lq, seed=11, noise='scene', batch=4)
    assert want.shape == (60, 76, 3) and len(torch.unique(want)) > 16
    assert torch.equal(_scene(pair, lq, seed=11, noise='scene', batch=3), want)
    for batch in (4, 3):
        assert torch.equal(_scene(pair, lq, seed=11, noise='stream', batch=batch), want), batch
    sde.graph = True                                      # full groups replay one graph over a rewritten table
    try:
        assert torch.equal(_scene(pair, lq, seed=11, noise='stream', batch=4), want)
    finally:
        sde.graph = False
    assert (sde.rng, sde.first_image) == ('engine', 0) and getattr(net, '_noise_tiles', None) is None
    from fastdiffsr_amd import scene as S
    with pytest.raises(ValueError, match="noise='tile'"):
        _scene(pair, lq, seed=11, noise='scene', noise_budget=S.noise_field_bytes(SDE['T'] + 1, 60, 76) - 1)
    assert torch.equal(_scene(pair, lq, seed=11, noise_budget=1), want)       # 'stream' (the default) has no field to budget


def test_a_second_scene_finds_the_first_one_s_tables(pair):
    """The per-group-size origins buffers stay with the network (scene.stream_table): a second scene writes into the same memory --
    the address the step graph keys on -- and gives the same bytes."""
    net, sde = pair
    lq = _lq(15, 19, 2)
    first = _scene(pair, lq, seed=11, noise='stream', batch=4)
    ptrs = {k: t.data_ptr() for k, t in net._scene_tables.items()}
    assert {k[0] for k in ptrs} >= {4, 1}                     # nine tiles: groups of 4, 4 and 1
    second = _scene(pair, lq, seed=11, noise='stream', batch=4)
    assert {k: t.data_ptr() for k, t in net._scene_tables.items()} == ptrs
    assert torch.equal(second, first) and len(torch.unique(first)) > 16


def test_a_group_that_comes_back_short_is_refused(pair, monkeypatch):
    from fastdiffsr_amd.ediffsr import test as T
    net, sde = pair
    real = T.reverse_sde_guarded
    monkeypatch.setattr(T, 'reverse_sde_guarded', lambda *a, **kw: real(*a, **kw)[:-1])
    with pytest.raises(RuntimeError, match=r'returned 3 image\(s\) for 4 tiles'):
        _scene(pair, _lq(15, 19, 2), seed=11, batch=4)
    assert getattr(net, '_noise_tiles', None) is None         # 'stream': the table is cleared on the way out


def test_both_setters_refuse_a_bad_table_in_the_same_words(pair):
    from fastdiffsr_amd import scene as S
    from fastdiffsr_amd.arch import UNetConfig
    from fastdiffsr_amd.engine import Engine
    net, _ = pair
    eng = Engine(UNetConfig(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 4, 4), attn_res=(),
                            res_blocks=1, dropout=0.0, image_size=32))
    good = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    bad = {'not int32': good.long(), 'not contiguous': torch.zeros(4, 4, dtype=torch.int32, device=DEV)[:, ::2],
           '[n,3]': torch.zeros(4, 3, dtype=torch.int32, device=DEV), 'empty': good[:0], 'on the host': good.cpu()}
    assert tuple(bad['not contiguous'].shape) == (4, 2) and not bad['not contiguous'].is_contiguous()
    for what, t in bad.items():
        said = []
        for call in (lambda: eng.set_noise_tiles(t, 76), lambda: net.set_noise_tiles(t, 76), lambda: S.check_origins(t)):
            with pytest.raises(ValueError, match='origins must be a contiguous CUDA int32 tensor') as e:
                call()
            said.append(str(e.value))
        assert said[0] == said[1] == said[2], what
    assert getattr(eng, '_noise_tiles', None) is None and getattr(net, '_noise_tiles', None) is None   # nothing was set
    assert S.check_origins(good) == 4


def test_zero_overlap_tiles_are_their_own_samples(pair):
    from fastdiffsr_amd import metrics as M
    from fastdiffsr_amd.ediffsr.model import upscale
    net, sde = pair
    lq = _lq(16, 8, 3)                                    # 64 x 32: two tiles, one above the other
    got = _scene(pair, lq, seed=5, overlap=0, batch=2)
    mu_scene = upscale(lq[None], SCALE)
    sde.seed, sde.first_image = 5, 0
    for k in range(2):
        rows = slice(k * TILE, (k + 1) * TILE)
        mu = mu_scene[:, :, rows].contiguous()
        net.set_noise_tiles(torch.tensor([(k * TILE, 0)], dtype=torch.int32, device=DEV), 32)
        try:
            state = mu + net.randn(1, TILE, TILE, SDE['T'], 5, device=DEV) * sde.max_sigma
            sde.set_mu(mu)
            alone = sde.reverse_sde(state)
        finally:
            net.clear_noise_tiles()
        assert torch.equal(got[rows], M.tensor2img_batch(alone, min_max=(0, 1))[0]), k
    assert not torch.equal(got[:TILE], got[TILE:])


@pytest.mark.parametrize('noise', ['stream', 'tile'])
def test_seeds(pair, noise):
    lq = _lq(15, 19, 2)
    a = _scene(pair, lq, seed=11, noise=noise, batch=4)
    assert torch.equal(_scene(pair, lq, seed=11, noise=noise, batch=4), a)
    assert not torch.equal(_scene(pair, lq, seed=12, noise=noise, batch=4), a)


def test_first_image_with_a_table_is_refused(pair):
    from fastdiffsr_amd import _lib
    net, sde = pair
    mu = _lq(TILE, TILE, 4)[None].contiguous()
    net.set_noise_tiles(torch.zeros(1, 2, dtype=torch.int32, device=DEV), 76)
    try:
        with pytest.raises(_lib.FdsrError, match='first_image must be 0') as e:
            net.sample(mu, mu, seed=3, first_image=2)
        assert e.value.code == -1                           # FDSR_E_INVALID
        with pytest.raises(_lib.FdsrError, match='noise-tile table of 1') as e:
            net.sample(mu.repeat(2, 1, 1, 1), mu.repeat(2, 1, 1, 1), seed=3)
        assert e.value.code == -1
        with pytest.raises(ValueError, match='first_image must be 0'):
            net.randn(1, TILE, TILE, 0, 3, first_image=2)
        with_table = net.sample(mu, mu, seed=3)
    finally:
        net.clear_noise_tiles()
    assert torch.equal(net.sample(mu, mu, seed=3, first_image=2), net.sample(mu.repeat(3, 1, 1, 1), mu.repeat(3, 1, 1, 1), seed=3)[2:3])
    assert not torch.equal(with_table, net.sample(mu, mu, seed=3))     # origin (0, 0) of a 76-wide scene: other positions than a 32-wide image's


@pytest.mark.parametrize('precision', ['f16x3', 'f16'])
def test_precisions_and_the_f32_rerun(pair, precision, monkeypatch, caplog):
    """Both modes run end to end, within one grey level of f32 (the bar and the reasoning of test_gpu_ediffsr_f16.test_cli_precision
    for this network and schedule: the final-state error of the coarser mode, 3e-4, is 0.08 of a grey level, so a value can cross
    one rounding boundary and no more; overlap 0, so nothing is blended), and a group whose range flag is reported raised --
    by a stand-in for the reading, nothing is provoked on the device -- is run again in f32: its tile carries the f32 bytes, the
    other tile the mode's, and the network ends in the mode it was given."""
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    net, sde = pair
    lq = _lq(16, 8, 3)                                    # two tiles, overlap 0, one per group
    kw = dict(seed=5, overlap=0, batch=1)
    f32 = _scene(pair, lq, **kw)
    low = _scene(pair, lq, precision=precision, **kw)
    assert net.precision == 'f32'
    step = int((low.int() - f32.int()).abs().max())
    print('%s against f32: largest step %d grey level(s), %d of %d values differ' % (precision, step, int((low != f32).sum()), low.numel()))
    assert step <= 1
    real, calls, modes = ConditionalNAFNet.check_saturation, [], []

    def flagged_once(self):
        real(self)
        calls.append(self.precision)
        if len(calls) == 1:
            raise _lib.FdsrSaturated(_lib.FDSR_E_SATURATED, 'test: flag reported raised')

    monkeypatch.setattr(ConditionalNAFNet, 'check_saturation', flagged_once)
    monkeypatch.setattr(ConditionalNAFNet, 'set_precision',
                        lambda self, mode, _real=ConditionalNAFNet.set_precision: (modes.append(mode), _real(self, mode))[1])
    with caplog.at_level(logging.WARNING, logger='fastdiffsr_amd.ediffsr'):
        mixed = _scene(pair, lq, precision=precision, **kw)
    assert calls == [precision, precision] and modes == [precision, 'f32', precision, 'f32']
    assert any('tiles 0..0' in r.getMessage() and 'again in f32' in r.getMessage() for r in caplog.records)
    assert torch.equal(mixed[:TILE], f32[:TILE]) and torch.equal(mixed[TILE:], low[TILE:])
    assert net.precision == 'f32'


def test_cli_end_to_end(tmp_path):
    import yaml
    from PIL import Image
    from fastdiffsr_amd.ediffsr import scene as ES
    from fastdiffsr_amd.synth import synth_nafnet
    root = str(tmp_path)
    torch.save({k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}, os.path.join(root, 'latest_G.pth'))
    opt = {'name': 'Test-x4', 'suffix': None, 'sde': dict(SDE), 'degradation': {'scale': SCALE},
           'path': {'pretrain_model_G': os.path.join(root, 'latest_G.pth')},
           'network_G': {'which_model_G': 'ConditionalNAFNet', 'setting': TEST_SETTING}}
    with open(os.path.join(root, 'opt.yml'), 'w') as f:
        yaml.safe_dump(opt, f)
    lr = np.random.default_rng(9).integers(0, 256, (15, 19, 3), dtype=np.uint8)
    Image.fromarray(lr).save(os.path.join(root, 'lr.png'))
    base = ['-opt', os.path.join(root, 'opt.yml'), '--lr', os.path.join(root, 'lr.png'), '--tile', str(TILE), '--overlap', '8', '--seed', '5']
    r = ES.main(base + ['-o', os.path.join(root, 'stream.png'), '--batch', '4', '--graph'])
    assert r['tiles'] == 9 and r['shape'] == (60, 76)
    got = np.asarray(Image.open(os.path.join(root, 'stream.png')))
    assert got.shape == (60, 76, 3) and got.dtype == np.uint8 and len(np.unique(got)) > 16
    ES.main(base + ['-o', os.path.join(root, 'scene.tif'), '--batch', '3', '--noise', 'scene'])
    assert np.array_equal(np.asarray(Image.open(os.path.join(root, 'scene.tif'))), got)
