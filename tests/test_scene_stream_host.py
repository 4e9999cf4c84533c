"""Host side of field-free scene noise and the EDiffSR scene driver: the two CLIs' arguments, the refusal of noise='stream' where it
cannot work, and the presence of the new C entry points in the binding table and the header (no GPU)."""
import os
import re

import pytest

from fastdiffsr_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('fdsr_set_noise_tiles', 'fdsr_nafnet_set_noise_tiles', 'fdsr_nafnet_randn_tiles', 'fdsr_scene_gather_f32')


def test_unet_cli_takes_noise_stream(capsys):
    base = ['-c', 'cfg.json', '--sr', 'in.png', '-o', 'out.png']
    assert S.parse_args(base + ['--noise', 'stream']).noise == 'stream'              # the rng is then the configuration's to say
    a = S.parse_args(base + ['--noise', 'stream', '--rng', 'engine'])
    assert (a.noise, a.rng) == ('stream', 'engine')
    assert S.parse_args(base).noise == 'scene'                                         # the default stays
    with pytest.raises(SystemExit) as e:
        S.parse_args(base + ['--noise', 'stream', '--rng', 'torch'])
    assert e.value.code == 2
    assert '--noise stream requires --rng engine' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        S.parse_args(base + ['--noise', 'field'])
    assert 'invalid choice' in capsys.readouterr().err


def test_ediffsr_cli_arguments(capsys):
    from fastdiffsr_amd.ediffsr import scene as ES
    a = ES.parse_args(['-opt', 'o.yml', '--lr', 'in.png', '-o', 'out.png'])
    assert (a.opt, a.lr, a.out) == ('o.yml', 'in.png', 'out.png')
    assert (a.tile, a.overlap, a.batch, a.precision, a.seed, a.noise, a.graph) == (256, 32, 16, 'f32', 0, 'stream', False)
    a = ES.parse_args(['-opt', 'o.yml', '--lr', 'in.png', '-o', 'out.tif', '--noise', 'scene', '--tile', '64', '--overlap', '8', '--batch',
                       '3', '--precision', 'f16x3', '--seed', '9', '--graph'])
    assert (a.noise, a.tile, a.overlap, a.batch, a.precision, a.seed, a.graph) == ('scene', 64, 8, 3, 'f16x3', 9, True)
    for noise in ES.NOISES:
        assert ES.parse_args(['-opt', 'o', '--lr', 'i', '-o', 'o', '--noise', noise]).noise == noise
    for argv, said in ((['-opt', 'o', '-o', 'o.png'], 'required'),                                         # no --lr
                       (['-opt', 'o', '--lr', 'i', '-o', 'o', '--noise', 'field'], 'invalid choice'),
                       (['-opt', 'o', '--lr', 'i', '-o', 'o', '--precision', 'bf16'], 'invalid choice'),    # the NAFNet has no bf16 mode
                       (['-opt', 'o', '--lr', 'i', '-o', 'o', '--rng', 'torch'], 'unrecognized arguments'),  # no torch-generator variant
                       (['-opt', 'o', '--lr', 'i', '-o', 'o', '--tile', '64', '--overlap', '33'], '--overlap must lie in [0, tile // 2]'),
                       (['-opt', 'o', '--lr', 'i', '-o', 'o', '--batch', '0'], '--batch must be at least 1')):
        with pytest.raises(SystemExit) as e:
            ES.parse_args(argv)
        assert e.value.code == 2
        assert said in capsys.readouterr().err, argv


def test_ediffsr_scene_reuses_the_unet_scene_plan():
    """Imported, not copied: the plan, the tables, the blend, the finish, the tile key and the budget check are scene.py's objects."""
    from fastdiffsr_amd.ediffsr import scene as ES
    for name in ('plan_tiles', 'plan_tables', 'blend', 'finish', '_tile_key', 'check_noise_budget'):
        assert getattr(ES, name) is getattr(S, name), name


def test_new_entry_points_are_bound_and_declared():
    from fastdiffsr_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'fdsr.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    # the header says what an origin outside the scene does
    assert 'address a counter, not memory' in txt
