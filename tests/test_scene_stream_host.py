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
    """Imported, not copied: the plan, the tables, the blend, the finish, the tile key and the budget check are scene.py's objects,
    and so are the walk, the stream table, the fp32 gather and the origins check."""
    from fastdiffsr_amd.ediffsr import scene as ES
    for name in ('plan_tiles', 'plan_tables', 'blend', 'finish', '_tile_key', 'check_noise_budget',
                 'walk', 'stream_table', 'gather_f32', 'check_origins', 'check_request', 'timed_scene'):
        assert getattr(ES, name) is getattr(S, name), name
    assert not hasattr(ES, '_ptr')                            # the one _ptr left is scene.py's


class _Owner:
    """Stands in for an Engine / a ConditionalNAFNet: records what the shared helpers ask of it."""

    def __init__(self):
        self.calls = []

    def set_noise_tiles(self, table, scene_w):
        self.calls.append(('set', table, scene_w, table.clone()))

    def clear_noise_tiles(self):
        self.calls.append(('clear',))


def test_stream_table_is_one_buffer_per_group_size_and_device():
    import torch
    owner = _Owner()
    origins = torch.arange(24, dtype=torch.int32).reshape(12, 2)
    a = S.stream_table(owner, origins[0:5], 76)
    assert a.dtype == torch.int32 and tuple(a.shape) == (5, 2) and torch.equal(a, origins[0:5])
    b = S.stream_table(owner, origins[5:10], 76)
    assert b is a and torch.equal(a, origins[5:10])           # the same object, rewritten in place
    c = S.stream_table(owner, origins[10:12], 76)             # another group size
    assert c is not a and tuple(c.shape) == (2, 2) and torch.equal(c, origins[10:12]) and torch.equal(a, origins[5:10])
    d = S.stream_table(owner, origins[0:5].to('meta'), 76)    # another device
    assert d is not a and d.device.type == 'meta' and tuple(d.shape) == (5, 2)
    assert set(owner._scene_tables) == {(5, 'cpu'), (2, 'cpu'), (5, 'meta')}
    # the owner was handed the cached buffer, already filled, and the scene's width -- each time
    assert [(call[1] is t, call[2]) for call, t in zip(owner.calls, (a, a, c, d))] == [(True, 76)] * 4
    assert torch.equal(owner.calls[0][3], origins[0:5]) and torch.equal(owner.calls[1][3], origins[5:10])
    assert S.stream_table(_Owner(), origins[0:5], 76) is not a    # the cache is the owner's


def _cpu_walk(monkeypatch, n=12):
    """S.walk over a one-row plan of n tiles of side 2 with CPU stand-ins for the two device pieces; -> (plan, origins, blended)."""
    import torch
    plan = S.TilePlan([(0, 2 * k) for k in range(n)], [(0, 0, 0, 0)] * n, 2, 2, 2 * n)
    blended = []
    monkeypatch.setattr(S, 'plan_tables', lambda plan, device: (torch.tensor(plan.origins, dtype=torch.int32, device=device),
                                                                torch.tensor(plan.ramps, dtype=torch.int32, device=device)))
    monkeypatch.setattr(S, 'blend', lambda tiles, origins, ramps, acc, wsum: blended.append((tiles, origins, ramps, acc, wsum)))
    return plan, torch.tensor(plan.origins, dtype=torch.int32), blended


def test_walk_groups_in_plan_order(monkeypatch):
    import torch
    plan, origins, blended = _cpu_walk(monkeypatch)
    seen, lines = [], []

    def sample_group(k0, k1, org):
        seen.append((k0, k1, org.clone()))
        return torch.full((k1 - k0, 3, 2, 2), float(k0))

    acc, wsum = S.walk(plan, 'cpu', 5, sample_group, log=lines.append)
    assert [(k0, k1) for k0, k1, _ in seen] == [(0, 5), (5, 10), (10, 12)]          # the last group smaller, not padded
    for k0, k1, org in seen:
        assert torch.equal(org, origins[k0:k1]), (k0, k1)
    assert tuple(acc.shape) == (3, 2, 24) and tuple(wsum.shape) == (2, 24) and acc.dtype == wsum.dtype == torch.float32
    assert not acc.any() and not wsum.any()                   # zeros for the blend to add into
    assert [tuple(t.shape) for t, *_ in blended] == [(5, 3, 2, 2), (5, 3, 2, 2), (2, 3, 2, 2)]
    for (tiles, org, ramps, a, w), (k0, k1, _) in zip(blended, seen):
        assert float(tiles[0, 0, 0, 0]) == k0 and torch.equal(org, origins[k0:k1]) and tuple(ramps.shape) == (k1 - k0, 4)
        assert a is acc and w is wsum
    assert lines == ['scene: tiles 1..5 of 12', 'scene: tiles 6..10 of 12', 'scene: tiles 11..12 of 12']
    # a lone image without its batch axis gets it back
    plan1, _, blended1 = _cpu_walk(monkeypatch, n=1)
    S.walk(plan1, 'cpu', 4, lambda k0, k1, org: torch.zeros(3, 2, 2))
    assert tuple(blended1[0][0].shape) == (1, 3, 2, 2)


def test_walk_counts_the_images(monkeypatch):
    import torch
    plan, _, blended = _cpu_walk(monkeypatch)
    with pytest.raises(RuntimeError, match=r'returned 4 image\(s\) for 5 tiles'):
        S.walk(plan, 'cpu', 5, lambda k0, k1, org: torch.zeros(k1 - k0 - 1, 3, 2, 2))
    assert blended == []


def test_walk_sets_and_clears_the_stream_table(monkeypatch):
    import torch
    plan, origins, _ = _cpu_walk(monkeypatch)
    owner = _Owner()
    S.walk(plan, 'cpu', 5, lambda k0, k1, org: torch.zeros(k1 - k0, 3, 2, 2), stream=owner)
    assert [c[0] for c in owner.calls] == ['set', 'set', 'set', 'clear']
    assert [c[2] for c in owner.calls[:3]] == [24] * 3        # the scene's width
    for call, (k0, k1) in zip(owner.calls, ((0, 5), (5, 10), (10, 12))):
        assert torch.equal(call[3], origins[k0:k1])
    assert owner.calls[0][1] is owner.calls[1][1] and owner.calls[2][1] is not owner.calls[0][1]
    # the table is cleared on the way out of a failed group too, and was set before that group ran
    owner = _Owner()

    def second_group_fails(k0, k1, org):
        if k0:
            raise KeyError('the sampler failed')
        return torch.zeros(k1 - k0, 3, 2, 2)

    with pytest.raises(KeyError):
        S.walk(plan, 'cpu', 5, second_group_fails, stream=owner)
    assert [c[0] for c in owner.calls] == ['set', 'set', 'clear']
    # without a stream owner nobody is asked anything (noise='scene' / 'tile')
    S.walk(plan, 'cpu', 5, lambda k0, k1, org: torch.zeros(k1 - k0, 3, 2, 2))


def test_check_request():
    for modes in (('scene', 'tile', 'stream'), ('stream', 'scene', 'tile')):
        for noise in modes:
            S.check_request(noise, 1, modes)
        with pytest.raises(ValueError, match="noise must be one of .*got 'field'"):
            S.check_request('field', 4, modes)
        with pytest.raises(ValueError, match='batch must be at least 1'):
            S.check_request(modes[0], 0, modes)
    with pytest.raises(ValueError, match="got 'stream'"):
        S.check_request('stream', 4, ('scene', 'tile'))          # the set of modes is the driver's


def test_new_entry_points_are_bound_and_declared():
    from fastdiffsr_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'fdsr.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
    # the header says what an origin outside the scene does
    assert 'address a counter, not memory' in txt
