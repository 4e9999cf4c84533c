"""fastdiffsr_amd.scene without a GPU: the tile plan (coverage, origins, ramps), the blend weights it implies restated in fp64, the
refusals and the CLI's argument rules."""
import math

import numpy as np
import pytest

from fastdiffsr_amd import scene as S

TILE = 32        # the sweep: L = tile .. 3 tile + 7, overlap in {0, 1, 8, tile // 2}


def _axis_of(plan, axis):
    """(origins, leading ramps, trailing ramps) of the plan's tiles along `axis` (0: rows, 1: columns), from the 2-D tables."""
    seen = {}
    for (y0, x0), (top, left, bottom, right) in zip(plan.origins, plan.ramps):
        o, lead, trail = (y0, top, bottom) if axis == 0 else (x0, left, right)
        assert seen.setdefault(o, (lead, trail)) == (lead, trail)      # a column of tiles shares its ramps
    org = sorted(seen)
    return org, [seen[o][0] for o in org], [seen[o][1] for o in org]


def _w1(tile, lead, trail):
    """The 1-D weight of the issue's rule, fp64: (i + 1) / (r + 1) on a leading ramp, (r - i) / (r + 1) on a trailing one."""
    w = np.ones(tile, dtype=np.float64)
    for i in range(lead):
        w[i] *= (i + 1) / (lead + 1)
    for i in range(trail):
        w[tile - trail + i] *= (trail - i) / (trail + 1)
    return w


def weight_maps(plan):
    """[n, tile, tile] fp64 weights of the plan's tiles."""
    return np.stack([np.outer(_w1(plan.tile, top, bottom), _w1(plan.tile, left, right)) for top, left, bottom, right in plan.ramps])


@pytest.mark.parametrize('overlap', [0, 1, 8, TILE // 2])
def test_plan_sweep_one_axis(overlap):
    """L = tile .. 3 tile + 7 along the rows (the columns: one tile): coverage, origins, ramps, the issue's origin formula."""
    for L in range(TILE, 3 * TILE + 8):
        plan = S.plan_tiles(L, TILE, TILE, overlap)
        org, lead, trail = _axis_of(plan, 0)
        stride = TILE - overlap
        assert org == sorted(set(min(k * stride, L - TILE) for k in range(math.ceil((L - TILE) / stride) + 1))), (L, overlap)
        assert [o for o, _ in plan.origins] == org                 # row-major, non-decreasing
        assert org[0] == 0 and org[-1] + TILE == L                 # the last tile ends at the border, nothing is padded
        cover = np.zeros(L, dtype=int)
        for o in org:
            cover[o:o + TILE] += 1
        assert cover.min() >= 1 and cover.max() <= 3, (L, overlap)
        assert lead[0] == 0 and trail[-1] == 0                     # scene borders carry full weight
        for k in range(1, len(org)):
            r = org[k - 1] + TILE - org[k]                         # the overlap with the neighbour
            assert lead[k] == r == trail[k - 1] and 0 <= r < TILE, (L, overlap, k)
            if k < len(org) - 1:
                assert r == overlap                                # only the shifted last tile overlaps by more
            else:
                assert r >= overlap
        if len(org) == 1:
            assert plan.ramps == [(0, 0, 0, 0)]                    # a single tile has no ramp
        xo, xl, xt = _axis_of(plan, 1)
        assert xo == [0] and xl == [0] and xt == [0]


def test_single_tile_has_weight_one():
    plan = S.plan_tiles(TILE, TILE, TILE, 8)
    assert plan.origins == [(0, 0)] and plan.ramps == [(0, 0, 0, 0)]
    assert (weight_maps(plan) == 1.0).all()


@pytest.mark.parametrize('overlap', [0, 1, 8, TILE // 2])
def test_weight_sums(overlap):
    """The 2-D weight sum of every scene of the sweep (H = L, W = the sweep's L mirrored, so both axes see every length): at least
    WSUM_MIN everywhere, and 1 to 1e-15 wherever at most two tiles overlap per axis."""
    assert S.WSUM_MIN > 0
    lengths = list(range(TILE, 3 * TILE + 8))
    for L in lengths:
        M = lengths[len(lengths) - 1 - lengths.index(L)]
        plan = S.plan_tiles(L, M, TILE, overlap)
        w = weight_maps(plan)
        total = np.zeros((L, M))
        rows, cols = np.zeros(L, dtype=int), np.zeros(M, dtype=int)
        for (y0, x0), wk in zip(plan.origins, w):
            total[y0:y0 + TILE, x0:x0 + TILE] += wk
        for o in _axis_of(plan, 0)[0]:
            rows[o:o + TILE] += 1
        for o in _axis_of(plan, 1)[0]:
            cols[o:o + TILE] += 1
        assert rows.min() >= 1 and cols.min() >= 1                  # every pixel is covered
        assert total.min() >= S.WSUM_MIN - 1e-15, (L, M, overlap, total.min())
        two = np.outer(rows <= 2, cols <= 2)
        assert np.abs(total[two] - 1.0).max() <= 1e-15, (L, M, overlap)


def test_refusals():
    with pytest.raises(ValueError, match='largest usable tile is 24'):
        S.plan_tiles(31, 40, 32, 8, multiple=8)                     # scene smaller than the tile: names what would fit
    with pytest.raises(ValueError, match='largest usable tile is 31'):
        S.plan_tiles(40, 31, 32, 8)
    with pytest.raises(ValueError, match=r'overlap must lie in \[0, tile // 2\] = \[0, 16\]'):
        S.plan_tiles(64, 64, 32, 17)
    with pytest.raises(ValueError, match='overlap'):
        S.plan_tiles(64, 64, 32, -1)
    S.plan_tiles(64, 64, 32, 16)
    # the noise field of noise='scene': [P,3,SH,SW] fp32 against the byte budget
    assert S.noise_field_bytes(20, 4096, 4096) == 20 * 3 * 4096 * 4096 * 4
    assert S.check_noise_budget(20, 4096, 4096) == 20 * 3 * 4096 * 4096 * 4          # 3.75 GiB: inside the default 16 GiB
    with pytest.raises(ValueError, match=r"noise='tile'") as e:
        S.check_noise_budget(1001, 4096, 4096)                      # SR3's T + 1 planes: 188 GiB
    assert str(1001 * 3 * 4096 * 4096 * 4) in str(e.value) and 'GiB' in str(e.value)
    with pytest.raises(ValueError, match=r"noise='tile'"):
        S.check_noise_budget(20, 64, 64, budget=20 * 3 * 64 * 64 * 4 - 1)
    S.check_noise_budget(20, 64, 64, budget=20 * 3 * 64 * 64 * 4)


def test_tile_keys_differ():
    keys = {S._tile_key(s, i) for s in range(4) for i in range(64)}
    assert len(keys) == 4 * 64 and all(0 <= k < 2 ** 63 for k in keys)


def test_cli_arguments(capsys):
    a = S.parse_args(['-c', 'cfg.json', '--lr', 'in.png', '--scale', '4', '-o', 'out.tif'])
    assert (a.lr, a.sr, a.scale, a.out) == ('in.png', None, 4, 'out.tif')
    assert (a.tile, a.overlap, a.batch, a.seed, a.noise, a.rng, a.precision) == (256, 32, 16, 0, 'scene', None, 'f16x3')
    a = S.parse_args(['-c', 'cfg.json', '--sr', 'in.png', '-o', 'out.png', '--noise', 'tile', '--tile', '128', '--seed', '7'])
    assert (a.lr, a.sr, a.noise, a.tile, a.seed) == (None, 'in.png', 'tile', 128, 7)
    for argv in (['-c', 'c', '--lr', 'in.png', '-o', 'o.png'],                                   # --lr requires --scale
                 ['-c', 'c', '--lr', 'a.png', '--scale', '4', '--sr', 'b.png', '-o', 'o.png'],    # mutually exclusive
                 ['-c', 'c', '-o', 'o.png'],                                                      # one of them is required
                 ['-c', 'c', '--sr', 'b.png', '--scale', '4', '-o', 'o.png']):
        with pytest.raises(SystemExit) as e:
            S.parse_args(argv)
        assert e.value.code == 2
    err = capsys.readouterr().err
    assert '--lr requires --scale' in err and 'not allowed with argument' in err


def test_tiles_per_call_follows_what_a_facade_returns():
    """tesr and gdp return ret_img[-1], the last image of a batch: one tile per call.  The flagship and SR3 return the batch."""
    import types
    from fastdiffsr_amd import diffusion as flagship
    from fastdiffsr_amd.gdp import diffusion as gdp
    from fastdiffsr_amd.sr3 import diffusion as sr3
    from fastdiffsr_amd.tesr import diffusion as tesr
    for mod, want in ((flagship, 16), (sr3, 16), (tesr, 1), (gdp, 1)):
        cls = mod.GaussianDiffusion
        facade = types.SimpleNamespace(_result=lambda img, cls=cls: cls._result(None, img))
        assert S.tiles_per_call(facade, 16) == want, mod.__name__
