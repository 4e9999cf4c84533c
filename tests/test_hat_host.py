"""HAT without a GPU: the fp64 restatement against the reference's recorded fp32 run (tests/golden/hat.npz, made by
tools/make_hat_golden.py), the sensitivity of that comparison to ten wrong forms, the state_dict keys (the two index buffers,
the aliased upsampling keys), and the host side of the C ABI (create, workspace_bytes, the envelope)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hat_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hat.npz')


def case(name):
    from fastdiffsr_amd.hat.arch import HATConfig, tap_names
    from fastdiffsr_amd.synth import synth_hat
    base, upscale, hw, with_taps, _ = R.CASES[name]
    cfg = HATConfig(upscale=upscale, **base)
    keys = ['out'] + (R.recorded_taps(tap_names(cfg)) if with_taps else [])
    return cfg, synth_hat(cfg, R.SEED), hw, keys


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == R.SEED and sorted(g['cases'].tolist()) == sorted(R.GOLDEN_CASES)
    return g


@pytest.fixture(scope='module')
def fp64(golden):
    """name -> (x, taps of the fp64 restatement, e32 per tap): shared by the tests below.  e32 of a case outside the golden file
    (s8_16x16) is the restatement in fp32 against itself in fp64, at the output only."""
    out = {}
    for name in R.CASES:
        cfg, w, hw, keys = case(name)
        x = R.case_input(name, 1, *hw)
        taps = R.hat_forward(w, cfg, x, torch.float64)
        if name in R.GOLDEN_CASES:
            assert torch.equal(x, torch.from_numpy(golden[name + '/x']))
            e32 = {k: float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, taps[k])).max()) for k in keys}
        else:
            e32 = {'out': float((R.hat_forward(w, cfg, x, torch.float32)['out'].double() - taps['out']).abs().max())}
        out[name] = (x, taps, e32)
    return out


def test_fp64_restatement_matches_the_reference(fp64):
    """e32 = max |reference in fp32 - fp64 restatement| per case and tap: the reference's own arithmetic noise, around 1e-5 on
    values of a few units.  A restatement that differed from the reference in substance would be off by 1e-3 or more (the
    sensitivity test below), so 1e-4 separates the two."""
    for name, (x, taps, e32) in fp64.items():
        for k, e in e32.items():
            print('e32 %-12s %-26s %.3e  (max |x| %.2f)' % (name, k, e, float(taps[k].abs().max())))
            assert e < 1e-4, (name, k, e)
        cfg, _, hw, _ = case(name)
        # not cropped: the padded size times the scale
        assert tuple(taps['out'].shape) == (1, 3, -(-hw[0] // 16) * 16 * cfg.upscale, -(-hw[1] // 16) * 16 * cfg.upscale)
    assert tuple(fp64['s4_20x36'][1]['out'].shape) == (1, 3, 128, 192)


@pytest.mark.parametrize('broken', R.BROKEN)
def test_broken_restatements_move_the_output(fp64, broken):
    """Each wrong form moves the output by at least 100 e32 of its case: the 4 e32 tolerance of the GPU tests cannot hide one.
    Two forms are no wrong form on some cases and are not judged there: with a single 16-wide window per axis the roll by +8
    IS the roll by -8 (the same permutation mod 16), so 'roll_reversed' is judged on the three inputs of more than one window;
    and 'pool_unpadded' differs from the reference only where the input is padded, the 20x36 case."""
    judged = 0
    for name, (x, taps, e32) in fp64.items():
        cfg, w, hw, _ = case(name)
        if broken == 'roll_reversed' and max(hw) <= 16:
            continue
        if broken == 'pool_unpadded' and hw[0] % 16 == 0 and hw[1] % 16 == 0:
            continue
        moved = float((R.hat_forward(w, cfg, x, torch.float64, broken=broken)['out'] - taps['out']).abs().max())
        print('%-18s %-12s moves the output by %.3e = %.0f e32' % (broken, name, moved, moved / e32['out']))
        assert moved >= 100 * e32['out'], (broken, name, moved, e32['out'])
        judged += 1
    assert judged >= (1 if broken == 'pool_unpadded' else 3)


def test_synthetic_weights_keep_activations_in_range(fp64):
    """O(1) through all 36 HABs and 6 OCABs of the full configuration, and at every tap of the small one."""
    for name, (x, taps, _) in fp64.items():
        for k, t in taps.items():
            assert 0.1 < float(t.abs().max()) < 50, (name, k, float(t.abs().max()))


def test_oca_bias_index_wraps_round_the_table():
    from fastdiffsr_amd.hat.arch import oca_table_rows, relative_position_index_oca
    idx = relative_position_index_oca(16, 24)
    assert idx.shape == (256, 576) and idx.min() == -880 and idx.max() == 640
    rows = oca_table_rows(16, 24)
    assert rows.min() == 0 and rows.max() == 1520 and len(np.unique(rows)) == 1521
    t = torch.arange(1521)
    assert torch.equal(t[torch.from_numpy(idx).reshape(-1)], torch.from_numpy(rows).reshape(-1))     # what PyTorch indexing does


def small(**over):
    return dict(dict(R.SMALL, upscale=4), **over)


def full_state(m, seed=3):
    """A checkpoint as the reference saves it: every key of the schema, buffers and aliased keys included."""
    from fastdiffsr_amd.hat.arch import alias_of, buffer_value, is_buffer
    from fastdiffsr_amd.synth import synth_hat
    w = synth_hat(m.cfg, seed)
    return {k: torch.from_numpy(buffer_value(m.cfg, k) if is_buffer(k) else w[alias_of(k)]) for k in m.schema}


def test_state_dict_round_trip():
    from fastdiffsr_amd.hat import HAT
    m = HAT(**small())
    keys = list(m.state_dict())
    assert keys[:3] == ['relative_position_index_SA', 'relative_position_index_OCA', 'conv_first.weight']
    assert [k for k in keys if k.startswith('upsample.')] == ['upsample.upsampling.0.weight', 'upsample.upsampling.0.bias',
                                                              'upsample.upsampling.2.weight', 'upsample.upsampling.2.bias']
    assert 'layers.1.residual_group.overlap_attn.relative_position_bias_table' in keys
    assert tuple(m.state_dict()['layers.0.residual_group.blocks.1.conv_block.cab.3.attention.1.weight'].shape) == (3, 36, 1, 1)
    sd = full_state(m)
    assert list(sd) == keys
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert back['upsample.upsampling.2.weight'].data_ptr() == back['upsample.upsampling.0.weight'].data_ptr()
    assert len(HAT(**small(upscale=8)).state_dict()) == len(keys) + 2 and len(HAT(**small(upscale=3)).state_dict()) == len(keys) - 2
    # a buffer that contradicts the geometry, unequal copies of the shared convolution, a missing and an unknown key are refused
    for key in ('relative_position_index_SA', 'relative_position_index_OCA'):
        with pytest.raises(RuntimeError, match='geometry'):
            HAT(**small()).load_state_dict(dict(sd, **{key: sd[key] + 1}), strict=True)
    with pytest.raises(RuntimeError, match='shared convolution'):
        HAT(**small()).load_state_dict(dict(sd, **{'upsample.upsampling.2.bias': sd['upsample.upsampling.2.bias'] + 1}), strict=True)
    with pytest.raises(RuntimeError, match='Missing'):
        HAT(**small()).load_state_dict({k: v for k, v in sd.items() if k != 'norm.weight'}, strict=True)
    with pytest.raises(RuntimeError, match='Unexpected'):
        HAT(**small()).load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)


def test_the_defaults_are_the_reference_s():
    from fastdiffsr_amd.hat import HAT
    from fastdiffsr_amd.hat.arch import param_schema
    m = HAT(upscale=4, img_size=64)
    c = m.cfg
    assert (c.embed_dim, c.depths, c.num_heads, c.window_size, c.mlp_hidden) == (180, [6] * 6, [6] * 6, 16, 720)
    assert (c.compress_ratio, c.squeeze_factor, c.conv_scale, c.overlap_win_size) == (3, 30, 0.01, 24)
    assert HAT().cfg.upscale == 2
    n = sum(int(np.prod(s)) for s in param_schema(c).values())
    assert abs(n / 1e6 - 26.08) < 0.01, n


@pytest.mark.parametrize('kw', [dict(upsampler='pixelshuffledirect'), dict(upsampler=''), dict(resi_connection='identity'), dict(patch_size=2),
                                dict(ape=True), dict(in_chans=1), dict(window_size=8), dict(overlap_ratio=0.25), dict(upscale=5),
                                dict(img_size=16), dict(embed_dim=36, num_heads=[5, 5]), dict(embed_dim=132, num_heads=[4, 4]),
                                dict(embed_dim=528, num_heads=[24, 24]), dict(compress_ratio=5), dict(squeeze_factor=37),
                                dict(depths=[1] * 9, num_heads=[6] * 9), dict(qkv_bias=False), dict(qk_scale=0.5)])
def test_out_of_envelope_arguments_are_refused(kw):
    from fastdiffsr_amd.hat import HAT
    with pytest.raises(NotImplementedError):
        HAT(**small(**kw))


def test_create_and_workspace_bytes_need_no_gpu():
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.hat import HAT
    lib = _lib.load()
    m = HAT(**small())
    b1, b2, b3 = m.workspace_bytes(1, 16, 16), m.workspace_bytes(2, 16, 16), m.workspace_bytes(1, 20, 36)
    assert 0 < b1 < b2 and b3 == m.workspace_bytes(1, 32, 48) > b1
    # the largest tensor is the last pixel shuffle's: 64 channels at 16 times the padded pixels
    assert b1 >= 4 * 64 * 16 * 256
    # an input too small to reflect-pad (F.pad's rule: pad < size) is refused on the host; 9 -> 16 pads by 7 < 9
    for h, w in ((8, 16), (16, 8), (17, 8)):
        with pytest.raises(_lib.FdsrError, match='reflect'):
            m.workspace_bytes(1, h, w)
    assert m.workspace_bytes(1, 9, 16) == b1
    with pytest.raises(_lib.FdsrError):
        m.workspace_bytes(0, 16, 16)

    def create(**over):
        c = _lib.FdsrHatConfig()
        c.embed_dim, c.n_layers, c.window_size, c.mlp_hidden, c.upscale, c.patch_norm, c.img_range = 36, 2, 16, 144, 4, 1, 1.0
        c.compress_ratio, c.squeeze_factor, c.conv_scale, c.overlap_win_size = 3, 12, 0.01, 24
        c.depths[0] = c.depths[1] = 2
        c.num_heads[0] = c.num_heads[1] = 6
        for k, v in over.items():
            if k in ('depths', 'num_heads'):
                getattr(c, k)[0] = v
            else:
                setattr(c, k, v)
        h = C.c_void_p()
        rc = lib.fdsr_hat_create(C.byref(c), C.byref(h))
        if rc == 0:
            lib.fdsr_hat_destroy(h)
        return rc, (lib.fdsr_last_error(None) or b'').decode()

    assert create()[0] == 0
    for over, word in ((dict(window_size=8), 'window_size'), (dict(overlap_win_size=20), 'overlap'), (dict(num_heads=5), 'heads'),
                       (dict(embed_dim=66, num_heads=2), 'head_dim'), (dict(upscale=5), 'upscale'), (dict(n_layers=9), 'layers'),
                       (dict(n_layers=0), 'layers'), (dict(depths=0), 'depth'), (dict(embed_dim=516), 'embed_dim'),
                       (dict(compress_ratio=5), 'compress_ratio'), (dict(squeeze_factor=37), 'squeeze_factor'),
                       (dict(squeeze_factor=0), 'squeeze_factor'), (dict(img_range=0.0), 'img_range')):
        rc, msg = create(**over)
        assert rc == -1 and word in msg, (over, rc, msg)          # FDSR_E_INVALID, with a message
