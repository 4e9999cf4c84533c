"""SwinIR without a GPU: the fp64 restatement against the reference's recorded fp32 run (tests/golden/swinir.npz, made by
tools/make_swinir_golden.py), the sensitivity of that comparison to a wrong mask / bias index / roll / GELU form, the
state_dict keys, and the host side of the C ABI (create, workspace_bytes, the envelope)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import swinir_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'swinir.npz')


def case(name):
    from fastdiffsr_amd.swinir.arch import SwinIRConfig, tap_names
    from fastdiffsr_amd.synth import synth_swinir
    base, upscale, hw, with_taps = R.CASES[name]
    cfg = SwinIRConfig(upscale=upscale, **base)
    keys = ['out'] + (R.recorded_taps(tap_names(cfg)) if with_taps else [])
    return cfg, synth_swinir(cfg, R.SEED), hw, keys


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == R.SEED and sorted(g['cases'].tolist()) == sorted(R.CASES)
    return g


@pytest.fixture(scope='module')
def fp64(golden):
    """name -> (taps of the fp64 restatement, e32 per tap): shared by the tests below."""
    out = {}
    for name in R.CASES:
        cfg, w, hw, keys = case(name)
        x = torch.from_numpy(golden[name + '/x'])
        assert torch.equal(x, R.case_input(name, 1, *hw))
        taps = R.swinir_forward(w, cfg, x, torch.float64)
        out[name] = (taps, {k: float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, taps[k])).max()) for k in keys})
    return out


def test_fp64_restatement_matches_the_reference(golden, fp64):
    """e32 = max |reference in fp32 - fp64 restatement| per case and tap: the reference's own arithmetic noise, a few 1e-6 on
    values of a few units.  A restatement that differed from the reference in substance would be off by 1e-3 or more (the
    sensitivity test below), so 1e-4 separates the two by a wide margin on both sides."""
    for name, (taps, e32) in fp64.items():
        for k, e in e32.items():
            print('e32 %-12s %-26s %.3e  (max |x| %.2f)' % (name, k, e, float(taps[k].abs().max())))
            assert e < 1e-4, (name, k, e)
        cfg, _, hw, _ = case(name)
        assert tuple(taps['out'].shape) == (1, 3, hw[0] * cfg.upscale, hw[1] * cfg.upscale)


@pytest.mark.parametrize('broken', R.BROKEN)
def test_broken_restatements_move_the_output(golden, fp64, broken):
    """Each wrong form moves the output by at least 100 e32 of its case: the 4 e32 tolerance of the GPU tests cannot hide one.
    The one pair left out is no wrong form: with a single 8-wide window per axis the roll by +4 IS the roll by -4 (the same
    permutation mod 8), so 'roll_reversed' is the identity on the 8x8 cases and is judged on the three larger ones."""
    judged = 0
    for name, (taps, e32) in fp64.items():
        cfg, w, hw, _ = case(name)
        if broken == 'roll_reversed' and hw == (8, 8):
            continue
        moved = float((R.swinir_forward(w, cfg, torch.from_numpy(golden[name + '/x']), torch.float64, broken=broken)['out']
                       - taps['out']).abs().max())
        print('%-16s %-12s moves the output by %.3e = %.0f e32' % (broken, name, moved, moved / e32['out']))
        assert moved >= 100 * e32['out'], (broken, name, moved, e32['out'])
        judged += 1
    assert judged >= 3


def test_synthetic_weights_keep_activations_in_range(fp64):
    """O(1) through all 36 blocks of the full configuration, and at every recorded tap of the small one."""
    for name, (taps, _) in fp64.items():
        for k, t in taps.items():
            assert 0.1 < float(t.abs().max()) < 50, (name, k, float(t.abs().max()))


def reference_keys(cfg):
    """The reference's state_dict key set, rebuilt from param_schema and the two buffer kinds."""
    from fastdiffsr_amd.swinir.arch import param_schema
    keys = set(param_schema(cfg))
    for i, depth in enumerate(cfg.depths):
        for j in range(depth):
            b = 'layers.%d.residual_group.blocks.%d' % (i, j)
            keys.add(b + '.attn.relative_position_index')
            if j % 2:
                keys.add(b + '.attn_mask')
    return keys


def test_state_dict_round_trip():
    from fastdiffsr_amd.swinir import SwinIR
    from fastdiffsr_amd.swinir.arch import attn_mask, relative_position_index
    from fastdiffsr_amd.synth import synth_swinir
    kw = dict(R.SMALL, upscale=4, in_chans=3, img_range=1., upsampler='pixelshuffle', resi_connection='1conv')
    m = SwinIR(**kw)
    assert set(m.state_dict()) == reference_keys(m.cfg)
    sd = {k: torch.from_numpy(v) for k, v in synth_swinir(m.cfg, 3).items()}
    for k in reference_keys(m.cfg) - set(sd):
        sd[k] = (torch.from_numpy(relative_position_index(8)) if k.endswith('index') else torch.from_numpy(attn_mask(64, 64, 8, 4)))
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # a checkpoint trained at another img_size carries attn_mask buffers of another size: accepted, never used
    other = dict(sd)
    for k in other:
        if k.endswith('.attn_mask'):
            other[k] = torch.from_numpy(attn_mask(48, 48, 8, 4))
    SwinIR(**kw).load_state_dict(other, strict=True)
    # a buffer that contradicts the geometry is refused, as are a missing and an unknown key
    bad = dict(sd)
    bad['layers.0.residual_group.blocks.1.attn.relative_position_index'] = torch.from_numpy(relative_position_index(8).T.copy())
    with pytest.raises(RuntimeError, match='geometry'):
        SwinIR(**kw).load_state_dict(bad, strict=True)
    with pytest.raises(RuntimeError, match='Missing'):
        SwinIR(**kw).load_state_dict({k: v for k, v in sd.items() if k != 'norm.weight'}, strict=True)
    with pytest.raises(RuntimeError, match='Unexpected'):
        SwinIR(**kw).load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)


@pytest.mark.parametrize('kw', [dict(upsampler='pixelshuffledirect'), dict(upsampler='nearest+conv'), dict(upsampler=''),
                                dict(resi_connection='3conv'), dict(patch_size=2), dict(ape=True), dict(in_chans=1), dict(window_size=7),
                                dict(upscale=5), dict(img_size=8), dict(embed_dim=36, num_heads=[5, 5]), dict(embed_dim=132, num_heads=[4, 4])])
def test_out_of_envelope_arguments_are_refused(kw):
    from fastdiffsr_amd.swinir import SwinIR
    with pytest.raises(NotImplementedError):
        SwinIR(**dict(dict(R.SMALL, upscale=4), **kw))


def test_create_and_workspace_bytes_need_no_gpu():
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.swinir import SwinIR
    lib = _lib.load()
    m = SwinIR(**dict(R.SMALL, upscale=4))
    b1, b2, b3 = m.workspace_bytes(1, 8, 8), m.workspace_bytes(2, 8, 8), m.workspace_bytes(1, 12, 20)
    assert 0 < b1 < b2 and b3 == m.workspace_bytes(1, 16, 24) > b1
    # the largest tensor is the last pixel shuffle's: 64 channels at 16 times the padded pixels
    assert b1 >= 4 * 64 * 16 * 64
    # an input too small to reflect-pad (F.pad's rule: pad < size) is refused on the host; 5 -> 8 pads by 3 < 5
    for h, w in ((4, 8), (8, 3), (9, 4)):
        with pytest.raises(_lib.FdsrError, match='reflect'):
            m.workspace_bytes(1, h, w)
    assert m.workspace_bytes(1, 5, 8) == b1
    with pytest.raises(_lib.FdsrError):
        m.workspace_bytes(0, 8, 8)

    def create(**over):
        c = _lib.FdsrSwinirConfig()
        c.embed_dim, c.n_layers, c.window_size, c.mlp_hidden, c.upscale, c.patch_norm, c.img_range = 36, 2, 8, 72, 4, 1, 1.0
        c.depths[0] = c.depths[1] = 2
        c.num_heads[0] = c.num_heads[1] = 6
        for k, v in over.items():
            if k in ('depths', 'num_heads'):
                getattr(c, k)[0] = v
            else:
                setattr(c, k, v)
        h = C.c_void_p()
        rc = lib.fdsr_swinir_create(C.byref(c), C.byref(h))
        if rc == 0:
            lib.fdsr_swinir_destroy(h)
        return rc, (lib.fdsr_last_error(None) or b'').decode()

    assert create()[0] == 0
    for over, word in ((dict(window_size=7), 'window_size'), (dict(num_heads=5), 'heads'), (dict(embed_dim=66, num_heads=2), 'head_dim'),
                       (dict(upscale=5), 'upscale'), (dict(n_layers=9), 'layers'), (dict(n_layers=0), 'layers'), (dict(depths=0), 'depth'),
                       (dict(embed_dim=516), 'embed_dim'), (dict(img_range=0.0), 'img_range')):
        rc, msg = create(**over)
        assert rc == -1 and word in msg, (over, rc, msg)          # FDSR_E_INVALID, with a message
