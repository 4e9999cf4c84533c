"""TransENet without a GPU: the restatement against the reference's recorded fp32 run (tests/golden/transenet.npz, made by
tools/make_transenet_golden.py), the sensitivity of that comparison to nine wrong forms, the state_dict keys, the refusals of
the module and the host side of the C ABI (create, workspace_bytes, the envelope)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import transenet_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'transenet.npz')


def case(name):
    from fastdiffsr_amd.synth import synth_transenet
    _, _, batch, hw, with_taps, _ = R.CASES[name]
    cfg = R.case_config(name)
    keys = ['out'] + (R.recorded_taps(cfg) if with_taps else [])
    return cfg, synth_transenet(cfg, R.SEED), batch, hw, keys


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == R.SEED and sorted(g['cases'].tolist()) == sorted(R.GOLDEN_CASES)
    return g


@pytest.fixture(scope='module')
def fp64(golden):
    """name -> (x, taps of the fp64 restatement, e32 per tap): shared by the tests below.  e32 of a case outside the golden file
    is the restatement in fp32 against itself in fp64, at the output only."""
    out = {}
    for name in R.CASES:
        cfg, w, batch, hw, keys = case(name)
        x = R.case_input(name, batch, *hw)
        taps = R.transenet_forward(w, cfg, x, torch.float64)
        if name in R.GOLDEN_CASES:
            assert torch.equal(x, torch.from_numpy(golden[name + '/x']))
            e32 = {k: float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, taps[k])).max()) for k in keys}
        else:
            e32 = {'out': float((R.transenet_forward(w, cfg, x, torch.float32)['out'].double() - taps['out']).abs().max())}
        out[name] = (x, taps, e32)
    return out


def test_schema_of_the_full_configuration():
    """Key count and parameter total of the reference's network, counted from transenet.py by hand: 4 MeanShift tensors, 2 head,
    60 ResBlock, 10 for the five 1x1, 4 upsampler, 2 tail, 10 patch Linears; an encoder layer has 11 tensors (LN 2, to_qkv 1,
    to_out 2, LN 2, net 4), a decoder layer 18."""
    from fastdiffsr_amd.transenet.arch import TransENetConfig, state_schema
    s = state_schema(TransENetConfig())
    enc_layer, dec_layer = 2 + 1 + 2 + 2 + 4, (2 + 1 + 2) + (2 + 3 + 2) + (2 + 4)
    assert len(s) == 4 + 2 + 60 + 10 + 4 + 2 + 10 + 4 * 8 * enc_layer + 3 * dec_layer
    assert list(s)[:3] == ['sub_mean.weight', 'sub_mean.bias', 'head.0.weight']
    assert s['encoder_up.layers.3.0.fn.fn.to_qkv.weight'] == (576, 512) and 'encoder_up.layers.3.0.fn.fn.to_qkv.bias' not in s
    assert s['decoder2.layers.0.1.fn.fn.to_k.weight'] == (192, 512)
    assert s['patch_to_embedding_high.weight'] == (512, 1024) and s['embedding_to_patch.weight'] == (1024, 512)
    assert list(s)[-1] == 'decoder3.layers.0.2.fn.fn.net.3.bias'
    n = sum(int(np.prod(v)) for v in s.values())
    conv = 12 + 12 + (64 * 27 + 64) + 30 * (64 * 64 * 9 + 64) + 4 * (64 * 16 + 16) + (16 * 64 + 64) + 2 * (256 * 64 * 9 + 256) + (3 * 64 * 9 + 3)
    lin = 4 * (1024 * 512 + 512) + (512 * 1024 + 1024)
    attn, ff = 1024 + 576 * 512 + (192 * 512 + 512), 1024 + 2 * (512 * 512 + 512)
    cross = 1024 + 3 * 192 * 512 + (192 * 512 + 512)
    assert n == conv + lin + 32 * (attn + ff) + 3 * (attn + cross + ff) == PARAMS_FULL


PARAMS_FULL = 37458907        # sum(p.numel()) over the reference module's own state_dict


def test_restatement_matches_the_reference(fp64):
    """e32 = max |reference in fp32 - fp64 restatement| per case and tap: the reference's own arithmetic noise, a few 1e-5 on
    values of up to 50 (fp32 epsilon 6e-8 times 50, times the square root of a few thousand terms).  A restatement that differed
    from the reference in substance would be off by 1e-3 or more (the sensitivity test below), so 2e-4 separates the two."""
    for name, (x, taps, e32) in fp64.items():
        for k, e in e32.items():
            print('e32 %-14s %-26s %.3e  (max |x| %.2f)' % (name, k, e, float(taps[k].abs().max())))
            assert e < 2e-4, (name, k, e)
        cfg, _, batch, hw, _ = case(name)
        assert tuple(taps['out'].shape) == (batch, 3, hw[0] * cfg.scale, hw[1] * cfg.scale)


def test_fp32_restatement_is_within_its_own_noise_of_the_golden(fp64, golden):
    """The restatement in fp32 against the reference in fp32: both are fp32 sums of the same terms, so they differ by no more than
    each differs from fp64."""
    for name in ('s4_32x32', 's4_32x40'):
        cfg, w, batch, hw, keys = case(name)
        t32 = R.transenet_forward(w, cfg, fp64[name][0], torch.float32)
        for k in keys:
            d = float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, t32[k])).max())
            assert d <= 2 * fp64[name][2][k] + 1e-7, (name, k, d, fp64[name][2][k])


@pytest.mark.parametrize('broken', R.BROKEN)
def test_broken_restatements_move_the_output(fp64, broken):
    """Each wrong form moves the output by at least 100 e32 of its case: the 4 e32 tolerance of the GPU tests cannot hide one.
    Every form shows on every case here: channels = n_feats / 4 is 4 in the small configuration (patch_order needs more than
    one channel) and the three stages carry their own weights (decoder_order needs them distinct).  The full configuration is
    judged once, at 64x64."""
    judged = 0
    for name, (x, taps, e32) in fp64.items():
        if name == 'full_64x32_b2':
            continue
        cfg, w, _, _, _ = case(name)
        moved = float((R.transenet_forward(w, cfg, x, torch.float64, broken=broken)['out'] - taps['out']).abs().max())
        print('%-18s %-12s moves the output by %.3e = %.0f e32' % (broken, name, moved, moved / e32['out']))
        assert moved >= 100 * e32['out'], (broken, name, moved, e32['out'])
        judged += 1
    assert judged == len(R.CASES) - 1


def test_synthetic_weights_keep_activations_in_range(fp64):
    for name, (x, taps, _) in fp64.items():
        for k, t in taps.items():
            assert 0.1 < float(t.abs().max()) < 100, (name, k, float(t.abs().max()))


def test_mean_shifts_are_off_the_identity():
    from fastdiffsr_amd.synth import synth_transenet
    w = synth_transenet(R.case_config('s4_32x32'), R.SEED)
    for k in ('sub_mean.weight', 'add_mean.weight'):
        off = w[k].reshape(3, 3) - np.eye(3, dtype=np.float32)
        assert np.abs(off).max() > 0.05 and np.abs(off[~np.eye(3, dtype=bool)]).max() > 0.05, k


def small(**over):
    return dict(dict(R.SMALL, scale=4, hr_patch_size=128), **over)


def test_state_dict_round_trip_and_the_reference_s_lenient_load():
    from fastdiffsr_amd.synth import synth_transenet
    from fastdiffsr_amd.transenet import TransENet, state_schema
    m = TransENet(**small())
    keys = list(m.state_dict())
    assert keys == list(state_schema(m.cfg)) and 'upsampler.2.weight' in keys and 'upsampler.4.weight' not in keys
    sd = {k: torch.from_numpy(v) for k, v in synth_transenet(m.cfg, 3).items()}
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert len(TransENet(**small(scale=8, hr_patch_size=256)).state_dict()) == len(keys) + 2
    assert len(TransENet(**small(scale=3, hr_patch_size=96)).state_dict()) == len(keys) - 2
    # the reference's rule: a wrong shape under `tail` is skipped, anywhere else it is an error; unknown keys pass unless strict
    m2 = TransENet(**small())
    m2.load_reference_state_dict(dict(sd, **{'tail.weight': torch.zeros(1, 16, 3, 3), 'extra': torch.zeros(1)}))
    assert torch.equal(m2.state_dict()['head.0.weight'], sd['head.0.weight']) and not m2.state_dict()['tail.weight'].any()
    with pytest.raises(RuntimeError, match='head.0.weight'):
        m2.load_reference_state_dict(dict(sd, **{'head.0.weight': torch.zeros(16, 1, 3, 3)}))
    with pytest.raises(KeyError, match='unexpected'):
        m2.load_reference_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)
    with pytest.raises(KeyError, match='missing'):
        m2.load_reference_state_dict({k: v for k, v in sd.items() if k != 'add_mean.bias'}, strict=True)


def test_constructor_takes_the_reference_s_arguments_and_refuses_what_it_refuses():
    from fastdiffsr_amd.transenet import TransENet
    m = TransENet(n_feats=64, scale=4, n_basic_modules=10, n_colors=3, hr_patch_size=256, back_projection_iters=10, en_depth=8, de_depth=1,
                  conv=None)
    assert (m.cfg.n_feats, m.cfg.channels, m.cfg.patch_dim, m.cfg.en_depth, m.cfg.de_depth) == (64, 16, 1024, 8, 1)
    assert TransENet().cfg == m.cfg
    for kw in (dict(n_colors=1), dict(scale=5), dict(n_feats=24), dict(n_feats=272), dict(en_depth=0), dict(de_depth=0), dict(en_depth=33),
               dict(conv=torch.nn.Conv2d)):
        with pytest.raises(NotImplementedError):
            TransENet(**small(**kw))
    # the reference's two assertions: the LR side is a multiple of the patch, and more than 12 patches (an LR side of 32 at least)
    for kw in (dict(hr_patch_size=100), dict(hr_patch_size=96), dict(hr_patch_size=130)):
        with pytest.raises(ValueError):
            TransENet(**small(**kw))


def test_forward_refuses_the_shapes_the_reference_cannot_compute():
    from fastdiffsr_amd.transenet import TransENet
    m = TransENet(**small())
    with pytest.raises(ValueError, match='hr_patch_size // p'):       # names the reference's line
        m(torch.zeros(1, 3, 40, 32))
    with pytest.raises(ValueError, match='hr_patch_size'):
        m.debug_tensor('head', torch.zeros(1, 3, 64, 32))
    with pytest.raises(ValueError, match='multiples of the patch size 8'):
        m(torch.zeros(1, 3, 32, 36))
    with pytest.raises(ValueError, match='multiples of the patch size 8'):
        m(torch.zeros(1, 3, 36, 32))
    with pytest.raises(ValueError, match='no CPU path'):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 32, 32))


def test_create_and_workspace_bytes_need_no_gpu():
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.transenet import TransENet
    lib = _lib.load()
    m = TransENet(**small())
    b1, b2, b3 = m.workspace_bytes(1, 32, 32), m.workspace_bytes(2, 32, 32), m.workspace_bytes(1, 32, 40)
    assert 0 < b1 < b2 and b1 < b3 < b2
    # the largest tensors are the upsampler's: n_feats channels at 16 times the pixels, twice (its input at half the size aside)
    assert b1 >= 4 * 16 * 16 * 32 * 32
    # the engine takes its geometry from the input: any multiples of 8
    assert m.workspace_bytes(1, 8, 8) > 0 and m.workspace_bytes(1, 128, 128) > b2
    for h, w in ((32, 36), (36, 32), (4, 8)):
        with pytest.raises(_lib.FdsrError, match='multiples of 8'):
            m.workspace_bytes(1, h, w)
    with pytest.raises(_lib.FdsrError):
        m.workspace_bytes(0, 32, 32)

    def create(**over):
        c = _lib.FdsrTransenetConfig()
        c.n_feats, c.scale, c.n_colors, c.en_depth, c.de_depth = 16, 4, 3, 2, 1
        for k, v in over.items():
            setattr(c, k, v)
        h = C.c_void_p()
        rc = lib.fdsr_transenet_create(C.byref(c), C.byref(h))
        if rc == 0:
            lib.fdsr_transenet_destroy(h)
        return rc, (lib.fdsr_last_error(None) or b'').decode()

    assert create()[0] == 0
    assert create(n_feats=256, scale=8, en_depth=32, de_depth=32)[0] == 0
    for over, word in ((dict(n_colors=1), 'n_colors'), (dict(n_feats=24), 'n_feats'), (dict(n_feats=0), 'n_feats'), (dict(n_feats=272), 'n_feats'),
                       (dict(scale=5), 'scale'), (dict(scale=1), 'scale'), (dict(en_depth=0), 'en_depth'), (dict(en_depth=33), 'en_depth'),
                       (dict(de_depth=0), 'de_depth'), (dict(de_depth=33), 'de_depth')):
        rc, msg = create(**over)
        assert rc == -1 and word in msg, (over, rc, msg)          # FDSR_E_INVALID, with a message
