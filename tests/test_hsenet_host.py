"""HSENet without a GPU: the restatement against the reference's recorded fp32 run (tests/golden/hsenet.npz, made by
tools/make_hsenet_golden.py), the sensitivity of that comparison to eleven wrong forms, the softmax conditions under which the
tests mean something, the two interpolation rules, the state_dict keys, the loading rule and the host side of the C ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hsenet_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hsenet.npz')
TAPPED = [k for k, v in R.CASES.items() if v[5]]


def case(name):
    _, _, _, batch, hw, with_taps, _ = R.CASES[name]
    cfg = R.case_config(name)
    keys = ['out'] + (R.recorded_taps(cfg) if with_taps else [])
    return cfg, R.case_weights(name), batch, hw, keys


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    assert int(g['seed']) == R.SEED and sorted(g['cases'].tolist()) == sorted(R.GOLDEN_CASES)
    return g


@pytest.fixture(scope='module')
def fp64(golden):
    """name -> (x, taps of the fp64 restatement, e32 per tap, the attention calls' statistics): shared by the tests below.  e32
    of a case outside the golden file is the restatement in fp32 against itself in fp64, at the output only."""
    out = {}
    for name in R.CASES:
        cfg, w, batch, hw, keys = case(name)
        x = R.case_input(name, batch, *hw)
        stats = []
        taps = R.hsenet_forward(w, cfg, x, torch.float64, stats=stats)
        if name in R.GOLDEN_CASES:
            assert torch.equal(x, torch.from_numpy(golden[name + '/x']))
            e32 = {k: float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, taps[k])).max()) for k in keys}
        else:
            e32 = {'out': float((R.hsenet_forward(w, cfg, x, torch.float32)['out'].double() - taps['out']).abs().max())}
        out[name] = (x, taps, e32, stats)
    return out


def test_schema_is_the_reference_s_state_dict(golden):
    """The golden tool records the keys, shapes and parameter count of the reference's own HSENET(64, 4, 10).state_dict()."""
    from fastdiffsr_amd.hsenet.arch import HSENetConfig, state_schema, tap_names
    s = state_schema(HSENetConfig(64, 4, 3, 10))
    assert list(s) == golden['schema/keys'].tolist() and len(s) == 552
    for (k, shape), rec in zip(s.items(), golden['schema/shapes']):
        assert tuple(shape) == tuple(int(v) for v in rec[:len(shape)]), k
    n = sum(int(np.prod(v)) for v in s.values())
    assert n == int(golden['schema/params']) and round(n / 1e6, 2) == 5.43
    # counted by hand: an SSEM has 18 tensors, an HSEM 8 + 2 * 18 + 2, a BasicModule 4 + 46 + 4
    assert len(state_schema(HSENetConfig(16, 3, 3, 2))) == 4 + 2 * 54 + 2 + 2 + 2
    assert len(state_schema(HSENetConfig(16, 8, 3, 2))) == 4 + 2 * 54 + 2 + 6 + 2
    assert s['body_modulist.3.body.0.NonLocal_base.W.weight'] == (64, 32, 1, 1)
    assert len(tap_names(HSENetConfig(16, 4, 3, 2))) == 1 + 2 * 12 + 2


def test_restatement_matches_the_reference(fp64):
    """e32 = max |reference in fp32 - fp64 restatement| per case and tap: the reference's own arithmetic noise, a few 1e-6 on
    values of up to 13 (fp32 epsilon 6e-8 times 13, times the square root of the 576 terms of a convolution, through up to 130 of
    them).  A restatement that differed from the reference in substance would be off by 1e-3 or more (the sensitivity test
    below), so 1e-4 separates the two."""
    for name, (x, taps, e32, _) in fp64.items():
        for k, e in e32.items():
            print('e32 %-14s %-14s %.3e  (max |x| %.2f)' % (name, k, e, float(taps[k].abs().max())))
            assert e < 1e-4, (name, k, e)
        cfg, _, batch, hw, _ = case(name)
        assert tuple(taps['out'].shape) == (batch, 3, hw[0] * cfg.scale, hw[1] * cfg.scale)


def test_fp32_restatement_is_within_its_own_noise_of_the_golden(fp64, golden):
    """The restatement in fp32 against the reference in fp32 at every recorded tap and the output: both are fp32 sums of the same
    terms, so they differ by no more than each differs from fp64."""
    for name in R.GOLDEN_CASES:
        cfg, w, batch, hw, keys = case(name)
        t32 = R.hsenet_forward(w, cfg, fp64[name][0], torch.float32)
        for k in keys:
            d = float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, t32[k])).max())
            assert d <= 2 * fp64[name][2][k] + 1e-7, (name, k, d, fp64[name][2][k])


def test_softmax_is_neither_flat_nor_one_hot(fp64):
    """Under plain fan-in weights every softmax here is uniform to three digits and a test of the attention sees a mean.  The
    cases' theta / phi gains are fixed so that in every case at least half of the attention calls have a median row maximum above
    4 / Nk and at least half one below 0.9; the sharp case has a logit above 100 (expf overflows at 88) and a row maximum above
    0.99."""
    for name, (_, _, _, stats) in fp64.items():
        cfg = R.case_config(name)
        assert len(stats) == 3 * cfg.n_basic_modules
        above = sum(1 for nq, nk, med, top, logit in stats if med > 4.0 / nk)
        below = sum(1 for nq, nk, med, top, logit in stats if med < 0.9)
        print('%-14s %2d calls: median row maximum above 4/Nk in %2d, below 0.9 in %2d; largest |logit| %.1f, largest row maximum %.3f'
              % (name, len(stats), above, below, max(s[4] for s in stats), max(s[3] for s in stats)))
        assert 2 * above >= len(stats) and 2 * below >= len(stats), (name, above, below)
    sharp = fp64['sharp_16x16'][3]
    assert max(s[4] for s in sharp) > 100 and max(s[3] for s in sharp) > 0.99


@pytest.mark.parametrize('hw', [(9, 7), (13, 16)])
def test_interpolation_rules_are_f_interpolate_s(hw):
    t = torch.rand(2, 3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    d = R.down_half(t)
    assert tuple(d.shape[2:]) == (hw[0] // 2, hw[1] // 2)
    assert float((d - F.interpolate(t, scale_factor=0.5, mode='bilinear')).abs().max()) < 1e-15
    assert float((R.up_to(d, hw) - F.interpolate(d, size=hw, mode='bilinear')).abs().max()) < 1e-15
    assert float((R.up_to(d, hw, True) - F.interpolate(d, size=hw, mode='bilinear', align_corners=True)).abs().max()) < 1e-15
    assert float((R.up_to(d, hw, True) - R.up_to(d, hw)).abs().max()) > 1e-2


@pytest.mark.parametrize('broken', R.BROKEN)
def test_broken_restatements_move_the_output(fp64, broken):
    """Each wrong form moves the output by more than 100 e32 on the cases with taps: the 4 e32 tolerance of the GPU tests cannot
    hide one."""
    for name in TAPPED:
        x, taps, e32, _ = fp64[name]
        cfg, w, _, _, _ = case(name)
        moved = float((R.hsenet_forward(w, cfg, x, torch.float64, broken=broken)['out'] - taps['out']).abs().max())
        print('%-22s %-8s moves the output by %.3e = %.0f e32' % (broken, name, moved, moved / e32['out']))
        assert moved > 100 * e32['out'], (broken, name, moved, e32['out'])


def test_synthetic_weights(fp64):
    """W is not the reference's zero; the mean shifts are the reference's constants; activations stay in range."""
    from fastdiffsr_amd.hsenet.arch import RGB_MEAN
    w = R.case_weights('s4_8x8')
    assert all(np.abs(v).max() > 0.1 for k, v in w.items() if k.endswith('.W.weight'))
    assert np.array_equal(w['sub_mean.weight'].reshape(3, 3), np.eye(3, dtype=np.float32))
    assert np.array_equal(w['add_mean.weight'].reshape(3, 3), np.eye(3, dtype=np.float32))
    assert np.array_equal(w['sub_mean.bias'], -np.asarray(RGB_MEAN, np.float32)) and np.array_equal(w['add_mean.bias'], np.asarray(RGB_MEAN, np.float32))
    for name, (x, taps, _, _) in fp64.items():
        for k, t in taps.items():
            assert 0.1 < float(t.abs().max()) < 100, (name, k, float(t.abs().max()))


def small(**over):
    return dict(dict(R.SMALL, scale=4), **over)


def test_state_dict_round_trip_and_the_reference_s_lenient_load():
    from fastdiffsr_amd.hsenet import HSENet, state_schema
    from fastdiffsr_amd.synth import synth_hsenet
    m = HSENet(**small())
    keys = list(m.state_dict())
    assert keys == list(state_schema(m.cfg)) and 'tail.0.2.weight' in keys and 'tail.0.4.weight' not in keys
    sd = {k: torch.from_numpy(v) for k, v in synth_hsenet(m.cfg, 3).items()}
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert len(HSENet(**small(scale=8)).state_dict()) == len(keys) + 2
    assert len(HSENet(**small(scale=3)).state_dict()) == len(keys) - 2
    # the reference's rule: a wrong shape under `tail` is skipped, anywhere else it is an error; unknown keys pass unless strict
    m2 = HSENet(**small())
    m2.load_reference_state_dict(dict(sd, **{'tail.1.weight': torch.zeros(1, 16, 3, 3), 'extra': torch.zeros(1)}))
    assert torch.equal(m2.state_dict()['head.0.weight'], sd['head.0.weight']) and not m2.state_dict()['tail.1.weight'].any()
    # 'tail' anywhere in the name, as the reference's `name.find('tail') == -1` has it
    m2.load_reference_state_dict({'body_modulist.0.tail.0.0.weight': torch.zeros(1, 16, 3, 3)})
    with pytest.raises(RuntimeError, match='head.0.weight'):
        m2.load_reference_state_dict(dict(sd, **{'head.0.weight': torch.zeros(16, 1, 3, 3)}))
    with pytest.raises(KeyError, match='unexpected'):
        m2.load_reference_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)
    with pytest.raises(KeyError, match='missing'):
        m2.load_reference_state_dict({k: v for k, v in sd.items() if k != 'add_mean.bias'}, strict=True)


def test_constructor_takes_the_reference_s_arguments_and_refuses_what_it_refuses():
    from fastdiffsr_amd.hsenet import HSENet
    m = HSENet(n_feats=64, scale=3, n_basic_modules=10, n_colors=3, conv=None)
    assert (m.cfg.n_feats, m.cfg.inter, m.cfg.scale, m.cfg.n_basic_modules) == (64, 32, 3, 10)
    assert HSENet().cfg == m.cfg
    for kw in (dict(n_colors=1), dict(scale=5), dict(n_feats=24), dict(n_feats=128), dict(n_basic_modules=0), dict(conv=torch.nn.Conv2d)):
        with pytest.raises(NotImplementedError):
            HSENet(**small(**kw))
    with pytest.raises(ValueError, match='at least 2'):
        m(torch.zeros(1, 3, 1, 8))
    with pytest.raises(ValueError, match='no CPU path'):
        m(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 1, 8, 8))


def test_the_c_abi_refuses_without_a_gpu():
    """create, workspace_bytes and the checks of load and forward that come before the device is touched."""
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.hsenet import HSENet
    lib = _lib.load()
    m = HSENet(**small())
    b1, b2, b3 = m.workspace_bytes(1, 8, 8), m.workspace_bytes(2, 8, 8), m.workspace_bytes(1, 8, 10)
    assert 0 < b1 < b2 and b1 < b3 < b2
    assert b1 >= 4 * 16 * 16 * 8 * 8 * 2           # the upsampler's last two maps: n_feats channels at 4 and 16 times the pixels
    assert m.workspace_bytes(1, 2, 2) > 0 and m.workspace_bytes(3, 9, 7) > 0
    for h, w in ((1, 8), (8, 1), (1, 1)):
        with pytest.raises(_lib.FdsrError, match='at least 2') as e:
            m.workspace_bytes(1, h, w)
        assert e.value.code == -1
    with pytest.raises(_lib.FdsrError):
        m.workspace_bytes(0, 8, 8)
    with pytest.raises(_lib.FdsrError, match='too many pixels'):
        m.workspace_bytes(64, 1024, 1024)

    def create(**over):
        c = _lib.FdsrHsenetConfig()
        c.n_feats, c.scale, c.n_colors, c.n_basic_modules = 16, 4, 3, 2
        for k, v in over.items():
            setattr(c, k, v)
        h = C.c_void_p()
        rc = lib.fdsr_hsenet_create(C.byref(c), C.byref(h))
        if rc == 0:
            lib.fdsr_hsenet_destroy(h)
        return rc, (lib.fdsr_last_error(None) or b'').decode()

    assert create()[0] == 0
    assert create(n_feats=64, scale=8, n_basic_modules=10)[0] == 0 and create(n_feats=32, scale=3)[0] == 0
    for over, word in ((dict(n_colors=1), 'n_colors'), (dict(n_feats=24), 'n_feats'), (dict(n_feats=0), 'n_feats'), (dict(n_feats=128), 'n_feats'),
                       (dict(scale=5), 'scale'), (dict(scale=1), 'scale'), (dict(n_basic_modules=0), 'n_basic_modules')):
        rc, msg = create(**over)
        assert rc == -1 and word in msg, (over, rc, msg)          # FDSR_E_INVALID, with a message

    # load: the name and the shape are checked before anything is copied; forward: the shape before the tensors and the device
    handle = m._handle()

    def load(name, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        return lib.fdsr_hsenet_load(handle, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim), (lib.fdsr_last_error(None) or b'').decode()

    rc, msg = load('body_modulist.0.body.0.NonLocal_base.psi.weight', np.zeros((8, 16, 1, 1)))
    assert rc == -2 and 'unknown tensor' in msg                   # FDSR_E_KEY
    rc, msg = load('body_modulist.2.head.0.0.weight', np.zeros((16, 16, 3, 3)))      # two modules only
    assert rc == -2 and 'unknown tensor' in msg
    rc, msg = load('body_modulist.0.body.0.NonLocal_base.theta.weight', np.zeros((16, 16, 1, 1)))     # [8][16][1][1]
    assert rc == -2 and 'wrong shape' in msg
    rc, msg = load('sub_mean.weight', np.zeros((3, 3)))
    assert rc == -2 and 'wrong shape' in msg
    buf = (C.c_float * 16)()
    rc = lib.fdsr_hsenet_forward(handle, buf, 1, 1, 8, buf, buf, 0, None, 0)
    assert rc == -1 and b'at least 2' in lib.fdsr_last_error(None)
    rc = lib.fdsr_hsenet_forward(handle, buf, 1, 8, 8, buf, buf, 0, None, 2)
    assert rc == -1                                               # an unknown flag
