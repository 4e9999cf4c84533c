"""EDiffSR without a GPU: the restatement against the golden made from the reference's own modules, the package's IRSDE tables
bitwise, the key schema, the load_state_dict round trip, option parsing, and the ABI's refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ediffsr_restatement as R

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'ediffsr.npz')
TEST_SETTING = dict(width=16, enc_blk_nums=[2, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
SHIPPED_SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
FDSR_E_INVALID, FDSR_E_KEY, FDSR_E_STATE = -1, -2, -3
# fp32 restatement vs the reference's fp32 modules: the same torch kernels in the same order, except that the restatement's pools
# are x.mean(dim=(2, 3)) where the reference calls AdaptiveAvgPool2d(1) -- rounding noise of one sum.  2^-20 relative to max|ref|.
NOISE = 2.0 ** -20


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLD) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module')
def sd():
    from fastdiffsr_amd.synth import synth_nafnet
    torch.set_num_threads(min(8, torch.get_num_threads()))
    return {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}


def test_synthetic_weights_match_the_golden_and_are_not_identity(gold, sd):
    from fastdiffsr_amd.synth import state_dict_sha256
    assert state_dict_sha256({k: v.numpy() for k, v in sd.items()}) == str(gold['synth_sha256'])
    for k, v in sd.items():
        if k.endswith(('.beta', '.gamma')):
            assert float(v.abs().min()) > 0, k


def test_restatement_forward_equals_the_reference(gold, sd):
    taps = {}
    with torch.no_grad():
        y = R.forward(sd, torch.from_numpy(gold['fwd_x']), torch.from_numpy(gold['fwd_cond']), int(gold['fwd_time']), taps)
    assert sorted(taps) == sorted(gold['tap_names'].tolist())
    for k in gold['tap_names'].tolist():
        ref = gold['tap_' + k]
        assert tuple(taps[k].shape) == tuple(gold['tapshape_' + k]), k
        d = float(np.abs(taps[k].reshape(-1)[::53].numpy() - ref).max())
        print('%-16s max|restatement - reference| %.3g  max|ref| %.3g' % (k, d, np.abs(ref).max()))
        assert d <= NOISE * np.abs(ref).max(), k
    d = float(np.abs(y.numpy() - gold['fwd_out']).max())
    print('output: %.3g of max %.3g' % (d, np.abs(gold['fwd_out']).max()))
    assert d <= NOISE * np.abs(gold['fwd_out']).max()
    with torch.no_grad():
        y2 = R.forward(sd, torch.from_numpy(gold['fwd2_x']), torch.from_numpy(gold['fwd2_cond']), torch.from_numpy(gold['fwd2_time']))
    d = float(np.abs(y2.numpy() - gold['fwd2_out']).max())
    print('per-image float times: %.3g of max %.3g' % (d, np.abs(gold['fwd2_out']).max()))
    assert d <= NOISE * np.abs(gold['fwd2_out']).max()


def test_restatement_loops_equal_the_reference(gold, sd):
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    s = IRSDE(max_sigma=50, T=10, schedule='cosine', eps=0.5, device='cpu')
    tb = R.cast_tables(s, torch.float32)
    state, cond, noise = (torch.from_numpy(gold[k]) for k in ('loop_state', 'loop_cond', 'loop_noise'))
    with torch.no_grad():
        xs = R.reverse_loop(sd, tb, state, cond, noise)
        xo = R.reverse_loop(sd, tb, state, cond, ode=True)
    for name, x, ref in (('sde', xs, gold['loop_sde']), ('ode', xo, gold['loop_ode'])):
        d = float(np.abs(x.numpy() - ref).max())
        print('%s loop: %.3g of max %.3g' % (name, d, np.abs(ref).max()))
        assert d <= 10 * NOISE * np.abs(ref).max()      # ten steps


@pytest.mark.parametrize('schedule', ['cosine', 'linear', 'constant'])
def test_sde_tables_are_bitwise_the_reference(gold, schedule):
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    s = IRSDE(max_sigma=50, T=100, schedule=schedule, eps=0.005, device='cpu')
    assert s.dt.dtype == torch.float32
    for name in ('thetas', 'sigmas', 'sigma_bars', 'thetas_cumsum', 'dt'):
        ours, ref = getattr(s, name).numpy(), gold['sde_%s_%s' % (schedule, name)]
        assert ours.dtype == ref.dtype and ours.shape == ref.shape and ours.tobytes() == ref.tobytes(), name
    assert s.max_sigma == 50 / 255


@pytest.mark.parametrize('name,setting', [('test', TEST_SETTING), ('shipped', SHIPPED_SETTING)])
def test_key_schema_is_the_reference_state_dict(gold, name, setting):
    from fastdiffsr_amd.ediffsr.arch import NAFNetConfig, param_schema
    ours = ['%s %s' % (k, ','.join(map(str, v))) for k, v in param_schema(NAFNetConfig(3, **setting)).items()]
    assert ours == gold['schema_' + name].tolist()
    if name == 'shipped':
        assert len(ours) == 424


def test_engine_schema_is_the_python_schema():
    from fastdiffsr_amd import build
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    build.build(force=False, verbose=False)
    for setting in (TEST_SETTING, SHIPPED_SETTING):
        m = ConditionalNAFNet(**setting)
        assert m.engine_schema() == [(k, tuple(v)) for k, v in m.schema.items()]


def test_load_state_dict_strict_round_trip(sd):
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    m = ConditionalNAFNet(**TEST_SETTING)
    assert list(m.state_dict()) == list(sd)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'ending.bias'}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(sd, **{'ending.bias': torch.zeros(4)}), strict=True)


def test_training_is_refused():
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    s = IRSDE(max_sigma=50, T=10, schedule='cosine', eps=0.5, device='cpu')
    with pytest.raises(NotImplementedError):
        s.generate_random_states(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def test_yaml_options():
    from fastdiffsr_amd.ediffsr.test import parse_options
    opt = parse_options(os.path.join(os.path.dirname(__file__), 'golden', 'ediffsr_setting_mfe_Test_x4.yml'))
    assert opt['sde'] == {'max_sigma': 50, 'T': 100, 'schedule': 'cosine', 'eps': 0.005}
    assert opt['degradation']['scale'] == 4 and opt['scale'] == 4
    assert opt['network_G']['setting'] == SHIPPED_SETTING
    assert list(opt['datasets']) == ['test1', 'test2']
    assert opt['datasets']['test1']['dataroot_LQ'].endswith('Test_Potsdam_64_256/lr_64')
    assert opt['path']['pretrain_model_G'].endswith('latest_G.pth')


def _lib():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load(), _lib


def _cfg(L, width=16, levels=4, img=3):
    c = L.FdsrNafnetConfig()
    c.img_channel, c.width, c.n_levels, c.middle_blk_num = img, width, levels, 1
    for i in range(min(levels, 8)):
        c.enc_blk_nums[i], c.dec_blk_nums[i] = 1, 1
    return c


def test_abi_refusals_without_a_gpu():
    lib, L = _lib()
    h = C.c_void_p()
    for bad in (_cfg(L, width=24), _cfg(L, levels=0), _cfg(L, levels=9), _cfg(L, img=1)):
        assert lib.fdsr_nafnet_create(C.byref(bad), C.byref(h)) == FDSR_E_INVALID
    assert lib.fdsr_nafnet_create(None, C.byref(h)) == FDSR_E_INVALID
    assert lib.fdsr_nafnet_create(C.byref(_cfg(L)), C.byref(h)) == 0 and h.value
    try:
        def load(name, shape):
            a = np.zeros(int(np.prod(shape)), dtype=np.float32)
            return lib.fdsr_nafnet_load_weight(h, name.encode(), C.c_void_p(a.ctypes.data), (C.c_int64 * len(shape))(*shape), len(shape))
        assert load('encoders.0.0.conv9.weight', (32, 16, 1, 1)) == FDSR_E_KEY
        assert b'conv9' in lib.fdsr_last_error(None)
        assert load('ups.0.0.bias', (256,)) == FDSR_E_KEY            # the reference's ups have no bias
        assert load('encoders.0.0.conv1.weight', (16, 32, 1, 1)) == FDSR_E_KEY
        assert load('encoders.0.0.norm1.g', (16,)) == FDSR_E_KEY      # [1, c, 1, 1] in the checkpoint
        assert load('encoders.0.0.conv1.weight', (32, 16, 1, 1)) == 0
        assert lib.fdsr_nafnet_weights_complete(h) == 0
        fake, big = C.c_void_p(4096), C.c_size_t(1 << 40)            # never dereferenced: the checks come first
        assert lib.fdsr_nafnet_sample(h, fake, fake, None, 0, 0, 0, fake, None, 1, 32, 32, fake, big, None) == FDSR_E_STATE
        assert b'set_sde' in lib.fdsr_last_error(None)
        assert lib.fdsr_nafnet_forward(h, fake, fake, fake, fake, 1, 32, 32, fake, big, None) == FDSR_E_STATE   # weights missing
        assert lib.fdsr_nafnet_forward(h, fake, fake, fake, fake, 0, 32, 32, fake, big, None) == FDSR_E_INVALID
        n, m = C.c_size_t(), C.c_size_t()
        assert lib.fdsr_nafnet_workspace_bytes(h, 0, 8, 8, C.byref(n)) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_workspace_bytes(h, 1, 33, 33, C.byref(n)) == 0 and lib.fdsr_nafnet_workspace_bytes(h, 1, 48, 48, C.byref(m)) == 0
        assert n.value == m.value > 0                                 # 33 pads to 48
        assert lib.fdsr_upscale_bicubic_f32(fake, fake, 1, 3, 8, 8, 0, None) == FDSR_E_INVALID
    finally:
        lib.fdsr_nafnet_destroy(h)


EMPTY_SETTING = dict(width=16, enc_blk_nums=[1, 0], middle_blk_num=0, dec_blk_nums=[0, 1])      # empty encoder, middle and decoder lists
# (setting, (B, H, W)): (fdsr_nafnet_workspace_bytes, fdsr_nafnet_train_workspace_bytes), recorded from the library before the
# sampling and the training forward became one walk over two destination tables: the plans' offsets and totals did not move
WORKSPACE_BYTES = {
    ('test', (1, 33, 33)): (1129728, 8948224),
    ('test', (2, 48, 48)): (2258944, 17235712),
    ('test', (3, 36, 44)): (3388416, 25525248),
    ('test', (16, 256, 256)): (507984896, 3779138816),
    ('shipped', (1, 33, 33)): (4225792, 98427392),
    ('shipped', (2, 48, 48)): (8451584, 187938816),
    ('shipped', (3, 36, 44)): (12677376, 277451264),
    ('shipped', (16, 256, 256)): (1893724160, 40736108800),
    ('empty', (1, 33, 33)): (598272, 2733568),
    ('empty', (2, 48, 48)): (2123008, 9616384),
    ('empty', (3, 36, 44)): (2190848, 9919744),
    ('empty', (16, 256, 256)): (482622464, 2177958144),
}


def test_workspace_sizes_are_pinned():
    lib, L = _lib()
    settings = {'test': TEST_SETTING, 'shipped': SHIPPED_SETTING, 'empty': EMPTY_SETTING}
    for (name, shape), want in WORKSPACE_BYTES.items():
        s = settings[name]
        c = L.FdsrNafnetConfig()
        c.img_channel, c.width, c.n_levels, c.middle_blk_num = 3, s['width'], len(s['enc_blk_nums']), s['middle_blk_num']
        for i, (e, d) in enumerate(zip(s['enc_blk_nums'], s['dec_blk_nums'])):
            c.enc_blk_nums[i], c.dec_blk_nums[i] = e, d
        h = C.c_void_p()
        assert lib.fdsr_nafnet_create(C.byref(c), C.byref(h)) == 0
        try:
            fwd, train = C.c_size_t(), C.c_size_t()
            assert lib.fdsr_nafnet_workspace_bytes(h, *shape, C.byref(fwd)) == 0
            assert lib.fdsr_nafnet_train_workspace_bytes(h, *shape, C.byref(train)) == 0
            assert (fwd.value, train.value) == want, (name, shape)
        finally:
            lib.fdsr_nafnet_destroy(h)
