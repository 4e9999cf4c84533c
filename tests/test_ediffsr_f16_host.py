"""The f16 storage mode of the NAFNet without a GPU: the ABI of fdsr_nafnet_set_storage, its mutual exclusion with f16x3, and the
mode's arithmetic emulated on the CPU (tests/ediffsr_f16_emulation.py), which must stay within CAP of the fp64 restatement on
every tap -- the condition tests/test_gpu_ediffsr_f16.py puts on its yardstick."""
import ctypes as C
import os
import re

import pytest
import torch

import ediffsr_f16_emulation as E
import ediffsr_restatement as R

TEST_SETTING = dict(width=16, enc_blk_nums=[2, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
SHIPPED_SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
EMPTY_SETTING = dict(width=16, enc_blk_nums=[1, 0], middle_blk_num=0, dec_blk_nums=[0, 1])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDSR_E_INVALID = -1
CAP = 5e-3          # of max|ref|: the emulation's largest allowed distance to fp64 (the GPU test's second clause)


def _inputs(seed, b, h, w):
    g = torch.Generator().manual_seed(seed)
    cond = torch.rand(b, 3, h, w, generator=g)
    return cond + torch.randn(b, 3, h, w, generator=g) * (50 / 255), cond


def _handle(lib, _lib):
    c = _lib.FdsrNafnetConfig()
    c.img_channel, c.width, c.n_levels, c.middle_blk_num = 3, 16, 4, 1
    for i in range(4):
        c.enc_blk_nums[i], c.dec_blk_nums[i] = 1, 1
    h = C.c_void_p()
    assert lib.fdsr_nafnet_create(C.byref(c), C.byref(h)) == 0
    return h


def test_set_storage_accepts_the_two_modes_without_a_gpu():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    assert (_lib.FDSR_NAF_STORE_F32, _lib.FDSR_NAF_STORE_F16) == (0, 1)
    h = _handle(lib, _lib)
    try:
        for mode in (0, 1, 1, 0):
            assert lib.fdsr_nafnet_set_storage(h, mode) == 0, mode
        for bad in (2, -1):
            assert lib.fdsr_nafnet_set_storage(h, bad) == FDSR_E_INVALID, bad
            assert b'fdsr_nafnet_set_storage' in lib.fdsr_last_error(None)
        assert lib.fdsr_nafnet_set_storage(None, 0) == FDSR_E_INVALID
        assert b'fdsr_nafnet_set_storage' in lib.fdsr_last_error(None)
    finally:
        lib.fdsr_nafnet_destroy(h)


def test_storage_and_f16x3_exclude_each_other_in_both_orders():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    F32, F16X3 = _lib.PRECISIONS['f32'], _lib.PRECISIONS['f16x3']
    h = _handle(lib, _lib)
    try:
        assert lib.fdsr_nafnet_set_precision(h, F16X3) == 0
        assert lib.fdsr_nafnet_set_storage(h, 1) == FDSR_E_INVALID
        assert b'fdsr_nafnet_set_storage' in lib.fdsr_last_error(None)
        assert lib.fdsr_nafnet_set_storage(h, 0) == 0                  # the default stays settable
        assert lib.fdsr_nafnet_set_precision(h, F32) == 0
        assert lib.fdsr_nafnet_set_storage(h, 1) == 0
        assert lib.fdsr_nafnet_set_precision(h, F16X3) == FDSR_E_INVALID
        assert b'fdsr_nafnet_set_precision' in lib.fdsr_last_error(None)
        assert lib.fdsr_nafnet_set_precision(h, F32) == 0
        assert lib.fdsr_nafnet_set_storage(h, 0) == 0
        assert lib.fdsr_nafnet_set_precision(h, F16X3) == 0
    finally:
        lib.fdsr_nafnet_destroy(h)


def test_the_symbol_is_declared_and_bound():
    from fastdiffsr_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'fdsr.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert 'fdsr_nafnet_set_storage' in set(re.findall(r'\b(fdsr_[a-z_0-9]+)\s*\(', code))
    assert 'fdsr_nafnet_set_storage' in _lib.SYMBOLS
    assert re.search(r'#define\s+FDSR_NAF_STORE_F32\s+0\b', code) and re.search(r'#define\s+FDSR_NAF_STORE_F16\s+1\b', code)


def test_model_precision_names_without_a_gpu():
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    assert ConditionalNAFNet.PRECISIONS == ('f32', 'f16x3', 'f16')
    m = ConditionalNAFNet(**TEST_SETTING)
    for mode in ('f16', 'f16x3', 'f32', 'f16', 'f32', 'f16x3', 'f32', 'f16', 'f16'):      # every switch passes through the engine's exclusion
        m.set_precision(mode)
        assert m.precision == mode
    m.set_precision('f16x3')
    with pytest.raises(ValueError, match='f32'):                                    # the one switch that goes through 'f32'
        m.set_precision('f16')
    assert m.precision == 'f16x3'
    m.set_precision('f32')
    m.set_precision('f16')
    with pytest.raises(ValueError):
        m.set_precision('bf16')
    assert m.precision == 'f16'


def test_rounding_helper_clamps_and_is_idempotent():
    v = torch.tensor([1.0, -3.14159274, 1e-3, 65504.0, 65519.0, 1e5, -7e4, float('inf'), 0.0, 123.456, 2049.0, 2051.0])
    r = E.rnd(v)
    assert r.dtype == torch.float32
    assert torch.equal(E.rnd(r), r)
    assert r[3] == 65504.0 and r[4] == 65504.0 and r[5] == 65504.0 and r[6] == -65504.0 and r[7] == 65504.0
    assert r[0] == 1.0 and r[8] == 0.0
    assert r[10] == 2048.0 and r[11] == 2052.0                        # ties to even at 11 bits
    assert float((r[:3] - v[:3]).abs().max()) <= 3.15 * 2.0 ** -11


@pytest.mark.parametrize('name,setting,hw,t,seed', [('test 36x44', TEST_SETTING, (36, 44), 37, 21), ('test 32x32', TEST_SETTING, (32, 32), 37, 21),
                                                    ('empty 18x26', EMPTY_SETTING, (18, 26), 37, 24),
                                                    ('shipped 32x32', SHIPPED_SETTING, (32, 32), 50, 23)])
def test_emulated_forward_stays_near_fp64(name, setting, hw, t, seed):
    """the GPU tests' forward inputs: every tap and the output within CAP of the fp64 restatement, relative to the tap's own peak"""
    from fastdiffsr_amd.synth import synth_nafnet
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **setting).items()}
    x, cond = _inputs(seed, 2, *hw)
    t64, te = {}, {}
    with torch.no_grad():
        y32 = R.forward(sd, x, cond, t)
        y64 = R.forward(R.cast_sd(sd, torch.float64), x.double(), cond.double(), t, t64)
    ye = E.forward(sd, x, cond, t, te)
    assert ye.dtype == torch.float32 and set(te) == set(t64)
    t64['output'], te['output'] = y64, ye
    fails, peak_act = [], 0.0
    for k in t64:
        assert te[k].shape == t64[k].shape, k
        s = float((te[k].double() - t64[k]).abs().max())
        peak = float(t64[k].abs().max())
        peak_act = max(peak_act, peak)
        print('%s %-16s max|emul - f64| %.3g = %.3g of max|ref| %.3g (cap %.3g)' % (name, k, s, s / peak, peak, CAP))
        if not s <= CAP * peak:
            fails.append(k)
    print('%s: largest activation %.3g' % (name, peak_act))
    assert not fails, fails
    assert not torch.equal(ye, y32)                                   # the emulation is not the fp32 restatement again
    stored = [k for k in te if k not in ('ending', 'output')]
    assert all(torch.equal(E.rnd(te[k]), te[k]) for k in stored)      # every stored tap holds f16 values
    assert not torch.equal(E.rnd(te['ending']), te['ending'])         # eps stays fp32


def test_emulated_loop_stays_near_fp64():
    """T = 10 / eps 0.5 at 36x44, the GPU loop test's inputs: every step of the trajectory within CAP of fp64"""
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    from fastdiffsr_amd.synth import synth_nafnet
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}
    T, hw, seed = 10, (36, 44), 31
    s = IRSDE(max_sigma=50, T=T, schedule='cosine', eps=0.5, device='cpu')
    state, cond = _inputs(seed, 1, *hw)
    noise = torch.randn(T, 1, 3, *hw, generator=torch.Generator().manual_seed(seed + 1))
    tr64, tre = [], []
    with torch.no_grad():
        R.reverse_loop(R.cast_sd(sd, torch.float64), R.cast_tables(s, torch.float64), state.double(), cond.double(), noise.double(), False, tr64)
    E.reverse_loop(sd, R.cast_tables(s, torch.float32), state, cond, noise, False, tre)
    for k in range(T):
        d = float((tre[k].double() - tr64[k]).abs().max())
        peak = float(tr64[k].abs().max())
        print('step %d max|emul - f64| %.3g = %.3g of max|x| %.3g' % (k, d, d / peak, peak))
        assert d <= CAP * peak
