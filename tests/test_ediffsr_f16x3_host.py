"""The f16x3 mode of the NAFNet's GEMMs without a GPU: its arithmetic, emulated on the CPU (tests/ediffsr_f16x3_emulation.py),
must be fp32-grade for this network -- within 1e-4 max|ref| of the fp64 restatement -- and the ABI accepts exactly the two modes."""
import ctypes as C
import os
import re

import pytest
import torch

import ediffsr_f16x3_emulation as E
import ediffsr_restatement as R

TEST_SETTING = dict(width=16, enc_blk_nums=[2, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
SHIPPED_SETTING = dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDSR_E_INVALID = -1


def _inputs(seed, b, h, w):
    g = torch.Generator().manual_seed(seed)
    cond = torch.rand(b, 3, h, w, generator=g)
    return cond + torch.randn(b, 3, h, w, generator=g) * (50 / 255), cond


@pytest.mark.parametrize('name,setting,hw,t', [('test 32x32', TEST_SETTING, (32, 32), 37), ('test 36x44', TEST_SETTING, (36, 44), 37),
                                               ('shipped 32x32', SHIPPED_SETTING, (32, 32), 50)])
def test_emulated_mode_is_fp32_grade(name, setting, hw, t):
    from fastdiffsr_amd.synth import synth_nafnet
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **setting).items()}
    x, cond = _inputs(21, 2, *hw)
    t32, t64, te = {}, {}, {}
    with torch.no_grad():
        y32 = R.forward(sd, x, cond, t, t32)
        y64 = R.forward(R.cast_sd(sd, torch.float64), x.double(), cond.double(), t, t64)
    ye = E.forward(sd, x, cond, t, te)
    assert ye.dtype == torch.float32 and R.F is torch.nn.functional      # the patch is gone again
    t32['output'], t64['output'], te['output'] = y32, y64, ye
    fails = []
    for k in t64:
        d = float((te[k].double() - t64[k]).abs().max())
        spread = float((t32[k].double() - t64[k]).abs().max())
        peak = float(t64[k].abs().max())
        print('%s %-16s max|emul - f64| %.3g  f32-f64 spread %.3g  bar %.3g  max|ref| %.3g' % (name, k, d, spread, 1e-4 * peak, peak))
        if not d <= 1e-4 * peak:
            fails.append(k)
    assert not fails, fails
    assert not torch.equal(ye, y32)                                      # the emulation is not the fp32 restatement again


def test_split_keeps_22_bits_and_clamps():
    v = torch.tensor([1.0, -3.14159274, 1e-3, 65504.0, 1e5, -7e4, 0.0, 123.456])
    hi, lo = E.split(v)
    c = v.clamp(-65504, 65504).double()
    assert float(((hi + lo) - c).abs().max()) <= float(c.abs().max()) * 2.0 ** -21
    assert float((hi + lo)[4]) == 65504.0 and float((hi + lo)[5]) == -65504.0
    assert float((hi + lo)[0]) == 1.0 and float(lo[0]) == 0.0


def test_set_precision_accepts_the_two_modes_without_a_gpu():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    c = _lib.FdsrNafnetConfig()
    c.img_channel, c.width, c.n_levels, c.middle_blk_num = 3, 16, 4, 1
    for i in range(4):
        c.enc_blk_nums[i], c.dec_blk_nums[i] = 1, 1
    h = C.c_void_p()
    assert lib.fdsr_nafnet_create(C.byref(c), C.byref(h)) == 0
    try:
        for mode in ('f32', 'f16x3', 'f16x3', 'f32'):
            assert lib.fdsr_nafnet_set_precision(h, _lib.PRECISIONS[mode]) == 0, mode
        for bad in (_lib.PRECISIONS['bf16'], _lib.PRECISIONS['f16'], 7, -1):
            assert lib.fdsr_nafnet_set_precision(h, bad) == FDSR_E_INVALID, bad
            assert b'fdsr_nafnet_set_precision' in lib.fdsr_last_error(None)
        assert lib.fdsr_nafnet_set_precision(None, 0) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_check_saturation(None, None) == FDSR_E_INVALID
    finally:
        lib.fdsr_nafnet_destroy(h)


def test_new_symbols_are_declared_and_bound():
    from fastdiffsr_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'fdsr.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(fdsr_[a-z_0-9]+)\s*\(', txt))
    for name in ('fdsr_nafnet_set_precision', 'fdsr_nafnet_check_saturation'):
        assert name in declared and name in _lib.SYMBOLS
    assert declared == set(_lib.SYMBOLS)


def test_model_precision_property_without_a_gpu():
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    m = ConditionalNAFNet(**TEST_SETTING)
    assert m.precision == 'f32'
    m.set_precision('f16x3')
    assert m.precision == 'f16x3'
    for bad in ('bf16', 'f16', 'fp32'):
        with pytest.raises(ValueError):
            m.set_precision(bad)
    m.set_precision('f32')
    assert m.precision == 'f32'
