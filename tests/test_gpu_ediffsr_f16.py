"""EDiffSR's f16 storage mode (ConditionalNAFNet.set_precision('f16'): f16 NHWC activations, one f16 MFMA per product, fp32
accumulators) on the device.  A PSNR-grade 16-bit mode, so the yardstick is the mode's own arithmetic: per tensor, with
d = max|dev - f64| and s = max|emul - f64| (tests/ediffsr_f16_emulation.py, computed here on the CPU, never taken from the device),
pass if d <= 4 s and s <= 5e-3 max|ref|.  The factor 4 is what the suite gives a device over a CPU spread (test_gpu_ediffsr.py,
_f16x3.py): device and emulation take the same roundings but order their fp32 sums differently, so single values fall on the other
side of an f16 boundary.  The second clause keeps a broken emulation from widening the bar; a wrong channel, stride or plane is an
O(1) error against s ~ 1e-3.  Every measured value is printed before it is judged.  Shapes, inputs and the synthetic pairs are those
of tests/test_gpu_ediffsr.py."""
import os

import numpy as np
import pytest
import torch

import ediffsr_f16_emulation as E
import ediffsr_restatement as R
from test_gpu_ediffsr import DEV, SHIPPED_SETTING, TEST_SETTING, _inputs, _model, _write_pairs

pytestmark = pytest.mark.gpu
CAP = 5e-3


def _judge(name, dev, r64, rem, scale=None):
    """scale: what the cap is relative to (default: the tensor's own max|ref|)"""
    s = float((rem.double() - r64).abs().max())
    d = float((dev.double().cpu() - r64).abs().max())
    peak = float(r64.abs().max()) if scale is None else scale
    print('%-16s max|dev - f64| %.3g  max|emul - f64| %.3g (%.3g of %.3g)  bar %.3g' % (name, d, s, s / peak, peak, 4 * s))
    return d <= 4 * s and s <= CAP * peak


def _two(sd, x, cond, t, taps=False):
    """fp64 restatement, emulated f16 storage: (outputs, tap dicts)"""
    t64, tem = ({}, {}) if taps else (None, None)
    with torch.no_grad():
        y64 = R.forward(R.cast_sd(sd, torch.float64), x.double(), cond.double(), t, t64)
    yem = E.forward(sd, x, cond, t, tem)
    return (y64, yem), (t64, tem)


@pytest.fixture(scope='module')
def net():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m, sd = _model(TEST_SETTING)
    m.set_precision('f16')
    return m, sd


def _layerwise(m, sd, x, cond, t):
    from fastdiffsr_amd.ediffsr.arch import tap_names
    (y64, yem), (t64, tem) = _two(sd, x, cond, t, taps=True)
    fails = [name for name in tap_names(m.cfg) if not _judge(name, m.debug_tensor(name, x.to(DEV), cond.to(DEV), t), t64[name], tem[name])]
    ok = _judge('output', m(x.to(DEV), cond.to(DEV), t), y64, yem)
    m.check_saturation()
    return ok, fails


@pytest.mark.parametrize('hw', [(36, 44), (32, 32)])
def test_layerwise_and_forward(net, hw):
    m, sd = net
    assert m.precision == 'f16'
    x, cond = _inputs(21, 2, *hw)
    ok, fails = _layerwise(m, sd, x, cond, 37)
    assert ok and not fails, fails


def test_stored_taps_hold_f16_values(net):
    """debug_tensor returns the stored values widened: every tap but ending's fp32 eps survives a round trip through f16"""
    m, sd = net
    x, cond = _inputs(21, 2, 36, 44)
    for name in ('intro', 'enhance', 'encoders.0.1', 'downs.0', 'ups.3', 'decoders.3.0'):
        v = m.debug_tensor(name, x.to(DEV), cond.to(DEV), 37)
        assert torch.equal(v.half().float(), v), name
    v = m.debug_tensor('ending', x.to(DEV), cond.to(DEV), 37)
    assert not torch.equal(v.half().float(), v)


def test_empty_block_lists_layerwise_and_forward():
    """the setting of test_gpu_ediffsr.py whose empty block lists make the walk copy (half the bytes here)"""
    from fastdiffsr_amd.ediffsr.arch import tap_names
    from test_gpu_ediffsr import EMPTY_SETTING
    m, sd = _model(EMPTY_SETTING)
    m.set_precision('f16')
    assert len(tap_names(m.cfg)) == 9
    x, cond = _inputs(24, 2, 18, 26)
    ok, fails = _layerwise(m, sd, x, cond, 37)
    assert ok and not fails, fails


def test_workspace_does_not_grow(net):
    m, _ = net
    import ctypes as C
    from fastdiffsr_amd import _lib
    need = C.c_size_t()
    _lib.check(None, _lib.load().fdsr_nafnet_workspace_bytes(m._handle(), 16, 256, 256, C.byref(need)))
    f16 = need.value
    try:
        m.set_precision('f32')
        _lib.check(None, _lib.load().fdsr_nafnet_workspace_bytes(m._handle(), 16, 256, 256, C.byref(need)))
    finally:
        m.set_precision('f16')
    print('workspace at B = 16, 256x256: f16 %d bytes, f32 %d bytes' % (f16, need.value))
    assert 0 < f16 <= need.value


def test_forward_per_image_float_times(net):
    m, sd = net
    x, cond = _inputs(22, 3, 36, 44)
    t = torch.tensor([3.25, 58.5, 99.0])
    (y64, yem), _ = _two(sd, x, cond, t)
    batch = m(x.to(DEV), cond.to(DEV), t.to(DEV))
    assert _judge('float times', batch, y64, yem)
    one = m(x[1:2].to(DEV), cond[1:2].to(DEV), 58.5)
    assert torch.equal(one, batch[1:2])


@pytest.fixture(scope='module')
def shipped():
    """the shipped setting at 32x32, B = 2, t = 50: the device's f32 and f16 outputs and the CPU yardsticks"""
    m, sd = _model(SHIPPED_SETTING)
    x, cond = _inputs(23, 2, 32, 32)
    y_f32 = m(x.to(DEV), cond.to(DEV), 50)
    m.set_precision('f16')
    y_h = m(x.to(DEV), cond.to(DEV), 50)
    m.check_saturation()
    with torch.no_grad():
        y32 = R.forward(sd, x, cond, 50)
    return m, y_f32, y_h, y32, _two(sd, x, cond, 50)[0]


def test_forward_shipped_setting(shipped):
    _, _, y_h, _, (y64, yem) = shipped
    assert _judge('shipped output', y_h, y64, yem)


def test_mode_engages(shipped):
    m, y_f32, y_h, y32, (y64, _) = shipped
    assert m.precision == 'f16'
    nd = int((y_f32 != y_h).sum())
    print('shipped setting: %d of %d output elements differ between f32 and f16; max|f32 - f16| %.3g' %
          (nd, y_f32.numel(), float((y_f32 - y_h).abs().max())))
    assert nd >= 1
    bound = min(4 * float((y32.double() - y64).abs().max()), 1e-4 * float(y64.abs().max()))     # the f32 test's own bound
    assert float((y_f32.double().cpu() - y64).abs().max()) <= bound      # the f32 half of the pair is the exact kernel's result


def _loop(m, sd, T, eps, hw, ode=False, seed=31):
    """device trajectory; fp64 and emulated-f16 restatement trajectories of one loop with explicit noise"""
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    s = IRSDE(max_sigma=50, T=T, schedule='cosine', eps=eps, device='cpu')
    s.set_model(m)
    state, cond = _inputs(seed, 1, *hw)
    noise = torch.randn(T, 1, 3, *hw, generator=torch.Generator().manual_seed(seed + 1))
    tr64, trem = [], []
    with torch.no_grad():
        R.reverse_loop(R.cast_sd(sd, torch.float64), R.cast_tables(s, torch.float64), state.double(), cond.double(), noise.double(), ode, tr64)
    E.reverse_loop(sd, R.cast_tables(s, torch.float32), state, cond, noise, ode, trem)
    s.set_mu(cond.to(DEV))
    if ode:
        out, traj = s.reverse_ode(state.to(DEV), trajectory=True)
    else:
        out, traj = s.reverse_sde(state.to(DEV), noise=noise.to(DEV), trajectory=True)
    assert torch.equal(out, traj[-1])
    m.check_saturation()
    return traj.cpu(), torch.stack(tr64), torch.stack(trem)


def test_loop_mild_schedule(net):
    m, sd = net
    traj, t64, tem = _loop(m, sd, 10, 0.5, (36, 44))
    assert torch.isfinite(traj).all()
    assert all([_judge('step %d' % k, traj[k], t64[k], tem[k]) for k in range(10)])


def test_loop_ode(net):
    m, sd = net
    traj, t64, tem = _loop(m, sd, 10, 0.5, (32, 32), ode=True)
    assert all([_judge('ode step %d' % k, traj[k], t64[k], tem[k]) for k in range(10)])


def test_loop_reference_schedule(net):
    """T 100, eps 0.005 at 32x32, relative to max|x| of the fp64 trajectory as in test_gpu_ediffsr.test_loop_reference_schedule:
    d <= 4 s and s <= 5e-3 peak over the whole trajectory; the state stays finite and below 1e3."""
    m, sd = net
    traj, t64, tem = _loop(m, sd, 100, 0.005, (32, 32))
    assert torch.isfinite(traj).all()
    peak = float(t64.abs().max())
    print('T=100: max|x| %.4g  final-state dev %.3g' % (peak, float((traj[-1].double() - t64[-1]).abs().max())))
    assert peak < 1e3 and float(traj.abs().max()) < 1e3
    assert _judge('T=100 trajectory', traj, t64, tem, scale=peak)


def test_properties_bitwise(net):
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    m, sd = net
    T, hw = 6, (36, 44)
    s = IRSDE(max_sigma=50, T=T, schedule='cosine', eps=0.5, device='cpu')
    s.set_model(m)
    state, cond = _inputs(41, 5, *hw)
    noise = torch.randn(T, 5, 3, *hw, generator=torch.Generator().manual_seed(42))
    state, cond, noise = state.to(DEV), cond.to(DEV), noise.to(DEV)
    a, ta = m.sample(state, cond, noise=noise, trajectory=True)
    b, tb = m.sample(state, cond, noise=noise, trajectory=True)
    assert torch.equal(a, b) and torch.equal(ta, tb), 'rerun'
    g, tg = m.sample(state, cond, noise=noise, trajectory=True, graph=True)
    assert torch.equal(a, g) and torch.equal(ta, tg), 'graph == eager'
    assert torch.equal(a, m.sample(state, cond, noise=noise, graph=True)), 'graph replay'
    one = m.sample(state[3:4], cond[3:4], noise=noise[:, 3:4].contiguous())
    assert torch.equal(one, a[3:4]), 'B = 1 vs index 3 of B = 5'
    seed = 0x5EED
    planes = torch.stack([m.randn(5, *hw, k, seed, device=DEV) for k in range(T)])
    drawn = m.sample(state, cond, noise=None, seed=seed)
    assert torch.equal(drawn, m.sample(state, cond, noise=planes)), 'noise = NULL under a seed == the documented planes'
    assert torch.equal(drawn, m.sample(state, cond, noise=None, seed=seed, graph=True))
    part = m.sample(state[3:5], cond[3:5], noise=None, seed=seed, first_image=3)
    assert torch.equal(part, drawn[3:5]), 'stream positions are per global image index'
    # the mode leaves nothing behind: f16 -> f32 -> f16 is the first f16 result, and f32 in between is a fresh f32 model's
    fresh, _ = _model(TEST_SETTING)
    s.set_model(fresh)
    want32 = fresh.sample(state, cond, noise=noise)
    want32g = fresh.sample(state, cond, noise=noise, graph=True)
    assert torch.equal(want32, want32g)
    try:
        m.set_precision('f32')
        assert m.precision == 'f32'
        assert torch.equal(m.sample(state, cond, noise=noise), want32), 'f32 after f16 == a fresh f32 model'
        assert torch.equal(m.sample(state, cond, noise=noise, graph=True), want32), 'the graph was dropped with the mode'
        assert torch.equal(m(state, cond, 3), fresh(state, cond, 3))
    finally:
        m.set_precision('f16')
    assert not torch.equal(a, want32), 'the two modes are different arithmetic'
    assert torch.equal(m.sample(state, cond, noise=noise), a), 'f16 -> f32 -> f16'
    assert torch.equal(m.sample(state, cond, noise=noise, graph=True), a)
    try:
        m.set_precision('f16x3')
        h3 = m.sample(state, cond, noise=noise)
        assert not torch.equal(h3, a) and not torch.equal(h3, want32)
        with pytest.raises(ValueError):
            m.set_precision('f16')             # not over 'f16x3' directly
    finally:
        m.set_precision('f32')
        m.set_precision('f16')
    assert torch.equal(m.sample(state, cond, noise=noise, graph=True), a), 'f16 -> f16x3 -> f16'
    assert torch.equal(m.sample(state, cond, noise=noise), a)


def test_range_guard(net):
    from fastdiffsr_amd import _lib
    m, sd = net
    x, cond = _inputs(51, 2, 36, 44)
    x, cond = x.to(DEV), cond.to(DEV)
    m(x, cond, 37)
    m.check_saturation()                       # in range: clear
    y = m(x * 1e5, cond, 37)                   # intro stages x - cond: beyond +-65504, clamped and flagged
    assert torch.isfinite(y).all()
    with pytest.raises(_lib.FdsrSaturated) as e:
        m.check_saturation()
    assert e.value.code == _lib.FDSR_E_SATURATED and '65504' in str(e.value)
    m.check_saturation()                       # cleared by the read
    bad = x.clone()
    bad[1, 2, 5, 7] = float('nan')             # a NaN is out of range too
    m(bad, cond, 37)
    with pytest.raises(_lib.FdsrSaturated):
        m.check_saturation()
    try:
        m.set_precision('f32')
        m(x, cond, 37)
        m.check_saturation()
        m(x * 1e5, cond, 37)
        m.check_saturation()                   # the exact kernel has no such limit
    finally:
        m.set_precision('f16')
    m(x, cond, 37)
    m.check_saturation()


def test_range_guard_at_a_store():
    """every input intro stages is in range; its bias puts its OUTPUT beyond the range: the flag comes from the store"""
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    from fastdiffsr_amd.synth import synth_nafnet
    sd = {k: torch.from_numpy(v).clone() for k, v in synth_nafnet(0, **TEST_SETTING).items()}
    sd['intro.bias'] = sd['intro.bias'] * 0 + 1e5
    m = ConditionalNAFNet(**TEST_SETTING)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    m.set_precision('f16')
    x, cond = _inputs(51, 2, 36, 44)
    assert float(torch.cat([x - cond, cond], 1).abs().max()) < 10
    v = m.debug_tensor('intro', x.to(DEV), cond.to(DEV), 37)
    assert float(v.max()) == 65504.0 and torch.isfinite(v).all()
    with pytest.raises(_lib.FdsrSaturated):
        m.check_saturation()
    m.check_saturation()


def test_training_is_refused_and_a_switch_sees_trained_weights():
    from fastdiffsr_amd import _lib
    from test_gpu_ediffsr_train import _batch, _model as _train_model
    m, sd, sde = _train_model(TEST_SETTING)
    gt, mu, state, ts = _batch(7, 2, 32, 32, [20, 80], sde)
    args = (state.to(DEV), mu.to(DEV), gt.to(DEV), ts)
    m.set_precision('f16')
    with pytest.raises(_lib.FdsrError, match='f16') as e:
        m.train_grads(*args)
    assert e.value.code == -1 and 'f16x3' not in str(e.value)      # FDSR_E_INVALID, and the message names this mode
    m.set_precision('f32')
    loss = m.train_grads(*args)
    assert torch.isfinite(loss).all()
    m.optim_step('Adam', 1e-3)
    y32 = m(args[0], args[1], 37)
    m.set_precision('f16')                     # the hi planes are built from the stepped weights
    y = m(args[0], args[1], 37)
    m.check_saturation()
    with pytest.raises(_lib.FdsrError, match='f16') as e:
        m.optim_step('Adam', 1e-3)
    assert e.value.code == -1 and 'f16x3' not in str(e.value)
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    twin = ConditionalNAFNet(**TEST_SETTING)
    twin.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    twin = twin.to(DEV).eval()
    assert not torch.equal(twin.state_dict()['intro.weight'].cpu(), sd['intro.weight'])
    assert torch.equal(twin(args[0], args[1], 37), y32)
    twin.set_precision('f16')
    assert torch.equal(twin(args[0], args[1], 37), y)
    m.set_precision('f32')
    assert torch.equal(m(args[0], args[1], 37), y32)
    assert torch.isfinite(m.train_grads(*args)).all()     # training goes on after the round trip


def _cli_root(tmp_path, n=8):
    import yaml
    from fastdiffsr_amd.synth import synth_nafnet
    root = str(tmp_path)
    _write_pairs(root, n=n)
    torch.save({k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}, os.path.join(root, 'latest_G.pth'))
    opt = {'name': 'Test-x4', 'suffix': None, 'sde': {'max_sigma': 50, 'T': 10, 'schedule': 'cosine', 'eps': 0.5},
           'degradation': {'scale': 4}, 'path': {'pretrain_model_G': os.path.join(root, 'latest_G.pth')},
           'datasets': {'test1': {'name': 'synth', 'mode': 'LQGT', 'dataroot_GT': os.path.join(root, 'hr'), 'dataroot_LQ': os.path.join(root, 'lr')}},
           'network_G': {'which_model_G': 'ConditionalNAFNet', 'setting': TEST_SETTING}}
    with open(os.path.join(root, 'opt.yml'), 'w') as f:
        yaml.safe_dump(opt, f)
    return root, ['-opt', os.path.join(root, 'opt.yml'), '--rng', 'engine', '--seed', '7']


def test_cli_precision(tmp_path):
    """The eight synthetic 64^2 -> 256^2 pairs of test_gpu_ediffsr.test_cli_end_to_end, T 10 / eps 0.5.  Against the f32 PNGs the
    largest step is one grey level: the emulation's final-state error, 3e-4, is 0.08 of a grey level, and a step of 2 would need
    more than 13 times that."""
    from PIL import Image
    from fastdiffsr_amd.ediffsr import test as cli
    root, base = _cli_root(tmp_path)
    r1 = cli.main(base + ['--precision', 'f16', '--results', os.path.join(root, 'h1')])['synth']
    r4 = cli.main(base + ['--precision', 'f16', '--batch', '4', '--graph', '--results', os.path.join(root, 'h4')])['synth']
    cli.main(base + ['--precision', 'f32', '--batch', '4', '--results', os.path.join(root, 'f4')])
    assert len(r1['per_image']) == 8
    for a, b in zip(r1['per_image'], r4['per_image']):
        assert {k: v for k, v in a.items() if k != 'lpips'} == {k: v for k, v in b.items() if k != 'lpips'}, (a, b)
    differ = total = worst = 0
    for row in r1['per_image']:
        h = np.asarray(Image.open(os.path.join(root, 'h1', 'synth', row['name']))).astype(np.int32)
        assert np.array_equal(h, np.asarray(Image.open(os.path.join(root, 'h4', 'synth', row['name']))))
        f = np.asarray(Image.open(os.path.join(root, 'f4', 'synth', row['name']))).astype(np.int32)
        differ, total, worst = differ + int((h != f).sum()), total + h.size, max(worst, int(np.abs(h - f).max()))
    print('f16 vs f32 PNGs: %d of %d values differ (%.3g), largest step %d grey level(s)' % (differ, total, differ / total, worst))
    assert worst <= 1


def test_cli_reruns_a_flagged_batch_in_f32(tmp_path, monkeypatch, caplog):
    """A batch whose range flag is raised (here: reported raised for the first batch) is run again in f32 with a logged warning:
    its PNGs are the --precision f32 ones, the other batches stay f16 and the model ends in f16."""
    import logging
    from PIL import Image
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet, test as cli
    root, base = _cli_root(tmp_path, n=4)
    base = base + ['--batch', '2']
    cli.main(base + ['--precision', 'f32', '--results', os.path.join(root, 'f')])
    cli.main(base + ['--precision', 'f16', '--results', os.path.join(root, 'h')])
    real, calls, modes = ConditionalNAFNet.check_saturation, [], []

    def flagged_once(self):
        real(self)
        calls.append(self.precision)
        if len(calls) == 1:
            raise _lib.FdsrSaturated(_lib.FDSR_E_SATURATED, 'test: flag reported raised')

    monkeypatch.setattr(ConditionalNAFNet, 'check_saturation', flagged_once)
    monkeypatch.setattr(ConditionalNAFNet, 'set_precision',
                        lambda self, mode, _real=ConditionalNAFNet.set_precision: (modes.append(mode), _real(self, mode))[1])
    with caplog.at_level(logging.WARNING, logger='fastdiffsr_amd.ediffsr'):
        cli.main(base + ['--precision', 'f16', '--results', os.path.join(root, 'm')])
    assert calls == ['f16', 'f16'] and modes == ['f16', 'f32', 'f16']
    assert any('again in f32' in r.getMessage() for r in caplog.records)
    png = lambda d, i: np.asarray(Image.open(os.path.join(root, d, 'synth', '%02d.png' % i)))
    for i in (0, 1):
        assert np.array_equal(png('m', i), png('f', i))
    for i in (2, 3):
        assert np.array_equal(png('m', i), png('h', i))
    assert not all(np.array_equal(png('h', i), png('f', i)) for i in range(4))      # the two modes' PNGs are not the same files
