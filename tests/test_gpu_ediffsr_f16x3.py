"""EDiffSR's f16x3 mode (ConditionalNAFNet.set_precision('f16x3'): the GEMMs on three f16 MFMAs per product, everything else
fp32) on the device.  Accuracy is judged against the fp64 restatement with the rule of tests/test_gpu_ediffsr.py and the mode's own
arithmetic as the reference: per tensor d <= min(4 x max(spread_f32, spread_emul), 1e-4 max|ref|), where spread_f32 is the fp32
restatement's distance to fp64 and spread_emul that of the CPU emulation of the split (tests/ediffsr_f16x3_emulation.py).  Every
measured value is printed before it is judged.  Shapes, inputs and the synthetic pairs are those of tests/test_gpu_ediffsr.py."""
import os

import numpy as np
import pytest
import torch

import ediffsr_f16x3_emulation as E
import ediffsr_restatement as R
from test_gpu_ediffsr import DEV, SHIPPED_SETTING, TEST_SETTING, _inputs, _model, _write_pairs

pytestmark = pytest.mark.gpu


def _bar(r64, r32, rem):
    s32 = float((r32.double() - r64).abs().max())
    sem = float((rem.double() - r64).abs().max())
    return min(4 * max(s32, sem), 1e-4 * float(r64.abs().max())), s32, sem


def _judge(name, dev, r64, r32, rem):
    bar, s32, sem = _bar(r64, r32, rem)
    d = float((dev.double().cpu() - r64).abs().max())
    print('%-16s max|dev - f64| %.3g  spread f32 %.3g  emul %.3g  bar %.3g  max|ref| %.3g' % (name, d, s32, sem, bar, float(r64.abs().max())))
    return d <= bar


def _three(sd, x, cond, t, taps=False):
    """fp32 restatement, fp64 restatement, emulated f16x3: (outputs, tap dicts)"""
    t32, t64, tem = ({}, {}, {}) if taps else (None, None, None)
    with torch.no_grad():
        y32 = R.forward(sd, x, cond, t, t32)
        y64 = R.forward(R.cast_sd(sd, torch.float64), x.double(), cond.double(), t, t64)
    yem = E.forward(sd, x, cond, t, tem)
    return (y32, y64, yem), (t32, t64, tem)


@pytest.fixture(scope='module')
def net():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m, sd = _model(TEST_SETTING)
    m.set_precision('f16x3')
    return m, sd


@pytest.mark.parametrize('hw', [(36, 44), (32, 32)])
def test_layerwise_and_forward(net, hw):
    from fastdiffsr_amd.ediffsr.arch import tap_names
    m, sd = net
    assert m.precision == 'f16x3'
    x, cond = _inputs(21, 2, *hw)
    (y32, y64, yem), (t32, t64, tem) = _three(sd, x, cond, 37, taps=True)
    fails = [name for name in tap_names(m.cfg)
             if not _judge(name, m.debug_tensor(name, x.to(DEV), cond.to(DEV), 37), t64[name], t32[name], tem[name])]
    ok = _judge('output', m(x.to(DEV), cond.to(DEV), 37), y64, y32, yem)
    m.check_saturation()
    assert ok and not fails, fails


def test_empty_block_lists_layerwise_and_forward():
    """the setting of test_gpu_ediffsr.py whose empty block lists make the walk copy"""
    from fastdiffsr_amd.ediffsr.arch import tap_names
    from test_gpu_ediffsr import EMPTY_SETTING
    m, sd = _model(EMPTY_SETTING)
    m.set_precision('f16x3')
    x, cond = _inputs(24, 2, 18, 26)
    (y32, y64, yem), (t32, t64, tem) = _three(sd, x, cond, 37, taps=True)
    assert len(tap_names(m.cfg)) == 9
    fails = [name for name in tap_names(m.cfg)
             if not _judge(name, m.debug_tensor(name, x.to(DEV), cond.to(DEV), 37), t64[name], t32[name], tem[name])]
    ok = _judge('output', m(x.to(DEV), cond.to(DEV), 37), y64, y32, yem)
    m.check_saturation()
    assert ok and not fails, fails


def test_forward_per_image_float_times(net):
    m, sd = net
    x, cond = _inputs(22, 3, 36, 44)
    t = torch.tensor([3.25, 58.5, 99.0])
    (y32, y64, yem), _ = _three(sd, x, cond, t)
    batch = m(x.to(DEV), cond.to(DEV), t.to(DEV))
    assert _judge('float times', batch, y64, y32, yem)
    one = m(x[1:2].to(DEV), cond[1:2].to(DEV), 58.5)
    assert torch.equal(one, batch[1:2])


@pytest.fixture(scope='module')
def shipped():
    """the shipped setting at 32x32, B = 2, t = 50: the device's f32 and f16x3 outputs and the three CPU yardsticks"""
    m, sd = _model(SHIPPED_SETTING)
    x, cond = _inputs(23, 2, 32, 32)
    y_f32 = m(x.to(DEV), cond.to(DEV), 50)
    m.set_precision('f16x3')
    y_h3 = m(x.to(DEV), cond.to(DEV), 50)
    m.check_saturation()
    return m, y_f32, y_h3, _three(sd, x, cond, 50)[0]


def test_forward_shipped_setting(shipped):
    _, _, y_h3, (y32, y64, yem) = shipped
    assert _judge('shipped output', y_h3, y64, y32, yem)


def test_mode_engages(shipped):
    m, y_f32, y_h3, (y32, y64, _) = shipped
    assert m.precision == 'f16x3'
    nd = int((y_f32 != y_h3).sum())
    print('shipped setting: %d of %d output elements differ between f32 and f16x3; max|f32 - f16x3| %.3g' %
          (nd, y_f32.numel(), float((y_f32 - y_h3).abs().max())))
    assert nd >= 1
    bound = min(4 * float((y32.double() - y64).abs().max()), 1e-4 * float(y64.abs().max()))
    assert float((y_f32.double().cpu() - y64).abs().max()) <= bound      # the f32 half of the pair is the exact kernel's result


def _loop(m, sd, T, eps, hw, ode=False, seed=31):
    """device trajectory; fp32, fp64 and emulated-f16x3 restatement trajectories of one loop with explicit noise"""
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    s = IRSDE(max_sigma=50, T=T, schedule='cosine', eps=eps, device='cpu')
    s.set_model(m)
    state, cond = _inputs(seed, 1, *hw)
    noise = torch.randn(T, 1, 3, *hw, generator=torch.Generator().manual_seed(seed + 1))
    tr32, tr64, trem = [], [], []
    with torch.no_grad():
        R.reverse_loop(sd, R.cast_tables(s, torch.float32), state, cond, noise, ode, tr32)
        R.reverse_loop(R.cast_sd(sd, torch.float64), R.cast_tables(s, torch.float64), state.double(), cond.double(), noise.double(), ode, tr64)
    E.reverse_loop(sd, R.cast_tables(s, torch.float32), state, cond, noise, ode, trem)
    s.set_mu(cond.to(DEV))
    if ode:
        out, traj = s.reverse_ode(state.to(DEV), trajectory=True)
    else:
        out, traj = s.reverse_sde(state.to(DEV), noise=noise.to(DEV), trajectory=True)
    assert torch.equal(out, traj[-1])
    m.check_saturation()
    return traj.cpu(), torch.stack(tr32), torch.stack(tr64), torch.stack(trem)


def test_loop_mild_schedule(net):
    m, sd = net
    traj, t32, t64, tem = _loop(m, sd, 10, 0.5, (36, 44))
    assert torch.isfinite(traj).all()
    assert all([_judge('step %d' % k, traj[k], t64[k], t32[k], tem[k]) for k in range(10)])


def test_loop_ode(net):
    m, sd = net
    traj, t32, t64, tem = _loop(m, sd, 10, 0.5, (32, 32), ode=True)
    assert all([_judge('ode step %d' % k, traj[k], t64[k], t32[k], tem[k]) for k in range(10)])


def test_loop_reference_schedule(net):
    """T 100, eps 0.005 at 32x32, judged as test_gpu_ediffsr.test_loop_reference_schedule: relative to max|x| of the fp64
    trajectory, d <= min(4 x max(spread_f32, spread_emul), 1e-4 peak); the state stays finite and below 1e3."""
    m, sd = net
    traj, t32, t64, tem = _loop(m, sd, 100, 0.005, (32, 32))
    assert torch.isfinite(traj).all()
    peak = float(t64.abs().max())
    s32 = float((t32.double() - t64).abs().max())
    sem = float((tem.double() - t64).abs().max())
    d = float((traj.double() - t64).abs().max())
    print('T=100: max|x| %.4g  spread f32 %.3g  emul %.3g (%.3g of max|x|)  max|dev - f64| %.3g  final-state dev %.3g' %
          (peak, s32, sem, max(s32, sem) / peak, d, float((traj[-1].double() - t64[-1]).abs().max())))
    assert peak < 1e3
    assert d <= min(4 * max(s32, sem), 1e-4 * peak)


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
    # the mode leaves nothing behind: f16x3 -> f32 -> f16x3 is the first f16x3 result, and f32 in between is a fresh f32 model's
    fresh, _ = _model(TEST_SETTING)
    s.set_model(fresh)
    want32 = fresh.sample(state, cond, noise=noise)
    want32g = fresh.sample(state, cond, noise=noise, graph=True)
    assert torch.equal(want32, want32g)
    try:
        m.set_precision('f32')
        assert m.precision == 'f32'
        assert torch.equal(m.sample(state, cond, noise=noise), want32), 'f32 after f16x3 == a fresh f32 model'
        assert torch.equal(m.sample(state, cond, noise=noise, graph=True), want32), 'the graph was dropped with the mode'
        assert torch.equal(m(state, cond, 3), fresh(state, cond, 3))
    finally:
        m.set_precision('f16x3')
    assert not torch.equal(a, want32), 'the two modes are different arithmetic'
    assert torch.equal(m.sample(state, cond, noise=noise), a), 'f16x3 -> f32 -> f16x3'
    assert torch.equal(m.sample(state, cond, noise=noise, graph=True), a)


def test_range_guard(net):
    from fastdiffsr_amd import _lib
    m, sd = net
    x, cond = _inputs(51, 2, 36, 44)
    x, cond = x.to(DEV), cond.to(DEV)
    m(x, cond, 37)
    m.check_saturation()                       # in range: clear
    y = m(x * 1e5, cond, 37)                   # intro reads x - cond: beyond +-65504, clamped and flagged
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
        m.set_precision('f16x3')
    m(x, cond, 37)
    m.check_saturation()


def test_training_is_refused_and_a_switch_sees_trained_weights():
    from fastdiffsr_amd import _lib
    from test_gpu_ediffsr_train import _batch, _model as _train_model
    m, sd, sde = _train_model(TEST_SETTING)
    gt, mu, state, ts = _batch(7, 2, 32, 32, [20, 80], sde)
    args = (state.to(DEV), mu.to(DEV), gt.to(DEV), ts)
    m.set_precision('f16x3')
    with pytest.raises(_lib.FdsrError, match='f16x3') as e:
        m.train_grads(*args)
    assert e.value.code == -1                  # FDSR_E_INVALID
    m.set_precision('f32')
    loss = m.train_grads(*args)
    assert torch.isfinite(loss).all()
    m.optim_step('Adam', 1e-3)
    y32 = m(args[0], args[1], 37)
    m.set_precision('f16x3')                   # the split forms are built from the stepped weights
    y = m(args[0], args[1], 37)
    m.check_saturation()
    with pytest.raises(_lib.FdsrError, match='f16x3'):
        m.optim_step('Adam', 1e-3)
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    twin = ConditionalNAFNet(**TEST_SETTING)
    twin.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    twin = twin.to(DEV).eval()
    assert not torch.equal(twin.state_dict()['intro.weight'].cpu(), sd['intro.weight'])
    assert torch.equal(twin(args[0], args[1], 37), y32)
    twin.set_precision('f16x3')
    assert torch.equal(twin(args[0], args[1], 37), y)
    m.set_precision('f32')
    assert torch.equal(m(args[0], args[1], 37), y32)
    assert torch.isfinite(m.train_grads(*args)).all()     # training goes on after the round trip


def test_cli_precision(tmp_path):
    """The eight synthetic 64^2 -> 256^2 pairs of test_gpu_ediffsr.test_cli_end_to_end, T 10 / eps 0.5."""
    import yaml
    from PIL import Image
    from fastdiffsr_amd.ediffsr import test as cli
    from fastdiffsr_amd.synth import synth_nafnet
    root = str(tmp_path)
    _write_pairs(root)
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}
    torch.save(sd, os.path.join(root, 'latest_G.pth'))
    opt = {'name': 'Test-x4', 'suffix': None, 'sde': {'max_sigma': 50, 'T': 10, 'schedule': 'cosine', 'eps': 0.5},
           'degradation': {'scale': 4}, 'path': {'pretrain_model_G': os.path.join(root, 'latest_G.pth')},
           'datasets': {'test1': {'name': 'synth', 'mode': 'LQGT', 'dataroot_GT': os.path.join(root, 'hr'), 'dataroot_LQ': os.path.join(root, 'lr')}},
           'network_G': {'which_model_G': 'ConditionalNAFNet', 'setting': TEST_SETTING}}
    with open(os.path.join(root, 'opt.yml'), 'w') as f:
        yaml.safe_dump(opt, f)
    base = ['-opt', os.path.join(root, 'opt.yml'), '--rng', 'engine', '--seed', '7']
    r1 = cli.main(base + ['--precision', 'f16x3', '--results', os.path.join(root, 'h1')])['synth']
    r4 = cli.main(base + ['--precision', 'f16x3', '--batch', '4', '--graph', '--results', os.path.join(root, 'h4')])['synth']
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
    print('f16x3 vs f32 PNGs: %d of %d values differ (%.3g), largest step %d grey level(s)' % (differ, total, differ / total, worst))
    assert worst <= 1


def test_cli_reruns_a_flagged_batch_in_f32(tmp_path, monkeypatch, caplog):
    """A batch whose range flag is raised (here: reported raised for the first batch) is run again in f32 with a logged warning:
    its PNGs are the --precision f32 ones, the other batches stay f16x3 and the model ends in f16x3."""
    import logging
    import yaml
    from PIL import Image
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet, test as cli
    from fastdiffsr_amd.synth import synth_nafnet
    root = str(tmp_path)
    _write_pairs(root, n=4)
    torch.save({k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}, os.path.join(root, 'latest_G.pth'))
    opt = {'name': 'Test-x4', 'suffix': None, 'sde': {'max_sigma': 50, 'T': 10, 'schedule': 'cosine', 'eps': 0.5},
           'degradation': {'scale': 4}, 'path': {'pretrain_model_G': os.path.join(root, 'latest_G.pth')},
           'datasets': {'test1': {'name': 'synth', 'mode': 'LQGT', 'dataroot_GT': os.path.join(root, 'hr'), 'dataroot_LQ': os.path.join(root, 'lr')}},
           'network_G': {'which_model_G': 'ConditionalNAFNet', 'setting': TEST_SETTING}}
    with open(os.path.join(root, 'opt.yml'), 'w') as f:
        yaml.safe_dump(opt, f)
    base = ['-opt', os.path.join(root, 'opt.yml'), '--rng', 'engine', '--seed', '7', '--batch', '2']
    cli.main(base + ['--precision', 'f32', '--results', os.path.join(root, 'f')])
    cli.main(base + ['--precision', 'f16x3', '--results', os.path.join(root, 'h')])
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
        cli.main(base + ['--precision', 'f16x3', '--results', os.path.join(root, 'm')])
    assert calls == ['f16x3', 'f16x3'] and modes == ['f16x3', 'f32', 'f16x3']
    assert any('again in f32' in r.getMessage() for r in caplog.records)
    png = lambda d, i: np.asarray(Image.open(os.path.join(root, d, 'synth', '%02d.png' % i)))
    for i in (0, 1):
        assert np.array_equal(png('m', i), png('f', i))
    for i in (2, 3):
        assert np.array_equal(png('m', i), png('h', i))
