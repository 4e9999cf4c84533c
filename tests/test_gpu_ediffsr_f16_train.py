"""EDiffSR training under f16 activation storage (ConditionalNAFNet.set_train_precision('f16'): the f16-storage forward into
half-size slots, fp32 gradients) on the device.  Every measured value is printed before it is judged.

Gradients, per tensor k, against fp64 autograd over tests/ediffsr_train_restatement.py: max|g_dev - g64| <= max(4 s_k, b_k), where
s_k = max|g_emul - g64| is the distance of the CPU emulation of the mode's arithmetic (tests/ediffsr_f16_train_emulation.py, computed
here) and b_k the fp32 bound of tests/test_gpu_ediffsr_train.py: 1e-4 max|g64_k| for a tensor with max|g64_k| >= 1e-5 typ, 1e-4 typ
for a smaller one, typ the median over tensors of max|g64|.  Loss: |l_dev - l64| <= max(4 |l_emul - l64|, 2^-22 |l64|)."""
import math
import warnings

import numpy as np
import pytest
import torch

import ediffsr_f16_train_emulation as ET
from test_gpu_ediffsr_train import DEV, SHIPPED_SETTING, TEST_SETTING, _batch, _model

pytestmark = pytest.mark.gpu


def _f16_model(setting, seed=0):
    m, sd, sde = _model(setting, seed)
    m.set_train_precision('f16')
    return m, sd, sde


@pytest.mark.parametrize('case', list(ET.CASES))
def test_gradients(case):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    setting, b, h, w, t, loss_type = ET.CASES[case]
    r = ET.reference(case)
    gt, mu, state, ts = r['batch']
    m, sd, sde = _f16_model(setting)
    out = m.train_grads(state.to(DEV), mu.to(DEV), gt.to(DEV), ts, loss_type=loss_type).cpu()
    m.check_saturation()
    gdev = m.grads()
    g64, s = r['g64'], r['s']
    assert len(gdev) == len(g64)
    mx = {k: float(v.abs().max()) for k, v in g64.items()}
    typ = float(np.median(list(mx.values())))
    fails = []
    for k, ref in g64.items():
        d = float((gdev[k].double() - ref).abs().max())
        big = mx[k] >= 1e-5 * typ
        bk = 1e-4 * (mx[k] if big else typ)
        bound = max(4 * s[k], bk)
        ok = d <= bound
        print('%-44s max|g64| %.3e  max|dev - g64| %.3e  s %.3e  b %.3e (%s)  bound %.3e%s' % (
            k, mx[k], d, s[k], bk, 'rel' if big else 'abs', bound, '' if ok else '  FAIL'))
        if not ok:
            fails.append(k)
    ldev, l64, le = float(out[0]), r['l64'], r['l_emul']
    lbound = max(4 * abs(le - l64), 2.0 ** -22 * abs(l64))
    print('case %s: typ %.3e; loss dev %.9g  emul %.9g  f64 %.12g  |dev - f64| %.3e  bound %.3e' % (case, typ, ldev, le, l64, abs(ldev - l64), lbound))
    assert not fails, fails
    assert abs(ldev - l64) <= lbound


@pytest.fixture(scope='module')
def small():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return _f16_model(TEST_SETTING)


def test_bitwise_properties(small):
    m, sd, sde = small
    gt, mu, state, ts = _batch(32, 2, 36, 44, [3, 64], sde)
    x, c, g = state.to(DEV), mu.to(DEV), gt.to(DEV)
    before = m(x, c, 37)
    l1 = m.train_grads(x, c, g, ts).cpu()
    g1 = m.grads()
    after = m(x, c, 37)
    l2 = m.train_grads(x, c, g, ts).cpu()
    g2 = m.grads()
    assert torch.equal(before, after)                # the fp32 inference forward: training f16 does not touch it
    assert torch.equal(l1, l2)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert any(float(v.abs().max()) > 0 for v in g1.values())
    # through the bridge: out is the sampling 'f16' forward bit for bit, and backward from the built-in loss's own d out gives
    # train_grads' gradients bit for bit
    tt = ts.reshape(-1).float().to(DEV)
    try:
        m.requires_grad_(True)
        out = m(x, c, tt)
        assert out.requires_grad
        out.backward(_builtin_dout(sde, out.detach().cpu(), state, mu, gt, ts).to(DEV))
        gb = {k: p.grad.detach().cpu() for k, p in m.named_reference_parameters()}
    finally:
        m.requires_grad_(False)
    m.set_precision('f16')
    try:
        want = m(x, c, tt)
    finally:
        m.set_precision('f32')
    assert torch.equal(out.detach(), want)
    diffs = [k for k in g1 if not torch.equal(gb[k], g1[k])]
    assert not diffs, diffs
    assert m.train_precision == 'f16' and m.precision == 'f32'


def _builtin_dout(sde, eps, x, mu, x0, ts, weight=1.0):
    """d loss / d eps of the engine's l1 loss head (fdsr_nafnet_train_grads), its rounded fp32 operations in its order, on the CPU"""
    f = torch.float32
    t = ts.reshape(-1, 1, 1, 1)
    theta, sigma, sbar, dt = sde.thetas[t].to(f), sde.sigmas[t].to(f), sde.sigma_bars[t].to(f), sde.dt.to(f)
    dtd = float(dt)
    A = torch.exp(-sde.thetas[t].double() * dtd)
    B = torch.exp(-sde.thetas_cumsum[t].double() * dtd)
    C = torch.exp(-sde.thetas_cumsum[t - 1].double() * dtd)
    term1, term2 = (A * (1 - C * C) / (1 - B * B)).float(), (C * (1 - A * A) / (1 - B * B)).float()
    s2 = sigma * sigma
    score = (-eps) / sbar
    expect = x - (theta * (mu - x) - s2 * score) * dt
    optimum = (term1 * (x - mu) + term2 * (x0 - mu)) + mu
    b, _, h, w = x.shape
    gscale = torch.tensor(weight, dtype=f) / (torch.tensor(float(b), dtype=f) * 3.0 * float(h * w))
    return torch.sign(expect - optimum) * gscale * (-(s2 / sbar) * dt)


def _fresh(setting, state_dict):
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    twin = ConditionalNAFNet(**setting)
    twin.load_state_dict({k: v.detach().cpu() for k, v in state_dict.items()}, strict=True)
    return twin.to(DEV).eval()


def _forwards(m, x, c):
    out = {}
    try:
        for mode in ('f16', 'f32', 'f16x3', 'f32'):
            m.set_precision(mode)
            out[mode] = m(x, c, 37)
            m.check_saturation()
    finally:
        m.set_precision('f32')
    return out


@pytest.mark.parametrize('path', ['engine', 'bridge'])
def test_forms_after_stepping_equal_a_fresh_upload(path):
    """three AdamW steps under train f16; the f16 forms the device rebuilt serve the NEXT f16 forward (forward_train under the bridge,
    bit-equal to the sampling 'f16' forward of a twin whose forms the host built), and every sampling mode equals the twin's"""
    m, sd, sde = _f16_model(TEST_SETTING)
    opt = None
    if path == 'bridge':
        m.requires_grad_(True)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.99), weight_decay=0.01)
    for step in range(3):
        gt, mu, state, ts = _batch(60 + step, 2, 32, 32, [5 + 30 * step, 90 - 20 * step], sde)
        x, c, g = state.to(DEV), mu.to(DEV), gt.to(DEV)
        if path == 'engine':
            assert torch.isfinite(m.train_grads(x, c, g, ts)).all()
            m.optim_step('AdamW', 1e-3, (0.9, 0.99), 1e-8, 0.01)
        else:
            opt.zero_grad(set_to_none=True)
            (m(x, c, ts.reshape(-1).float().to(DEV)) - g).abs().mean().backward()
            opt.step()
    m.check_saturation()
    tt = torch.tensor([11.0, 63.0], device=DEV)
    if path == 'engine':
        m.requires_grad_(True)
    kept = m(x, c, tt).detach()                 # forward_train on the rebuilt forms (the bridge hands the weights over first)
    m.requires_grad_(False)
    stepped = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert any(not torch.equal(stepped[k], sd[k]) for k in sd)
    twin = _fresh(TEST_SETTING, stepped)
    twin.set_precision('f16')
    assert torch.equal(twin(x, c, tt), kept)
    twin.set_precision('f32')
    a, b = _forwards(m, x, c), _forwards(twin, x, c)
    for mode in a:
        assert torch.equal(a[mode], b[mode]), mode


def test_workspace_is_about_half():
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    m = ConditionalNAFNet(**SHIPPED_SETTING)
    f32 = m.train_workspace_bytes(16, 256, 256)
    small32 = m.train_workspace_bytes(2, 32, 32)
    m.set_train_precision('f16')
    f16 = m.train_workspace_bytes(16, 256, 256)
    print('train workspace B 16 at 256x256: f32 %.2f GiB, f16 %.2f GiB, ratio %.3f' % (f32 / 2 ** 30, f16 / 2 ** 30, f16 / f32))
    assert f16 <= 0.60 * f32
    m.set_train_precision('f32')
    assert m.train_workspace_bytes(16, 256, 256) == f32 and m.train_workspace_bytes(2, 32, 32) == small32


def _opt(setting, niter=4):
    return dict(is_train=True, network_G=dict(which_model_G='ConditionalNAFNet', setting=setting), path=dict(pretrain_model_G=None),
                train=dict(optimizer='AdamW', lr_G=1e-3, lr_scheme='TrueCosineAnnealingLR', beta1=0.9, beta2=0.99, niter=niter, eta_min=1e-7,
                           loss_type='l1', weight=1.0))


def test_range_guard_skips_the_step():
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.ediffsr import IRSDE
    from fastdiffsr_amd.ediffsr.denoising_model import DenoisingModel
    from fastdiffsr_amd.synth import synth_nafnet
    from test_gpu_ediffsr_train import SDE
    good = {k: torch.from_numpy(v).clone() for k, v in synth_nafnet(0, **TEST_SETTING).items()}
    bad = dict(good)
    bad['intro.bias'] = good['intro.bias'] * 0 + 1e5          # every staged input is in range; intro's OUTPUT is not
    dm = DenoisingModel(_opt(TEST_SETTING), train_precision='f16')
    assert dm.model.train_precision == 'f16'
    dm.model.load_state_dict(bad, strict=True)
    sde = IRSDE(device='cpu', **SDE)
    sde.set_model(dm.model)
    gt, mu, state, ts = _batch(35, 2, 36, 44, [20, 80], sde)
    dm.model.train_grads(state.to(DEV), mu.to(DEV), gt.to(DEV), ts)
    with pytest.raises(_lib.FdsrSaturated, match='set_train_storage'):
        dm.model.check_saturation()
    dm.model.check_saturation()                                # cleared by the read
    dm.feed_data(state, mu, gt)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        dm.optimize_parameters(7, ts, sde)
    assert len(w) == 1 and 'iteration 7' in str(w[0].message)
    assert (dm.skipped_steps, dm.consecutive_skips) == (1, 1)
    now = {k: v.detach().cpu() for k, v in dm.model.state_dict().items()}
    assert all(torch.equal(now[k], bad[k]) for k in bad)       # the step was not taken
    dm.model.load_state_dict(good, strict=True)                # a clean batch afterwards trains
    dm.optimize_parameters(8, ts, sde)
    assert (dm.skipped_steps, dm.consecutive_skips) == (1, 0) and math.isfinite(dm.log_dict['loss'])
    now = {k: v.detach().cpu() for k, v in dm.model.state_dict().items()}
    assert any(not torch.equal(now[k], good[k]) for k in good)


def test_refusals(small):
    from fastdiffsr_amd import _lib
    m, sd, sde = small
    gt, mu, state, ts = _batch(36, 2, 32, 32, [20, 80], sde)
    x, c, g = state.to(DEV), mu.to(DEV), gt.to(DEV)
    tt = ts.reshape(-1).float().to(DEV)
    plain, _, _ = _model(TEST_SETTING)
    try:
        for mode in ('f16x3', 'f16'):                          # the sampling side decides, whatever the train setting
            msgs = []
            for mod in (plain, m):
                mod.set_precision(mode)
                with pytest.raises(_lib.FdsrError) as e:
                    mod.train_grads(x, c, g, ts)
                assert e.value.code == -1
                msgs.append(str(e.value))
                mod.set_precision('f32')
            print('%s: %s' % (mode, msgs[1]))
            assert msgs[0] == msgs[1] and 'only' in msgs[1]
    finally:
        plain.set_precision('f32')
        m.set_precision('f32')
    try:                                                       # a switch between forward_train and backward: the ticket is stale
        m.requires_grad_(True)
        for switch in ('f32', 'f16'):
            out = m(x, c, tt)
            m.set_train_precision('f32' if m.train_precision == 'f16' else 'f16')
            with pytest.raises(_lib.FdsrError, match='fdsr_nafnet_set_train_storage') as e:
                out.sum().backward()
            print(e.value)
            assert 'stale' in str(e.value) and e.value.code == -3      # FDSR_E_STATE
        assert m.train_precision == 'f16'
        m(x, c, tt).sum().backward()                           # and the module still trains
    finally:
        m.requires_grad_(False)
        m.set_train_precision('f16')


def _write_pairs(root, n=8):
    from PIL import Image
    rng = np.random.RandomState(7)
    for d in ('hr', 'lr'):
        (root / d).mkdir()
    for i in range(n):
        hr = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
        Image.fromarray(hr).save(root / 'hr' / ('%d.png' % i))
        Image.fromarray(hr.reshape(16, 4, 16, 4, 3).mean(axis=(1, 3)).astype(np.uint8)).save(root / 'lr' / ('%d.png' % i))


def test_cli_end_to_end(tmp_path):
    """python -m fastdiffsr_amd.ediffsr.train --precision f16 on eight synthetic 16^2 -> 64^2 pairs: four steps, a checkpoint, a resume.
    The CLI draws its data stream anew on a resume, so the bitwise repeat is checked one level down, on DenoisingModel with the same
    files the CLI writes: steps 1 2 3 without a stop against steps 1 2, {2}_G.pth + {2}.state, a fresh model, step 3."""
    import yaml
    from fastdiffsr_amd.ediffsr import IRSDE, train
    from fastdiffsr_amd.ediffsr.denoising_model import DenoisingModel
    from fastdiffsr_amd.synth import synth_nafnet
    from test_gpu_ediffsr_train import SDE
    _write_pairs(tmp_path)
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}
    torch.save(sd, tmp_path / 'init_G.pth')
    ds = dict(dataroot_GT=str(tmp_path / 'hr'), dataroot_LQ=str(tmp_path / 'lr'))
    opt = dict(name='cli16', sde=dict(max_sigma=50, T=4, schedule='cosine', eps=0.005), degradation=dict(scale=4),
               datasets=dict(train=dict(ds, name='t', batch_size=2, GT_size=64, use_flip=True, use_rot=True)),
               network_G=dict(which_model_G='ConditionalNAFNet', setting=TEST_SETTING),
               path=dict(pretrain_model_G=str(tmp_path / 'init_G.pth'), strict_load=True, resume_state=None),
               train=dict(optimizer='AdamW', lr_G=4e-5, lr_scheme='TrueCosineAnnealingLR', beta1=0.9, beta2=0.99, niter=4, warmup_iter=-1,
                          eta_min=1e-7, is_weighted=False, loss_type='l1', weight=1.0, manual_seed=0),
               logger=dict(print_freq=1, save_checkpoint_freq=2))
    (tmp_path / 'opt.yml').write_text(yaml.safe_dump(opt))
    root = tmp_path / 'exp'
    res = train.main(['-opt', str(tmp_path / 'opt.yml'), '--root', str(root), '--precision', 'f16'])
    print(res)
    assert res['iter'] == 4 and len(res['losses']) == 4 and all(math.isfinite(v) for v in res['losses']) and res['skipped'] == 0
    saved = torch.load(root / 'models' / '4_G.pth', map_location='cpu', weights_only=True)
    assert any(not torch.equal(saved[k], sd[k]) for k in sd)
    opt['path']['resume_state'] = str(root / 'training_state' / '2.state')
    (tmp_path / 'opt2.yml').write_text(yaml.safe_dump(opt))
    res2 = train.main(['-opt', str(tmp_path / 'opt2.yml'), '--root', str(root), '--precision', 'f16'])
    print(res2)
    assert res2['iter'] == 4 and len(res2['losses']) == 2 and res2['opt_step'] == 4 and all(math.isfinite(v) for v in res2['losses'])

    sde = IRSDE(device='cpu', **SDE)
    batches = [_batch(70 + k, 2, 64, 64, [10 + 40 * k, 95 - 30 * k], sde) for k in range(3)]

    def model_at(weights, state_dir):
        o = _opt(TEST_SETTING)
        o['path'] = dict(pretrain_model_G=None, models=str(state_dir), training_state=str(state_dir))
        dm = DenoisingModel(o, train_precision='f16')
        dm.model.load_state_dict(weights, strict=True)
        sde.set_model(dm.model)
        return dm

    def step(dm, k):
        gt, mu, state, ts = batches[k]
        dm.feed_data(state, mu, gt)
        dm.optimize_parameters(k + 1, ts, sde)
        dm.update_learning_rate(k + 1)
        return dm.log_dict['loss']

    (tmp_path / 'ck').mkdir()
    whole = model_at(sd, tmp_path / 'ck')
    step(whole, 0)
    step(whole, 1)
    g_path, s_path = whole.save(2), whole.save_training_state(0, 2)
    l_whole = step(whole, 2)
    resumed = model_at(torch.load(g_path, map_location='cpu', weights_only=True), tmp_path / 'ck')
    resumed.resume_training(torch.load(s_path, map_location='cpu', weights_only=False))
    l_resumed = step(resumed, 2)
    print('step 3: uninterrupted %.9g, resumed %.9g' % (l_whole, l_resumed))
    assert l_whole == l_resumed
    a, b = whole.model.state_dict(), resumed.model.state_dict()
    assert all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)
