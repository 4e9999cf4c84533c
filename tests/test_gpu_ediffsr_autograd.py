"""torch autograd through ConditionalNAFNet on the engine (fdsr_nafnet_forward_train / fdsr_nafnet_backward) against fp64 autograd
over tests/ediffsr_restatement.py, computed here.  Every measured value is printed before it is judged.

The loss is one the built-in head cannot form, L = (out Wmap).sum() + 0.5 (out^2).mean() with Wmap seeded normal, so the upstream
gradient is dense and O(1).  Parameter gradients are judged by the rule of tests/test_gpu_ediffsr_train.py (its _judge_grads:
1e-4 max|g64_k|, small tensors against 1e-4 typ); d inp and d cond by max|dev - g64| <= 1e-4 max|g64|.  The reference's loop
(IR-SDE l1 loss in torch, torch.optim.AdamW) is judged per step as test_short_trajectory judges its losses:
|l_dev - l64| <= max(4 |l32 - l64|, 1e-5 |l64|)."""
import copy
import gc

import pytest
import torch

import ediffsr_restatement as R
import ediffsr_train_restatement as TR
from test_gpu_ediffsr_train import DEV, EMPTY_SETTING, SDE, SHIPPED_SETTING, TEST_SETTING, _batch, _judge_grads, _model

pytestmark = pytest.mark.gpu

# the smallest sizes at which padding, crop, empty block lists and the wide level 0 can each go wrong
CASES = {
    'test': (TEST_SETTING, 2, 36, 44, [1, 100]),        # pads to 48 x 48
    'empty': (EMPTY_SETTING, 2, 18, 26, [3, 64]),       # empty block lists; pads to 20 x 28
    'shipped': (SHIPPED_SETTING, 2, 32, 32, [12, 88]),
}


def _loss(out, wmap):
    return (out * wmap).sum() + 0.5 * (out * out).mean()


def _inputs(b, h, w, t, sde):
    _, mu, state, _ = _batch(31, b, h, w, t, sde)
    wmap = torch.randn(b, 3, h, w, generator=torch.Generator().manual_seed(77))
    return state, mu, torch.tensor(t, dtype=torch.float32), wmap


def _bridge(m, x, c, t, wmap, inp_grad=True, cond_grad=True):
    """One forward + backward through the bridge: (out, d inp, d cond, {key: gradient}); what was not asked for is None."""
    for p in m.parameters():
        p.grad = None
    x = x.detach().clone().requires_grad_(inp_grad)
    c = c.detach().clone().requires_grad_(cond_grad)
    out = m(x, c, t)
    _loss(out, wmap).backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_reference_parameters()}
    return out.detach(), x.grad, c.grad, grads


@pytest.mark.parametrize('case', list(CASES))
def test_gradients(case):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    setting, b, h, w, t = CASES[case]
    m, sd, sde = _model(setting)
    x, c, tt, wmap = _inputs(b, h, w, t, sde)
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64, c64 = x.double().requires_grad_(True), c.double().requires_grad_(True)
    l64 = _loss(R.forward(leaves, x64, c64, tt), wmap.double())
    keys = list(leaves)
    gs = torch.autograd.grad(l64, [leaves[k] for k in keys] + [x64, c64], allow_unused=True)
    g64 = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(keys, gs)}
    m.requires_grad_(True)
    out, dx, dc, gdev = _bridge(m, x.to(DEV), c.to(DEV), tt, wmap.to(DEV))
    assert all(g is not None for g in gdev.values())
    fails = _judge_grads({k: v.cpu() for k, v in gdev.items()}, g64)
    for name, dev, ref in (('d inp', dx, gs[-2]), ('d cond', dc, gs[-1])):
        d, mx = float((dev.cpu().double() - ref).abs().max()), float(ref.abs().max())
        print('%-44s max|g64| %.3e  max|dev - g64| %.3e  bound %.3e' % (name, mx, d, 1e-4 * mx))
        if not d <= 1e-4 * mx:
            fails.append(name)
    assert not fails, fails


@pytest.fixture(scope='module')
def small():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m, sd, sde = _model(TEST_SETTING)
    m.requires_grad_(True)
    x, c, tt, wmap = _inputs(2, 36, 44, [1, 100], sde)
    return m, sde, x.to(DEV), c.to(DEV), tt, wmap.to(DEV)


def test_out_equals_the_no_grad_forward_and_two_runs_are_bitwise_equal(small):
    m, sde, x, c, tt, wmap = small
    with torch.no_grad():
        plain = m(x, c, tt)
    out1, dx1, dc1, g1 = _bridge(m, x, c, tt, wmap)
    out2, dx2, dc2, g2 = _bridge(m, x, c, tt, wmap)
    print('bridge out == no_grad forward: %s;  second run: out %s, d inp %s, d cond %s, parameters %d of %d equal' % (
        torch.equal(out1, plain), torch.equal(out1, out2), torch.equal(dx1, dx2), torch.equal(dc1, dc2),
        sum(torch.equal(g1[k], g2[k]) for k in g1), len(g1)))
    assert torch.equal(out1, plain) and torch.equal(out1, out2)
    assert torch.equal(dx1, dx2) and torch.equal(dc1, dc2)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert float(dx1.abs().max()) > 0 and float(dc1.abs().max()) > 0


def test_partial_requests_return_the_same_bits(small):
    m, sde, x, c, tt, wmap = small
    _, dx, dc, g = _bridge(m, x, c, tt, wmap)
    _, dx_p, dc_p, g_p = _bridge(m, x, c, tt, wmap, inp_grad=False, cond_grad=False)       # only the parameters
    assert dx_p is None and dc_p is None
    m.requires_grad_(False)
    try:
        _, dx_i, dc_i, g_i = _bridge(m, x, c, tt, wmap, cond_grad=False)                   # only inp
    finally:
        m.requires_grad_(True)
    assert dc_i is None and all(v is None for v in g_i.values())
    print('only parameters: %d of %d equal;  only inp: d inp equal %s' % (sum(torch.equal(g[k], g_p[k]) for k in g), len(g),
                                                                           torch.equal(dx, dx_i)))
    assert all(torch.equal(g[k], g_p[k]) for k in g)
    assert torch.equal(dx, dx_i)


def test_ticket_rules(small):
    m, sde, x, c, tt, wmap = small
    gt = torch.rand(x.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    ts = torch.tensor([3, 64]).reshape(2, 1, 1, 1)

    def stale(between, match):
        out = m(x, c, tt)
        between()
        with pytest.raises(Exception, match=match) as e:
            _loss(out, wmap).backward()
        print('%s: %s' % (match, e.value))
        assert 'stale' in str(e.value)

    stale(lambda: m(x, c, tt), 'fdsr_nafnet_forward_train')
    stale(lambda: m.train_grads(x, c, gt, ts), 'fdsr_nafnet_train_grads')
    stale(lambda: m.optim_step('AdamW', 1e-6, (0.9, 0.99), 1e-8, 0.0), 'fdsr_nafnet_optim_step')
    loss = _loss(m(x, c, tt), wmap)
    loss.backward(retain_graph=True)
    with pytest.raises(Exception, match='fdsr_nafnet_backward') as e:
        loss.backward()
    print('second backward: %s' % e.value)
    assert 'stale' in str(e.value)
    # the 16-bit modes: what train_grads raises, under the bridge's own name
    try:
        for mode in ('f16x3', 'f16'):
            m.set_precision(mode)
            with pytest.raises(Exception) as e_train:
                m.train_grads(x, c, gt, ts)
            with pytest.raises(Exception) as e_bridge:
                m(x, c, tt)
            print('%s: %s' % (mode, e_bridge.value))
            assert type(e_bridge.value) is type(e_train.value)
            assert 'only' in str(e_train.value)
            assert str(e_bridge.value) == str(e_train.value).replace('fdsr_nafnet_train_grads', 'fdsr_nafnet_forward_train')
            m.set_precision('f32')
    finally:
        m.set_precision('f32')
    _bridge(m, x, c, tt, wmap)   # and the module still trains


def _matching_l1(predict, target):
    return (predict - target).abs().flatten(1).mean(dim=1).mean()


def test_the_reference_loop_and_the_device_weight_path(monkeypatch):
    """Five steps of the reference's optimize_parameters with its own pieces: IRSDE's loss terms in torch, backward(), AdamW."""
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet, IRSDE
    lib, host_loads = _lib.load(), []
    real = lib.fdsr_nafnet_load_weight
    monkeypatch.setattr(lib, 'fdsr_nafnet_load_weight', lambda *a: (host_loads.append(a[1]), real(*a))[1])
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m, sd, sde_cpu = _model(TEST_SETTING)
    m.requires_grad_(True)
    sde = IRSDE(device=DEV, **SDE)
    sde.set_model(m)
    lr, betas, eps, wd = 4e-5, (0.9, 0.99), 1e-8, 0.0
    opt = torch.optim.AdamW(m.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=wd)
    t32, t64 = TR.cast_tables(sde_cpu, torch.float32), TR.cast_tables(sde_cpu, torch.float64)
    w32 = {k: v.clone() for k, v in sd.items()}
    w64 = R.cast_sd(sd, torch.float64)
    s32, s64 = {k: {} for k in sd}, {k: {} for k in sd}
    fails = []
    for step in range(5):
        gt, mu, state, ts = _batch(50 + step, 2, 32, 32, [5 + 17 * step, 96 - 11 * step], sde_cpu)
        x, c, g, t = state.to(DEV), mu.to(DEV), gt.to(DEV), ts.to(DEV)
        sde.set_mu(c)
        opt.zero_grad()
        noise = sde.noise_fn(x, t.squeeze())
        score = sde.get_score_from_noise(noise, t)
        loss = _matching_l1(sde.reverse_sde_step_mean(x, score, t), sde.reverse_optimum_step(x, g, t))
        loss.backward()
        opt.step()
        ldev = float(loss.detach())
        l32, g32 = TR.loss_and_grads(w32, t32, state, mu, gt, ts)
        l64, g64 = TR.loss_and_grads(w64, t64, state.double(), mu.double(), gt.double(), ts)
        w32 = {k: TR.optim_step('AdamW', w32[k], g32[k], s32[k], lr, *betas, eps, wd) for k in w32}
        w64 = {k: TR.optim_step('AdamW', w64[k], g64[k], s64[k], lr, *betas, eps, wd) for k in w64}
        l32, l64 = float(l32), float(l64)
        bound = max(4 * abs(l32 - l64), 1e-5 * abs(l64))
        print('step %d: loss dev %.9g  f32 %.9g  f64 %.12g  |f32 - f64| %.3e  |dev - f64| %.3e  bound %.3e' % (
            step + 1, ldev, l32, l64, abs(l32 - l64), abs(ldev - l64), bound))
        if not abs(ldev - l64) <= bound:
            fails.append(step + 1)
        if step == 0:
            first_upload = len(host_loads)
    assert not fails, fails
    print('tensors loaded through the host: %d by the first forward, %d by the four steps after it' % (first_upload, len(host_loads) - first_upload))
    assert first_upload == len(sd) and len(host_loads) == first_upload      # a torch optimizer's step costs no host round trip
    monkeypatch.undo()
    # the weights the engine holds came over the device path; a fresh module packs the same state_dict on the host
    stepped = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert any(not torch.equal(stepped[k], sd[k]) for k in sd)
    short = IRSDE(max_sigma=50, T=4, schedule='cosine', eps=0.005, device='cpu')
    short.set_model(m)
    x4, c4 = x.detach(), c.detach()
    noise4 = torch.randn(4, 2, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    got = m.sample(x4, c4, noise=noise4)
    fresh = ConditionalNAFNet(**TEST_SETTING)
    fresh.load_state_dict(stepped, strict=True)
    fresh = fresh.to(DEV).eval()
    short.set_model(fresh)
    want = fresh.sample(x4, c4, noise=noise4)
    print('sample after five bridged steps == a fresh module: %s (max|diff| %.3e)' % (torch.equal(got, want), float((got - want).abs().max())))
    assert torch.equal(got, want)


def test_deep_copy_of_a_module_with_a_handle(small):
    _, sde, x, c, tt, wmap = small
    m, _, _ = _model(TEST_SETTING)
    m.requires_grad_(True)
    _bridge(m, x, c, tt, wmap)          # a model in training: it has an engine object, workspaces and an upload stamp
    assert m._h is not None
    ema = copy.deepcopy(m)              # what ema_pytorch.EMA does
    assert ema._h is None and ema._uploaded is None and not ema._ws
    with torch.no_grad():
        a, b = m(x, c, tt), ema(x, c, tt)
    assert ema._h is not None and ema._h.value != m._h.value
    print('copy == original: %s' % torch.equal(a, b))
    assert torch.equal(a, b)
    del m
    gc.collect()
    with torch.no_grad():
        assert torch.equal(ema(x, c, tt), a)
    second = copy.deepcopy(ema)
    del ema
    gc.collect()
    with torch.no_grad():
        assert torch.equal(second(x, c, tt), a)
