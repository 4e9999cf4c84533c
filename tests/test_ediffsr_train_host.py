"""EDiffSR training without a GPU: IRSDE's training terms against the plain-torch restatement and the reference's draw order,
the host-side learning-rate schedules against torch's, the options fixture, and the new C-ABI calls' refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import ediffsr_train_restatement as TR

FDSR_E_INVALID, FDSR_E_KEY, FDSR_E_STATE = -1, -2, -3
SDE = dict(max_sigma=50, T=100, schedule='cosine', eps=0.005)


def _sde():
    from fastdiffsr_amd.ediffsr.sde import IRSDE
    return IRSDE(device='cpu', **SDE)


def test_generate_random_states_draws_randint_then_randn():
    s = _sde()
    g = torch.Generator().manual_seed(3)
    x0, mu = torch.rand(3, 3, 12, 20, generator=g), torch.rand(3, 3, 12, 20, generator=g)
    with pytest.raises(NotImplementedError, match='set_model'):
        s.generate_random_states(x0, mu)          # no model yet: nothing to train
    s.set_model(lambda x, mu, t: x)                # any callable; train.py sets the network before its loop, as the reference does
    torch.manual_seed(11)
    ts, states = s.generate_random_states(x0, mu)
    torch.manual_seed(11)
    want_t = torch.randint(1, s.T + 1, (3, 1, 1, 1)).long()
    mean = mu + (x0 - mu) * torch.exp(-s.thetas_cumsum[want_t] * s.dt)
    want = torch.randn_like(mean) * s.sigma_bars[want_t] + mean
    assert ts.dtype == torch.int64 and tuple(ts.shape) == (3, 1, 1, 1) and torch.equal(ts, want_t)
    assert states.dtype == torch.float32 and torch.equal(states, want)
    assert int(ts.min()) >= 1 and int(ts.max()) <= s.T


def test_sde_training_terms_equal_the_restatement():
    s = _sde()
    g = torch.Generator().manual_seed(4)
    x0, mu, xt, noise = (torch.rand(2, 3, 8, 8, generator=g) for _ in range(4))
    t = torch.tensor([1, 100]).reshape(2, 1, 1, 1)
    s.set_mu(mu)
    tb = TR.cast_tables(s, torch.float32)
    score = s.get_score_from_noise(noise, t)
    assert torch.equal(score, -noise / s.sigma_bars[t])
    assert torch.equal(s.reverse_sde_step_mean(xt, score, t), TR.reverse_sde_step_mean(tb, xt, mu, score, t))
    opt = s.reverse_optimum_step(xt, x0, t)
    assert torch.equal(opt, TR.reverse_optimum_step(tb, xt, x0, mu, t))
    assert torch.equal(opt[0], x0[0])      # t = 1: term1 is exactly 0 and term2 exactly 1 -- the optimum is x0
    o64 = TR.reverse_optimum_step(TR.cast_tables(s, torch.float64), xt.double(), x0.double(), mu.double(), t)
    assert float((opt.double() - o64).abs().max()) < 1e-5


def test_restatement_loss_and_optimizers_against_torch():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(3, 3, 5, 7, generator=g), torch.randn(3, 3, 5, 7, generator=g)
    assert torch.allclose(TR.matching_loss(a, b, 'l1'), torch.nn.functional.l1_loss(a, b), rtol=1e-6)
    assert torch.allclose(TR.matching_loss(a, b, 'l2'), torch.nn.functional.mse_loss(a, b), rtol=1e-6)
    for kind, cls in (('Adam', torch.optim.Adam), ('AdamW', torch.optim.AdamW)):
        for wd in (0.0, 0.01):
            p = torch.nn.Parameter(torch.randn(64, generator=g))
            o = cls([p], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, foreach=False)
            mine, st = p.detach().clone().double(), {}
            for _ in range(3):
                grad = torch.randn(64, generator=g)
                p.grad = grad.clone()
                o.step()
                mine = TR.optim_step(kind, mine, grad.double(), st, 1e-3, 0.9, 0.99, 1e-8, wd)
            assert float((p.detach().double() - mine).abs().max()) < 1e-6, (kind, wd)
    p, st = torch.tensor([1.0, -2.0, 3.0]), {}
    q = TR.optim_step('Lion', p, torch.tensor([0.5, -0.5, 0.0]), st, 0.1, 0.9, 0.99, 0.0, 0.5)
    assert torch.allclose(q, p * 0.95 - 0.1 * torch.tensor([1.0, -1.0, 0.0]))
    assert torch.allclose(st['exp_avg'], torch.tensor([0.005, -0.005, 0.0]))


def test_lr_schedules():
    from fastdiffsr_amd.ediffsr.denoising_model import cosine_annealing_lr, multistep_restart_lr
    p = torch.nn.Parameter(torch.zeros(1))
    o = torch.optim.SGD([p], lr=4e-5)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=40, eta_min=1e-7)
    for k in range(1, 41):
        o.step()
        sch.step()
        assert math.isclose(o.param_groups[0]['lr'], cosine_annealing_lr(4e-5, k, 40, 1e-7), rel_tol=1e-9, abs_tol=1e-15), k
    # the reference's MultiStepLR_Restart recursion: restart -> initial_lr * weight; milestone -> lr * gamma; else unchanged
    ms, restarts, weights, gamma = [5, 9, 14, 17], [12], [0.5], 0.5
    lr = 1e-3
    for k in range(1, 25):
        if k in restarts:
            lr = 1e-3 * weights[restarts.index(k)]
        elif k in ms:
            lr *= gamma
        assert math.isclose(lr, multistep_restart_lr(1e-3, k, ms, gamma, restarts, weights), rel_tol=1e-12), k


def test_train_options_fixture():
    from fastdiffsr_amd.ediffsr.train import parse_options
    opt = parse_options(os.path.join(os.path.dirname(__file__), 'golden', 'ediffsr_setting_mfe_Train_x4.yml'))
    t = opt['train']
    assert (t['optimizer'], t['lr_G'], t['lr_scheme'], t['beta1'], t['beta2']) == ('AdamW', 4e-5, 'TrueCosineAnnealingLR', 0.9, 0.99)
    assert (t['loss_type'], t['weight'], t['is_weighted'], t['eta_min']) == ('l1', 1.0, False, 1e-7)
    assert opt['datasets']['train']['batch_size'] == 2 and opt['datasets']['train']['GT_size'] == 256 and opt['scale'] == 4
    assert opt['network_G']['setting'] == dict(width=64, enc_blk_nums=[14, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def test_train_abi_refusals_without_a_gpu():
    from fastdiffsr_amd import _lib as L, build
    build.build(force=False, verbose=False)
    lib = L.load()
    c = L.FdsrNafnetConfig()
    c.img_channel, c.width, c.n_levels, c.middle_blk_num = 3, 16, 4, 1
    for i in range(4):
        c.enc_blk_nums[i], c.dec_blk_nums[i] = 1, 1
    h = C.c_void_p()
    assert lib.fdsr_nafnet_create(C.byref(c), C.byref(h)) == 0
    try:
        fake, big, n = C.c_void_p(4096), C.c_size_t(1 << 40), C.c_size_t()
        assert lib.fdsr_nafnet_train_workspace_bytes(h, 0, 8, 8, C.byref(n)) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_train_workspace_bytes(h, 1, 8, 8, None) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_train_workspace_bytes(h, 2, 33, 33, C.byref(n)) == 0
        m, f = C.c_size_t(), C.c_size_t()
        assert lib.fdsr_nafnet_train_workspace_bytes(h, 2, 48, 48, C.byref(m)) == 0 and lib.fdsr_nafnet_workspace_bytes(h, 2, 48, 48, C.byref(f)) == 0
        assert m.value >= n.value > f.value > 0       # 33 pads to 48; only the loss's block sums depend on the unpadded size
        args = (0, 1.0, fake, 1, 32, 32, fake, big, None)
        assert lib.fdsr_nafnet_train_grads(h, fake, fake, fake, None, *args) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_train_grads(None, fake, fake, fake, fake, *args) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_train_grads(h, fake, fake, fake, fake, 0 | L.FDSR_NAFNET_LOSS_WEIGHTED, 1.0, fake, 1, 32, 32, fake, big, None) == FDSR_E_INVALID
        assert b'is_weighted' in lib.fdsr_last_error(None)
        assert lib.fdsr_nafnet_train_grads(h, fake, fake, fake, fake, 2, 1.0, fake, 1, 32, 32, fake, big, None) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_train_grads(h, fake, fake, fake, fake, *args) == FDSR_E_STATE           # weights missing
        assert lib.fdsr_nafnet_optim_step(h, 3, 1e-3, 0.9, 0.99, 1e-8, 0.0, None) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_optim_step(h, 1, 1e-3, 1.0, 0.99, 1e-8, 0.0, None) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_optim_step(h, 1, 1e-3, 0.9, 0.99, 1e-8, 0.0, None) == FDSR_E_STATE    # no gradients
        buf = np.zeros(16 * 6 * 9, dtype=np.float32)
        assert lib.fdsr_nafnet_read_grad(h, b'intro.weight', C.c_void_p(buf.ctypes.data)) == FDSR_E_STATE
        assert lib.fdsr_nafnet_read_grad(h, b'intro.wait', C.c_void_p(buf.ctypes.data)) == FDSR_E_KEY
        assert lib.fdsr_nafnet_read_grad(h, b'intro.weight', None) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_read_weight(h, b'intro.weight', C.c_void_p(buf.ctypes.data), 0, None) == FDSR_E_STATE
        assert lib.fdsr_nafnet_read_weight(h, b'nope', C.c_void_p(buf.ctypes.data), 0, None) == FDSR_E_KEY
        p, cnt, step = C.c_void_p(), C.c_size_t(), C.c_int64()
        assert lib.fdsr_nafnet_grad_buffer(h, C.byref(p), C.byref(cnt)) == FDSR_E_STATE
        assert lib.fdsr_nafnet_grad_buffer(h, None, C.byref(cnt)) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_optim_get_state(h, b'intro.weight', None, None, C.byref(step)) == FDSR_E_STATE
        assert lib.fdsr_nafnet_optim_get_state(h, b'nope', None, None, C.byref(step)) == FDSR_E_KEY
        assert lib.fdsr_nafnet_optim_set_state(h, b'intro.weight', None, None, 3) == FDSR_E_STATE     # weights missing
        assert lib.fdsr_nafnet_optim_set_state(h, b'intro.weight', None, None, -1) == FDSR_E_INVALID
        cum = (C.c_float * 11)()
        assert lib.fdsr_nafnet_set_thetas_cumsum(h, 10, None) == FDSR_E_INVALID
        assert lib.fdsr_nafnet_set_thetas_cumsum(h, 10, cum) == FDSR_E_STATE                           # fdsr_nafnet_set_sde first
    finally:
        lib.fdsr_nafnet_destroy(h)


# ---- tests/golden/ediffsr_train_step.npz (tools/make_ediffsr_train_golden.py): the reference's own modules, fp32 ----
# The bar is test_ediffsr_host.py's for the forward golden: the same torch kernels in the same order up to one pool, 2^-20 of the
# tensor's max.  A gradient is judged against max(its own max, the median max over tensors): three tensors are exactly zero in the
# reference and rounding noise does not scale with them.  A tensor's fp64 sum may collect that noise from every element.
NOISE = 2.0 ** -20
GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'ediffsr_train_step.npz')
TEST_SETTING = dict(width=16, enc_blk_nums=[2, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


@pytest.fixture(scope='module')
def gold():
    with np.load(GOLD) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope='module')
def step(gold):
    """The restatement's fp32 step on the golden's inputs, computed once: (sd, loss l1, loss l2, expect, optimum, grads)."""
    from fastdiffsr_amd.synth import synth_nafnet
    torch.set_num_threads(min(8, torch.get_num_threads()))
    sd = {k: torch.from_numpy(v) for k, v in synth_nafnet(0, **TEST_SETTING).items()}
    tb = TR.cast_tables(_sde(), torch.float32)
    gt, mu, state, t = (torch.from_numpy(gold[k]) for k in ('gt', 'mu', 'state', 'timesteps'))
    with torch.no_grad():
        l2, _, _ = TR.loss(sd, tb, state, mu, gt, t, 'l2')
        _, expect, optimum = TR.loss(sd, tb, state, mu, gt, t, 'l1')
    l1, grads = TR.loss_and_grads(sd, tb, state, mu, gt, t, 'l1')
    return sd, float(l1), float(l2), expect, optimum, grads


def test_irsde_reproduces_the_golden_states(gold):
    s = _sde()
    s.set_model(lambda x, mu, t: x)
    gt, mu = torch.from_numpy(gold['gt']), torch.from_numpy(gold['mu'])
    torch.manual_seed(int(gold['seed']))
    ts, states = s.generate_random_states(gt, mu)
    assert np.array_equal(ts.numpy(), gold['gen_timesteps']) and np.array_equal(states.numpy(), gold['gen_states'])
    t, state = torch.from_numpy(gold['timesteps']), torch.from_numpy(gold['state'])
    s.set_mu(mu)
    assert np.array_equal((torch.from_numpy(gold['noise']) * s.sigma_bar(t) + s.mu_bar(gt, t)).numpy(), gold['state'])
    assert np.array_equal(s.reverse_optimum_step(state, gt, t).numpy(), gold['optimum'])
    eps = (state - gt) * 0.5          # any noise prediction: reverse_sde_step_mean is elementwise in it
    score = s.get_score_from_noise(eps, t)
    want = state - (s.thetas[t] * (mu - state) - s.sigmas[t] ** 2 * (-eps / s.sigma_bars[t])) * s.dt
    assert torch.equal(s.reverse_sde_step_mean(state, score, t), want)


def test_restatement_step_equals_the_reference(gold, step):
    sd, l1, l2, expect, optimum, grads = step
    for name, got, ref in (('loss l1', l1, float(gold['loss_l1'])), ('loss l2', l2, float(gold['loss_l2']))):
        print('%s: %.9g vs %.9g' % (name, got, ref))
        assert abs(got - ref) <= NOISE * abs(ref)
    for name, got in (('expect', expect), ('optimum', optimum)):
        d = float(np.abs(got.numpy() - gold[name]).max())
        print('%s: %.3g of max %.3g' % (name, d, np.abs(gold[name]).max()))
        assert d <= NOISE * np.abs(gold[name]).max()
    keys = gold['keys'].tolist()
    assert keys == list(grads) and len(keys) == 208
    typ = float(np.median(gold['grad_maxabs']))
    for i, k in enumerate(keys):
        scale = max(float(gold['grad_maxabs'][i]), typ)
        assert abs(float(grads[k].abs().max()) - gold['grad_maxabs'][i]) <= NOISE * scale, k
        assert abs(float(grads[k].double().sum()) - gold['grad_sum'][i]) <= NOISE * scale * grads[k].numel(), k
    for k in gold['full'].tolist():
        d = float(np.abs(grads[k].numpy() - gold['grad_' + k]).max())
        scale = max(float(np.abs(gold['grad_' + k]).max()), typ)
        print('%-40s max|restatement - reference| %.3g of %.3g' % (k, d, scale))
        assert d <= NOISE * scale, k


@pytest.mark.parametrize('kind', ['Adam', 'AdamW', 'Lion'])
def test_restatement_optimizers_equal_the_reference(gold, step, kind):
    """The first step of all three is sign-like (lr g / (|g| + eps), lr sign(g)).  With dg = the bar's noise on the gradient:
    where |g| <= 4 dg the update may land anywhere within +-lr; elsewhere Lion's is exact and Adam's moves by about lr dg / |g|
    (allowed: twice that).  On top of the bar itself."""
    sd, _, _, _, _, grads = step
    lr, b1, b2, eps, wd = (float(v) for v in gold['hyper'])
    typ = float(np.median(gold['grad_maxabs']))
    for k in gold['full'].tolist():
        got = TR.optim_step(kind, sd[k], grads[k], {}, lr, b1, b2, eps, wd).numpy()
        ref, gref = gold['%s_%s' % (kind, k)], np.abs(gold['grad_' + k])
        dg = NOISE * max(float(gref.max()), typ)
        sure = gref > 4 * dg
        bar = NOISE * max(float(np.abs(ref).max()), lr)
        tol = bar + np.where(sure, 0.0 if kind == 'Lion' else 2 * lr * dg / np.maximum(gref, dg), 2 * lr)
        d = np.abs(got - ref)
        print('%s %-40s max diff %.3g, worst diff / allowed %.3g, %d of %d elements near a zero gradient' % (
            kind, k, d.max(), (d / tol).max(), int((~sure).sum()), sure.size))
        assert (d <= tol).all(), k
