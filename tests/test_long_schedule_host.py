"""Host-side pieces of the siblings' long schedules (fdsr_sample_stepwise, fastdiffsr_amd.long_schedule): the C struct of the
options against its ctypes mirror, the reference's frame rule, and which entry point each facade takes for which T.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from fastdiffsr_amd import _lib, long_schedule as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_opts_struct_matches_header(tmp_path):
    hdr = open(os.path.join(ROOT, 'include', 'fdsr.h')).read()
    body = re.search(r'typedef struct fdsr_sample_opts \{(.*?)\} fdsr_sample_opts;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(\w+)\s+(\w+)\s*;', body)
    assert fields == [('int32_t', 'chunk_steps'), ('int32_t', 'traj_every')]
    assert [n for n, _ in _lib.FdsrSampleOpts._fields_] == [n for _, n in fields]
    assert all(t is C.c_int32 for _, t in _lib.FdsrSampleOpts._fields_)


def test_sample_opts_layout_matches_c_compiler(tmp_path):
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc: the C layout of fdsr_sample_opts is not checked')
    src = tmp_path / 'opts.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fdsr.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(fdsr_sample_opts), offsetof(fdsr_sample_opts, chunk_steps), offsetof(fdsr_sample_opts, traj_every)); '
                   'return 0; }\n')
    exe = tmp_path / 'opts'
    subprocess.check_call([gcc, '-std=c99', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    size, o0, o1 = map(int, subprocess.check_output([str(exe)]).split())
    assert (size, o0, o1) == (C.sizeof(_lib.FdsrSampleOpts), _lib.FdsrSampleOpts.chunk_steps.offset,
                              _lib.FdsrSampleOpts.traj_every.offset)


def test_stepwise_symbol_is_bound():
    assert 'fdsr_sample_stepwise' in _lib.SYMBOLS
    res, args = _lib.SYMBOLS['fdsr_sample_stepwise']
    assert res is C.c_int and len(args) == 13


@pytest.mark.parametrize('T', [8, 10, 12, 20, 1000, 2000])
def test_frame_selection_is_the_reference_rule(T):
    inter = 1 | (T // 10)
    ref = [t for t in reversed(range(T)) if t % inter == 0]
    assert L.frame_every(T) == inter
    assert L.kept_steps(T) == ref
    # the engine's slot count and slot order (include/fdsr.h): ceil(T / every) frames, t descending
    assert len(ref) == (T - 1) // inter + 1 == -(-T // inter)
    assert [(T - 1) // inter - t // inter for t in ref] == list(range(len(ref)))


class _FakeEngine:
    """Records what a facade hands the engine (entry point, noise tensor, training-step arguments); returns zeros of the right
    shapes."""

    def __init__(self, variant):
        self.cfg = type('cfg', (), {'variant': variant, 'dropout': 0.0})()
        self.calls = []
        self.events = []
        self.training = False

    def set_schedule(self, scalars):
        self.T = int(len(scalars['noise_level']))

    def set_precision(self, mode):
        pass

    def set_training(self, on, seed_from_torch=False):
        self.training = bool(on)

    def traj_slots(self, every=1):
        return (self.T - 1) // every + 1

    def sample(self, cond, noise=None, want_traj=False, graph=False, out=None, traj=None, stepwise=False, traj_every=1, chunk=0):
        self.calls.append(dict(stepwise=stepwise, graph=graph, traj_every=traj_every, noise=None if noise is None else tuple(noise.shape),
                               training=self.training, noise_tensor=None if noise is None else noise.clone()))
        img = torch.zeros_like(cond)
        if not want_traj:
            return img
        n = self.traj_slots(traj_every) if stepwise else self.T
        return img, torch.zeros((n,) + tuple(cond.shape))

    def train_grads(self, x, noise_level, target, loss_type='l1', loss_scale=1.0):
        self.events.append(('train_grads', dict(x=tuple(x.shape), loss_type=loss_type, loss_scale=loss_scale)))
        return 3.0

    def train_grads_pairs(self, hr, sr, gamma, noise=None, loss_type='l1', loss_scale=1.0):
        self.events.append(('train_grads_pairs', dict(x=tuple(hr.shape), loss_type=loss_type, loss_scale=loss_scale)))
        return 3.0

    def zero_grads(self, device=None):
        self.events.append(('zero_grads', {}))

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8):
        self.events.append(('adam_step', dict(lr=lr, betas=betas, eps=eps)))

    def schema(self):
        return []


class _FakeUNet(torch.nn.Module):
    def __init__(self, eng):
        super().__init__()
        self.engine = eng
        self.cfg = eng.cfg

    def sync_weights(self, *a, **k):
        pass


VARIANTS = ['fastdiffsr', 'ddpm', 'tesr', 'gdp']
SIBLINGS = VARIANTS[1:]


def _facade(variant, T, **kw):
    if variant == 'fastdiffsr':
        from fastdiffsr_amd.diffusion import GaussianDiffusion
    elif variant == 'ddpm':
        from fastdiffsr_amd.sr3.diffusion import GaussianDiffusion
    elif variant == 'tesr':
        from fastdiffsr_amd.tesr.diffusion import GaussianDiffusion
    else:
        from fastdiffsr_amd.gdp.diffusion import GaussianDiffusion
    eng = _FakeEngine(variant)
    g = GaussianDiffusion(_FakeUNet(eng), image_size=8, **kw)
    g.set_new_noise_schedule(dict(schedule='linear', n_timestep=T, linear_start=1e-4, linear_end=2e-2), 'cpu')
    return g, eng


def _planes(variant, T):
    return T + (1 if variant in ('ddpm', 'gdp') else 0)


@pytest.mark.parametrize('variant', SIBLINGS)
@pytest.mark.parametrize('T', [12, 50, 51, 1000])
def test_facades_route_stepwise_exactly_above_50(variant, T):
    g, eng = _facade(variant, T)
    assert g.graph == 'auto' and g.rng == 'torch'
    x = torch.zeros(1, 3, 8, 8)
    frames = g.p_sample_loop(x, continous=True)
    call = eng.calls[-1]
    assert call['stepwise'] == (T > 50) == L.use_stepwise(T)
    assert call['traj_every'] == (L.frame_every(T) if T > 50 else 1)
    assert call['noise'] == (_planes(variant, T), 1, 3, 8, 8)  # rng = 'torch': the reference's draws, pre-drawn
    assert frames.shape[0] == 1 + len(L.kept_steps(T))         # [x_in] + the kept frames, as ret_img
    g.rng = 'engine'
    g.graph = 'off'
    g.p_sample_loop(x, continous=False)
    assert eng.calls[-1]['noise'] is None and eng.calls[-1]['graph'] is False
    if T > 50:                                                 # 'on': the chunked graph from the first call of a shape
        g.graph = 'on'
        g.p_sample_loop(x, continous=False)
        assert eng.calls[-1]['graph'] is True and eng.calls[-1]['stepwise']


@pytest.mark.parametrize('variant', SIBLINGS)
def test_stepwise_follows_train_and_eval_mode(variant):
    """A training step leaves the engine in train mode; sampling puts it in the mode of denoise_fn (as the reference's
    netG.eval() / .train() do for nn.Dropout), on the stepwise path (T = 60) and on the fdsr_sample path (T = 12) alike, and samples
    eagerly while dropout is live."""
    for T in (60, 12):
        g, eng = _facade(variant, T)
        eng.cfg.dropout = 0.2
        x = torch.zeros(1, 3, 8, 8)
        g.train()
        for _ in range(2):                                      # graph = 'auto': the second call of a shape would capture
            g.p_sample_loop(x, continous=False)
            assert eng.calls[-1]['training'] is True and eng.calls[-1]['graph'] is False, T
        eng.set_training(True)                                  # what optimize_step leaves behind
        g.eval()
        g.p_sample_loop(x, continous=False)
        assert eng.calls[-1]['training'] is False and eng.calls[-1]['graph'] is (T > 50), T
        from fastdiffsr_amd.long_schedule import release_buffers
        assert any(k[0] == 'stepwise' for k in g._gbuf) == (T > 50)
        release_buffers(g)
        assert not any(k[0] == 'stepwise' for k in g._gbuf)


@pytest.mark.parametrize('graph', ['off', 'on'])
@pytest.mark.parametrize('T', [12, 60])
@pytest.mark.parametrize('variant', VARIANTS)
def test_torch_noise_is_drawn_in_the_reference_order(variant, T, graph):
    """rng = 'torch': the noise handed to the engine is, bitwise, the reference's stream: torch.randn(shape) once (p_sample_loop's
    start image), then one torch.randn_like(x) per remaining plane (p_sample's noise), eager or into the graph's buffer."""
    g, eng = _facade(variant, T)
    g.graph = graph
    x = torch.zeros(2, 3, 8, 8)
    torch.manual_seed(1234)
    g.p_sample_loop(x, continous=False)
    got = eng.calls[-1]['noise_tensor']
    torch.manual_seed(1234)
    ref = torch.stack([torch.randn(x.shape)] + [torch.randn_like(x) for _ in range(_planes(variant, T) - 1)])
    assert got.shape == (_planes(variant, T), 2, 3, 8, 8)
    assert torch.equal(got, ref)


@pytest.mark.parametrize('T', [12, 60])
@pytest.mark.parametrize('B', [1, 2])
@pytest.mark.parametrize('variant', VARIANTS)
def test_return_shapes(variant, B, T):
    """continous=False: the flagship returns the batch, SR3 ret_img[-1] of a single image and otherwise the batch, TESR / GDP
    ret_img[-1]; continous=True: [x_in] + the kept frames, each B images, along dim 0."""
    g, eng = _facade(variant, T)
    x = torch.zeros(B, 3, 8, 8)
    whole = variant == 'fastdiffsr' or (variant == 'ddpm' and B > 1)
    assert g.p_sample_loop(x, continous=False).shape == ((B, 3, 8, 8) if whole else (3, 8, 8))
    assert g.super_resolution(x, continous=True).shape == (B * (1 + len(L.kept_steps(T))), 3, 8, 8)


@pytest.mark.parametrize('T', [12, 60])
def test_flagship_never_takes_the_stepwise_entry(T):
    g, eng = _facade('fastdiffsr', T)
    for continous in (False, True):
        g.p_sample_loop(torch.zeros(1, 3, 8, 8), continous=continous)
        assert eng.calls[-1]['stepwise'] is False and eng.calls[-1]['traj_every'] == 1


@pytest.mark.parametrize('graph', ['auto', 'on', 'off'])
@pytest.mark.parametrize('variant', SIBLINGS)
def test_siblings_never_graph_the_short_loop(variant, graph):
    g, eng = _facade(variant, 12)
    g.graph = graph
    for _ in range(3):
        g.p_sample_loop(torch.zeros(1, 3, 8, 8), continous=False)
        assert eng.calls[-1]['graph'] is False and eng.calls[-1]['stepwise'] is False
    assert not g._gbuf


@pytest.mark.parametrize('variant,T', [('fastdiffsr', 12), ('tesr', 60)])
def test_graph_policy(variant, T):
    """'auto' captures from the second call of a shape on, 'on' from the first, 'off' never, live dropout never; the buffers of
    the last few shapes only are kept.  The flagship on fdsr_sample, a sibling on the stepwise entry."""
    x = torch.zeros(1, 3, 8, 8)

    def graphs(g, eng, n=3, x=x):
        out = []
        for _ in range(n):
            g.p_sample_loop(x, continous=False)
            out.append(eng.calls[-1]['graph'])
        return out

    g, eng = _facade(variant, T)
    assert g.graph == 'auto' and graphs(g, eng) == [False, True, True]
    assert graphs(g, eng, 2, torch.zeros(1, 3, 8, 16)) == [False, True]         # per shape
    assert g.p_sample_loop(x, continous=True) is not None and eng.calls[-1]['graph'] is False    # continous is part of the shape
    g, eng = _facade(variant, T)
    g.graph = 'on'
    assert graphs(g, eng) == [True, True, True]
    g, eng = _facade(variant, T)
    g.graph = 'off'
    assert graphs(g, eng) == [False, False, False] and not g._gbuf
    for mode in ('auto', 'on'):
        g, eng = _facade(variant, T)
        g.graph = mode
        eng.cfg.dropout = 0.2
        g.train()
        assert graphs(g, eng) == [False, False, False]
        assert all(c['training'] for c in eng.calls)
    for mode, n in (('on', 1), ('auto', 2)):
        g, eng = _facade(variant, T)
        g.graph = mode
        for w in range(8, 20, 2):                               # six shapes
            xs = torch.zeros(1, 3, 8, w)
            assert graphs(g, eng, n, xs)[-1] is True
            assert len(g._gbuf) <= 5
            assert [k for k in g._gbuf if (1, 3, 8, w) in k and g._gbuf[k]]
        assert len(g._gbuf) <= 5


@pytest.mark.parametrize('variant,kw,kind,squared,entry', [
    ('fastdiffsr', {}, 'l1', False, 'train_grads_pairs'),
    ('ddpm', {}, 'l1', False, 'train_grads'),
    ('tesr', {}, 'charbonnier', True, 'train_grads'),
    ('tesr', {'loss_type': 'l2'}, 'l2', False, 'train_grads'),
    ('gdp', {'loss_type': 'l1'}, 'l2', False, 'train_grads'),
    ('gdp', {'loss_type': 'l2'}, 'l2', False, 'train_grads'),
])
def test_optimize_step(variant, kw, kind, squared, entry):
    """The all-device training step of every facade: which engine entry and loss it asks for, the divisor (the GLOBAL element count;
    squared for TESR's Charbonnier mean), the order gradients -> grad_hook -> Adam, and the empty shard."""
    c, h, w = 3, 8, 8

    def batch(b):
        return {'HR': torch.zeros(b, c, h, w), 'SR': torch.zeros(b, c, h, w)}

    for b, gb in ((2, None), (2, 4), (0, 4)):
        g, eng = _facade(variant, 12, **kw)
        g.train()
        n = (gb or b) * c * h * w
        div = float(n) * float(n) if squared else float(n)
        loss = g.optimize_step(batch(b), lr=1e-4, grad_hook=lambda e: e.events.append(('hook', {})), global_batch=gb)
        names = [name for name, _ in eng.events]
        if b:
            assert names == [entry, 'hook', 'adam_step']
            args = eng.events[0][1]
            assert args['loss_type'] == kind
            assert args['loss_scale'] == pytest.approx(1.0 / div, rel=1e-12)
            assert args['x'] == ((b, c, h, w) if entry == 'train_grads_pairs' else (b, 2 * c, h, w))
            assert loss == pytest.approx(3.0 / div, rel=1e-12)
        else:
            assert names == ['zero_grads', 'hook', 'adam_step']
            assert loss == 0.0
        assert eng.events[-1][1] == dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
        assert g.denoise_fn._engine_ahead is True
    g, eng = _facade(variant, 12, **kw)
    with pytest.raises(ValueError):
        g.optimize_step(batch(2), lr=1e-4, global_batch=0)
    assert not eng.events
