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
    """Records which entry point a facade takes; returns zeros of the right shapes."""

    def __init__(self, variant):
        self.cfg = type('cfg', (), {'variant': variant, 'dropout': 0.0})()
        self.calls = []
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
                               training=self.training))
        img = torch.zeros_like(cond)
        if not want_traj:
            return img
        n = self.traj_slots(traj_every) if stepwise else self.T
        return img, torch.zeros((n,) + tuple(cond.shape))


class _FakeUNet(torch.nn.Module):
    def __init__(self, eng):
        super().__init__()
        self.engine = eng
        self.cfg = eng.cfg

    def sync_weights(self, *a, **k):
        pass


def _facade(variant, T):
    if variant == 'ddpm':
        from fastdiffsr_amd.sr3.diffusion import GaussianDiffusion
    elif variant == 'tesr':
        from fastdiffsr_amd.tesr.diffusion import GaussianDiffusion
    else:
        from fastdiffsr_amd.gdp.diffusion import GaussianDiffusion
    eng = _FakeEngine(variant)
    g = GaussianDiffusion(_FakeUNet(eng), image_size=8)
    g.set_new_noise_schedule(dict(schedule='linear', n_timestep=T, linear_start=1e-4, linear_end=2e-2), 'cpu')
    return g, eng


@pytest.mark.parametrize('variant', ['ddpm', 'tesr', 'gdp'])
@pytest.mark.parametrize('T', [12, 50, 51, 1000])
def test_facades_route_stepwise_exactly_above_50(variant, T):
    g, eng = _facade(variant, T)
    assert g.graph == 'auto' and g.rng == 'torch'
    x = torch.zeros(1, 3, 8, 8)
    frames = g.p_sample_loop(x, continous=True)
    call = eng.calls[-1]
    assert call['stepwise'] == (T > 50) == L.use_stepwise(T)
    assert call['traj_every'] == (L.frame_every(T) if T > 50 else 1)
    planes = T + (0 if variant == 'tesr' else 1)
    assert call['noise'] == (planes, 1, 3, 8, 8)              # rng = 'torch': the reference's draws, pre-drawn
    assert frames.shape[0] == 1 + len(L.kept_steps(T))         # [x_in] + the kept frames, as ret_img
    g.rng = 'engine'
    g.graph = 'off'
    g.p_sample_loop(x, continous=False)
    assert eng.calls[-1]['noise'] is None and eng.calls[-1]['graph'] is False
    if T > 50:                                                 # 'on': the chunked graph from the first call of a shape
        g.graph = 'on'
        g.p_sample_loop(x, continous=False)
        assert eng.calls[-1]['graph'] is True and eng.calls[-1]['stepwise']


@pytest.mark.parametrize('variant', ['ddpm', 'tesr', 'gdp'])
def test_stepwise_follows_train_and_eval_mode(variant):
    """A training step leaves the engine in train mode; the stepwise path puts it in the mode of denoise_fn (as the reference's
    netG.eval() / .train() do for nn.Dropout) and samples eagerly while dropout is live."""
    g, eng = _facade(variant, 60)
    eng.cfg.dropout = 0.2
    x = torch.zeros(1, 3, 8, 8)
    g.train()
    for _ in range(2):                                          # graph = 'auto': the second call of a shape would capture
        g.p_sample_loop(x, continous=False)
        assert eng.calls[-1]['training'] is True and eng.calls[-1]['graph'] is False
    eng.set_training(True)                                      # what optimize_step leaves behind
    g.eval()
    g.p_sample_loop(x, continous=False)
    assert eng.calls[-1]['training'] is False and eng.calls[-1]['graph'] is True
    from fastdiffsr_amd.long_schedule import release_buffers
    assert any(k[0] == 'stepwise' for k in g._gbuf)
    release_buffers(g)
    assert not any(k[0] == 'stepwise' for k in g._gbuf)
