"""Every device form of the weights follows the master copy through optimiser steps, single-tensor loads and switches of the
precision (csrc/fdsr_forms.h): an engine that was walked through such a sequence computes what a fresh engine computes that
was loaded with the walked engine's current weights.  Bitwise where both read host-packed or identically packed forms (eval
forward, sampling); within 1e-5 where a training-mode f16x3 forward reads the device-packed forms and the generic upsample kernel
(the bound test_gpu_train.py::test_adam_update_and_weights_in_use documents).  B = 1, 32x32, a two-step schedule."""
import ctypes as C

import pytest
import torch

from fastdiffsr_amd import _lib
from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_UNET, FASTDIFFSR_SCHEDULE_VAL
from fastdiffsr_amd.schedule import schedule_buffers, sampling_scalars
from fastdiffsr_amd.synth import synth_state_dict, synth_inputs

pytestmark = pytest.mark.gpu

PRECS = ('f32', 'f16x3', 'bf16', 'f16')
UP_KEY = 'ups.7.conv.weight'            # an upsample conv: it has a sub-pixel form


@pytest.fixture(scope='module')
def base():
    cfg = UNetConfig(**FASTDIFFSR_UNET)
    sd = synth_state_dict(cfg, 0)
    bufs, sp = schedule_buffers(dict(FASTDIFFSR_SCHEDULE_VAL, n_timestep=2))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 6, 32, 32, generator=g).cuda()
    target = torch.randn(1, 3, 32, 32, generator=g).cuda()
    cond, noise = synth_inputs(1, 32, 32, 2)
    return dict(cfg=cfg, sd=sd, sched=sampling_scalars(bufs, sp), x=x, target=target, nl=torch.tensor([0.4]).cuda(),
                cond=cond.cuda(), noise=noise.cuda())


def _engine(base, sd=None, cfg=None):
    from fastdiffsr_amd.engine import Engine
    eng = Engine(cfg or base['cfg'])
    eng.load_state_dict(sd or base['sd'])
    eng.set_schedule(base['sched'])
    return eng


def _step(eng, base, prec):
    eng.set_precision(prec)
    eng.train_grads(base['x'], base['nl'], base['target'], 'l1', 1.0 / base['target'].numel())
    eng.adam_step(1e-4)


def _weights(eng, base):
    """The walked engine's current weights as a state dict (never-executed tensors: as loaded)."""
    return {k: (eng.get_weight(k) if live else base['sd'][k]) for k, _, live in eng.schema()}


def _train_forward(eng, base):
    eng.set_training(True)
    _lib.check(eng.h, eng.lib.fdsr_set_dropout_seed(eng.h, C.c_uint64(7)))      # same masks on both engines
    try:
        return eng.unet_forward(base['x'], base['nl'].view(1, 1))
    finally:
        eng.set_training(False)


def _same_reads(walked, fresh, base, prec):
    """`walked` against `fresh` in precision `prec`: training-mode forward first (it must not lean on an eval read's refresh)."""
    if prec in ('f32', 'f16x3'):
        walked.set_precision(prec)
        fresh.set_precision(prec)
        ya, yb = _train_forward(walked, base), _train_forward(fresh, base)
        d = (ya - yb).abs().max().item()
        print(f'{prec} training-mode forward: max|walked - fresh| = {d:.3e}')
        assert d <= (1e-5 if prec == 'f16x3' else 0.0), d
    walked.set_precision(prec)
    fresh.set_precision(prec)
    ya, yb = walked.unet_forward(base['x'], base['nl'].view(1, 1)), fresh.unet_forward(base['x'], base['nl'].view(1, 1))
    assert torch.equal(ya, yb), (prec, 'forward', (ya - yb).abs().max().item())
    for graph in (False, True):
        sa, sb = walked.sample(base['cond'], base['noise'], graph=graph), fresh.sample(base['cond'], base['noise'], graph=graph)
        assert torch.equal(sa, sb), (prec, 'sample', graph, (sa - sb).abs().max().item())


@pytest.fixture(scope='module')
def stepped_weights(base):
    """Per step precision: a fresh engine holding the weights one optimiser step in that precision leaves (the step is bitwise
    reproducible, test_gpu_train.py::test_step_is_bitwise_reproducible, so every walked engine of a case holds the same)."""
    cache = {}

    def get(step_prec):
        if step_prec not in cache:
            eng = _engine(base)
            _step(eng, base, step_prec)
            cache[step_prec] = _weights(eng, base)
            cache[step_prec, 'fresh'] = _engine(base, cache[step_prec])
        return cache[step_prec], cache[step_prec, 'fresh']
    return get


@pytest.mark.parametrize('read', PRECS)
@pytest.mark.parametrize('step_prec', ['f16x3', 'f32'])
def test_reads_after_an_optimiser_step(base, stepped_weights, step_prec, read):
    sd1, fresh = stepped_weights(step_prec)
    walked = _engine(base)
    _step(walked, base, step_prec)
    assert all(torch.equal(torch.from_numpy(walked.get_weight(k)), torch.as_tensor(sd1[k])) for k in ('downs.0.weight', UP_KEY))
    _same_reads(walked, fresh, base, read)


@pytest.mark.parametrize('read', PRECS)
def test_reads_after_a_step_and_a_single_tensor_load(base, read):
    walked = _engine(base)
    _step(walked, base, 'f16x3')
    walked.load_weight(UP_KEY, walked.get_weight(UP_KEY) * 1.5)
    fresh = _engine(base, _weights(walked, base))
    _same_reads(walked, fresh, base, read)


@pytest.mark.parametrize('prec', ['f16x3', 'bf16'])
def test_captured_sample_graph_does_not_outlive_a_step(base, prec):
    eng = _engine(base)
    _step(eng, base, 'f16x3')
    eng.set_precision(prec)
    out = torch.empty(1, 3, 32, 32, device='cuda')
    before = eng.sample(base['cond'], base['noise'], graph=True, out=out).clone()
    eng.set_precision('f16x3')
    eng.train_grads(base['x'], base['nl'], base['target'], 'l1', 1.0 / base['target'].numel())
    eng.adam_step(1e-3)                                                       # a large step: the sample must move
    eng.set_precision(prec)
    after = eng.sample(base['cond'], base['noise'], graph=True, out=out).clone()     # same buffers: the old graph would match
    eager = eng.sample(base['cond'], base['noise'])
    assert torch.equal(after, eager)
    assert not torch.equal(after, before)
    fresh = _engine(base, _weights(eng, base))
    fresh.set_precision(prec)
    assert torch.equal(fresh.sample(base['cond'], base['noise']), eager)


def test_resumed_f16x3_run_steps_on_the_same_bits(base):
    """Two f16x3 steps uninterrupted, against an engine re-loaded from the weights and optimiser state after step 1."""
    a = _engine(base)
    _step(a, base, 'f16x3')
    b = _engine(base, _weights(a, base))
    for k, _, live in a.schema():
        if live:
            b.set_optimizer_state(k, *a.optimizer_state(k))
    for eng in (a, b):
        _step(eng, base, 'f16x3')
    assert torch.equal(a.grad_arena(), b.grad_arena())
    for k in ('downs.0.weight', UP_KEY, 'final_conv.block.3.bias'):
        assert torch.equal(torch.from_numpy(a.get_weight(k)), torch.from_numpy(b.get_weight(k))), k


def test_bf16_training_mode_forward_after_a_step_reads_current_weights(base):
    """The sequence the earlier freshness flags missed: train in f32, switch to bf16 (nothing lags yet), optimiser step,
    train mode, forward.  The bf16 fragments were then the ones packed BEFORE the step (max|walked - fresh| = 2.6 at the
    commit before the record, where every other case of this file passed).  Dropout 0: with live dropout a 16-bit training-mode
    forward is refused before it launches."""
    cfg = UNetConfig(**dict(FASTDIFFSR_UNET, dropout=0.0))
    walked = _engine(base, cfg=cfg)
    walked.set_precision('f32')
    walked.train_grads(base['x'], base['nl'], base['target'], 'l1', 1.0 / base['target'].numel())
    walked.set_precision('bf16')
    walked.adam_step(1e-3)
    fresh = _engine(base, _weights(walked, base), cfg=cfg)
    fresh.set_precision('bf16')
    ya, yb = _train_forward(walked, base), _train_forward(fresh, base)
    print(f'bf16 training-mode forward after a step: max|walked - fresh| = {(ya - yb).abs().max().item():.3e}')
    assert torch.equal(ya, yb)
