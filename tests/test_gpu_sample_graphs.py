"""The captured graphs of fdsr_sample and fdsr_sample_stepwise on one engine: both entry points alternating on the same buffers,
more distinct buffers than a list of graphs keeps, and a change of launcher options between graph calls.  Every result is compared
bitwise with the eager fdsr_sample of the same inputs; out and traj are the caller's and hold NaN before every call, so a call
that launched nothing, or a stale graph that wrote elsewhere, cannot pass."""
import pytest
import torch

from test_gpu_long_schedule import _engine

pytestmark = pytest.mark.gpu

T, B, H, W = 6, 2, 32, 32


@pytest.fixture(scope='module')
def setup():
    eng = _engine('fastdiffsr', T)
    g = torch.Generator().manual_seed(19)
    cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    noise = torch.randn((T, B, 3, H, W), generator=g).cuda()
    refs = {}

    def ref(prec):
        if prec not in refs:
            eng.set_precision(prec)
            refs[prec] = eng.sample(cond, noise, want_traj=True)
        return refs[prec]
    return eng, cond, noise, ref


def _buffers():
    return torch.empty(B, 3, H, W, device='cuda'), torch.empty(T, B, 3, H, W, device='cuda')


def _run(eng, cond, noise, out, traj, **kw):
    """One call into the caller's buffers, NaN beforehand; clones of what it left there."""
    out.fill_(float('nan'))
    traj.fill_(float('nan'))
    eng.sample(cond, noise, want_traj=True, out=out, traj=traj, **kw)
    return out.clone(), traj.clone()


LOOP = dict(graph=True)
STEP4 = dict(graph=True, stepwise=True, chunk=4)      # 6 = 4 + a remainder of 2
STEP3 = dict(graph=True, stepwise=True, chunk=3)


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_alternating_entry_points_on_the_same_buffers(setup, prec):
    """A lookup that returned the other entry point's graphs, or a key without the chunk, replays the wrong launches."""
    eng, cond, noise, ref = setup
    ref_out, ref_traj = ref(prec)
    eng.set_precision(prec)
    out, traj = _buffers()
    for i, kw in enumerate([LOOP, STEP4, LOOP, STEP4, STEP3, LOOP]):
        o, t = _run(eng, cond, noise, out, traj, **kw)
        assert torch.equal(o, ref_out) and torch.equal(t, ref_traj), (prec, i, kw)


@pytest.mark.parametrize('kw', [LOOP, STEP4], ids=['loop', 'stepwise'])
def test_more_buffers_than_a_list_keeps(setup, kw):
    """Ten distinct out buffers (a list keeps 8 graphs), then the first again: an eviction that destroyed a graph still listed, or
    left its entry behind, shows here."""
    eng, cond, noise, ref = setup
    ref_out, ref_traj = ref('f32')
    eng.set_precision('f32')
    traj = _buffers()[1]
    outs = [_buffers()[0] for _ in range(10)]
    for i, out in enumerate(outs + outs[:1]):
        o, t = _run(eng, cond, noise, out, traj, **kw)
        assert torch.equal(o, ref_out) and torch.equal(t, ref_traj), (i, kw)


def test_launcher_options_drop_the_captures(setup):
    """bf16_f16x3_steps = 2 runs the first two steps on other kernels: a graph captured before the option changed must not replay."""
    from fastdiffsr_amd import _lib
    eng, cond, noise, ref = setup
    ref_out, ref_traj = ref('bf16')
    eng.set_precision('bf16')
    out, traj = _buffers()
    a = _run(eng, cond, noise, out, traj, **LOOP)
    assert torch.equal(a[0], ref_out) and torch.equal(a[1], ref_traj)
    _lib.debug_option('bf16_f16x3_steps', 2)
    try:
        e2 = eng.sample(cond, noise, want_traj=True)
        assert not torch.equal(e2[0], a[0]), 'the option changes the result, or this test shows nothing'
        g2 = _run(eng, cond, noise, out, traj, **LOOP)
        assert torch.equal(g2[0], e2[0]) and torch.equal(g2[1], e2[1])
    finally:
        _lib.debug_option('bf16_f16x3_steps', 0)
    g = _run(eng, cond, noise, out, traj, **LOOP)
    assert torch.equal(g[0], a[0]) and torch.equal(g[1], a[1])
    s = _run(eng, cond, noise, out, traj, **STEP4)
    assert torch.equal(s[0], ref_out) and torch.equal(s[1], ref_traj)
