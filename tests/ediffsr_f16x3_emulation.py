"""CPU emulation of the NAFNet's f16x3 mode on top of tests/ediffsr_restatement.py: the yardstick of the mode's arithmetic,
independent of the device code.

Inside `split_convs()` every dense convolution (groups == 1) the restatement calls is replaced by the split arithmetic: input and
weight are clamped to +-65504, each is split into hi = f16(v) and lo = f16(v - hi), the three partial convolutions lo.hi, hi.lo and
hi.hi are evaluated in fp64 and added, the sum is rounded to fp32 and the bias is added in fp32.  Everything else -- LayerNorm, FiLM,
the depthwise convolution, gates, pools, residuals -- runs in the restatement's own fp32.  (The device additionally scales the
weights by a power of two before the split, which is exact and keeps their lo parts out of the f16 subnormals.)"""
import contextlib

import torch
import torch.nn.functional as F

import ediffsr_restatement as R

F16_MAX = 65504.0


def split(v):
    """fp32 tensor -> (hi, lo) as fp64 tensors holding f16 values"""
    v = v.float().clamp(-F16_MAX, F16_MAX)
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double(), lo.double()


def conv2d_f16x3(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    if groups != 1:
        return F.conv2d(x, w, b, stride, padding, dilation, groups)
    xh, xl = split(x)
    wh, wl = split(w)
    kw = dict(stride=stride, padding=padding, dilation=dilation)
    y = (F.conv2d(xl, wh, **kw) + F.conv2d(xh, wl, **kw) + F.conv2d(xh, wh, **kw)).float()
    return y if b is None else y + b.float().view(1, -1, 1, 1)


class _Functional:
    """torch.nn.functional with conv2d replaced"""
    conv2d = staticmethod(conv2d_f16x3)

    def __getattr__(self, name):
        return getattr(F, name)


@contextlib.contextmanager
def split_convs():
    """ediffsr_restatement's convolutions run the split arithmetic inside this block (the module itself is not edited)"""
    saved = R.F
    R.F = _Functional()
    try:
        yield
    finally:
        R.F = saved


def forward(sd, inp, cond, time, taps=None):
    """ediffsr_restatement.forward in fp32 with the split convolutions"""
    with split_convs(), torch.no_grad():
        return R.forward(sd, inp, cond, time, taps)


def reverse_loop(sd, tables, state, mu, noise=None, ode=False, trajectory=None):
    with split_convs(), torch.no_grad():
        return R.reverse_loop(sd, tables, state, mu, noise, ode, trajectory)
