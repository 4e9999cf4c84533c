"""The rider launches of the f16x3 16x16x32 kernels (fdsr_conv_k32.hip: block2 of a ResnetBlock with its 1x1 res_conv accumulated into
the same tile), one case per instantiation the sampling loop takes, and the f16x3 range guard of their raw inputs.  These tests pin
behaviour: the kernels' K loops carry the chunk kind and the activation of the main chunks as compile-time properties and raise the
range flag behind the loops, and nothing a caller can see may move with that.

The engine has no entry point for a single convolution launch, so a launch is reached through a small forward in debug mode: every
operator's stored inputs and output are read back (Engine.debug_tensor), and the rider launch is judged ALONE -- its output against
the same operator evaluated in fp64 on the device's own stored inputs (unet_16bit_emulation.Emu with every rounding off: GroupNorm
statistics in fp64 from the stored tensor, Swish, conv3x3 + bias + conv1x1 of the raw second input + bias), at the f16x3 bound of
tests/test_gpu_k32.py, 1e-4 * max(1, max|ref|).  One UNet (inner_channel 64, channel_mults (1, 2, 4)) gives every shape through the
map size; launcher options put the launch on the instantiation in question:

  64 -> 64, raw rider (64|64) and (128|64), N = 2, 20 x 64 map     k32_sb_min_wgs = 1: the 4-wave form, 6-row tiles (20 = 3 * 6 + 2: a
                                                                   ragged last tile row, two tile columns, 4 / 6 rider chunks)
  128 -> 128, rider 64, (128|128), (128|64), (256|128), 16 x 64    th_min_wgs = 1: 8-row tiles of <8, 4>, 2 x 2 tiles, 2 .. 12 rider chunks
  256 -> 256, rider 128, (256|256), (256|128), 8 x 32              th_min_wgs = 1: 4-row tiles of <4, 8>, two tile rows
  256 -> 256, the same riders, 4 x 32                              the default tile rule: 2-row tiles of <2, 8> with the GroupNorm
                                                                   table formed in the kernel (gn_consumer), two tile rows
(splitk = 0 everywhere: a launch with a K split keeps the rider-last kernels.)  That a case ran on the 16x16x32 kernels is shown by the
same forward with k32 = 0, which must differ.

Range guard (include/fdsr.h: fdsr_check_saturation).  The flag must be raised if and only if a RAW staged value exceeds 65504 in
magnitude, stay raised through the later launches of the forward until it is read, and be cleared by the read (a forward also clears
it when it starts: fdsr_unet_forward).  A value is planted where only a rider launch reads it raw: the output
of the block BEFORE the last block of a level is read by the last block's GroupNorm (re-scaled: no guard) and by its rider (raw), and
by nothing else.  That block is made exact -- block2 weights and both biases zero, its res_conv a selector of weight 2.0 from one
channel of its skip tensor (level 0: a copy of the network input's channel 0, through a selector conv_in and a zeroed downs.1) or
zero with a bias plane -- so its output holds the planted value and nothing else of size: 7e4 = 2 * 35000 raises, 65504 = 2 * 32752
does not.  The last channel of the last rider chunk belongs to the skip tensor downs.0, which the Downsample conv reads raw too: that
one case does not isolate the rider kernel (said in its id)."""
import contextlib

import numpy as np
import pytest
import torch

import unet_16bit_emulation as E
from fastdiffsr_amd.arch import UNetConfig, build_layers
from fastdiffsr_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

CFG = dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 4), attn_res=(), res_blocks=2,
           dropout=0.2, image_size=64)
TOL = 1e-4                                                   # tests/test_gpu_k32.py: TOL_FWD
DEFAULTS = dict(gn_consumer=1, k32=1275, k32_sb_min_wgs=1024, k32_stagger=0, th_min_wgs=256, splitk=1, strip=91, strip_min_wgs=512)
SMALL_WG = dict(k32_sb_min_wgs=1, splitk=0, strip=0)
LARGEST = dict(th_min_wgs=1, splitk=0)
F16_MAX = 65504.0


@contextlib.contextmanager
def options(**kw):
    from fastdiffsr_amd import _lib
    for k, v in kw.items():
        _lib.debug_option(k, v)
    try:
        yield
    finally:
        for k in kw:
            _lib.debug_option(k, DEFAULTS[k])


@pytest.fixture(scope='module')
def net():
    from fastdiffsr_amd.engine import Engine
    cfg = UNetConfig(**CFG)
    sd = synth_state_dict(cfg, 0)
    eng = Engine(cfg)
    eng.load_state_dict(sd)
    eng.set_precision('f16x3')
    emu = E.Emu(sd, cfg, None, torch.float64)
    yield cfg, eng, sd, emu
    eng.load_state_dict(sd)


_forwards = {}


def _forward(net, shape, opts):
    """one debug forward per (map, options), shared by the cases that read it: ({name: stored tensor}, nl, output with k32 = 0)"""
    key = (shape, tuple(sorted(opts.items())))
    if key not in _forwards:
        cfg, eng, sd, emu = net
        gen = torch.Generator().manual_seed(shape[2] * 1000 + shape[3])
        x = torch.randn(*shape, generator=gen)
        nl = torch.rand(shape[0], 1, generator=gen) * 0.9 + 0.05
        eng.load_state_dict(sd)
        with options(**opts):
            eng.set_debug(True)
            try:
                out = eng.unet_forward(x.cuda(), nl.cuda())
                torch.cuda.synchronize()
                stored = {op[0]: eng.debug_tensor(op[0]).cpu() for op in emu.operators()}
            finally:
                eng.set_debug(False)
            assert torch.equal(eng.unet_forward(x.cuda(), nl.cuda()), out)        # ordered sums only: a rerun is bitwise
            with options(k32=0):
                other = eng.unet_forward(x.cuda(), nl.cuda()).cpu()
        stored['input'] = x
        _forwards[key] = (stored, nl, out.cpu(), other)
    return _forwards[key]


# (id, map, options, couts of the launches under judgement, (C0, C1) of the raw riders that must be among them)
CASES = [
    ('64-4wave-6row', (2, 6, 20, 64), SMALL_WG, 64, [(64, 64), (128, 64)]),
    ('128-8x4', (2, 6, 32, 128), LARGEST, 128, [(64, 0), (128, 64), (128, 128), (256, 128)]),
    ('256-4x8', (2, 6, 32, 128), LARGEST, 256, [(128, 0), (256, 128), (256, 256)]),
    ('256-2x8-gn-consumer', (2, 6, 16, 128), dict(splitk=0), 256, [(128, 0), (256, 128), (256, 256)]),
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_rider_launch_vs_fp64(net, case):
    cid, shape, opts, cout, riders = case
    cfg, eng, sd, emu = net
    stored, nl, out, other = _forward(net, shape, opts)
    assert not torch.equal(out, other), 'the forward never took a 16x16x32 kernel'
    seen, worst = [], (0.0, '')
    for op in emu.operators():
        name, kind, L, ins = op
        if kind != 'block_out' or L.cout != cout or L.name + '.res_block.res_conv.weight' not in sd:
            continue
        ref = emu.run(op, stored, {}, nl).pre
        d = (stored[name].double() - ref).abs().max().item()
        scale = max(1.0, ref.abs().max().item())
        seen.append((L.cin - L.cskip, L.cskip))
        worst = max(worst, (d / scale, name))
        print(f'{cid}: {name} rider ({L.cin - L.cskip}|{L.cskip}) on {tuple(ref.shape[2:])}: max|d| {d:.3e} at max|ref| {scale:.3e}')
        assert d <= TOL * scale, f'{name}: {d:.3e} (scale {scale:.2f})'
    assert set(riders) <= set(seen), (riders, seen)


# ---- range guard ------------------------------------------------------------------------------------------------------------------
J, C = 7, 5            # skip channel the selector reads; output channel it writes


def _zero_block2(sd, p):
    sd[p + '.res_block.block2.block.3.weight'] = np.zeros_like(sd[p + '.res_block.block2.block.3.weight'])
    sd[p + '.res_block.block2.block.3.bias'] = np.zeros_like(sd[p + '.res_block.block2.block.3.bias'])


def _plant_net(sd0, layers, cout, plane=None, downs0_gain=1.0, downs0_ch=J):
    """the state dict with the block before the last `cout`-wide block of the up path made exact (module docstring).  plane: the value
    of its output channel C everywhere (res_conv zero); None: level 0, output channel C = 2 * network input channel 0"""
    sd = {k: np.array(v, copy=True) for k, v in sd0.items()}
    ups = [L for L in layers if L.name.startswith('ups.') and L.kind == 'res' and L.cout == cout]
    P = ups[-2].name
    _zero_block2(sd, P)
    w = np.zeros_like(sd[P + '.res_block.res_conv.weight'])
    sd[P + '.res_block.res_conv.bias'] = np.zeros_like(sd[P + '.res_block.res_conv.bias'])
    if plane is None:
        w[C, ups[-2].cin - ups[-2].cskip + J, 0, 0] = 2.0                    # from channel J of the skip tensor (downs.1)
        w0 = np.zeros_like(sd['downs.0.weight'])
        w0[downs0_ch, 0, 1, 1] = downs0_gain                                 # downs.0[downs0_ch] = gain * input[0]
        sd['downs.0.weight'] = w0
        sd['downs.0.bias'] = np.zeros_like(sd['downs.0.bias'])
        _zero_block2(sd, 'downs.1')                                          # downs.1 = downs.0 (identity residual)
    else:
        sd[P + '.res_block.block2.block.3.bias'][C] = np.float32(plane)
    sd[P + '.res_block.res_conv.weight'] = w
    return sd, P, ups[-1].name


def _raises(eng, x, nl):
    """one forward; True if the engine reports the range flag (which the report clears)"""
    from fastdiffsr_amd import _lib
    try:
        eng.unet_forward(x.cuda(), nl.cuda())
    except _lib.FdsrSaturated as e:
        assert e.code == _lib.FDSR_E_SATURATED
        return True
    return False


@pytest.fixture
def guard(net):
    cfg, eng, sd, emu = net
    eng.on_saturation, eng.check_saturation = 'raise', True
    yield cfg, eng, sd, build_layers(cfg)
    eng.on_saturation, eng.check_saturation = 'f32', True
    eng.load_state_dict(sd)


def _input(shape, pixel=None, value=0.0):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(9)).clamp(-3, 3)
    if pixel is not None:
        x[1, 0, pixel[0], pixel[1]] = value
    return x, torch.tensor([[0.2], [0.7]])


# 20 x 64 under 6-row x 32-column tiles: (3, 10) lies inside tile (0, 0); (6, 32) is the first pixel of tile (1, 1), staged by its
# neighbours as halo; (19, 63) the last pixel of the ragged last tile row
@pytest.mark.parametrize('pixel', [(3, 10), (6, 32), (19, 63)], ids=['interior', 'tile-corner', 'last-pixel'])
def test_guard_level0_rider_pixel(guard, pixel):
    cfg, eng, sd0, layers = guard
    sd, P, T = _plant_net(sd0, layers, 64)
    eng.load_state_dict(sd)
    shape = (2, 6, 20, 64)
    with options(**SMALL_WG):
        eng.set_debug(True)
        try:
            x, nl = _input(shape, pixel, 35000.0)
            assert _raises(eng, x, nl)                                      # 7e4 in the rider's raw input
            got = eng.debug_tensor(P)
            assert got[1, C, pixel[0], pixel[1]].item() == 70000.0 and (got.abs() > F16_MAX).sum().item() == 1
            for name in ('downs.0', 'downs.1', 'downs.2', 'downs.3'):        # nothing else read raw is out of range
                assert eng.debug_tensor(name).abs().max().item() < F16_MAX
        finally:
            eng.set_debug(False)
        x, nl = _input(shape, pixel, 32752.0)
        assert not _raises(eng, x, nl)                                      # a maximum of exactly 65504 is in range
        eng.set_debug(True)
        try:
            assert not _raises(eng, x, nl)
            assert eng.debug_tensor(P).abs().max().item() == F16_MAX
        finally:
            eng.set_debug(False)


def test_guard_level0_rider_last_channel_of_last_chunk_shared_with_downsample(guard):
    """channel 127 of the (64|64) rider = channel 63 of downs.0 -- which the Downsample conv stages raw as well (through the identity
    residuals), so the flag has two possible sources here"""
    cfg, eng, sd0, layers = guard
    sd, P, T = _plant_net(sd0, layers, 64, downs0_gain=2.0, downs0_ch=63)
    _zero_block2(sd, 'downs.2')         # downs.2 = downs.1 = downs.0 exactly: what the Downsample conv stages holds the planted value too
    eng.load_state_dict(sd)
    with options(**SMALL_WG):
        x, nl = _input((2, 6, 20, 64), (11, 40), 35000.0)
        assert _raises(eng, x, nl)
        x, nl = _input((2, 6, 20, 64), (11, 40), 32752.0)
        assert not _raises(eng, x, nl)


def test_guard_sticky_until_read_and_main_input_not_guarded(guard):
    cfg, eng, sd0, layers = guard
    sd, P, T = _plant_net(sd0, layers, 64)
    sd[T + '.res_block.block1.block.3.bias'][9] = np.float32(1.0e5)          # 1e5 in the GroupNorm'ed main input of the last block
    eng.load_state_dict(sd)
    shape = (2, 6, 20, 64)
    with options(**SMALL_WG):
        clean, nl = _input(shape)
        eng.set_debug(True)
        try:
            assert not _raises(eng, clean, nl)                               # a clean rider: the main input is re-scaled, no guard
            assert eng.debug_tensor(T + '.res_block.block1')[:, 9].abs().min().item() > 9.0e4
        finally:
            eng.set_debug(False)
    # Sticky: a forward clears the flag when it starts (fdsr_unet_forward), so "stays raised" is a statement about the launches of one
    # forward.  The plane of 7e4 is staged by the last 128-wide block's rider, in the middle of the up path; four rider launches with
    # clean inputs, the Upsample conv and final_conv run after it.  Nobody reads the flag during the forward; the first read afterwards
    # reports it and clears it, the second finds it clear.
    import ctypes
    from fastdiffsr_amd import _lib
    sd, P, T = _plant_net(sd0, layers, 128, plane=7.0e4)
    eng.load_state_dict(sd)
    x, nl = _input((2, 6, 32, 128))
    with options(**LARGEST):
        eng.check_saturation = False
        eng.unet_forward(x.cuda(), nl.cuda())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert eng.lib.fdsr_check_saturation(eng.h, st) == _lib.FDSR_E_SATURATED
        assert eng.lib.fdsr_check_saturation(eng.h, st) == 0
        eng.check_saturation = True


@pytest.mark.parametrize('cout,shape,opts', [(128, (2, 6, 32, 128), LARGEST), (256, (2, 6, 32, 128), LARGEST), (256, (2, 6, 16, 128), dict(splitk=0))],
                         ids=['128-8x4', '256-4x8', '256-2x8-gn-consumer'])
def test_guard_rider_plane(guard, cout, shape, opts):
    cfg, eng, sd0, layers = guard
    x, nl = _input(shape)
    with options(**opts):
        sd, P, T = _plant_net(sd0, layers, cout, plane=7.0e4)
        eng.load_state_dict(sd)
        assert _raises(eng, x, nl)
        sd, P, T = _plant_net(sd0, layers, cout, plane=F16_MAX)
        eng.load_state_dict(sd)
        assert not _raises(eng, x, nl)
        eng.set_debug(True)
        try:
            assert not _raises(eng, x, nl)
            assert eng.debug_tensor(P).abs().max().item() == F16_MAX
        finally:
            eng.set_debug(False)


def test_guard_upsample_conv_raw_input(guard):
    """the plant / no-plant pair through the sub-pixel upsample conv (conv_up2_k32_kernel): the last 128-wide block of the up path feeds
    the Upsample conv and nothing else; its output is a bias plane, the Upsample conv's own weights are zero so that nothing large
    travels on"""
    cfg, eng, sd0, layers = guard
    T = [L for L in layers if L.name.startswith('ups.') and L.kind == 'res' and L.cout == 128][-1].name
    U = [L for L in layers if L.name.startswith('ups.') and L.kind == 'up'][-1].name
    x, nl = _input((2, 6, 32, 128))
    for plane, want in ((7.0e4, True), (6.0e4, False)):
        sd = {k: np.array(v, copy=True) for k, v in sd0.items()}
        _zero_block2(sd, T)
        sd[T + '.res_block.res_conv.weight'] = np.zeros_like(sd[T + '.res_block.res_conv.weight'])
        sd[T + '.res_block.res_conv.bias'] = np.zeros_like(sd[T + '.res_block.res_conv.bias'])
        sd[T + '.res_block.block2.block.3.bias'][C] = np.float32(plane)
        sd[U + '.conv.weight'] = np.zeros_like(sd[U + '.conv.weight'])
        eng.load_state_dict(sd)
        assert _raises(eng, x, nl) == want, plane
