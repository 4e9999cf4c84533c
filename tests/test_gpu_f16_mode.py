"""FDSR_PREC_F16 (round 6): ONE f16 MFMA per product -- the hi plane of the f16x3 weight forms against un-split f16 activations -- and
f16 activations in HBM: the bf16 mode's kernels, bytes and MFMA rate with 11 mantissa bits instead of 8.  Judged like bf16, on PSNR
(north_star: within 0.01 dB of the reference), with bounds that can fail:

  * every layer of a forward within 0.4 % of the layer's range (2^-12 = 0.024 % per rounding; bf16's bound is 3 %);
  * the 20-step loop at 256 x 256 at least 68 dB from the oracle's image (measured 74.6; bf16: 57.6) and within 0.01 dB of it against
    a synthetic HR; every kernel selection (B = 1 / 2 / 5 / 16, 128 .. 512 pixels: 2-row tiles with the consumer-side GroupNorm, the
    strip kernels, the tail kernels, split K) at least 70 dB from the f16x3 result; hipGraph replay and a rerun bitwise; batch
    permutation bitwise;
  * values beyond the f16 range saturate instead of turning into inf;
  * the siblings (SR3, TESR, GDP): their attention kernels' f16 twins, a loop against f16x3 beside bf16.
The trained-like-weights figure (0.19 dB for bf16) is in tests/test_gpu_trained_weights.py.
(The bf16 / f16 kernels are judged per operator and per element against the modes' own arithmetic in tests/test_gpu_unet_16bit_layerwise.py.)"""
import math

import numpy as np
import pytest
import torch

from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_UNET, FASTDIFFSR_SCHEDULE_VAL, build_layers
from fastdiffsr_amd.schedule import schedule_buffers, sampling_scalars
from fastdiffsr_amd.synth import synth_state_dict, synth_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def full():
    from fastdiffsr_amd.engine import Engine
    cfg = UNetConfig(**FASTDIFFSR_UNET)
    eng = Engine(cfg)
    sd = synth_state_dict(cfg, 0)
    eng.load_state_dict(sd)
    bufs, sp = schedule_buffers(FASTDIFFSR_SCHEDULE_VAL)
    eng.set_schedule(sampling_scalars(bufs, sp))
    return cfg, eng, sd


def _psnr(a, b):
    return 20 * math.log10(2.0 / max((a - b).pow(2).mean().sqrt().item(), 1e-12))


def test_f16_layerwise_vs_oracle(full):
    from oracle import fdsr_oracle as O
    cfg, eng, sd = full
    eng.set_precision('f16')
    try:
        gen = torch.Generator().manual_seed(5)
        x = torch.randn(2, 6, 32, 48, generator=gen)
        nl = torch.tensor([[0.02098], [0.7074]])
        cap = {}
        with torch.no_grad():
            O.unet_forward(O.to_torch_sd(sd), cfg, x, nl, capture=cap)
        eng.set_debug(True)
        eng.unet_forward(x.cuda(), nl.cuda())
        torch.cuda.synchronize()
        worst = (0.0, '')
        for L in build_layers(cfg):
            got = eng.debug_tensor(L.name).cpu()
            d = (got - cap[L.name]).abs().max().item()
            scale = max(cap[L.name].abs().max().item(), 1.0)
            worst = max(worst, (d / scale, L.name))
            assert d <= 4e-3 * scale, f'{L.name}: {d:.3e} at |ref| {scale:.2f}'
        print(f'f16 layerwise: worst {worst[1]} at {worst[0]:.3e} of the range')
    finally:
        eng.set_debug(False)
        eng.set_precision('f32')


def test_f16_loop_256_vs_oracle_and_properties(full):
    from conftest import oracle_loop_image, plant_standard_pair
    from oracle import fdsr_oracle as O
    cfg, eng, sd = full
    cond, noise = synth_inputs(4, 256, 256, 20)
    plant_standard_pair(cond, noise, 3)                     # image 3: the session's shared oracle image
    c, n = cond.cuda(), noise.cuda()
    eng.set_precision('f16')
    try:
        out = eng.sample(c, n).clone()
        assert torch.isfinite(out).all() and out.abs().max().item() <= 1.5 + 1e-6
        assert torch.equal(eng.sample(c, n), out), 'rerun is not bitwise identical'
        assert torch.equal(eng.sample(c, n, graph=True), out) and torch.equal(eng.sample(c, n, graph=True), out), 'graph replay differs'
        perm = torch.tensor([2, 0, 3, 1])
        assert torch.equal(eng.sample(c[perm].contiguous(), n[:, perm].contiguous()), out[perm.cuda()]), 'images of a batch are not independent'
        ref = oracle_loop_image(sd, cfg, cond[3:4], noise[:, 3:4])
        o3 = out[3:4].cpu()
        p = _psnr(o3, ref)
        yy, xx = torch.meshgrid(torch.arange(256.0), torch.arange(256.0), indexing='ij')
        r = torch.stack([torch.sin(2 * math.pi * (yy / 64 + ch / 3)) * torch.cos(2 * math.pi * xx / 48) for ch in range(3)])[None]
        hr = O.tensor2img_u8((cond[3:4] + 0.5 * r).clamp(-1, 1)[0])
        dps = O.psnr_u8(O.tensor2img_u8(o3[0].clone()), hr) - O.psnr_u8(O.tensor2img_u8(ref[0].clone()), hr)
        print(f'f16 256x256 20 steps: PSNR(out, oracle) {p:.2f} dB, max|d| {(o3 - ref).abs().max().item():.3e}, PSNR delta vs HR {dps:+.5f} dB')
        assert p >= 68.0 and abs(dps) <= 0.01
    finally:
        eng.set_precision('f32')


@pytest.mark.parametrize('B,S', [(1, 256), (2, 256), (5, 128), (16, 256), (1, 512)])
def test_f16_every_kernel_selection_vs_f16x3(full, B, S):
    cfg, eng, sd = full
    cond, noise = synth_inputs(B, S, S, 20)
    c, n = cond.cuda(), noise.cuda()
    try:
        eng.set_precision('f16x3')
        ref = eng.sample(c, n).clone()
        eng.set_precision('bf16')
        pb = _psnr(eng.sample(c, n), ref)
        eng.set_precision('f16')
        out = eng.sample(c, n).clone()
        g = eng.sample(c, n, graph=True)
        p = _psnr(out, ref)
        print(f'B={B} {S}x{S}: f16 {p:.2f} dB from the f16x3 image (bf16: {pb:.2f})')
        assert torch.isfinite(out).all() and torch.equal(out, g)
        assert p >= 70.0 and p >= pb + 10.0
    finally:
        eng.set_precision('f32')


def test_f16_stores_saturate(full):
    """A residual stream beyond the f16 range: every stored activation stays finite (v_med3 to +-65504 in front of the conversion)."""
    cfg, eng, sd = full
    big = {k: v.copy() for k, v in sd.items()}
    big['downs.0.bias'] = (big['downs.0.bias'] + 3.0e5).astype(np.float32)      # the first conv's output IS the residual stream
    from fastdiffsr_amd.engine import Engine
    e2 = Engine(cfg)
    e2.load_state_dict(big)
    e2.set_precision('f16')
    e2.set_debug(True)
    x = torch.randn(1, 6, 32, 32, generator=torch.Generator().manual_seed(1))
    out = e2.unet_forward(x.cuda(), torch.tensor([0.5]).cuda())
    torch.cuda.synchronize()
    d0 = e2.debug_tensor('downs.0').cpu()
    assert torch.isfinite(d0).all() and d0.abs().max().item() == 65504.0
    assert torch.isfinite(out).all()


@pytest.mark.parametrize('variant', ['ddpm', 'tesr', 'gdp'])
def test_f16_siblings_attention(variant):
    """The siblings attend (ddpm_modules/unet.py:99, tesr_modules, gdp_modules/unet.py:392-488): their bf16 attention kernels have an f16
    twin (v_mfma_f32_32x32x16_f16, probabilities rounded to f16, O stored as f16).  A sampling loop in f16 against f16x3, beside bf16."""
    from fastdiffsr_amd.engine import Engine
    if variant == 'gdp':
        cfg = UNetConfig(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 2), attn_res=(2, 4), res_blocks=1,
                         dropout=0.0, image_size=32, variant='gdp')
    else:
        cfg = UNetConfig(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2, 4), attn_res=(8,), res_blocks=1,
                         dropout=0.0, image_size=32, variant=variant)
    eng = Engine(cfg)
    eng.load_state_dict(synth_state_dict(cfg, 5))
    bufs, sp = schedule_buffers(dict(schedule='linear', n_timestep=8, linear_start=1e-4, linear_end=2e-2))
    eng.set_schedule(sampling_scalars(bufs, sp))
    cond, noise = synth_inputs(2, 32, 32, 9 if variant in ('ddpm', 'gdp') else 8)
    c, n = cond.cuda(), noise.cuda()
    eng.set_precision('f16x3')
    ref = eng.sample(c, n).clone()
    eng.set_precision('bf16')
    pb = _psnr(eng.sample(c, n), ref)
    eng.set_precision('f16')
    out = eng.sample(c, n).clone()
    p = _psnr(out, ref)
    print(f'{variant}: f16 {p:.2f} dB from the f16x3 result (bf16: {pb:.2f})')
    assert torch.isfinite(out).all() and torch.equal(out, eng.sample(c, n, graph=True))
    assert p >= pb + 8.0 and p >= 55.0
