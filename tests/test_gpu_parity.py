"""GPU parity: the HIP path (through the C ABI) against the oracle and the
reference-generated goldens on identical inputs.  Tolerances (north_star):
|delta| < 1e-3 fp32 per pixel for the 20-step loop; the UNet forward is held to 1e-4."""
import os

import numpy as np
import pytest
import torch

from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_UNET, FASTDIFFSR_SCHEDULE_VAL, build_layers
from fastdiffsr_amd.synth import synth_state_dict, synth_inputs
from fastdiffsr_amd.schedule import schedule_buffers, sampling_scalars

pytestmark = pytest.mark.gpu

TOL_FWD = 1e-4
TOL_LOOP = 1e-3
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out', 'parity_report.txt')


def report(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, 'a') as f:
        f.write(line + '\n')
    print(line)


def _engine(cfg, seed, schedule=True):
    from fastdiffsr_amd.engine import Engine
    eng = Engine(cfg)
    sd = synth_state_dict(cfg, seed)
    eng.load_state_dict(sd)
    assert eng.weights_complete
    if schedule:
        bufs, sp = schedule_buffers(FASTDIFFSR_SCHEDULE_VAL)
        eng.set_schedule(sampling_scalars(bufs, sp))
    return eng, sd


@pytest.fixture(scope='module')
def small():
    cfg = UNetConfig(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 4, 4),
                     attn_res=(16,), res_blocks=2, dropout=0.2, image_size=32)
    eng, sd = _engine(cfg, 7)
    return cfg, eng, sd


@pytest.fixture(scope='module')
def full():
    cfg = UNetConfig(**FASTDIFFSR_UNET)
    eng, sd = _engine(cfg, 0)
    return cfg, eng, sd


def test_layerwise_small_vs_oracle(small, golden_dir):
    """Every reference module's output, layer by layer (debug plan keeps all buffers)."""
    from oracle import fdsr_oracle as O
    cfg, eng, sd = small
    g = np.load(os.path.join(golden_dir, 'unet_small.npz'))
    x = torch.from_numpy(g['x'])
    nl = torch.from_numpy(g['nl/3'])
    cap = {}
    with torch.no_grad():
        ref = O.unet_forward(O.to_torch_sd(sd), cfg, x, nl, capture=cap)
    eng.set_debug(True)
    out = eng.unet_forward(x.cuda(), nl.cuda())
    torch.cuda.synchronize()
    worst = 0.0
    for L in build_layers(cfg):
        got = eng.debug_tensor(L.name).cpu()
        d = (got - cap[L.name]).abs().max().item()
        scale = cap[L.name].abs().max().item()
        report(f'layer {L.name:12s} {L.kind:8s} max|d|={d:.3e} (max|ref|={scale:.2f})')
        worst = max(worst, d / max(scale, 1.0))
        assert d <= TOL_FWD * max(scale, 1.0), f'{L.name}: {d}'
    eng.set_debug(False)
    d = (out.cpu() - ref).abs().max().item()
    report(f'small fwd vs oracle max|d|={d:.3e}')
    assert d <= TOL_FWD


def test_layerwise_full_vs_oracle(full):
    """inner=64: exercises the GroupNorm groups that straddle the concat seam (C=384, C=192)."""
    from oracle import fdsr_oracle as O
    cfg, eng, sd = full
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 32, 48, generator=gen)       # non-square, partial tiles
    nl = torch.tensor([[0.02098], [0.7074]])
    cap = {}
    with torch.no_grad():
        ref = O.unet_forward(O.to_torch_sd(sd), cfg, x, nl, capture=cap)
    eng.set_debug(True)
    out = eng.unet_forward(x.cuda(), nl.cuda())
    torch.cuda.synchronize()
    for L in build_layers(cfg):
        got = eng.debug_tensor(L.name).cpu()
        d = (got - cap[L.name]).abs().max().item()
        scale = cap[L.name].abs().max().item()
        report(f'full  {L.name:12s} {L.kind:8s} max|d|={d:.3e} (max|ref|={scale:.2f})')
        assert d <= TOL_FWD * max(scale, 1.0), f'{L.name}: {d}'
    eng.set_debug(False)
    assert (out.cpu() - ref).abs().max().item() <= TOL_FWD


def test_unet_small_vs_golden(small, golden_dir):
    cfg, eng, sd = small
    g = np.load(os.path.join(golden_dir, 'unet_small.npz'))
    x = torch.from_numpy(g['x']).cuda()
    for i in range(4):
        eps = eng.unet_forward(x, torch.from_numpy(g[f'nl/{i}']).cuda()).cpu().numpy()
        d = np.abs(eps - g[f'eps/{i}']).max()
        report(f'unet_small golden eps/{i} max|d|={d:.3e}')
        assert d <= TOL_FWD


def test_unet_full_vs_golden(full, golden_dir):
    cfg, eng, sd = full
    g = np.load(os.path.join(golden_dir, 'unet_full.npz'))
    gen = torch.Generator().manual_seed(21)
    x64 = torch.randn(1, 6, 64, 64, generator=gen)
    x32 = torch.randn(2, 6, 32, 32, generator=gen)
    e64 = eng.unet_forward(x64.cuda(), torch.full((1, 1), 0.5).cuda()).cpu().numpy()
    e32 = eng.unet_forward(x32.cuda(), torch.tensor([[0.0209801132], [0.9919746]]).cuda()).cpu().numpy()
    d64, d32 = np.abs(e64 - g['eps64']).max(), np.abs(e32 - g['eps32']).max()
    report(f'unet_full golden eps64 max|d|={d64:.3e} eps32 max|d|={d32:.3e}')
    assert d64 <= TOL_FWD and d32 <= TOL_FWD


def test_sample_loop_vs_golden(full, golden_dir):
    """20-step trajectory, B=2, 32x32, against the reference's own p_sample outputs."""
    cfg, eng, sd = full
    g = np.load(os.path.join(golden_dir, 'sample_loop.npz'))
    cond, noise = synth_inputs(2, 32, 32, 20)
    out, traj = eng.sample(cond.cuda(), noise.cuda(), want_traj=True)
    out, traj = out.cpu().numpy(), traj.cpu().numpy()
    per_step = np.abs(traj - g['traj32']).reshape(20, -1).max(axis=1)
    report('loop32 per-step max|d|: ' + ' '.join(f'{v:.1e}' for v in per_step))
    d = np.abs(out - g['out32']).max()
    report(f'loop32 final max|d|={d:.3e}')
    assert per_step.max() <= TOL_LOOP and d <= TOL_LOOP
    # B=1 through the reference's own p_sample_loop entry point (continous False / True[-1])
    out1 = eng.sample(cond[:1].cuda(), noise[:, :1].contiguous().cuda()).cpu().numpy()
    assert np.abs(out1 - g['final32_b1']).max() <= TOL_LOOP
    assert np.abs(out1 - g['continous32_b1'][-1:]).max() <= TOL_LOOP
    cond64, noise64 = synth_inputs(1, 64, 64, 20)
    out64 = eng.sample(cond64.cuda(), noise64.cuda()).cpu().numpy()
    d64 = np.abs(out64 - g['out64']).max()
    report(f'loop64 final max|d|={d64:.3e}')
    assert d64 <= TOL_LOOP


def test_graph_replay_matches_eager(full):
    cfg, eng, sd = full
    cond, noise = synth_inputs(2, 64, 64, 20)
    c, n = cond.cuda(), noise.cuda()
    a = eng.sample(c, n).clone()
    out = torch.empty_like(a)
    torch.cuda.synchronize()          # the side stream shares the workspace with the eager run
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.sample(c, n, graph=True, out=out)      # capture + first launch
        eng.sample(c, n, graph=True, out=out)      # replay
    s.synchronize()
    d = (a - out).abs().max().item()
    report(f'graph vs eager max|d|={d:.3e}')
    assert d <= TOL_LOOP / 4


def _oracle_256(sd, cfg, idx, cond, noise):
    """Oracle image of one 256x256 loop (~7-25 s of CPU): cached for the whole session and shared with the other GPU test
    modules (tests/conftest.py: oracle_loop_image)."""
    from conftest import oracle_loop_image
    return oracle_loop_image(sd, cfg, cond, noise)


@pytest.mark.parametrize('prec', ['f32', 'f16x3'])
def test_full_size_256_vs_oracle(full, prec):
    """BASELINE config shape (256x256), B=1, full 20 steps against the oracle, in the exact-fp32 mode and in
    the fp32-grade split-f16 mode bench.py runs by default."""
    from oracle import fdsr_oracle as O
    cfg, eng, sd = full
    cond, noise = synth_inputs(1, 256, 256, 20)
    ref = _oracle_256(sd, cfg, 'b1', cond, noise)
    eng.set_precision(prec)
    try:
        out = eng.sample(cond.cuda(), noise.cuda()).cpu()
    finally:
        eng.set_precision('f32')
    d = (out - ref).abs().max().item()
    psnr_ref = O.psnr_u8(O.tensor2img_u8(ref[0]), O.tensor2img_u8(cond[0]))
    psnr_out = O.psnr_u8(O.tensor2img_u8(out[0]), O.tensor2img_u8(cond[0]))
    report(f'256x256 B=1 loop [{prec}] vs oracle max|d|={d:.3e}  PSNR(out,cond)={psnr_out:.4f} PSNR(ref,cond)={psnr_ref:.4f}')
    assert d <= TOL_LOOP
    assert abs(psnr_out - psnr_ref) <= 0.01
    # a second image on the B = 1 kernel selection (split-K launches, 2-row tiles: other kernels than a batch takes), eager and as a
    # replayed graph: image 3 of the B=16 test's batch, whose oracle image that test shares through the session cache
    cond16, noise16 = synth_inputs(16, 256, 256, 20)
    c3, n3 = cond16[3:4].contiguous(), noise16[:, 3:4].contiguous()
    ref3 = _oracle_256(sd, cfg, 'b16_3', c3, n3)
    eng.set_precision(prec)
    try:
        o3 = eng.sample(c3.cuda(), n3.cuda()).cpu()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            eng.sample(c3.cuda(), n3.cuda(), graph=True)
            g3 = eng.sample(c3.cuda(), n3.cuda(), graph=True).cpu()      # the second call replays
        s.synchronize()
    finally:
        eng.set_precision('f32')
    d3 = (o3 - ref3).abs().max().item()
    report(f'256x256 B=1 loop [{prec}], second image vs oracle max|d|={d3:.3e}; graph replay == eager: {torch.equal(g3, o3)}')
    assert d3 <= TOL_LOOP and torch.equal(g3, o3)


@pytest.mark.parametrize('prec', ['f32', 'f16x3'])
def test_batch16_properties(full, prec):
    """BASELINE configs[1] workload (B=16, 256x256) in both fp32-grade modes: batch independence, run-to-run
    stability (size-independent properties) and one image of the batch against the oracle."""
    cfg, eng, sd = full
    from conftest import plant_standard_pair
    cond, noise = synth_inputs(16, 256, 256, 20)
    plant_standard_pair(cond, noise, 15)       # image 15 is the one compared with the oracle: the session's shared image
    c, n = cond.cuda(), noise.cuda()
    eng.set_precision(prec)
    try:
        out = eng.sample(c, n).clone()
        assert torch.isfinite(out).all()
        assert out.abs().max().item() <= 1.5 + 1e-6          # clamp(r)/2 + cond, cond in [-1,1]
        out2 = eng.sample(c, n)
        d_rep = (out - out2).abs().max().item()
        i = 11
        one = eng.sample(c[i:i + 1].contiguous(), n[:, i:i + 1].contiguous())
        d_b = (one - out[i:i + 1]).abs().max().item()
        # the same images in another batch order: bitwise the same per image (no operator mixes batch elements)
        perm = torch.roll(torch.arange(16), 5)
        outp = eng.sample(c[perm].contiguous(), n[:, perm].contiguous())
        d_perm = (outp - out[perm.cuda()]).abs().max().item()
    finally:
        eng.set_precision('f32')
    report(f'B=16 256x256 [{prec}]: rerun max|d|={d_rep:.3e}  batch-independence max|d|={d_b:.3e}  permuted batch max|d|={d_perm:.3e}')
    # no atomics anywhere on the path (GroupNorm statistics are per-tile partials summed in a fixed
    # order): a rerun is bitwise identical, like the reference's CPU loop (SURVEY 8c noise floor)
    assert d_rep == 0.0 and d_perm == 0.0 and d_b <= TOL_LOOP / 4
    # and the last image of the batch against the oracle directly (its own cond and noise)
    ref = _oracle_256(sd, cfg, 'b16_15', cond[15:16], noise[:, 15:16])
    d_o = (out[15:16].cpu() - ref).abs().max().item()
    report(f'B=16 256x256 [{prec}]: image 15 of the batch vs oracle max|d|={d_o:.3e}')
    assert d_o <= TOL_LOOP
    # ... and a second one, with the batch's OWN cond and noise (not the session's shared pair): one more oracle loop, cached for
    # the other precision of this test
    ref3 = _oracle_256(sd, cfg, 'b16_3', cond[3:4], noise[:, 3:4])
    d_3 = (out[3:4].cpu() - ref3).abs().max().item()
    report(f'B=16 256x256 [{prec}]: image 3 of the batch vs oracle max|d|={d_3:.3e}')
    assert d_3 <= TOL_LOOP


@pytest.mark.parametrize('prec,tol_fwd,tol_loop', [('f16x3', 1e-4, 1e-3), ('bf16', 0.03, None)])
def test_precision_modes_layerwise_and_loop(full, golden_dir, prec, tol_fwd, tol_loop):
    """16-bit MFMA convolutions: f16x3 (hi/lo split, fp32-grade) must stay inside the fp32
    parity bounds; bf16 is judged on PSNR (north_star: PSNR within 0.01 dB), not on 1e-3 -- but its layers must stay within
    3 % of the layer's range (measured worst 1.1 %: bf16 has 8 mantissa bits, 2^-9 = 0.2 % per rounding) and the loop's output
    within 50 dB of the oracle's (a bound that CAN fail: the PSNR-against-HR difference below cannot, at a random-init network's 13 dB).
    (The bf16 / f16 kernels are judged per operator and per element against the modes' own arithmetic in tests/test_gpu_unet_16bit_layerwise.py.)"""
    from oracle import fdsr_oracle as O
    cfg, eng, sd = full
    eng.set_precision(prec)
    try:
        gen = torch.Generator().manual_seed(5)
        x = torch.randn(2, 6, 32, 48, generator=gen)
        nl = torch.tensor([[0.02098], [0.7074]])
        cap = {}
        with torch.no_grad():
            ref = O.unet_forward(O.to_torch_sd(sd), cfg, x, nl, capture=cap)
        eng.set_debug(True)
        out = eng.unet_forward(x.cuda(), nl.cuda())
        torch.cuda.synchronize()
        for L in build_layers(cfg):
            got = eng.debug_tensor(L.name).cpu()
            d = (got - cap[L.name]).abs().max().item()
            scale = cap[L.name].abs().max().item()
            report(f'{prec:5s} {L.name:12s} {L.kind:8s} max|d|={d:.3e} (max|ref|={scale:.2f})')
            assert d <= tol_fwd * max(scale, 1.0), f'{L.name}: {d}'
        eng.set_debug(False)
        g = np.load(os.path.join(golden_dir, 'sample_loop.npz'))
        cond, noise = synth_inputs(2, 32, 32, 20)
        o, traj = eng.sample(cond.cuda(), noise.cuda(), want_traj=True)
        per_step = np.abs(traj.cpu().numpy() - g['traj32']).reshape(20, -1).max(axis=1)
        d = np.abs(o.cpu().numpy() - g['out32']).max()
        report(f'{prec} loop32 per-step max|d|: ' + ' '.join(f'{v:.1e}' for v in per_step) + f' final {d:.3e}')
        cond64, noise64 = synth_inputs(1, 64, 64, 20)
        o64 = eng.sample(cond64.cuda(), noise64.cuda()).cpu()
        d64 = np.abs(o64.numpy() - g['out64']).max()
        rmse64 = float(np.sqrt(np.mean((o64.numpy() - g['out64']) ** 2)))     # (before tensor2img_u8 below clamps o64 in place)
        ref64 = torch.from_numpy(g['out64'])
        hr = (cond64 + 0.3 * torch.sin(torch.arange(64).float() / 5).view(1, 1, 1, 64)).clamp(-1, 1)
        dps = abs(O.psnr_u8(O.tensor2img_u8(o64[0]), O.tensor2img_u8(hr[0])) - O.psnr_u8(O.tensor2img_u8(ref64[0]), O.tensor2img_u8(hr[0])))
        report(f'{prec} loop64 final max|d|={d64:.3e} PSNR delta vs reference={dps:.5f} dB')
        if tol_loop is not None:
            assert per_step.max() <= tol_loop and d <= tol_loop and d64 <= tol_loop
        else:
            psnr_vs_ref = 20 * np.log10(2.0 / rmse64)              # images live in [-1, 1]: data range 2
            report(f'{prec} loop64 PSNR(out, reference out) = {psnr_vs_ref:.2f} dB (rmse {rmse64:.3e})')
            assert psnr_vs_ref >= 50.0
        assert dps <= 0.01
    finally:
        eng.set_debug(False)
        eng.set_precision('f32')


def test_error_paths(full):
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.engine import Engine
    cfg, eng, sd = full
    with pytest.raises(_lib.FdsrError):
        eng.load_weight('downs.0.weight', np.zeros((64, 5, 3, 3), np.float32))     # shape mismatch
    with pytest.raises(_lib.FdsrError):
        eng.load_weight('nope.weight', np.zeros((1,), np.float32))                 # unexpected key
    with pytest.raises(_lib.FdsrError):
        eng.workspace_bytes(1, 60, 64)                                             # not a multiple of 8
    # bf16 mode stores activations as bf16: refused where a kernel on the path would read them as fp32
    with pytest.raises(_lib.FdsrError, match='multiple of'):
        Engine(UNetConfig(in_channel=6, out_channel=3, inner_channel=24, norm_groups=8, channel_mults=(1, 2), res_blocks=1))
    e4 = Engine(UNetConfig(in_channel=6, out_channel=3, inner_channel=32, channel_mults=(1, 2), attn_res=(16,), res_blocks=1,
                           image_size=32, variant='ddpm'))
    e4.set_precision('bf16')            # every variant has a bf16 mode (attention on bf16 MFMA: test_gpu_sr3.py, _tesr, _gdp)
    e2 = Engine(cfg)
    with pytest.raises(_lib.FdsrError):                                            # weights missing
        e2.unet_forward(torch.zeros(1, 6, 32, 32).cuda(), torch.zeros(1).cuda())
    with pytest.raises(RuntimeError):
        eng.unet_forward(torch.zeros(1, 6, 32, 32), torch.zeros(1))                # CPU tensor: no fallback


@pytest.mark.parametrize('kw,shape', [
    (dict(in_channel=6, out_channel=3, inner_channel=32, channel_mults=(1, 2), res_blocks=3), (2, 40, 72)),
    (dict(in_channel=6, out_channel=3, inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=1), (1, 64, 96)),
    (dict(in_channel=6, out_channel=3, inner_channel=96, channel_mults=(1, 2, 2), res_blocks=2), (1, 32, 32)),
])
def test_other_architectures(kw, shape):
    """The UNet constructor's other hyper-parameters (channel multipliers incl. 512-channel levels, block
    counts, inner widths that are not powers of two, ragged sizes) in both fp32-grade modes."""
    from fastdiffsr_amd.engine import Engine
    from oracle import fdsr_oracle as O
    cfg = UNetConfig(**kw)
    sd = synth_state_dict(cfg, 3)
    eng = Engine(cfg)
    eng.load_state_dict(sd)
    B, H, W = shape
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(B, 6, H, W, generator=gen)
    nl = torch.rand(B, 1, generator=gen)
    with torch.no_grad():
        ref = O.unet_forward(O.to_torch_sd(sd), cfg, x, nl)
    for prec in ('f32', 'f16x3'):
        eng.set_precision(prec)
        out = eng.unet_forward(x.cuda(), nl.cuda()).cpu()
        d = (out - ref).abs().max().item()
        report(f'arch {kw["inner_channel"]}/{kw["channel_mults"]}/{kw["res_blocks"]} {shape} {prec}: max|d|={d:.3e} (max|ref|={ref.abs().max():.2f})')
        assert d <= TOL_FWD * max(1.0, ref.abs().max().item())


def test_infer_size_512(full):
    """infer.py runs the same network on 512x512 inputs: one forward against the oracle."""
    from oracle import fdsr_oracle as O
    cfg, eng, sd = full
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(1, 6, 512, 512, generator=gen)
    nl = torch.tensor([[0.4681449]])
    with torch.no_grad():
        ref = O.unet_forward(O.to_torch_sd(sd), cfg, x, nl)
    for prec in ('f16x3', 'f32'):
        eng.set_precision(prec)
        d = (eng.unet_forward(x.cuda(), nl.cuda()).cpu() - ref).abs().max().item()
        report(f'512x512 forward {prec}: max|d|={d:.3e}')
        assert d <= TOL_FWD
    eng.set_precision('f32')


@pytest.mark.timeout(900)
@pytest.mark.parametrize('mode', ['0', '1'])
def test_res_conv_as_its_own_launch_or_riding_by_rule(mode):
    """By default every ResnetBlock res_conv rides inside block2's 3x3 launch on the 16-bit kernels (ConvParams::xr0);
    the debug option rider=0 keeps it a launch of its own, =1 lets only the bandwidth-bound ones ride.  Each setting must meet
    the same layer-by-layer and 20-step-loop bounds against the oracle in f16x3 and bf16 (a fresh process per setting)."""
    import subprocess
    import sys
    env = dict(os.environ)
    env['FDSR_TEST_DEBUG_OPTION'] = f'rider={mode}'
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, '-m', 'pytest', here, '-m', 'gpu', '-q', '-x', '-k',
                        'test_precision_modes_layerwise_and_loop or test_other_architectures'],
                       env=env, capture_output=True, text=True, timeout=840, cwd=os.path.dirname(os.path.dirname(here)))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout
