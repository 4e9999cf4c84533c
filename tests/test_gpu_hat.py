"""HAT on the device against the fp64 restatement (tests/hat_restatement.py), judged by the reference's own fp32 noise:

    max |device - fp64| <= 4 e32          per case and tap,   e32 = max |reference in fp32 (tests/golden/hat.npz) - fp64|

e32 is computed here on the CPU, never from the device.  The factor 4 covers the different fp32 summation order of the MFMA
chains against the CPU's GEMM over K up to 1620 and of the softmax rows of 256 and 576 terms: both sides are fp32 sums of the
same terms.  tests/test_hat_host.py shows that each of ten wrong forms moves the output by more than 100 e32.  Then the
uncropped output shape, the determinism contract (reruns, batch independence, graph replay), the aliased upsampling keys of
the C ABI, and the command line."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hat_restatement as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'hat.npz')


def build(base, upscale, seed=R.SEED):
    from fastdiffsr_amd.hat import HAT, load_synthetic
    return load_synthetic(HAT(upscale=upscale, **base), seed).cuda()


@pytest.fixture(scope='module')
def nets():
    """(configuration name, upscale) -> the module on the device, built once."""
    cache = {}

    def get(which, upscale):
        if (which, upscale) not in cache:
            cache[(which, upscale)] = build(R.SMALL if which == 'small' else R.FULL, upscale)
        return cache[(which, upscale)]
    return get


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def reference(golden, name, m):
    """(x, fp64 taps, e32 per checked key) of a case, on the CPU.  A case outside the golden file is judged at the output, e32
    being the restatement in fp32 against itself in fp64."""
    from fastdiffsr_amd.hat.arch import tap_names
    from fastdiffsr_amd.synth import synth_hat
    base, upscale, hw, with_taps, in_golden = R.CASES[name]
    w = synth_hat(m.cfg, R.SEED)
    x = R.case_input(name, 1, *hw)
    taps = R.hat_forward(w, m.cfg, x, torch.float64)
    if not in_golden:
        return x, taps, {'out': float((R.hat_forward(w, m.cfg, x, torch.float32)['out'].double() - taps['out']).abs().max())}
    keys = ['out'] + (R.recorded_taps(tap_names(m.cfg)) if with_taps else [])
    return x, taps, {k: float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, taps[k])).max()) for k in keys}


@pytest.mark.parametrize('name', list(R.CASES))
def test_parity_with_the_fp64_restatement(nets, golden, name):
    """16x16: one window, the shifted HAB's roll wraps the whole image, all mask regions inside that window, 320 of the 576 OCA
    keys outside the image.  32x48 and 48x32: 2 x 3 and 3 x 2 windows, interior OCA keys from neighbouring windows.  20x36: reflect
    pad by 12 and 12, the pool over the padded map, the output stays 128x192.  Scales 2, 3 and 8: the pixel-shuffle factor, the
    shared convolution run once, twice, three times.  The full configuration: K = 180 / 540 / 720 / 1620, head_dim 30."""
    base, upscale, hw, _, _ = R.CASES[name]
    m = nets('small' if base is R.SMALL else 'full', upscale)
    x, taps, e32 = reference(golden, name, m)
    xd = x.cuda()
    worst = []
    for k, e in e32.items():
        dev = (m(xd) if k == 'out' else m.debug_tensor(k, xd)).cpu().double()
        assert dev.shape == taps[k].shape, (k, dev.shape, taps[k].shape)
        err = float((dev - taps[k]).abs().max())
        print('%-12s %-26s device error %.3e   e32 %.3e   ratio %.2f' % (name, k, err, e, err / e))
        if err > 4 * e:
            worst.append((name, k, err, e))
    assert not worst, worst
    if name == 's4_20x36':
        assert tuple(m(xd).shape) == (1, 3, 128, 192)      # (32 x 48) times 4: not cropped


def test_full_configuration_batch_of_two_off_square(nets):
    """32x48, B = 2: 2 x 3 windows, M = 3072 (24 GEMM tiles, 48 partial sums per image), no golden: e32 here is the fp32 run of the
    restatement against its fp64 run -- the same torch CPU arithmetic the golden cases record from the reference."""
    from fastdiffsr_amd.synth import synth_hat
    m = nets('full', 4)
    x = R.case_input('full_32x48', 2, 32, 48)
    w = synth_hat(m.cfg, R.SEED)
    r64 = R.hat_forward(w, m.cfg, x, torch.float64)['out']
    e32 = float((R.hat_forward(w, m.cfg, x, torch.float32)['out'].double() - r64).abs().max())
    err = float((m(x.cuda()).cpu().double() - r64).abs().max())
    print('full_32x48 B=2: device error %.3e   e32 %.3e   ratio %.2f' % (err, e32, err / e32))
    assert err <= 4 * e32, (err, e32)


def test_an_input_too_small_to_reflect_pad_is_refused(nets):
    from fastdiffsr_amd import _lib
    m = nets('small', 4)
    for h, w in ((8, 16), (16, 8)):
        with pytest.raises(_lib.FdsrError, match='reflect'):
            m(torch.rand(1, 3, h, w, device='cuda'))
    with pytest.raises(ValueError):
        m(torch.rand(1, 3, 16, 16))                    # a CPU tensor: there is no CPU path


def test_rerun_and_batch_independence_are_bitwise(nets):
    m = nets('small', 4)
    x = R.case_input('contract', 3, 32, 48).cuda()
    y = m(x)
    assert tuple(y.shape) == (3, 3, 128, 192)
    assert torch.equal(m(x), y)
    for i in range(3):
        assert torch.equal(m(x[i:i + 1])[0], y[i]), i
    assert not torch.equal(y[0], y[1])
    for tap in ('layers.0.blocks.1.cab', 'layers.0.ocab.attn', 'layers.1'):
        assert torch.equal(m.debug_tensor(tap, x), m.debug_tensor(tap, x)), tap


def test_graph_replay_equals_eager_bitwise(nets):
    m = build(R.SMALL, 4)                              # its own module: the test changes a weight
    x = R.case_input('contract', 3, 32, 48).cuda()
    eager = m(x)
    assert torch.equal(m(x, graph=True), eager)        # captured
    assert torch.equal(m(x, graph=True), eager)        # replayed
    x2 = R.case_input('contract2', 1, 16, 20).cuda()
    eager2 = m(x2)
    assert torch.equal(m(x2, graph=True), eager2)      # a second (B, H, W)
    assert torch.equal(m(x, graph=True), eager)        # the first graph is still there and still right
    assert torch.equal(m(x2 * 0.5, graph=True), m(x2 * 0.5))   # new values through the same graph
    # loading one tensor drops the graphs: the replay follows the new weights
    with torch.no_grad():
        m.state_dict()['layers.1.residual_group.overlap_attn.relative_position_bias_table'].mul_(-1.0)
    changed = m(x, graph=True)
    assert not torch.equal(changed, eager)
    assert torch.equal(changed, m(x))
    assert torch.equal(m(x2, graph=True), m(x2))


def test_c_abi_runs_x4_from_the_first_upsampling_key_alone(nets):
    """The engine keeps ONE upsampling convolution: loading upsample.upsampling.0.* is enough for both stages of x4, and the
    names .2.* load the same tensor."""
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.synth import synth_hat
    lib = _lib.load()
    m = nets('small', 4)
    w = synth_hat(m.cfg, R.SEED)
    assert not any(k.startswith('upsample.upsampling.2.') for k in w)
    h = m.__class__(upscale=4, **R.SMALL)               # a second engine, loaded by hand through the C ABI
    handle = h._handle()

    def load(name, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        return lib.fdsr_hat_load(handle, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim)

    for k, a in w.items():
        assert load(k, a) == 0, k
    x = R.case_input('abi', 1, 16, 16).cuda()
    want = m(x)
    out = torch.empty_like(want)
    ws = torch.empty(h.workspace_bytes(1, 16, 16), dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def forward():
        rc = lib.fdsr_hat_forward(handle, C.c_void_p(x.data_ptr()), 1, 16, 16, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                  C.c_void_p(st), 0)
        assert rc == 0, lib.fdsr_last_error(None)
        torch.cuda.synchronize()
        return out.clone()

    assert torch.equal(forward(), want)
    assert load('upsample.upsampling.2.bias', w['upsample.upsampling.0.bias'] + 1.0) == 0      # the alias reaches the one tensor
    assert not torch.equal(forward(), want)
    assert load('upsample.upsampling.4.bias', w['upsample.upsampling.0.bias']) != 0            # x4 has no third stage
    assert load('relative_position_index_SA', np.zeros((256, 256))) != 0                       # buffers never go to the device


def test_smoke_small_configuration(nets):
    m = nets('small', 4)
    y = m(torch.rand(2, 3, 16, 16, device='cuda'))
    assert tuple(y.shape) == (2, 3, 64, 64) and bool(torch.isfinite(y).all())


def test_command_line(nets, tmp_path, capsys):
    """Four synthetic PNGs in two class folders: the written PNGs are to_u8(model(lr)) cut to (H * 4, W * 4) and the printed PSNR is
    the host metric on those files."""
    from PIL import Image
    from fastdiffsr_amd import metrics
    from fastdiffsr_amd.hat import test as cli, to_u8
    rng = np.random.default_rng(3)
    hr_dir = tmp_path / 'hr'
    files = []
    for cls in ('a', 'b'):
        (hr_dir / cls).mkdir(parents=True)
        for i in range(2):
            yy, xx = np.mgrid[0:82, 0:97]
            img = np.stack([128 + 90 * np.sin(0.2 * xx + c + i) * np.cos(0.15 * yy + 2 * c) for c in range(3)], -1) + rng.normal(0, 6, (82, 97, 3))
            p = hr_dir / cls / ('im%d.png' % i)
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(p)
            files.append((cls, p))
    m = nets('small', 4)
    ckpt = tmp_path / 'generator_param.pkl'
    torch.save(m.state_dict(), ckpt)
    out_dir = tmp_path / 'out'
    rc = cli.main(['--model', str(ckpt), '--hr', str(hr_dir), '--scale', '4', '-o', str(out_dir), '--batch', '2', '--embed-dim',
                   str(R.SMALL['embed_dim']), '--depths', '2,2', '--num-heads', '6,6', '--squeeze-factor', str(R.SMALL['squeeze_factor'])])
    assert rc in (0, None)
    printed = capsys.readouterr().out
    assert 'HAT' in printed and 'SwinIR' not in printed
    psnrs = []
    for cls, p in files:
        hr = np.asarray(Image.open(p).convert('RGB'))
        hr = hr[:hr.shape[0] // 4 * 4, :hr.shape[1] // 4 * 4]                       # 80 x 96
        lr = np.asarray(Image.fromarray(hr).resize((hr.shape[1] // 4, hr.shape[0] // 4), Image.BICUBIC))      # 20 x 24: padded to 32 x 32
        x = torch.from_numpy(lr.copy()).permute(2, 0, 1).float().div(255).unsqueeze(0).cuda()
        sr = m(x)
        assert tuple(sr.shape) == (1, 3, 128, 128)
        want = to_u8(sr[:, :, :80, :96])[0].cpu().numpy()
        got = np.asarray(Image.open(out_dir / cls / p.name))
        assert np.array_equal(got, want), p
        psnrs.append(metrics.calculate_psnr(got, hr))
    assert ('PSNR %.4f' % np.mean(psnrs)) in printed, printed
