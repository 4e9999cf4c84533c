"""SwinIR on the device against the fp64 restatement (tests/swinir_restatement.py), judged by the reference's own fp32 noise:

    max |device - fp64| <= 4 e32          per case and tap,   e32 = max |reference in fp32 (tests/golden/swinir.npz) - fp64|

e32 is computed here on the CPU, never from the device.  The factor 4 covers the different fp32 summation order of the MFMA
chains against the CPU's GEMM over K up to 1620: both are fp32 sums of the same terms.  tests/test_swinir_host.py shows that a
wrong mask, bias index, roll or GELU form moves the output by more than 100 e32.  Then the determinism contract (reruns, batch
independence, graph replay), to_u8 and the command line."""
import os

import numpy as np
import pytest
import torch

import swinir_restatement as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'swinir.npz')


def build(base, upscale, seed=R.SEED):
    from fastdiffsr_amd.swinir import SwinIR, load_synthetic
    return load_synthetic(SwinIR(upscale=upscale, **base), seed).cuda()


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


def net_of(nets, name):
    base, upscale, hw, with_taps = R.CASES[name]
    return nets('small' if base is R.SMALL else 'full', upscale)


def reference(golden, name, m):
    """(x, fp64 taps, e32 per recorded key) of a golden case, on the CPU."""
    from fastdiffsr_amd.swinir.arch import tap_names
    from fastdiffsr_amd.synth import synth_swinir
    with_taps = R.CASES[name][3]
    keys = ['out'] + (R.recorded_taps(tap_names(m.cfg)) if with_taps else [])
    x = torch.from_numpy(golden[name + '/x'])
    taps = R.swinir_forward(synth_swinir(m.cfg, R.SEED), m.cfg, x, torch.float64)
    return x, taps, {k: float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, taps[k])).max()) for k in keys}


@pytest.mark.parametrize('name', list(R.CASES))
def test_parity_with_the_fp64_restatement(nets, golden, name):
    """8x8: one window, the shifted block's roll wraps the whole image, all mask regions inside that window, M = 64 under one GEMM
    tile.  16x24: 2 x 3 windows, not square.  12x20: reflect pad by 4 and 4, crop to 48x80.  Scales 2 and 3: the pixel-shuffle
    factor and channel order.  The full configuration: K = 180 / 360 / 1620, N = 540, head_dim 30."""
    m = net_of(nets, name)
    x, taps, e32 = reference(golden, name, m)
    xd = x.cuda()
    for k, e in e32.items():
        dev = (m(xd) if k == 'out' else m.debug_tensor(k, xd)).cpu().double()
        assert dev.shape == taps[k].shape, (k, dev.shape, taps[k].shape)
        err = float((dev - taps[k]).abs().max())
        print('%-12s %-26s device error %.3e   e32 %.3e   ratio %.2f' % (name, k, err, e, err / e))
        assert err <= 4 * e, (name, k, err, e)


def test_full_configuration_batch_of_two_off_square(nets):
    """24x40, B = 2: 3 x 5 windows, M = 1920 (fifteen GEMM tiles), no golden: e32 here is the fp32 run of the restatement against
    its fp64 run -- the same torch CPU arithmetic the golden cases record from the reference."""
    from fastdiffsr_amd.synth import synth_swinir
    m = nets('full', 4)
    x = R.case_input('full_24x40', 2, 24, 40)
    w = synth_swinir(m.cfg, R.SEED)
    r64 = R.swinir_forward(w, m.cfg, x, torch.float64)['out']
    e32 = float((R.swinir_forward(w, m.cfg, x, torch.float32)['out'].double() - r64).abs().max())
    err = float((m(x.cuda()).cpu().double() - r64).abs().max())
    print('full_24x40 B=2: device error %.3e   e32 %.3e   ratio %.2f' % (err, e32, err / e32))
    assert err <= 4 * e32, (err, e32)


def test_scale_eight_without_patch_norm():
    """Three pixel shuffles (the tail's buffers alternate once more) and patch_norm=False (patch_embed passes conv_first's output
    on), on 8x8 and on 9x13 (pad 7 and 3): no golden, e32 is the restatement in fp32 against itself in fp64."""
    from fastdiffsr_amd.swinir import SwinIR, load_synthetic
    from fastdiffsr_amd.synth import synth_swinir
    m = load_synthetic(SwinIR(upscale=8, patch_norm=False, **R.SMALL), R.SEED).cuda()
    w = synth_swinir(m.cfg, R.SEED)
    assert 'patch_embed.norm.weight' not in w
    for h, wd in ((8, 8), (9, 13)):
        x = R.case_input('s8_%dx%d' % (h, wd), 1, h, wd)
        r64 = R.swinir_forward(w, m.cfg, x, torch.float64)
        r32 = R.swinir_forward(w, m.cfg, x, torch.float32)
        for k in ('upsample.2', 'out'):
            e32 = float((r32[k].double() - r64[k]).abs().max())
            dev = (m(x.cuda()) if k == 'out' else m.debug_tensor(k, x.cuda())).cpu().double()
            assert dev.shape == r64[k].shape == ((1, 3, 8 * h, 8 * wd) if k == 'out' else (1, 64, 8 * 16 if h > 8 else 64, 8 * 16 if wd > 8 else 64))
            err = float((dev - r64[k]).abs().max())
            print('s8 %dx%d %-10s device error %.3e   e32 %.3e   ratio %.2f' % (h, wd, k, err, e32, err / e32))
            assert err <= 4 * e32, (h, wd, k, err, e32)


def test_an_input_too_small_to_reflect_pad_is_refused(nets):
    from fastdiffsr_amd import _lib
    m = nets('small', 4)
    for h, w in ((4, 8), (8, 3)):
        with pytest.raises(_lib.FdsrError, match='reflect'):
            m(torch.rand(1, 3, h, w, device='cuda'))
    with pytest.raises(ValueError):
        m(torch.rand(1, 3, 8, 8))                      # a CPU tensor: there is no CPU path


def test_rerun_and_batch_independence_are_bitwise(nets):
    m = nets('small', 4)
    x = R.case_input('contract', 3, 16, 24).cuda()
    y = m(x)
    assert torch.equal(m(x), y)
    for i in range(3):
        assert torch.equal(m(x[i:i + 1])[0], y[i]), i
    assert not torch.equal(y[0], y[1])
    assert torch.equal(m.debug_tensor('layers.1', x), m.debug_tensor('layers.1', x))


def test_graph_replay_equals_eager_bitwise(nets):
    m = build(R.SMALL, 4)                              # its own module: the test changes a weight
    x = R.case_input('contract', 3, 16, 24).cuda()
    eager = m(x)
    assert torch.equal(m(x, graph=True), eager)        # captured
    assert torch.equal(m(x, graph=True), eager)        # replayed
    x2 = R.case_input('contract2', 1, 8, 16).cuda()
    eager2 = m(x2)
    assert torch.equal(m(x2, graph=True), eager2)      # a second (B, H, W)
    assert torch.equal(m(x, graph=True), eager)        # the first graph is still there and still right
    assert torch.equal(m(x2 * 0.5, graph=True), m(x2 * 0.5))   # new values through the same graph
    # loading one tensor drops the graphs: the replay follows the new weights
    with torch.no_grad():
        m.state_dict()['layers.1.residual_group.blocks.1.attn.relative_position_bias_table'].mul_(-1.0)
    changed = m(x, graph=True)
    assert not torch.equal(changed, eager)
    assert torch.equal(changed, m(x))
    assert torch.equal(m(x2, graph=True), m(x2))


def test_to_u8_is_save_img1(nets):
    from fastdiffsr_amd.swinir import to_u8
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 9, 13, generator=g) * 1.6 - 0.3          # leaves [0, 1] on both sides
    x[0, :, 0, :6] = torch.tensor([0.0, 1.0, 254.999 / 255, 1.0 / 255, 0.5, 255.5 / 255])
    assert float(x.min()) < 0 and float(x.max()) > 1
    got = to_u8(x.cuda()).cpu().numpy()
    for i in range(2):
        assert np.array_equal(got[i], R.save_img1(x[i])), i


def test_smoke_small_configuration(nets):
    m = nets('small', 4)
    y = m(torch.rand(2, 3, 16, 16, device='cuda'))
    assert tuple(y.shape) == (2, 3, 64, 64) and bool(torch.isfinite(y).all())


def test_command_line(nets, tmp_path, capsys):
    """Four synthetic PNGs in two class folders: the written PNGs are to_u8(model(lr)) and the printed PSNR is the host metric on
    those files."""
    from PIL import Image
    from fastdiffsr_amd import metrics
    from fastdiffsr_amd.swinir import test as cli, to_u8
    rng = np.random.default_rng(3)
    hr_dir = tmp_path / 'hr'
    files = []
    for cls in ('a', 'b'):
        (hr_dir / cls).mkdir(parents=True)
        for i in range(2):
            yy, xx = np.mgrid[0:66, 0:49]
            img = np.stack([128 + 90 * np.sin(0.2 * xx + c + i) * np.cos(0.15 * yy + 2 * c) for c in range(3)], -1) + rng.normal(0, 6, (66, 49, 3))
            p = hr_dir / cls / ('im%d.png' % i)
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(p)
            files.append((cls, p))
    m = nets('small', 4)
    ckpt = tmp_path / 'generator_param.pkl'
    torch.save(m.state_dict(), ckpt)
    out_dir = tmp_path / 'out'
    base = R.SMALL
    rc = cli.main(['--model', str(ckpt), '--hr', str(hr_dir), '--scale', '4', '-o', str(out_dir), '--batch', '2', '--embed-dim', str(base['embed_dim']),
                   '--depths', '2,2', '--num-heads', '6,6'])
    assert rc in (0, None)
    printed = capsys.readouterr().out
    psnrs = []
    for cls, p in files:
        hr = np.asarray(Image.open(p).convert('RGB'))
        hr = hr[:hr.shape[0] // 4 * 4, :hr.shape[1] // 4 * 4]                       # 64 x 48
        lr = np.asarray(Image.fromarray(hr).resize((hr.shape[1] // 4, hr.shape[0] // 4), Image.BICUBIC))
        x = torch.from_numpy(lr.copy()).permute(2, 0, 1).float().div(255).unsqueeze(0).cuda()
        want = to_u8(m(x))[0].cpu().numpy()
        got = np.asarray(Image.open(out_dir / cls / p.name))
        assert np.array_equal(got, want), p
        psnrs.append(metrics.calculate_psnr(got, hr))
    assert ('PSNR %.4f' % np.mean(psnrs)) in printed, printed
