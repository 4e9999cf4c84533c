"""TransENet on the device against the fp64 restatement (tests/transenet_restatement.py), judged by the reference's own fp32
noise:

    max |device - fp64| <= 4 e32          per case and tap,   e32 = max |reference in fp32 (tests/golden/transenet.npz) - fp64|

e32 is computed here on the CPU, never from the device; for the two cases outside the golden file it is the restatement's fp32
run against its fp64 run.  The factor 4 is the project's (DESIGN sections 17 and 18) for fp32 sums of the same terms in
another order: the MFMA chains against the CPU's GEMM over K up to 1024, and softmax rows of 8 to 1024 terms.
tests/test_transenet_host.py shows that each of nine wrong forms moves the output by more than 100 e32.  Then the determinism
contract (reruns, batch independence, graph replay), the C ABI by hand, and the command line."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import transenet_restatement as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'transenet.npz')


def build(base, scale, hr_patch_size, seed=R.SEED):
    from fastdiffsr_amd.transenet import TransENet, load_synthetic
    return load_synthetic(TransENet(scale=scale, hr_patch_size=hr_patch_size, **base), seed).cuda()


@pytest.fixture(scope='module')
def nets():
    """(configuration name, scale, hr_patch_size) -> the module on the device, built once."""
    cache = {}

    def get(which, scale, hr):
        if (which, scale, hr) not in cache:
            cache[(which, scale, hr)] = build(R.SMALL if which == 'small' else R.FULL, scale, hr)
        return cache[(which, scale, hr)]
    return get


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def reference(golden, name, m):
    """(x, fp64 taps, e32 per checked key) of a case, on the CPU."""
    from fastdiffsr_amd.synth import synth_transenet
    _, _, batch, hw, with_taps, in_golden = R.CASES[name]
    w = synth_transenet(m.cfg, R.SEED)
    x = R.case_input(name, batch, *hw)
    taps = R.transenet_forward(w, m.cfg, x, torch.float64)
    if not in_golden:
        return x, taps, {'out': float((R.transenet_forward(w, m.cfg, x, torch.float32)['out'].double() - taps['out']).abs().max())}
    keys = ['out'] + (R.recorded_taps(m.cfg) if with_taps else [])
    return x, taps, {k: float(np.abs(golden[name + '/' + k] - R.sampled(name + '/' + k, taps[k])).max()) for k in keys}


@pytest.mark.parametrize('name', list(R.CASES))
def test_parity_with_the_fp64_restatement(nets, golden, name):
    """32x32 at x4: 16 low tokens (half an MFMA tile of keys and of queries), 256 high.  32x16: 8 and 128, an off-square token
    grid.  32x40: 20 and 160, no multiple of 32 nor of the 128-key chunk, a partial last chunk and a partial last query block.
    x3: 144 high tokens, PixelShuffle(3).  x2: 64.  x8: 1024 high tokens in eight key chunks, three upsampler stages.  The full
    configuration: channels 16 (K = 1024 in the patch GEMM), 64 / 1024 tokens, eight layers per encoder; then 32 / 512 tokens in
    a batch of two (the batch stride of the attention and of the patch gather and scatter).

    Measured on an MI355X (max over the taps of a case, device error / e32): see DESIGN section 19."""
    base, scale, _, hw, _, _ = R.CASES[name]
    m = nets('small' if base is R.SMALL else 'full', scale, hw[0] * scale)
    x, taps, e32 = reference(golden, name, m)
    xd = x.cuda()
    worst = []
    for k, e in e32.items():
        dev = (m(xd) if k == 'out' else m.debug_tensor(k, xd)).cpu().double()
        assert dev.shape == taps[k].shape, (k, dev.shape, taps[k].shape)
        err = float((dev - taps[k]).abs().max())
        print('%-14s %-26s device error %.3e   e32 %.3e   ratio %.2f' % (name, k, err, e, err / e))
        if err > 4 * e:
            worst.append((name, k, err, e))
    assert not worst, worst


def test_rerun_and_batch_independence_are_bitwise(nets):
    m = nets('small', 4, 128)
    x = R.case_input('contract', 3, 32, 40).cuda()
    y = m(x)
    assert tuple(y.shape) == (3, 3, 128, 160)
    assert torch.equal(m(x), y)
    for i in range(3):
        assert torch.equal(m(x[i:i + 1])[0], y[i]), i
    assert not torch.equal(y[0], y[1])
    for tap in ('encoder_up.0.attn', 'decoder2.0.cross', 'embedding_to_patch'):
        assert torch.equal(m.debug_tensor(tap, x), m.debug_tensor(tap, x)), tap


def test_graph_replay_equals_eager_bitwise(nets):
    m = build(R.SMALL, 4, 128)                         # its own module: the test changes a weight
    x = R.case_input('contract', 3, 32, 40).cuda()
    eager = m(x)
    assert torch.equal(m(x, graph=True), eager)        # captured
    assert torch.equal(m(x, graph=True), eager)        # replayed
    x2 = R.case_input('contract2', 1, 32, 16).cuda()
    eager2 = m(x2)
    assert torch.equal(m(x2, graph=True), eager2)      # a second (B, H, W)
    assert torch.equal(m(x, graph=True), eager)        # the first graph is still there and still right
    assert torch.equal(m(x2 * 0.5, graph=True), m(x2 * 0.5))   # new values through the same graph
    # loading one tensor drops the graphs: the replay follows the new weights
    with torch.no_grad():
        m.state_dict()['decoder2.layers.0.1.fn.fn.to_k.weight'].mul_(-1.0)
    changed = m(x, graph=True)
    assert not torch.equal(changed, eager)
    assert torch.equal(changed, m(x))
    assert torch.equal(m(x2, graph=True), m(x2))


def test_c_abi_loaded_by_hand_equals_the_module(nets):
    """The engine takes its geometry from the input: a 16x24 image runs through the C ABI although no module would pass it."""
    from fastdiffsr_amd import _lib
    from fastdiffsr_amd.synth import synth_transenet
    lib = _lib.load()
    m = nets('small', 4, 128)
    w = synth_transenet(m.cfg, R.SEED)
    h = m.__class__(scale=4, hr_patch_size=128, **R.SMALL)      # a second engine, loaded by hand through the C ABI
    handle = h._handle()

    def load(name, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        return lib.fdsr_transenet_load(handle, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim)

    x = R.case_input('abi', 1, 32, 32).cuda()
    want = m(x)
    out = torch.empty_like(want)
    ws = torch.empty(h.workspace_bytes(1, 32, 32), dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def forward(xx, oo, hh, ww):
        rc = lib.fdsr_transenet_forward(handle, C.c_void_p(xx.data_ptr()), 1, hh, ww, C.c_void_p(oo.data_ptr()), C.c_void_p(ws.data_ptr()),
                                        ws.numel(), C.c_void_p(st), 0)
        torch.cuda.synchronize()
        return rc

    last = list(w)[-1]
    for k, a in w.items():
        if k != last:
            assert load(k, a) == 0, k
    assert forward(x, out, 32, 32) == -3 and b'missing' in lib.fdsr_last_error(None)       # FDSR_E_STATE: one tensor is not loaded
    assert load(last, w[last]) == 0
    assert forward(x, out, 32, 32) == 0, lib.fdsr_last_error(None)
    assert torch.equal(out, want)
    assert load('encoder_up.layers.0.0.fn.fn.to_qkv.bias', np.zeros(576)) != 0             # bias=False: no such tensor
    assert load('sub_mean.weight', np.zeros((3, 3))) != 0                                  # the shape is [3][3][1][1]
    # 16x24: 6 low tokens, 96 high; the restatement takes its geometry from the input as well
    x3 = R.case_input('abi3', 1, 16, 24).cuda()
    out3 = torch.empty(1, 3, 64, 96, device='cuda')
    assert forward(x3, out3, 16, 24) == 0, lib.fdsr_last_error(None)
    r64 = R.transenet_forward(w, m.cfg, x3.cpu(), torch.float64)['out']
    e32 = float((R.transenet_forward(w, m.cfg, x3.cpu(), torch.float32)['out'].double() - r64).abs().max())
    err = float((out3.cpu().double() - r64).abs().max())
    print('abi 16x24: device error %.3e   e32 %.3e   ratio %.2f' % (err, e32, err / e32))
    assert err <= 4 * e32, (err, e32)


def test_smoke_small_configuration(nets):
    m = nets('small', 4, 128)
    y = m(torch.rand(2, 3, 32, 32, device='cuda'))
    assert tuple(y.shape) == (2, 3, 128, 128) and bool(torch.isfinite(y).all())


def test_command_line(nets, tmp_path, capsys):
    """Four synthetic 128x128 PNGs in two class folders, --crop-size 128: the written PNGs are to_u8(model(lr)) and the printed
    PSNR is the host metric on those files."""
    from PIL import Image
    from fastdiffsr_amd import metrics
    from fastdiffsr_amd.transenet import test as cli, to_u8
    rng = np.random.default_rng(3)
    hr_dir = tmp_path / 'hr'
    files = []
    for cls in ('a', 'b'):
        (hr_dir / cls).mkdir(parents=True)
        for i in range(2):
            yy, xx = np.mgrid[0:128, 0:128]
            img = np.stack([128 + 90 * np.sin(0.2 * xx + c + i) * np.cos(0.15 * yy + 2 * c) for c in range(3)], -1) + rng.normal(0, 6, (128, 128, 3))
            p = hr_dir / cls / ('im%d.png' % i)
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(p)
            files.append((cls, p))
    m = nets('small', 4, 128)
    ckpt = tmp_path / 'generator_param.pkl'
    torch.save(m.state_dict(), ckpt)
    out_dir = tmp_path / 'out'
    rc = cli.main(['--model', str(ckpt), '--hr', str(hr_dir), '--scale', '4', '-o', str(out_dir), '--batch', '2', '--crop-size', '128',
                   '--n-feats', str(R.SMALL['n_feats']), '--en-depth', str(R.SMALL['en_depth']), '--de-depth', str(R.SMALL['de_depth'])])
    assert rc in (0, None)
    printed = capsys.readouterr().out
    assert 'TransENet' in printed and 'SwinIR' not in printed and 'HAT' not in printed
    psnrs = []
    for cls, p in files:
        hr = np.asarray(Image.open(p).convert('RGB'))
        lr = np.asarray(Image.fromarray(hr).resize((32, 32), Image.BICUBIC))
        x = torch.from_numpy(lr.copy()).permute(2, 0, 1).float().div(255).unsqueeze(0).cuda()
        sr = m(x)
        assert tuple(sr.shape) == (1, 3, 128, 128)
        want = to_u8(sr)[0].cpu().numpy()
        got = np.asarray(Image.open(out_dir / cls / p.name))
        assert np.array_equal(got, want), p
        psnrs.append(metrics.calculate_psnr(got, hr))
    assert ('PSNR %.4f' % np.mean(psnrs)) in printed, printed
