"""fdsr_lpips_u8 (csrc/fdsr_lpips.hip) on the GPU against the reference's own values (tests/golden/lpips_alex.npz) and the fp64
restatement of test_lpips_host.py, total and per layer (|d| <= 1e-5 |v| + 1e-9): 64 x 64, an off size, 256 x 256 and 512 x 512
(infer.py's size).  Identical images give exactly 0; an image's value does not depend on the batch or its position in it;
reruns are bitwise identical; test_b = NULL equals the two-test call; H < 32 and a short workspace are refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_lpips_host import golden, golden_pairs, heads, lpips_f64

pytestmark = pytest.mark.gpu


def _tol(got, ref):
    return np.all(np.abs(np.asarray(got) - np.asarray(ref)) <= 1e-5 * np.abs(ref) + 1e-9)


@pytest.fixture(scope='module')
def model():
    from fastdiffsr_amd.metrics import LPIPS
    from fastdiffsr_amd.synth import synth_alexnet_features
    g = golden()
    sd = synth_alexnet_features(int(g['seed']))
    lin = heads(g)
    return LPIPS(sd, lin, device='cuda'), sd, lin


def _dev(*imgs):
    return torch.from_numpy(np.stack(imgs)).cuda()


def _texture(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(xx / (5.0 + seed))[..., None] * np.cos(yy / 7.0)[..., None] + rng.normal(0, 14, (h, w, 3))
    return base.clip(0, 255).astype(np.uint8)


def test_golden_pairs_and_restatement(model):
    lp, sd, lin = model
    for name, (test, truth, ref, ref_layers) in golden_pairs().items():
        out = lp.lpips_u8(_dev(truth), _dev(test)).cpu().numpy()
        assert out.shape == (1, 1, 6)
        got = out[0, 0]
        tot, per = lpips_f64(sd, lin, test, truth)
        assert _tol(got[0], tot) and _tol(got[1:], per), (name, got, tot, per)
        assert abs(got[0] - ref) <= 1e-5 * abs(ref) + 1e-9, (name, got[0], ref)
        assert _tol(got[1:], ref_layers), (name, got[1:], ref_layers)


@pytest.mark.parametrize('hw', [(64, 64), (72, 104), (256, 256), (512, 512), (32, 40)])
def test_two_tests_against_restatement(model, hw):
    lp, sd, lin = model
    h, w = hw
    truth = [_texture(1, h, w), _texture(2, h, w)]
    a = [(t.astype(np.int32) + np.random.default_rng(3 + j).integers(-9, 10, t.shape)).clip(0, 255).astype(np.uint8)
         for j, t in enumerate(truth)]
    b = [_texture(5 + j, h, w) for j in range(2)]
    out = lp.lpips_u8(_dev(*truth), _dev(*a), _dev(*b)).cpu().numpy()
    assert out.shape == (2, 2, 6)
    for j in range(2):
        for t, test in enumerate((a[j], b[j])):
            tot, per = lpips_f64(sd, lin, test, truth[j])
            assert _tol(out[t, j, 0], tot) and _tol(out[t, j, 1:], per), (hw, t, j, out[t, j], tot, per)
            assert abs(out[t, j, 1:].sum() - out[t, j, 0]) <= 1e-12 * out[t, j, 0]


def test_identical_batch_position_rerun_and_null(model):
    lp = model[0]
    h = w = 96
    truth = np.stack([_texture(10 + i, h, w) for i in range(16)])
    a = np.stack([_texture(40 + i, h, w) for i in range(16)])
    b = truth.copy()
    b[3] = a[3]
    T, A, Bt = (torch.from_numpy(x).cuda() for x in (truth, a, b))
    full = lp.lpips_u8(T, A, Bt).cpu().numpy()
    again = lp.lpips_u8(T, A, Bt).cpu().numpy()
    assert np.array_equal(full, again)                           # reruns: bitwise
    assert (full[1, [i for i in range(16) if i != 3]] == 0.0).all()   # identical images: exactly 0, every layer
    assert np.array_equal(full[1, 3], full[0, 3])
    assert (full[0, :, 0] > 0).all()
    one = lp.lpips_u8(T, A).cpu().numpy()                        # test_b = NULL
    assert np.array_equal(one[0], full[0])
    for i in (0, 7, 15):                                         # alone at B = 1: bitwise, whatever the position
        solo = lp.lpips_u8(T[i:i + 1], A[i:i + 1], Bt[i:i + 1]).cpu().numpy()
        assert np.array_equal(solo[:, 0], full[:, i]), i
    perm = torch.tensor([15, 0, 7, 3, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14]).cuda()
    shuf = lp.lpips_u8(T[perm], A[perm], Bt[perm]).cpu().numpy()
    assert np.array_equal(shuf, full[:, perm.cpu().numpy()])


def test_refusals(model):
    from fastdiffsr_amd import _lib
    lp = model[0]
    small = torch.zeros(2, 24, 64, 3, dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.FdsrError) as e:
        lp.lpips_u8(small, small)
    assert e.value.code == -1
    img = torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device='cuda')
    ws = lp.workspace(2, 64, 64)
    out = torch.empty(2, 2, 6, dtype=torch.float64, device='cuda')
    lib = _lib.load()
    p = C.c_void_p(img.data_ptr())
    rc = lib.fdsr_lpips_u8(lp._h, p, p, p, 2, 64, 64, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), 1024,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -4                                              # FDSR_E_WORKSPACE
