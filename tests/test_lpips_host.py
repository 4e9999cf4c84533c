"""LPIPS (AlexNet, v0.1 heads) on the host: an fp64 restatement of the reference's calculate_lpips (core/metrics.py:154-163),
written from its definition, held against tests/golden/lpips_alex.npz (the reference's own function on the synthetic backbone
and the real heads); the synthetic backbone's checksums; the [0,1]-input quirk; the state-dict mapping; the default paths.
No GPU.  The GPU tests import `lpips_f64` and `golden_pairs` from here."""
import os

import numpy as np
import pytest
import torch

from fastdiffsr_amd import metrics as M
from fastdiffsr_amd.synth import synth_alexnet_features

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips_alex.npz')
SHIFT = np.array([-.030, -.088, -.188], dtype=np.float32)
SCALE = np.array([.458, .448, .450], dtype=np.float32)


def golden():
    return np.load(GOLDEN)


def golden_pairs(g=None):
    """name -> (test uint8 HWC, truth uint8 HWC, lpips, per-layer[5])"""
    g = golden() if g is None else g
    return {str(n): (g['img/' + str(g[str(n) + '/test'])], g['img/' + str(g[str(n) + '/truth'])], float(g[str(n) + '/lpips']),
                     g[str(n) + '/layers']) for n in g['names']}


def heads(g=None):
    g = golden() if g is None else g
    return {'lin%d.model.1.weight' % k: g['lin%d' % k].reshape(1, -1, 1, 1).astype(np.float32) for k in range(5)}


def lpips_f64(backbone, lin, test, truth, normalize=False):
    """(LPIPS, [d_0..d_4]) of two uint8 HWC images, all in fp64 from the fp32 parameters: ToTensor (/255), optionally the
    `normalize=True` map to [-1,1] (which the reference does NOT use), ScalingLayer, AlexNet relu1..relu5 (conv 11/4/2,
    maxpool 3/2, conv 5/1/2, maxpool 3/2, conv 3/1/1 x3), unit-normalised channels (eps 1e-10), squared difference, 1x1 head,
    spatial mean, sum over the five layers."""
    F = torch.nn.functional
    d = torch.float64
    shift = torch.from_numpy(SHIFT).to(d).view(1, 3, 1, 1)
    scale = torch.from_numpy(SCALE).to(d).view(1, 3, 1, 1)

    def feats(img):
        x = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(d)[None] / 255.0
        if normalize:
            x = 2 * x - 1
        x = (x - shift) / scale
        w = {k: torch.from_numpy(np.asarray(v)).to(d) for k, v in backbone.items()}
        out = []
        x = F.relu(F.conv2d(x, w['features.0.weight'], w['features.0.bias'], stride=4, padding=2))
        out.append(x)
        x = F.relu(F.conv2d(F.max_pool2d(x, 3, 2), w['features.3.weight'], w['features.3.bias'], padding=2))
        out.append(x)
        x = F.relu(F.conv2d(F.max_pool2d(x, 3, 2), w['features.6.weight'], w['features.6.bias'], padding=1))
        out.append(x)
        x = F.relu(F.conv2d(x, w['features.8.weight'], w['features.8.bias'], padding=1))
        out.append(x)
        x = F.relu(F.conv2d(x, w['features.10.weight'], w['features.10.bias'], padding=1))
        out.append(x)
        return out

    f0, f1 = feats(test), feats(truth)
    per = []
    for k in range(5):
        a = f0[k] / (f0[k].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        b = f1[k] / (f1[k].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        wk = torch.from_numpy(np.asarray(lin['lin%d.model.1.weight' % k])).to(d).view(1, -1, 1, 1)
        per.append(float(((a - b) ** 2 * wk).sum(1).mean()))
    return float(sum(per)), np.array(per)


def test_synthetic_backbone_checksums():
    g = golden()
    sd = synth_alexnet_features(int(g['seed']))
    assert list(sd) == list(M.LPIPS_BACKBONE)
    for k, v in sd.items():
        assert v.dtype == np.float32 and v.shape == M.LPIPS_BACKBONE[k]
        x = v.astype(np.float64).ravel()
        got = np.array([x.sum(), np.abs(x).sum(), (x * np.linspace(-1.0, 1.0, x.size)).sum()])
        np.testing.assert_allclose(got, g['checksum/' + k], rtol=1e-12, atol=1e-12, err_msg=k)


def test_restatement_matches_reference_golden():
    g = golden()
    sd, lin = synth_alexnet_features(int(g['seed'])), heads(g)
    pairs = golden_pairs(g)
    assert {'p64_noise', 'p64_shift', 'p64_other', 'p72x104', 'p256_bic', 'p256_noisy'} <= set(pairs)
    for name, (test, truth, ref, ref_layers) in pairs.items():
        tot, per = lpips_f64(sd, lin, test, truth)
        assert abs(tot - ref) <= 1e-6 * abs(ref), (name, tot, ref)
        # the reference runs in fp32: its own rounding reaches 2.9e-6 of a deep layer's term (15 x 15 maps, K up to 3456) on
        # these near pairs, so the per-layer terms get 5e-6; the totals hold 1e-6 (7e-7 at most here)
        np.testing.assert_allclose(per, ref_layers, rtol=5e-6, atol=0, err_msg=name)
        assert abs(sum(per) - tot) <= 1e-12 * tot


def test_normalize_true_semantics_do_not_match():
    """The reference feeds the [0,1] ToTensor image straight in; `normalize=True` ([-1,1]) gives other values."""
    g = golden()
    sd, lin = synth_alexnet_features(int(g['seed'])), heads(g)
    for name, (test, truth, ref, _) in golden_pairs(g).items():
        if name.startswith('p64'):
            tot, _ = lpips_f64(sd, lin, test, truth, normalize=True)
            assert abs(tot - ref) > 1e-3 * abs(ref), (name, tot, ref)


def test_identical_images_give_zero():
    g = golden()
    sd, lin = synth_alexnet_features(int(g['seed'])), heads(g)
    img = golden_pairs(g)['p64_noise'][1]
    assert lpips_f64(sd, lin, img, img)[0] == 0.0


def test_state_mapping_from_saved_files(tmp_path):
    g = golden()
    sd = {k: torch.from_numpy(v) for k, v in synth_alexnet_features(1).items()}
    sd['classifier.1.weight'] = torch.zeros(4096, 9216)[:8, :8].clone()
    sd['classifier.1.bias'] = torch.zeros(8)
    lin = {k: torch.from_numpy(v) for k, v in heads(g).items()}
    bpath, lpath = str(tmp_path / 'alexnet.pth'), str(tmp_path / 'alex.pth')
    torch.save(sd, bpath)
    torch.save(lin, lpath)
    st = M.lpips_state(M._as_state_dict(bpath), M._as_state_dict(lpath))
    assert list(st) == list(M.LPIPS_BACKBONE) + list(M.LPIPS_LIN)        # classifier.* ignored, load order fixed
    for k, v in st.items():
        assert v.dtype == np.float32 and v.flags['C_CONTIGUOUS']
        ref = sd[k] if k in sd else lin[k]
        np.testing.assert_array_equal(v, ref.numpy())
    # wrong names and shapes are refused
    bad = dict(sd)
    bad['features.1.weight'] = torch.zeros(3)
    with pytest.raises(KeyError, match='features.1.weight'):
        M.lpips_state(bad, lin)
    bad = dict(sd)
    bad['features.3.weight'] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match='features.3.weight'):
        M.lpips_state(bad, lin)
    bad = dict(lin)
    del bad['lin4.model.1.weight']
    with pytest.raises(KeyError, match='lin4'):
        M.lpips_state(sd, bad)
    bad = dict(lin)
    bad['lin2.model.1.weight'] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match='lin2'):
        M.lpips_state(sd, bad)
    with pytest.raises(KeyError):                 # the heads file has no classifier exemption
        M.lpips_state(sd, dict(lin, **{'classifier.1.weight': torch.zeros(2)}))


def test_default_paths_name_the_missing_file(tmp_path, monkeypatch):
    monkeypatch.setenv('TORCH_HOME', str(tmp_path / 'th'))
    with pytest.raises(FileNotFoundError, match='alexnet-owt-7be5be79.pth') as e:
        M.LPIPS.default_paths()
    assert str(tmp_path / 'th' / 'hub' / 'checkpoints') in str(e.value)
    # the backbone present, the lpips package (with its weights) absent
    ck = tmp_path / 'th' / 'hub' / 'checkpoints'
    ck.mkdir(parents=True)
    (ck / 'alexnet-owt-7be5be79.pth').write_bytes(b'x')
    import importlib.util
    monkeypatch.setattr(importlib.util, 'find_spec', lambda name, *a: None)
    with pytest.raises(FileNotFoundError, match='v0.1/alex.pth'):
        M.LPIPS.default_paths()
    # a package found by find_spec (never imported) that ships the heads
    pkg = tmp_path / 'site' / 'lpips'
    (pkg / 'weights' / 'v0.1').mkdir(parents=True)
    (pkg / 'weights' / 'v0.1' / 'alex.pth').write_bytes(b'x')

    class Spec:
        submodule_search_locations = [str(pkg)]
    monkeypatch.setattr(importlib.util, 'find_spec', lambda name, *a: Spec() if name == 'lpips' else None)
    assert M.LPIPS.default_paths() == (str(ck / 'alexnet-owt-7be5be79.pth'), str(pkg / 'weights' / 'v0.1' / 'alex.pth'))
