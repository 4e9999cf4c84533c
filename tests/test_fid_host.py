"""FID on the host, without a GPU: the network table (fid_restatement.py against metrics.FID_LAYERS and the issue's counts),
fid_state's key checks, the synthetic weights' activation scale, frechet_distance against closed / independent forms and its
two fall-back branches, and the CLI's folder listing and .npz statistics."""
import os

import numpy as np
import pytest
import torch

import fid_restatement as R


@pytest.fixture(scope='module')
def sd():
    from fastdiffsr_amd.synth import synth_inception_fid
    return synth_inception_fid(0)


@pytest.fixture(scope='module')
def ref(sd):
    return R.forward(sd, R.seeded_images(5, 1, 96, 120), torch.float32)


def test_restatement_sizes_params_and_macs(ref):
    from fastdiffsr_amd.metrics import FID_LAYERS, FID_MODULES
    convs = ref['convs']
    assert len(convs) == 94
    params = sum(co * ci * kh * kw + 2 * co for _, ci, co, kh, kw, *_ in convs)
    assert params == 21785568                      # + fc 2,049,000 + AuxLogits 3,326,696 = torchvision's 27,161,264
    macs = sum(ci * co * kh * kw * ho * wo for _, ci, co, kh, kw, _, _, ho, wo in convs)
    assert round(macs / 1e9, 3) == 5.711
    # the restatement and the library's table agree layer by layer (names, shapes, strides, paddings)
    assert [(n, ci, co, kh, kw, s, p) for n, ci, co, kh, kw, s, p, _, _ in convs] == \
        [(n, ci, co, kh, kw, s, (ph, pw)) for n, ci, co, kh, kw, s, ph, pw in FID_LAYERS]
    sides = [ref[k].shape[2] for k in range(18)]
    assert sides == [s for _, s, _ in FID_MODULES] and [ref[k].shape[1] for k in range(18)] == [c for _, _, c in FID_MODULES]
    assert [149, 147, 147, 73, 73, 71, 35, 35, 35, 35, 17, 17, 17, 17, 17, 8, 8, 8] == sides
    assert ref['input'].shape[-2:] == (299, 299) and ref['pool3'].shape == (1, 2048)


def test_synthetic_weights_keep_activations_order_one(ref):
    for k in range(18):
        rms = float(ref[k].pow(2).mean().sqrt())
        assert 0.05 <= rms <= 20, (k, rms)
    rms = float(ref['pool3'].pow(2).mean().sqrt())
    assert 0.05 <= rms <= 20


def test_fid_state_keys(sd):
    from fastdiffsr_amd.metrics import FID_TENSORS, fid_state
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    full['fc.weight'] = torch.zeros(1008, 2048)
    full['fc.bias'] = torch.zeros(1008)
    full['Mixed_5b.branch1x1.bn.num_batches_tracked'] = torch.tensor(0)
    out = fid_state(full)
    assert list(out) == list(FID_TENSORS) and len(out) == 470
    assert all(v.dtype == np.float32 for v in out.values())
    with pytest.raises(KeyError, match='AuxLogits.conv0.conv.weight'):
        fid_state(dict(full, **{'AuxLogits.conv0.conv.weight': torch.zeros(128, 768, 1, 1)}))
    missing = dict(full)
    del missing['Mixed_7c.branch_pool.bn.running_var']
    with pytest.raises(KeyError, match='Mixed_7c.branch_pool.bn.running_var'):
        fid_state(missing)
    bad = dict(full, **{'Mixed_6b.branch7x7_2.conv.weight': torch.zeros(128, 128, 7, 1)})
    with pytest.raises(ValueError, match='Mixed_6b.branch7x7_2.conv.weight'):
        fid_state(bad)


def _spd(rng, d, rank=None):
    a = rng.normal(size=(d, rank or 2 * d))
    return a @ a.T / a.shape[1] + 1e-3 * np.eye(d)


def test_frechet_distance_diagonal_closed_form():
    from fastdiffsr_amd.metrics import frechet_distance
    rng = np.random.default_rng(0)
    a, b = rng.uniform(0.1, 3, 16), rng.uniform(0.1, 3, 16)
    m1, m2 = rng.normal(size=16), rng.normal(size=16)
    want = float(np.sum((np.sqrt(a) - np.sqrt(b)) ** 2) + np.sum((m1 - m2) ** 2))
    got = frechet_distance(m1, np.diag(a), m2, np.diag(b))
    assert abs(got - want) <= 1e-12 * max(1.0, want)


def test_frechet_distance_full_rank_against_eigh_form():
    """tr sqrtm(s1 s2) = tr sqrt(sqrt(s1) s2 sqrt(s1)), computed with eigh only"""
    from fastdiffsr_amd.metrics import frechet_distance
    rng = np.random.default_rng(1)
    for d in (8, 64):
        s1, s2 = _spd(rng, d), _spd(rng, d)
        m1, m2 = rng.normal(size=d), rng.normal(size=d)
        w, v = np.linalg.eigh(s1)
        r1 = (v * np.sqrt(w)) @ v.T
        tr = float(np.sum(np.sqrt(np.clip(np.linalg.eigvalsh(r1 @ s2 @ r1), 0, None))))
        want = float((m1 - m2) @ (m1 - m2) + np.trace(s1) + np.trace(s2) - 2 * tr)
        got = frechet_distance(m1, s1, m2, s2)
        assert abs(got - want) <= 1e-9 * abs(want), (d, got, want)


def test_frechet_distance_offset_retry_and_imaginary_error(monkeypatch):
    import scipy.linalg
    from fastdiffsr_amd.metrics import frechet_distance
    rng = np.random.default_rng(2)
    s1, s2 = _spd(rng, 6), _spd(rng, 6)
    mu = np.zeros(6)
    real_sqrtm = scipy.linalg.sqrtm
    calls = []

    def nan_first(a, *args, **kw):
        calls.append(a.copy())
        if len(calls) == 1:
            return np.full_like(a, np.nan)
        return real_sqrtm(a, *args, **kw)
    monkeypatch.setattr(scipy.linalg, 'sqrtm', nan_first)
    got = frechet_distance(mu, s1, mu, s2)
    assert len(calls) == 2
    off = 1e-6 * np.eye(6)
    assert np.array_equal(calls[1], (s1 + off).dot(s2 + off))
    want = float(np.trace(s1) + np.trace(s2) - 2 * np.trace(real_sqrtm((s1 + off).dot(s2 + off)).real))
    assert abs(got - want) <= 1e-12 * abs(want)

    def imaginary(a, *args, **kw):
        return real_sqrtm(a).astype(np.complex128) + 1j * 0.01 * np.eye(a.shape[0])
    monkeypatch.setattr(scipy.linalg, 'sqrtm', imaginary)
    with pytest.raises(ValueError, match='imaginary'):
        frechet_distance(mu, s1, mu, s2)

    def tiny_imaginary(a, *args, **kw):
        return real_sqrtm(a).astype(np.complex128) + 1j * 1e-5 * np.eye(a.shape[0])
    monkeypatch.setattr(scipy.linalg, 'sqrtm', tiny_imaginary)
    want = float(np.trace(s1) + np.trace(s2) - 2 * np.trace(real_sqrtm(s1.dot(s2)).real))
    assert abs(frechet_distance(mu, s1, mu, s2) - want) <= 1e-12 * abs(want)     # below 1e-3: the real part is kept


def test_activation_statistics_is_fp64_numpy_cov():
    from fastdiffsr_amd.metrics import activation_statistics
    f = np.random.default_rng(3).normal(size=(20, 5)).astype(np.float32)
    mu, sigma = activation_statistics(torch.from_numpy(f))
    assert mu.dtype == np.float64 and sigma.shape == (5, 5)
    assert np.array_equal(mu, f.astype(np.float64).mean(0)) and np.array_equal(sigma, np.cov(f.astype(np.float64), rowvar=False))


def test_folder_listing_rules(tmp_path):
    from fastdiffsr_amd.fid import list_images
    names = ['b.png', 'a.PNG', '10_sr.tif', '2_sr.tif', 'c.jpeg', 'd.webp', 'e.txt', 'f.tiff', 'g.JPG', 'h.bmp', 'i.ppm', 'j.pgm',
             'k.jpg', 'noext']
    for n in names:
        (tmp_path / n).write_bytes(b'')
    (tmp_path / 'sub').mkdir()
    (tmp_path / 'sub' / 'z.png').write_bytes(b'')
    got = [os.path.basename(p) for p in list_images(str(tmp_path))]
    assert got == ['10_sr.tif', '2_sr.tif', 'b.png', 'c.jpeg', 'd.webp', 'f.tiff', 'h.bmp', 'i.ppm', 'j.pgm', 'k.jpg']


def test_npz_statistics_in_and_out(tmp_path):
    from fastdiffsr_amd import fid as cli
    rng = np.random.default_rng(4)
    mu, sigma = rng.normal(size=4), _spd(rng, 4)
    p = str(tmp_path / 's.npz')
    np.savez_compressed(p, mu=mu, sigma=sigma)
    m2, s2 = cli.path_statistics(None, p)
    assert np.array_equal(m2, mu) and np.array_equal(s2, sigma)
    with pytest.raises(FileNotFoundError):
        cli.path_statistics(None, str(tmp_path / 'missing'))
    # two .npz paths need no device: FID.py's line, the value of frechet_distance
    from fastdiffsr_amd.metrics import frechet_distance
    q = str(tmp_path / 't.npz')
    mu2, sigma2 = rng.normal(size=4), _spd(rng, 4)
    np.savez_compressed(q, mu=mu2, sigma=sigma2)
    assert cli.main([p, q]) == frechet_distance(mu, sigma, mu2, sigma2)
    out = str(tmp_path / 'copy.npz')
    assert cli.main([p, '--save-stats', out]) is None
    with np.load(out) as f:
        assert np.array_equal(f['mu'], mu) and np.array_equal(f['sigma'], sigma)
