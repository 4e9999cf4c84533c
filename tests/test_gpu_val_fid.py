"""`val.run(..., fid=...)` / `python -m fastdiffsr_amd.val --fid-weights PATH` and the training loop's validation passes on the
GPU, synthetic Inception weights: bic_fid / sr_fid equal `python -m fastdiffsr_amd.fid` run on the written .tif files / the
bicubic folder against the HR folder (the same per-image features, in the same order), agree with the CPU restatement
(fid_restatement.py) within 1e-3 relative, and ride on the two log lines; without the flag the lines are those of a run
without the feature; a training run computes the HR / bicubic features once."""
import json
import os

import numpy as np
import pytest
import torch

import fid_restatement as R
from test_gpu_val_lpips import _config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from fastdiffsr_amd.synth import synth_inception_fid
    from test_val_host import make_dataset
    tmp = tmp_path_factory.mktemp('fid_val')
    root = make_dataset(str(tmp / 'data'), n=5, l=16, r=64, seed=23)
    cpath = tmp / 'cfg.json'
    cpath.write_text(json.dumps(_config(root)))
    sd = synth_inception_fid(0)
    wpath = str(tmp / 'pt_inception.pth')
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, wpath)
    return tmp, root, cpath, sd, wpath


def _folder(d):
    from PIL import Image
    from fastdiffsr_amd.fid import list_images
    return np.stack([np.asarray(Image.open(p).convert('RGB')) for p in list_images(d)])


def test_val_run_and_cli_with_fid(setup):
    from fastdiffsr_amd import fid as fid_cli
    from fastdiffsr_amd import val
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.metrics import FID, activation_statistics, frechet_distance
    tmp, root, cpath, sd, wpath = setup
    model = FID(wpath)
    lines0, lines = [], []
    torch.manual_seed(5)
    plain = val.run(load_config(str(cpath), phase='val'), batch=2, results=str(tmp / 'plain'), log=lines0.append)
    torch.manual_seed(5)
    res = val.run(load_config(str(cpath), phase='val'), batch=2, results=str(tmp / 'f'), log=lines.append, fid=model)
    assert 'bic_fid' not in plain and 'fid' not in ''.join(lines0)
    assert res['images'] == 5 and res['bic_fid'] > 0 and res['sr_fid'] > 0
    assert lines[0] == lines0[0] + ', bic_fid: {:.5e}'.format(res['bic_fid'])
    assert lines[1] == lines0[1] + ', sr_fid: {:.5e}'.format(res['sr_fid'])
    for k in ('bic_mse', 'bic_psnr', 'bic_ssim', 'bic_ergas', 'sr_mse', 'sr_psnr', 'sr_ssim', 'sr_ergas'):
        assert res[k] == plain[k], k
    # FID.py on the files the loop wrote (0_1_sr.tif .. 0_5_sr.tif: index order) and the dataset's folders
    hr_dir, inf_dir, sr_dir = os.path.join(root, 'hr_64'), os.path.join(root, 'sr_16_64'), str(tmp / 'f')
    sr_cli = fid_cli.main([sr_dir, hr_dir, '--weights', wpath, '--batch', '3'])
    bic_cli = fid_cli.main([inf_dir, hr_dir, '--weights', wpath])
    print('val sr_fid %.12g cli %.12g; val bic_fid %.12g cli %.12g' % (res['sr_fid'], sr_cli, res['bic_fid'], bic_cli))
    assert sr_cli == res['sr_fid'] and bic_cli == res['bic_fid']
    # the CPU restatement (fp32) of the same images: 1e-3 relative (test_gpu_fid.py measures the device-vs-restatement FID
    # agreement at 48 images to ~1e-6)
    hr, inf, sr = _folder(hr_dir), _folder(inf_dir), _folder(sr_dir)
    feats = {n: R.forward(sd, x, torch.float32, taps=False)['pool3'] for n, x in (('hr', hr), ('inf', inf), ('sr', sr))}
    s_hr = activation_statistics(feats['hr'])
    for name, key in (('inf', 'bic_fid'), ('sr', 'sr_fid')):
        want = frechet_distance(*activation_statistics(feats[name]), *s_hr)
        print('%s: val %.9g restatement %.9g' % (key, res[key], want))
        assert abs(res[key] - want) <= 1e-3 * want, (key, res[key], want)
    # batch size and the CLI flag: the same values
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        torch.manual_seed(5)
        r = val.main(['-c', str(cpath), '--batch', '3', '--no-save', '--fid-weights', wpath])
        assert r['bic_fid'] == res['bic_fid']
        r0 = val.main(['-c', str(cpath), '--batch', '3', '--no-save'])
        assert 'bic_fid' not in r0 and 'sr_fid' not in r0
    finally:
        os.chdir(cwd)


class _Counting:
    def __init__(self, model):
        self.model, self.calls = model, []

    def features_u8(self, x):
        self.calls.append(int(x.shape[0]))
        return self.model.features_u8(x)


def test_training_val_passes_compute_reference_features_once(setup):
    from fastdiffsr_amd import train
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.metrics import FID
    tmp, root, cpath, sd, wpath = setup
    cfg = json.loads(cpath.read_text())
    cfg['phase'] = 'train'
    cfg['datasets']['val']['data_len'] = 2
    cfg['train']['val_freq'] = 1
    tpath = tmp / 'train.json'
    tpath.write_text(json.dumps(cfg))
    counting = _Counting(FID(wpath))
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        lines = []
        torch.manual_seed(3)
        np.random.seed(3)
        train.run(load_config(str(tpath), phase='train'), log=lines.append, fid=counting)
    finally:
        os.chdir(cwd)
    val_lines = [m for m in lines if 'bic_mse' in m or 'sr_mse' in m]
    assert len(val_lines) == 4
    assert all(', bic_fid: ' in m for m in val_lines[0::2]) and all(', sr_fid: ' in m for m in val_lines[1::2])
    assert val_lines[0].split(', bic_fid: ')[1] == val_lines[2].split(', bic_fid: ')[1]
    # pass 1: HR + bicubic + SR of every image (val batch 1); pass 2: SR only
    n = len(counting.calls) // 2
    assert n >= 1 and counting.calls == [3] * n + [1] * n, counting.calls
