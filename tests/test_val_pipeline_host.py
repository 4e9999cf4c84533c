"""val.run's pipeline on a GPU-less box, one rank: the stand-in model and device side of test_val_cli_gloo.py around the
product's loop, finisher, reduction and report.  What a pass returns and writes (the `res` keys, the two log lines, the file
names) in its plain, infer, host_metrics and LPIPS + FID forms, that the averages do not depend on the batch size, and that a
failure on the sampling thread or on the finisher thread ends the pass with that error, its threads gone and the
interpreter's switch interval put back."""
import json
import os
import sys
import threading

import numpy as np
import pytest
import torch

from fastdiffsr_amd import metrics as M
from fastdiffsr_amd import val
from fastdiffsr_amd.config import load_config
from test_val_cli_gloo import HostOps, OracleDDPM, _config
from test_val_fid_gloo import FidHostOps, _known as _fid_known
from test_val_host import make_dataset

N = 5
COLUMNS = [side + '_' + f for side in ('bic', 'sr') for f in ('mse', 'psnr', 'ssim', 'ergas')]
RES_KEYS = {'images', 'sample_seconds_this_rank', 'result_path', 'host_seconds'} | set(COLUMNS)
HOST_SECONDS_KEYS = {'setup', 'stage', 'post', 'tail', 'total', 'workers'}


def _lpips_known(truth_u8):
    """per image: (bic, sr) = (1e-3 (1 + mean / 255), 2e-3 (1 + mean / 255)) of the HR image"""
    m = truth_u8.reshape(truth_u8.shape[0], -1).to(torch.float64).mean(1) / 255.0
    return 1e-3 * (1 + m), 2e-3 * (1 + m)


class LpipsFidOps(FidHostOps):
    def lpips(self, model, truth_u8, test_a_u8, test_b_u8):
        assert model == 'lpips stand-in'
        out = torch.zeros(2, truth_u8.shape[0], 6, dtype=torch.float64)
        out[0, :, 0], out[1, :, 0] = _lpips_known(truth_u8)
        return out


class LandFails(HostOps):
    """the second 'sr' landing raises: a failure on the sampling thread, inside the loop"""
    calls = 0

    def land(self, tag, slot, t):
        if tag == 'sr':
            self.calls += 1
            if self.calls == 2:
                raise RuntimeError('land failed')
        return super().land(tag, slot, t)


class _BadEvent:
    def synchronize(self):
        raise RuntimeError('event failed')


class MarkFails(HostOps):
    """the second batch's event raises when it is waited for: a failure on the finisher thread"""
    calls = 0

    def mark(self):
        self.calls += 1
        return _BadEvent() if self.calls == 2 else super().mark()


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    """The dataset, its config file, one stand-in model and the plain pass at batch 2 -- shared, and left unchanged."""
    from PIL import Image
    tmp = tmp_path_factory.mktemp('val_pipeline')
    root = make_dataset(str(tmp / 'data'), n=N, l=8, r=32)
    cpath = str(tmp / 'cfg.json')
    with open(cpath, 'w') as f:
        json.dump(_config(root, 8, 32), f)
    model = OracleDDPM()

    def run(name, ops=None, **kw):
        lines = []
        res = val.run(load_config(cpath, phase='val'), results=str(tmp / name), log=lines.append, diffusion=model,
                      ops=ops or HostOps(), workers=2, **kw)
        return res, lines, str(tmp / name)

    def load(folder, pattern):
        return [np.asarray(Image.open(os.path.join(folder, pattern % (i + 1)))) for i in range(N)]

    return dict(tmp=str(tmp), run=run, load=load, plain=run('plain', batch=2), hr=load(os.path.join(root, 'hr_32'), '%05d.png'),
                bic=load(os.path.join(root, 'sr_8_32'), '%05d.png'))


def _mean(values):
    """the pass's own average: a sum in index order, divided by the count"""
    s = 0.0
    for v in values:
        s += v
    return s / len(values)


def _host_rows(test, truth):
    return [[M.compare_mse(a, b), M.compare_psnr(a, b), M.compare_ssim(a, b), M.calculate_ergas(a, b, scale=4)] for a, b in zip(test, truth)]


def test_plain_pass_lines_keys_and_files(setup):
    res, lines, folder = setup['plain']
    assert sorted(os.listdir(folder)) == ['0_%d_sr.tif' % i for i in range(1, N + 1)]
    assert set(res) == RES_KEYS and set(res['host_seconds']) == HOST_SECONDS_KEYS
    assert res['images'] == N and res['result_path'] == folder
    sr = setup['load'](folder, '0_%d_sr.tif')
    want = []
    for side, test in (('bic', setup['bic']), ('sr', sr)):
        avg = [_mean(col) for col in zip(*_host_rows(test, setup['hr']))]
        want.append('<epoch:  0, iter:       0> ' + ', '.join('{}_{}: {:.5e}'.format(side, f, v) for f, v in zip(('mse', 'psnr', 'ssim', 'ergas'), avg)))
    assert lines == want


def test_averages_do_not_depend_on_the_batch(setup):
    plain = setup['plain'][0]
    for b in (1, 5):
        res, lines, _ = setup['run']('b%d' % b, batch=b)
        for k in ['images'] + COLUMNS:
            assert res[k] == plain[k], (b, k, res[k], plain[k])
        assert lines == setup['plain'][1]


def test_infer_writes_png_and_one_line(setup):
    res, lines, folder = setup['run']('infer', batch=2, infer=True)
    assert sorted(os.listdir(folder)) == ['0_%d_sr.png' % i for i in range(1, N + 1)]
    assert len(lines) == 1 and lines[0].startswith('inference: 5 images,') and lines[0].endswith('on this rank (batch 2)')
    assert res['images'] == N


def test_host_metrics_agree_with_the_sums_path(setup):
    plain = setup['plain'][0]
    res, lines, _ = setup['run']('host', batch=2, host_metrics=True)
    assert set(res) == RES_KEYS and len(lines) == 2
    for k in COLUMNS:
        assert abs(res[k] - plain[k]) < 1e-9, (k, res[k], plain[k])


def test_lpips_and_fid_columns(setup):
    plain, plain_lines, _ = setup['plain']
    res, lines, folder = setup['run']('lpfid', ops=LpipsFidOps(), batch=2, lpips='lpips stand-in', fid='stand-in')
    assert set(res) == RES_KEYS | {'bic_lpips', 'sr_lpips', 'bic_fid', 'sr_fid'}
    assert set(res['host_seconds']) == HOST_SECONDS_KEYS | {'fid_statistics'}
    for k in COLUMNS:
        assert res[k] == plain[k]
    lb, ls = _lpips_known(torch.from_numpy(np.stack(setup['hr'])))
    assert abs(res['bic_lpips'] - _mean(lb.tolist())) <= 1e-15 and abs(res['sr_lpips'] - _mean(ls.tolist())) <= 1e-15
    stats = {k: M.activation_statistics(_fid_known(torch.from_numpy(np.stack(v))).numpy())
             for k, v in (('hr', setup['hr']), ('bic', setup['bic']), ('sr', setup['load'](folder, '0_%d_sr.tif')))}
    assert res['bic_fid'] == M.frechet_distance(*stats['bic'], *stats['hr']) > 0
    assert res['sr_fid'] == M.frechet_distance(*stats['sr'], *stats['hr']) > 0
    assert lines[0] == plain_lines[0] + ', bic_lpips: {:.5e}, bic_fid: {:.5e}'.format(res['bic_lpips'], res['bic_fid'])
    assert lines[1] == plain_lines[1] + ', sr_lpips: {:.5e}, sr_fid: {:.5e}'.format(res['sr_lpips'], res['sr_fid'])


@pytest.mark.timeout(120)
def test_a_failure_in_the_loop_is_raised_and_cleaned_up(setup):
    threads, switch = threading.active_count(), sys.getswitchinterval()
    with pytest.raises(RuntimeError, match='land failed'):
        setup['run']('loop_fails', ops=LandFails(), batch=2)
    assert threading.active_count() == threads and sys.getswitchinterval() == switch


@pytest.mark.timeout(120)
def test_a_failure_in_the_finisher_is_raised_after_the_drain(setup):
    threads, switch = threading.active_count(), sys.getswitchinterval()
    with pytest.raises(RuntimeError, match='event failed'):
        setup['run']('finisher_fails', ops=MarkFails(), batch=2)
    # batches are (1, 2), (3, 4), (5): the loop went on past the failed one, and the drain waited for the writes
    assert sorted(os.listdir(os.path.join(setup['tmp'], 'finisher_fails'))) == ['0_1_sr.tif', '0_2_sr.tif', '0_5_sr.tif']
    assert threading.active_count() == threads and sys.getswitchinterval() == switch
