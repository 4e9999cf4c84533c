"""`val.run(..., lpips=...)` / `python -m fastdiffsr_amd.val --lpips-backbone A --lpips-lin B` and the training loop's validation
pass on the GPU: bic_lpips / sr_lpips equal the fp64 restatement (test_lpips_host.py) averaged over the images the loop wrote and
the HR files; the log lines carry them; the four other averages are bitwise those of a run without LPIPS; batch 1 and 3 agree."""
import json
import os

import numpy as np
import pytest
import torch

from test_lpips_host import golden, heads, lpips_f64

pytestmark = pytest.mark.gpu


def _config(root):
    sched = dict(schedule='linear_cosine', n_timestep=20, linear_start=1e-6, linear_end=1e-2)
    return {
        "name": "sr_fastdiffsr_lpips", "phase": "val", "gpu_ids": [0],
        "path": {"log": "logs", "tb_logger": "tb_logger", "results": "results", "checkpoint": "checkpoint", "resume_state": None},
        "datasets": {"train": {"name": "t", "mode": "HR", "dataroot": root, "datatype": "img", "l_resolution": 16,
                               "r_resolution": 64, "batch_size": 2, "num_workers": 0, "use_shuffle": True, "data_len": -1},
                     "val": {"name": "v", "mode": "LRHR", "dataroot": root, "datatype": "img", "l_resolution": 16,
                             "r_resolution": 64, "data_len": -1}},
        "model": {"which_model_G": "fastdiffsr", "finetune_norm": False,
                  "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": 32, "channel_multiplier": [1, 2, 2],
                           "attn_res": [16], "res_blocks": 1, "dropout": 0.2},
                  "beta_schedule": {"train": dict(sched), "val": dict(sched)},
                  "diffusion": {"image_size": 64, "channels": 3, "conditional": True}},
        "train": {"n_iter": 2, "val_freq": 2, "save_checkpoint_freq": 100, "print_freq": 1,
                  "optimizer": {"type": "adam", "lr": 1e-4},
                  "ema_scheduler": {"step_start_ema": 5000, "update_ema_every": 1, "ema_decay": 0.9999}},
        "wandb": {"project": "x"}}


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from fastdiffsr_amd.synth import synth_alexnet_features
    from test_val_host import make_dataset
    tmp = tmp_path_factory.mktemp('lpips_val')
    root = make_dataset(str(tmp / 'data'), n=5, l=16, r=64, seed=21)
    cpath = tmp / 'cfg.json'
    cpath.write_text(json.dumps(_config(root)))
    g = golden()
    sd = synth_alexnet_features(int(g['seed']))
    lin = heads(g)
    bpath, lpath = str(tmp / 'alexnet.pth'), str(tmp / 'alex.pth')
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, bpath)
    torch.save({k: torch.from_numpy(v) for k, v in lin.items()}, lpath)
    return tmp, root, cpath, sd, lin, bpath, lpath


def _expected(root, outdir, sd, lin, n):
    from PIL import Image
    bic, sr = [], []
    for i in range(n):
        hr = np.asarray(Image.open(os.path.join(root, 'hr_64', '%05d.png' % (i + 1))))
        inf = np.asarray(Image.open(os.path.join(root, 'sr_16_64', '%05d.png' % (i + 1))))
        out = np.asarray(Image.open(os.path.join(outdir, '0_%d_sr.tif' % (i + 1))))
        bic.append(lpips_f64(sd, lin, inf, hr)[0])
        sr.append(lpips_f64(sd, lin, out, hr)[0])
    return np.mean(bic), np.mean(sr)


def test_val_run_and_cli_with_lpips(setup):
    from fastdiffsr_amd import val
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.metrics import LPIPS
    tmp, root, cpath, sd, lin, bpath, lpath = setup
    lp = LPIPS(bpath, lpath)
    runs = {}
    for tag, batch, use in (('plain', 2, None), ('b1', 1, lp), ('b3', 3, lp)):
        lines = []
        torch.manual_seed(5)
        res = val.run(load_config(str(cpath), phase='val'), batch=batch, results=str(tmp / tag), log=lines.append, lpips=use)
        runs[tag] = (res, lines)
    plain, lines0 = runs['plain']
    assert 'bic_lpips' not in plain and 'lpips' not in ''.join(lines0)
    for tag in ('b1', 'b3'):
        res, lines = runs[tag]
        assert res['images'] == 5
        assert lines[0].endswith(', bic_lpips: {:.5e}'.format(res['bic_lpips'])) and ', bic_ergas: ' in lines[0]
        assert lines[1].endswith(', sr_lpips: {:.5e}'.format(res['sr_lpips']))
        assert lines[0].split(', bic_lpips')[0] == lines0[0]
        for k in ('bic_mse', 'bic_psnr', 'bic_ssim', 'bic_ergas'):
            assert res[k] == plain[k], k                          # the bicubic metrics are batch-independent: bitwise
        eb, es = _expected(root, str(tmp / tag), sd, lin, 5)
        assert abs(res['bic_lpips'] - eb) <= 1e-5 * eb, (res['bic_lpips'], eb)
        assert abs(res['sr_lpips'] - es) <= 1e-5 * es, (res['sr_lpips'], es)
    # same batch, same noise: the four SR averages are bitwise those of the run without LPIPS
    torch.manual_seed(5)
    res2 = val.run(load_config(str(cpath), phase='val'), batch=2, results=str(tmp / 'b2'), log=[].append, lpips=lp)
    for k in ('sr_mse', 'sr_psnr', 'sr_ssim', 'sr_ergas', 'bic_mse', 'bic_psnr', 'bic_ssim', 'bic_ergas'):
        assert res2[k] == plain[k], k
    # batch 1 vs batch 3: the bicubic LPIPS (same inputs) agree bitwise-in-average up to summation order
    assert abs(runs['b1'][0]['bic_lpips'] - runs['b3'][0]['bic_lpips']) <= 1e-15
    # host metrics: LPIPS still from the device
    torch.manual_seed(5)
    res3 = val.run(load_config(str(cpath), phase='val'), batch=2, results=str(tmp / 'h'), log=[].append, lpips=lp, host_metrics=True)
    assert res3['bic_lpips'] == res2['bic_lpips'] and res3['sr_lpips'] == res2['sr_lpips']
    # the CLI
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        r = val.main(['-c', str(cpath), '--batch', '3', '--no-save', '--lpips-backbone', bpath, '--lpips-lin', lpath])
        assert r['bic_lpips'] == runs['b3'][0]['bic_lpips']
        r0 = val.main(['-c', str(cpath), '--batch', '3', '--no-save'])
        assert 'bic_lpips' not in r0 and 'sr_lpips' not in r0
    finally:
        os.chdir(cwd)


def test_training_val_pass_logs_lpips(setup):
    from fastdiffsr_amd import train
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.metrics import LPIPS
    tmp, root, cpath, sd, lin, bpath, lpath = setup
    cfg = json.loads(cpath.read_text())
    cfg['phase'] = 'train'
    cfg['datasets']['val']['data_len'] = 2
    tpath = tmp / 'train.json'
    tpath.write_text(json.dumps(cfg))
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        lines = []
        torch.manual_seed(3)
        np.random.seed(3)
        train.run(load_config(str(tpath), phase='train'), log=lines.append, lpips=LPIPS(bpath, lpath))
    finally:
        os.chdir(cwd)
    val_lines = [m for m in lines if 'bic_mse' in m or 'sr_mse' in m]
    assert len(val_lines) == 2
    assert ', bic_lpips: ' in val_lines[0] and ', sr_lpips: ' in val_lines[1]
