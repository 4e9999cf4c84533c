"""The LPIPS plumbing of val.run under two ranks on a GPU-less box (gloo): a stand-in device side whose `lpips` returns a known
function of each image, sharded over the ranks and all-reduced with the other sums -- rank 0's bic_lpips / sr_lpips are the
full-set averages and its log lines carry them.  Without LPIPS the stand-in that has no `lpips` method still runs unchanged."""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_val_cli_gloo import HostOps, OracleDDPM, _config, _free_port


def _known(truth_u8):
    """per image: (bic, sr) = (1e-3 (1 + mean / 255), 2e-3 (1 + mean / 255)) of the HR image"""
    m = truth_u8.reshape(truth_u8.shape[0], -1).to(torch.float64).mean(1) / 255.0
    return 1e-3 * (1 + m), 2e-3 * (1 + m)


class LpipsHostOps(HostOps):
    def lpips(self, model, truth_u8, test_a_u8, test_b_u8):
        assert model == 'stand-in'
        b, s = _known(truth_u8)
        out = torch.zeros(2, truth_u8.shape[0], 6, dtype=torch.float64)
        out[0, :, 0], out[1, :, 0] = b, s
        return out


def _rank(rank, world, port, cpath, out_dir, cwd, q):
    from fastdiffsr_amd import val
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.parallel import init_process_group
    import torch.distributed as dist
    os.chdir(cwd)
    torch.set_num_threads(2)
    os.environ.update({'RANK': str(rank), 'LOCAL_RANK': str(rank), 'WORLD_SIZE': str(world), 'MASTER_ADDR': '127.0.0.1',
                       'MASTER_PORT': str(port)})
    os.environ.pop('FDSR_DIST_BACKEND', None)
    init_process_group()
    lines = []
    res = val.run(load_config(cpath, phase='val'), batch=2, results=out_dir, rank=rank, world=world, log=lines.append,
                  diffusion=OracleDDPM(), ops=LpipsHostOps(), workers=2, lpips='stand-in')
    dist.destroy_process_group()
    q.put((rank, ({k: v for k, v in res.items() if k not in ('result_path', 'host_seconds')}, lines)))


@pytest.mark.timeout(600)
def test_val_lpips_two_ranks_gloo(tmp_path):
    from PIL import Image
    from test_val_host import make_dataset
    from fastdiffsr_amd import val
    from fastdiffsr_amd.config import load_config
    root = make_dataset(str(tmp_path / 'data'), n=5, l=8, r=32, seed=9)
    cpath = str(tmp_path / 'cfg.json')
    with open(cpath, 'w') as f:
        json.dump(_config(root, 8, 32), f)
    hr = torch.from_numpy(np.stack([np.asarray(Image.open(os.path.join(root, 'hr_32', '%05d.png' % (i + 1)))) for i in range(5)]))
    eb, es = (float(x.mean()) for x in _known(hr))
    # one rank; the stand-in WITHOUT an lpips method runs as before when no LPIPS is asked for
    plain_lines = []
    plain = val.run(load_config(cpath, phase='val'), batch=2, results=str(tmp_path / 'p'), log=plain_lines.append,
                    diffusion=OracleDDPM(), ops=HostOps(), workers=2)
    assert not hasattr(HostOps, 'lpips') and 'bic_lpips' not in plain and 'lpips' not in ''.join(plain_lines)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, cpath, str(tmp_path / 'two'), str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=500) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    res0, lines0 = got[0]
    assert res0['images'] == 5
    assert abs(res0['bic_lpips'] - eb) <= 1e-15 and abs(res0['sr_lpips'] - es) <= 1e-15, (res0, eb, es)
    assert got[1][0]['bic_lpips'] == res0['bic_lpips'] and got[1][1] == []
    assert lines0[0] == plain_lines[0] + ', bic_lpips: {:.5e}'.format(res0['bic_lpips'])
    assert lines0[1] == plain_lines[1] + ', sr_lpips: {:.5e}'.format(res0['sr_lpips'])
    for k in ('bic_mse', 'bic_psnr', 'bic_ssim', 'bic_ergas', 'sr_mse', 'sr_psnr', 'sr_ssim', 'sr_ergas'):
        assert abs(res0[k] - plain[k]) <= 1e-12 * max(1.0, abs(plain[k])), k
