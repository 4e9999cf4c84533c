"""The FID plumbing of val.run under two ranks on a GPU-less box (gloo): a stand-in device side whose `fid_features` returns a
known vector per image (a function of its pixels), sharded over the ranks; rank 0 gathers the features in index order, so its
bic_fid / sr_fid equal the single-rank values bitwise, at any batch size, and its log lines carry them."""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_val_cli_gloo import HostOps, OracleDDPM, _config, _free_port

D = 6


def _known(u8):
    """per image: D numbers from its pixels (channel means, channel stds / 64)"""
    x = u8.reshape(u8.shape[0], -1, 3).to(torch.float64)
    return torch.cat([x.mean(1) / 255, x.std(1) / 64], 1).to(torch.float32)


class FidHostOps(HostOps):
    def fid_features(self, model, imgs_u8):
        assert model == 'stand-in'
        return torch.cat([_known(t) for t in imgs_u8])


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
                  diffusion=OracleDDPM(), ops=FidHostOps(), workers=2, fid='stand-in')
    dist.destroy_process_group()
    q.put((rank, ({k: v for k, v in res.items() if k not in ('result_path', 'host_seconds')}, lines)))


@pytest.mark.timeout(600)
def test_val_fid_two_ranks_gloo(tmp_path):
    from fastdiffsr_amd import val
    from fastdiffsr_amd.config import load_config
    from test_val_host import make_dataset
    root = make_dataset(str(tmp_path / 'data'), n=5, l=8, r=32, seed=9)
    cpath = str(tmp_path / 'cfg.json')
    with open(cpath, 'w') as f:
        json.dump(_config(root, 8, 32), f)
    plain_lines = []
    plain = val.run(load_config(cpath, phase='val'), batch=2, results=str(tmp_path / 'p'), log=plain_lines.append,
                    diffusion=OracleDDPM(), ops=HostOps(), workers=2)
    assert not hasattr(HostOps, 'fid_features') and 'bic_fid' not in plain and 'fid' not in ''.join(plain_lines)
    single = {}
    for b in (1, 3):
        lines = []
        single[b] = (val.run(load_config(cpath, phase='val'), batch=b, results=str(tmp_path / ('s%d' % b)), log=lines.append,
                             diffusion=OracleDDPM(), ops=FidHostOps(), workers=2, fid='stand-in'), lines)
    s1 = single[1][0]
    assert s1['bic_fid'] > 0 and s1['sr_fid'] > 0
    assert single[3][0]['bic_fid'] == s1['bic_fid'] and single[3][0]['sr_fid'] == s1['sr_fid']
    # a cache kept between passes (the training loop): the second pass asks for SR features only, same values
    cache, asked = {}, []

    class Counting(FidHostOps):
        def fid_features(self, model, imgs_u8):
            asked.append(len(imgs_u8))
            return super().fid_features(model, imgs_u8)
    for _ in range(2):
        r = val.run(load_config(cpath, phase='val'), batch=2, results=str(tmp_path / 'c'), log=[].append, diffusion=OracleDDPM(),
                    ops=Counting(), workers=2, fid='stand-in', fid_cache=cache)
        assert r['bic_fid'] == s1['bic_fid'] and r['sr_fid'] == s1['sr_fid']
    assert asked == [3, 3, 3, 1, 1, 1]
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
    assert res0['bic_fid'] == s1['bic_fid'] and res0['sr_fid'] == s1['sr_fid'], (res0, s1)
    assert got[1][0]['sr_fid'] == res0['sr_fid'] and got[1][1] == []
    assert lines0[0] == plain_lines[0] + ', bic_fid: {:.5e}'.format(res0['bic_fid'])
    assert lines0[1] == plain_lines[1] + ', sr_fid: {:.5e}'.format(res0['sr_fid'])
