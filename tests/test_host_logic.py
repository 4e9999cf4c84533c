"""Host-side logic that needs no GPU: schedule algebra, schema via the C ABI, plan and
workspace errors, config reader, sharding."""
import os

import numpy as np
import pytest
import torch

from fastdiffsr_amd import _lib
from fastdiffsr_amd.arch import (UNetConfig, FASTDIFFSR_UNET, FASTDIFFSR_SCHEDULE_VAL, SCHEDULE_BUFFERS, build_layers,
                                 param_schema, dead_keys)
from fastdiffsr_amd.config import parse_json_with_comments, dict_to_nonedict
from fastdiffsr_amd.engine import Engine
from fastdiffsr_amd.parallel import shard_range, flatten_state_dict, unflatten_state_dict
from fastdiffsr_amd.schedule import make_beta_schedule, schedule_buffers, sampling_scalars
from fastdiffsr_amd.synth import synth_state_dict, state_dict_sha256
from oracle import fdsr_oracle as O


def test_product_schedule_equals_oracle_and_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'schedule.npz'))
    for key in [k for k in g.files if k.startswith('betas/')]:
        _, name, T = key.split('/')
        ls, le = (1e-6, 1e-2) if name in ('linear_cosine', 'linear') else (1e-4, 2e-2)
        np.testing.assert_array_equal(make_beta_schedule(name, int(T), ls, le), g[key])
        np.testing.assert_array_equal(make_beta_schedule(name, int(T), ls, le), O.make_beta_schedule(name, int(T), ls, le))
    for T in (20, 10):
        opt = dict(schedule='linear_cosine', n_timestep=T, linear_start=1e-6, linear_end=1e-2)
        bufs, sp = schedule_buffers(opt)
        assert list(bufs.keys()) == list(SCHEDULE_BUFFERS)          # registration order = state_dict order
        for k in SCHEDULE_BUFFERS:
            np.testing.assert_array_equal(bufs[k], g[f'buf/{T}/{k}'])
        np.testing.assert_array_equal(sp, g[f'buf/{T}/sqrt_alphas_cumprod_prev_f64'])
    with pytest.raises(NotImplementedError):
        make_beta_schedule('bogus', 5)


def test_sampling_scalars_match_reference_formation():
    bufs, sp = schedule_buffers(FASTDIFFSR_SCHEDULE_VAL)
    sc = sampling_scalars(bufs, sp)
    assert all(v.dtype == np.float32 and v.shape == (20,) for v in sc.values())
    assert sc['noise_level'][19] == np.float32(sp[20]) and abs(sc['noise_level'][19] - 6.634494e-07) < 1e-12
    # sigma = exp(0.5*logvar) in fp32 (diffusion.py:190), NOT sqrt(posterior_variance)
    np.testing.assert_array_equal(sc['sigma'], (0.5 * torch.from_numpy(bufs['posterior_log_variance_clipped'])).exp().numpy())
    assert abs(sc['sigma'][0] - 1e-10) < 1e-16 and sc['coef1'][0] == 1.0 and sc['coef2'][0] == 0.0


@pytest.mark.parametrize('kw', [FASTDIFFSR_UNET,
                                dict(in_channel=6, out_channel=3, inner_channel=32, channel_mults=(1, 2, 4, 4), res_blocks=2),
                                dict(in_channel=6, out_channel=3, inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=1),
                                dict(in_channel=3, out_channel=3, inner_channel=32, channel_mults=(1, 2), res_blocks=3)])
def test_native_plan_schema_matches_python_schema(kw):
    """csrc/fdsr_plan.cpp (build_plan, called by fdsr_create) derives the same checkpoint schema as arch.param_schema (C ABI, no GPU)."""
    cfg = UNetConfig(**kw)
    eng = Engine(cfg)
    py = param_schema(cfg)
    native = eng.schema()
    assert [k for k, _, _ in native] == list(py.keys())
    assert all(tuple(py[k]) == s for k, s, _ in native)
    assert sorted(k for k, _, live in native if not live) == sorted(dead_keys(cfg))
    assert not eng.weights_complete


def test_plan_fingerprints_are_the_parents(golden_dir):
    """The static plan of csrc/fdsr_plan.cpp, seen through the C ABI, is the one tests/golden/plan_fingerprints.json recorded from
    the library of the commit before the plan builders moved there (tools/make_plan_fingerprints.py): per config the sha256 of the
    (key, shape, live) schema, workspace_bytes at three shapes plain and in debug mode, train_workspace_bytes at two (it plans
    without a device, so it is part of the record; training mode on where the config has dropout).  These follow tensor count and
    order, widths, levels, liveness, need_part and the GroupNorm / dropout slot counts; a swapped gamma / beta index is for the
    GPU suite to see."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location(
        'make_plan_fingerprints', os.path.join(os.path.dirname(__file__), '..', 'tools', 'make_plan_fingerprints.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    doc = json.load(open(os.path.join(golden_dir, 'plan_fingerprints.json')))
    assert [tuple(s) for s in doc['shapes']] == tool.SHAPES
    now = {name: {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()} for name, kw in tool.configs().items()}
    assert {name: rec['config'] for name, rec in doc['configs'].items()} == now       # the file covers the tool's configs, as they are
    for name, rec in doc['configs'].items():
        assert tool.fingerprint(rec['config']) == rec['fingerprint'], name


def test_fastdiffsr_counts():
    cfg = UNetConfig(**FASTDIFFSR_UNET)
    sch = param_schema(cfg)
    assert len(sch) == 317
    assert sum(int(np.prod(s)) for s in sch.values()) == 23802277
    dead = sum(int(np.prod(sch[k])) for k in dead_keys(cfg))
    assert dead == 892864
    kinds = [L.kind for L in build_layers(cfg)]
    assert kinds.count('res') == 22 and kinds.count('down') == 3 and kinds.count('up') == 3


def test_plan_rejects_bad_configs_and_shapes():
    with pytest.raises(_lib.FdsrError):
        Engine(UNetConfig(in_channel=6, out_channel=3, inner_channel=48, channel_mults=(1, 2)))     # 48 % 32 != 0
    with pytest.raises(_lib.FdsrError):
        Engine(UNetConfig(in_channel=9, out_channel=3, inner_channel=32, channel_mults=(1, 2)))
    eng = Engine(UNetConfig(**FASTDIFFSR_UNET))
    for bad in [(0, 64, 64), (1, 60, 64), (1, 64, 4)]:
        with pytest.raises(_lib.FdsrError):
            eng.workspace_bytes(*bad)
    a, b = eng.workspace_bytes(1, 64, 64), eng.workspace_bytes(4, 64, 64)
    assert 0 < a < b <= 4 * a + 4096
    # liveness reuse keeps the B=16 256x256 workspace near 2 GiB (every-layer-distinct would be ~8 GiB)
    assert eng.workspace_bytes(16, 256, 256) < 3 * 2 ** 30
    eng.set_debug(True)
    assert eng.workspace_bytes(1, 64, 64) > a


def test_synth_weights_are_pinned():
    cfg = UNetConfig(**FASTDIFFSR_UNET)
    sd = synth_state_dict(cfg, 0)
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'unet_full.npz'))
    assert state_dict_sha256(sd) == str(g['weights_sha256'])
    flat = flatten_state_dict(sd, cfg)
    back = unflatten_state_dict(flat, cfg)
    assert all(np.array_equal(back[k], sd[k]) for k in sd)


def test_config_reader():
    txt = '{\n "name": "x", // comment\n "model": {"which_model_G": "fastdiffsr", // c2\n "unet": {"inner_channel": 64}}\n}'
    opt = dict_to_nonedict(parse_json_with_comments(txt))
    assert opt['model']['which_model_G'] == 'fastdiffsr' and opt['model']['unet']['inner_channel'] == 64
    assert opt['missing'] is None and opt['model']['nope'] is None


def test_shard_range():
    for total, world in [(512, 8), (16, 3), (5, 8), (256, 8)]:
        spans = [shard_range(total, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
        sizes = [hi - lo for lo, hi in spans]
        assert max(sizes) - min(sizes) <= 1


def test_facade_state_dict_roundtrip_cpu():
    from fastdiffsr_amd import diffusion, unet
    net = unet.UNet(**{**FASTDIFFSR_UNET, 'channel_mults': [1, 2, 4, 4]})
    G = diffusion.GaussianDiffusion(net, image_size=256, channels=3, loss_type='l1', conditional=True, schedule_opt=None)
    G.set_loss('cpu')
    G.set_new_noise_schedule(FASTDIFFSR_SCHEDULE_VAL, 'cpu')
    sd = G.state_dict()
    assert len(sd) == 329 and list(sd.keys())[:12] == list(SCHEDULE_BUFFERS)   # own buffers first, as in the reference
    ck = {('denoise_fn.' + k): torch.from_numpy(v) for k, v in synth_state_dict(net.cfg, 0).items()}
    ck.update({k: sd[k] for k in SCHEDULE_BUFFERS})
    G.load_state_dict(ck, strict=True)
    assert torch.equal(G.state_dict()['denoise_fn.downs.0.weight'], ck['denoise_fn.downs.0.weight'])
    with pytest.raises(RuntimeError):
        G.load_state_dict({k: v for k, v in ck.items() if 'mid.0.conv' not in k}, strict=True)   # dead keys are required
    with pytest.raises((RuntimeError, _lib.FdsrError)):
        G.super_resolution(torch.zeros(1, 3, 32, 32))            # CPU tensor / no GPU: fails loudly, no fallback
    with pytest.raises(NotImplementedError):
        G.sample(1)


def test_config_reader_matches_reference_parser(golden_dir):
    """load_config vs the reference's own core.logger.parse on its fastdiffsr/ddpm configs
    (tests/golden/configs.json, made by oracle/make_goldens.py).  The config files it parsed are stored
    verbatim, comments included, under tests/golden/configs/."""
    import json
    import os
    from fastdiffsr_amd.config import load_config
    from fastdiffsr_amd.arch import SR3_UNET
    with open(os.path.join(golden_dir, 'configs.json')) as f:
        gold = json.load(f)
    assert len(gold) == 11
    # the constants the engine is benchmarked with ARE the reference's val config
    m = gold['sr_fastdiffsr_test_64_256.json|val|None|0']['model']
    u = m['unet']
    assert m['which_model_G'] == 'fastdiffsr'
    assert (u['in_channel'], u['out_channel'], u['inner_channel'], u['res_blocks'], u['dropout']) == (
        FASTDIFFSR_UNET['in_channel'], FASTDIFFSR_UNET['out_channel'], FASTDIFFSR_UNET['inner_channel'],
        FASTDIFFSR_UNET['res_blocks'], FASTDIFFSR_UNET['dropout'])
    assert tuple(u['channel_multiplier']) == tuple(FASTDIFFSR_UNET['channel_mults'])
    assert m['beta_schedule']['val'] == dict(FASTDIFFSR_SCHEDULE_VAL)
    u3 = gold['sr_ddpm_test_64_256.json|val|None|0']['model']['unet']
    assert tuple(u3['channel_multiplier']) == tuple(SR3_UNET['channel_mults']) and u3['inner_channel'] == SR3_UNET['inner_channel']
    cfg_dir = os.path.join(golden_dir, 'configs')
    assert sorted(os.listdir(cfg_dir)) == sorted({key.split('|')[0] for key in gold})
    for key, want in gold.items():
        name, phase, gpu_ids, debug = key.split('|')
        got = load_config(os.path.join(cfg_dir, name), phase=phase, gpu_ids=None if gpu_ids == 'None' else gpu_ids,
                          debug=bool(int(debug)))
        got = json.loads(json.dumps(got))
        got.pop('path', None)
        assert got == want, key


def test_parameter_count_matches_reference():
    """print_network reports 23,802,277 parameters = '22.700 M' (the reference divides by 1024**2, model.py:121;
    SURVEY section 6): the facade registers exactly the reference's parameters, dead ones included."""
    from fastdiffsr_amd import diffusion, unet
    net = unet.UNet(**{**FASTDIFFSR_UNET, 'channel_mults': [1, 2, 4, 4]})
    G = diffusion.GaussianDiffusion(net, image_size=256, channels=3, loss_type='l1', conditional=True, schedule_opt=None)
    n = sum(p.numel() for p in G.parameters())
    assert n == 23802277 and '%.3f' % (n / (1024 * 1024)) == '22.700'


def test_init_weights_orthogonal_matches_reference(golden_dir):
    """define_G in the train phase runs init_weights(netG, 'orthogonal') (networks.py:113-115): same tensors as the
    reference's own call under the same torch seed (same RNG consumption order over the schema)."""
    import os
    import torch
    from fastdiffsr_amd import networks
    from fastdiffsr_amd.unet import UNet
    from fastdiffsr_amd.diffusion import GaussianDiffusion
    g = np.load(os.path.join(golden_dir, 'init_weights.npz'))
    torch.manual_seed(int(g['seed']))
    net = UNet(in_channel=6, out_channel=3, norm_groups=32, inner_channel=32, channel_mults=(1, 2, 4, 4), attn_res=(16,),
               res_blocks=2, dropout=0.2, image_size=32)
    G = GaussianDiffusion(net, image_size=32, channels=3, loss_type='l1', conditional=True)
    networks.init_weights(G, init_type='orthogonal')
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['keys']]
    for (k, v), (s1, s2) in zip(sd.items(), g['stats']):
        v64 = v.double()
        assert abs(v64.sum().item() - s1) <= 1e-9 + 1e-12 * abs(s1), k
        assert abs((v64 ** 2).sum().item() - s2) <= 1e-9 + 1e-12 * abs(s2), k
    for k in ('downs.0.weight', 'mid.0.ca.fc2.weight', 'ups.4.res_block.noise_func.noise_func.0.weight'):
        assert np.array_equal(sd[k].numpy(), g['full/' + k]), k


def test_host_threads_follow_the_ranks_on_the_host(monkeypatch):
    """Loader / writer pools are sized from the cores the job may really use divided by the ranks on the host (verdict r5 #5:
    eight ranks on a 16-core lease must not start 8 x 8 loader threads)."""
    from fastdiffsr_amd import parallel, train
    assert parallel.host_threads_per_rank(cores=16, ranks=8) == 2          # floor
    assert parallel.host_threads_per_rank(cores=16, ranks=1) == 8          # cap
    assert parallel.host_threads_per_rank(cores=64, ranks=8) == 7          # share minus the rank's own sampling thread
    assert parallel.host_threads_per_rank(cap=16, cores=192, ranks=8) == 16
    monkeypatch.setenv('LOCAL_WORLD_SIZE', '8')
    monkeypatch.setattr(parallel, 'host_cores', lambda: 16)
    assert parallel.local_world_size() == 8
    assert parallel.host_threads_per_rank() == 2
    assert train.loader_workers(8) == 2 and train.loader_workers(None) == 2
    monkeypatch.setenv('LOCAL_WORLD_SIZE', '1')
    monkeypatch.setattr(parallel, 'host_cores', lambda: 32)
    assert train.loader_workers(8) == 8 and train.loader_workers(0) == 16 and train.loader_workers(64) == 16
    monkeypatch.delenv('LOCAL_WORLD_SIZE')
    monkeypatch.setenv('WORLD_SIZE', '4')
    assert parallel.local_world_size() == 4
    monkeypatch.undo()
    n = parallel.host_cores()
    assert 1 <= n <= (__import__('os').cpu_count() or 1)
