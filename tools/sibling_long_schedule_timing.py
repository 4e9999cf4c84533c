"""Time of one image for the sibling denoisers at their own schedule lengths (SR3 / GDP T = 1000, TESR T = 2000) through
fdsr_sample_stepwise, at the sizes the reference's configs give them (tools/siblings_default_probe.py), 256 x 256, B = 1 and 16,
in f16x3 / f16 / bf16, eager vs the chunked graph, with the engine's own noise (rng = 'engine': no noise tensor).

Every step of the stepwise loop launches the same kernels with the same arguments, so the time of a step does not depend on T.
By default the tool runs `--steps` steps (a linear schedule of that length) after one warm-up call and reports the measured ms per
step and ms per image = ms per step x the sibling's own T, marked `projected`; `--steps 0` runs the full T instead (marked
`measured`).  Memory: torch_mib = what torch holds after the call (cond, out, the kept frames, the engine's workspace);
device_used_mib = the device's used memory (mem_get_info: also the engine's weights, its embedding table and step state).
With rng = 'torch' a caller adds the pre-drawn noise, (T + 1) x B x 3 x 256 x 256 floats (768 KiB per plane per image).

Usage (GPU box):  python tools/sibling_long_schedule_timing.py [--variants ddpm tesr gdp] [--batches 1 16] [--steps 25]
                   > profiles/sibling_long_schedule_timing.txt"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {   # reference configs (config/sr_{ddpm,tesr,gdp}_test_64_256.json via model/networks.py) and their own T
    'ddpm': dict(inner_channel=64, channel_mults=(1, 1, 2, 2, 4, 4), attn_res=(16,), T=1000),
    'tesr': dict(inner_channel=64, channel_mults=(1, 2, 4, 8, 8), attn_res=(16,), T=2000),
    'gdp': dict(inner_channel=128, channel_mults=(1, 2, 4, 8), attn_res=(32, 16, 8), T=1000),
}


def run(variant, B, steps, precs, size):
    from fastdiffsr_amd.arch import UNetConfig
    from fastdiffsr_amd.engine import Engine
    from fastdiffsr_amd.long_schedule import frame_every
    from fastdiffsr_amd.schedule import schedule_buffers, sampling_scalars
    from fastdiffsr_amd.synth import synth_state_dict
    c = CONFIGS[variant]
    T_own = c['T']
    T = steps or T_own
    cfg = UNetConfig(in_channel=6, out_channel=3, inner_channel=c['inner_channel'], norm_groups=32, channel_mults=c['channel_mults'],
                     attn_res=c['attn_res'], res_blocks=2, dropout=0.0, image_size=size, variant=variant)
    eng = Engine(cfg)
    eng.load_state_dict(synth_state_dict(cfg, 3))
    bufs, sp = schedule_buffers(dict(schedule='linear', n_timestep=T, linear_start=1e-4, linear_end=2e-2))
    eng.set_schedule(sampling_scalars(bufs, sp))
    cond = (torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    out = torch.empty_like(cond)
    every = frame_every(T_own)
    traj = torch.empty((eng.traj_slots(every),) + tuple(cond.shape), device='cuda')
    stream = torch.cuda.Stream()
    rows = []
    for prec in precs:
        eng.set_precision(prec)
        for graph in (False, True):
            with torch.cuda.stream(stream):
                eng.sample(cond, None, want_traj=True, graph=graph, out=out, traj=traj, stepwise=True, traj_every=every)   # warm-up / capture
                stream.synchronize()
                t0 = time.perf_counter()
                eng.sample(cond, None, want_traj=True, graph=graph, out=out, traj=traj, stepwise=True, traj_every=every)
                stream.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
            free, total = torch.cuda.mem_get_info()
            ms_step = dt / T
            row = dict(variant=variant, T=T_own, size=size, B=B, prec=prec, mode='graph' if graph else 'eager', steps_run=T,
                       ms_per_step=round(ms_step, 3), ms_per_image=round(ms_step * T_own / B, 1),
                       kind='measured' if T == T_own else 'projected',
                       torch_mib=round(torch.cuda.memory_allocated() / 2 ** 20, 1), device_used_mib=round((total - free) / 2 ** 20),
                       finite=bool(torch.isfinite(out).all().item()))
            print(json.dumps(row), flush=True)
            rows.append(row)
    del eng
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variants', nargs='+', default=['ddpm', 'tesr', 'gdp'])
    ap.add_argument('--batches', nargs='+', type=int, default=[1, 16])
    ap.add_argument('--precs', nargs='+', default=['f16x3', 'f16', 'bf16'])
    ap.add_argument('--steps', type=int, default=25, help='steps timed per call (0: the sibling\'s own T)')
    ap.add_argument('--size', type=int, default=256)
    a = ap.parse_args()
    print(f'# {torch.cuda.get_device_name(0)}; fdsr_sample_stepwise, engine rng, continous frames every 1 | (T // 10) steps')
    print('# python tools/sibling_long_schedule_timing.py ' + ' '.join(sys.argv[1:]) + f'  (effective: {vars(a)})')
    for v in a.variants:
        for B in a.batches:
            run(v, B, a.steps, a.precs, a.size)


if __name__ == '__main__':
    main()
