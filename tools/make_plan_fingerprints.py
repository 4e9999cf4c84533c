"""Write tests/golden/plan_fingerprints.json: what the static plan (csrc/fdsr_plan.cpp) of a set of configs looks like from outside
the library, for tests/test_host_logic.py::test_plan_fingerprints_are_the_parents.  No GPU: the library plans without a device.

    FDSR_LIB=<library built from the commit whose plans are the reference> python tools/make_plan_fingerprints.py

Per config: sha256 over the (key, shape, live) list of Engine.schema(); workspace_bytes at SHAPES, plain and under set_debug(True);
train_workspace_bytes at the first two of SHAPES, in training mode where the config has dropout.  These depend on tensor count and
order, channel widths, levels, liveness, need_part and the GroupNorm / dropout slot counts.  Regenerate only for a change that is
meant to alter the plan, and from a library whose GPU suite is green."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_UNET, SR3_UNET, TESR_UNET, GDP_UNET     # noqa: E402
from fastdiffsr_amd.engine import Engine     # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'plan_fingerprints.json')
SHAPES = [(1, 32, 32), (2, 64, 64), (4, 64, 96)]     # every config below accepts them
N_TRAIN_SHAPES = 2


def configs():
    """name -> UNetConfig keywords: the flagship configs of tests/test_host_logic.py and tests/test_gpu_parity.py (the second with
    dropout), the val configs, and the small SR3 / TESR / GDP configs of tests/test_gpu_{sr3,tesr,gdp}.py with an attention
    resolution that is hit and one that is not, at one and two residual blocks per level."""
    out = {
        'flagship': FASTDIFFSR_UNET,
        'flagship_32_1244_rb2': dict(in_channel=6, out_channel=3, inner_channel=32, channel_mults=(1, 2, 4, 4), res_blocks=2),
        'flagship_64_12488_rb1': dict(in_channel=6, out_channel=3, inner_channel=64, channel_mults=(1, 2, 4, 8, 8), res_blocks=1),
        'flagship_32_12_rb3_in3': dict(in_channel=3, out_channel=3, inner_channel=32, channel_mults=(1, 2), res_blocks=3),
        'flagship_32_1244_rb2_dropout': dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 4, 4),
                                             attn_res=(16,), res_blocks=2, dropout=0.2, image_size=32),
        'sr3_val': SR3_UNET, 'tesr_val': TESR_UNET, 'gdp_val': GDP_UNET,
    }
    for variant, name in (('ddpm', 'sr3'), ('tesr', 'tesr')):
        for hit, attn in (('attn', (8,)), ('noattn', (3,))):      # levels run at 32, 16, 8, 4
            for rb in (1, 2):
                out[f'{name}_{hit}_rb{rb}'] = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 2, 4),
                                                  attn_res=attn, res_blocks=rb, dropout=0.2, image_size=32, variant=variant)
    for hit, attn in (('attn', (2, 4)), ('noattn', (16,))):      # downsample rates 1, 2, 4; the middle block always attends
        for rb in (1, 2):
            out[f'gdp_{hit}_rb{rb}'] = dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 2),
                                            attn_res=attn, res_blocks=rb, dropout=0.1, image_size=32, variant='gdp')
    return out


def fingerprint(kw):
    cfg = UNetConfig(**kw)
    eng = Engine(cfg)
    sch = [[k, list(s), bool(live)] for k, s, live in eng.schema()]
    fp = {'schema_sha256': hashlib.sha256(json.dumps(sch).encode()).hexdigest(), 'n_schema': len(sch)}
    fp['workspace_bytes'] = [eng.workspace_bytes(*s) for s in SHAPES]
    eng.set_debug(True)
    fp['workspace_bytes_debug'] = [eng.workspace_bytes(*s) for s in SHAPES]
    eng.set_debug(False)
    if cfg.dropout > 0:
        eng.set_training(True)
    fp['train_workspace_bytes'] = [eng.train_workspace_bytes(*s) for s in SHAPES[:N_TRAIN_SHAPES]]
    return fp


def main():
    doc = {'shapes': [list(s) for s in SHAPES], 'configs': {}}
    for name, kw in configs().items():
        kw = {k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}
        doc['configs'][name] = {'config': kw, 'fingerprint': fingerprint(kw)}
    with open(OUT, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', os.path.normpath(OUT), len(doc['configs']), 'configs')


if __name__ == '__main__':
    main()
