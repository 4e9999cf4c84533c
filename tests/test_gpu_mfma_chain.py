"""f16x3 products as one dependent MFMA chain per accumulator (lo(x) hi(w), hi(x) lo(w), hi(x) hi(w) back to back; EXPERIMENTS.md):
the one mistake a re-ordered issue sequence can make is a wrong PLANE in a chain -- hi hi issued twice, lo lo in place of a cross
term.  That is an error of relative size 2^-11 .. 2^-12 per product, far below the 1e-4 layer bound of the other conv tests, so here
every f16x3 form is forced at its smallest eligible shape and compared, layer by layer, with the exact-fp32 path of the SAME engine on
the same input under the bound the suite uses for cross-form agreement (tests/test_gpu_k32.py): 0 < |d| <= 2e-5 * max(1, |ref|).  A
dropped or doubled term misses that by more than 10x.  Each case also reruns bitwise."""
import pytest
import torch

from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_UNET, build_layers
from fastdiffsr_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu
TOL = 2e-5

DEFAULTS = {'k32': 1275, 'th_min_wgs': 256, 'k32_sb_min_wgs': 1024, 'k32_stagger': 0, 'splitk': 1, 'strip': 91, 'strip_min_wgs': 512, 'tail': 1}
# launcher settings that put the eligible launches of a small forward on one family of kernels each (as the tests of the families do)
FORMS = {
    'default': {},                                                     # the default tile rule: 2-row tiles, split K, riders, up2 on the 16x16x32 form, both tail kernels
    'two-row-all': {'k32': 13},                                        # 2-row tiles with riders, the 32x32x16 up / down convs
    'four-row-tiles': {'th_min_wgs': 1, 'k32': 27},                    # largest tile whatever the grid: 4 x 32 pixels per wave (8- and 4-row workgroups), split K
    'small-workgroups': {'k32': 1275 | 512, 'k32_sb_min_wgs': 1, 'splitk': 0, 'k32_stagger': 3},   # 6-row tiles, rider chunks first
    'h-kernels': {'k32': 0, 'strip': 0, 'tail': 0},                    # every conv on the 32x32x16 kernels
    'strip': {'strip': 127 - 4, 'strip_min_wgs': 1, 'splitk': 0},      # the column-strip form on every eligible launch
}
NETS = {64: dict(inner_channel=64, norm_groups=32), 48: dict(inner_channel=48, norm_groups=16)}
SHAPES = {'64x64': ((2, 6, 64, 64), 41), '40x64': ((1, 6, 40, 64), 42)}   # the second: 40 rows of 64 pixels, ragged strip segments

_ENG, _REF = {}, {}


def _engine(inner):
    if inner not in _ENG:
        from fastdiffsr_amd.engine import Engine
        kw = dict(FASTDIFFSR_UNET)
        kw.update(NETS[inner])
        cfg = UNetConfig(**kw)
        eng = Engine(cfg)
        eng.load_state_dict(synth_state_dict(cfg, 4))
        _ENG[inner] = (cfg, eng)
    return _ENG[inner]


def _reference(inner, shape_id):
    """every layer of the engine's exact-fp32 forward, computed once per (network, input)"""
    key = (inner, shape_id)
    if key not in _REF:
        cfg, eng = _engine(inner)
        shape, seed = SHAPES[shape_id]
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(*shape, generator=gen)
        nl = torch.rand(shape[0], 1, generator=gen) * 0.9 + 0.05
        eng.set_precision('f32')
        eng.set_debug(True)
        try:
            out = eng.unet_forward(x.cuda(), nl.cuda()).cpu()
            torch.cuda.synchronize()
            layers = {L.name: eng.debug_tensor(L.name).cpu() for L in build_layers(cfg)}
        finally:
            eng.set_debug(False)
            eng.set_precision('f16x3')
        _REF[key] = (x, nl, out, layers)
    return _REF[key]


CASES = [(64, '64x64', f) for f in ('default', 'two-row-all', 'four-row-tiles', 'small-workgroups', 'h-kernels')] + \
        [(48, '64x64', f) for f in ('default', 'four-row-tiles', 'h-kernels')] + [(64, '40x64', 'strip')]


@pytest.mark.parametrize('inner,shape_id,form', CASES, ids=['%d-%s-%s' % c for c in CASES])
def test_f16x3_chain_matches_exact_fp32(inner, shape_id, form):
    from fastdiffsr_amd import _lib
    cfg, eng = _engine(inner)
    x, nl, ref_out, ref_layers = _reference(inner, shape_id)
    eng.set_precision('f16x3')
    for k, v in FORMS[form].items():
        _lib.debug_option(k, v)
    try:
        eng.set_debug(True)
        out = eng.unet_forward(x.cuda(), nl.cuda())
        torch.cuda.synchronize()
        worst, diff = (0.0, ''), 0.0
        fails = []
        for L in build_layers(cfg):
            ref = ref_layers[L.name]
            d = (eng.debug_tensor(L.name).cpu() - ref).abs().max().item()
            scale = max(ref.abs().max().item(), 1.0)
            worst, diff = max(worst, (d / scale, L.name)), max(diff, d)
            if d > TOL * scale:
                fails.append(f'{L.name}: {d:.3e} (scale {scale:.2f})')
        eng.set_debug(False)
        d_out = (out.cpu() - ref_out).abs().max().item()
        print(f'{inner}-{shape_id}-{form}: worst layer {worst[1]} at {worst[0]:.3e} of its scale; output {d_out:.3e}')
        assert not fails, fails[:8]
        assert 0.0 < diff and 0.0 < d_out <= TOL * max(ref_out.abs().max().item(), 1.0), d_out   # (0.0: the f16x3 kernels never ran)
        assert torch.equal(eng.unet_forward(x.cuda(), nl.cuda()), out)                            # ordered reductions only
    finally:
        eng.set_debug(False)
        for k in FORMS[form]:
            _lib.debug_option(k, DEFAULTS[k])
