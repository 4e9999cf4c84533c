"""tests/unet_16bit_emulation.py without a GPU: the emulation of the UNet's bf16 / f16 modes is the oracle's network once its
roundings are off (structure pin), the per-element judge of tests/test_gpu_unet_16bit_layerwise.py rejects single faults planted in
E64's own outputs and accepts E32, and the cap that keeps the judge's bar from widening (the fp32 / fp64 spread of an operator's
pre-rounding value, and the rms of what undecided operand roundings can move it, stay at or below one spacing of the format at the
output's rms) holds for every operator at every shape the GPU
test runs.  Config FASTDIFFSR_UNET, weights synth_state_dict(cfg, 0)."""
import os

import pytest
import torch

import unet_16bit_emulation as E
from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_UNET
from fastdiffsr_amd.synth import synth_state_dict
from oracle import fdsr_oracle as O

torch.set_num_threads(min(16, os.cpu_count() or 1))
FMTS = ['bf16', 'f16']
GPU_SHAPES = [(2, 6, 32, 48), (1, 6, 24, 64), (1, 6, 24, 128), (1, 6, 40, 64), (1, 6, 136, 64)]   # test_gpu_unet_16bit_layerwise.py: CASES


@pytest.fixture(scope='module')
def net():
    cfg = UNetConfig(**FASTDIFFSR_UNET)
    return cfg, synth_state_dict(cfg, 0)


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g), torch.rand(shape[0], 1, generator=g) * 0.9 + 0.05


def test_rounding_helpers_agree_with_the_native_casts():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 9)
    v = torch.cat([v, torch.tensor([0.0, 65504.0, 65519.9, 65520.0, 1e6, -1e6, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 3 * 2.0 ** -25])])
    for fmt in FMTS:
        native = E.rnd(v, fmt)                                   # fp32 in: torch's own casts
        assert torch.equal(E.rnd(v.double(), fmt).float(), native), fmt        # fp64 in: frexp / round-half-even
        assert torch.equal(E.rnd(native, fmt), native)
        up = native + E.ulp(native, fmt).float()
        assert torch.equal(E.rnd(up, fmt), up) or fmt == 'f16'   # one spacing on is a format value again (f16: but for the clamp)
        t = E.rnd(v.double(), fmt, trunc=True)
        assert (t.abs() <= v.double().abs()).all() and ((t - E.rnd(v.double(), fmt)).abs() <= E.ulp(v.double(), fmt)).all()
    assert E.ulp(torch.tensor([1.0, 1.99, 2.0, 0.0]), 'bf16').tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]
    assert E.ulp(torch.tensor([1.0, 1e-9]), 'f16').tolist() == [2.0 ** -10, 2.0 ** -24]


def test_boundary_distance_is_where_the_rounding_changes():
    g = torch.Generator().manual_seed(0)
    v = (torch.randn(200000, generator=g).double() * torch.exp(torch.randn(200000, generator=g).double() * 6)).abs()
    v = torch.cat([v, torch.tensor([1.0, 1.0 + 1e-9, 1.0 - 1e-9, 2.0 ** -14, 2.0 ** -14 * (1 + 1e-9), 2.0 ** -24 * 0.3, 65503.0, 4.0 * (1 + 1e-12)],
                                   dtype=torch.float64)])
    for fmt in FMTS:
        d, r = E.boundary_distance(v, fmt), E.rnd(v, fmt)
        sat = v >= 65504 if fmt == 'f16' else torch.zeros_like(v, dtype=torch.bool)
        stays = (E.rnd(v + d * 0.999, fmt) == r) & (E.rnd((v - d * 0.999).clamp(min=0), fmt) == r)
        leaves = (E.rnd(v + d * 1.001 + 1e-300, fmt) != r) | (E.rnd(v - d * 1.001 - 1e-300, fmt) != r)
        assert (d >= 0).all() and (stays | sat).all() and (leaves | sat).all(), fmt


def test_structure_pin_roundings_off_is_the_oracle(net):
    """E64 with every rounding off, chained, equals O.unet_forward in fp64 on every build_layers name, and each block1 equals a restated
    `block` + noise shift: <= 1e-12 * max|ref|"""
    cfg, sd = net
    x, nl = _inputs((2, 6, 16, 24), 1)
    sd64 = {k: v.double() for k, v in O.to_torch_sd(sd).items()}
    cap = {}
    with torch.no_grad():
        ref = O.unet_forward(sd64, cfg, x.double(), nl.double(), capture=cap)
    e = E.Emu(sd, cfg, None, torch.float64)
    pre, stored = e.forward(x, nl)
    names = [L.name for L in O.build_layers(cfg)]
    assert set(names) == set(cap) and len(names) == 30
    for n in names:
        d = (stored[n] - cap[n]).abs().max().item()
        assert d <= 1e-12 * cap[n].abs().max().item(), (n, d)
        assert torch.equal(stored[n], pre[n])
    assert torch.equal(stored['final_conv'], pre['final_conv']) and (stored['final_conv'] - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    t = O.noise_level_mlp(sd64, nl.double(), cfg.inner_channel)
    n_b1 = 0
    with torch.no_grad():
        for name, kind, L, ins in e.operators():
            if kind != 'block1':
                continue
            xin = torch.cat([stored[i] for i in ins], dim=1)
            r = L.name + '.res_block'
            h = O.block(sd64, r + '.block1', xin, cfg.norm_groups)
            shift = torch.nn.functional.linear(t, sd64[r + '.noise_func.noise_func.0.weight'], sd64[r + '.noise_func.noise_func.0.bias'])
            h = h + shift.view(x.shape[0], -1, 1, 1)
            assert (stored[name] - h).abs().max().item() <= 1e-12 * h.abs().max().item(), name
            n_b1 += 1
    assert n_b1 == 22


def _applies(mut, op):
    name, kind, L, ins = op
    conv = kind != 'attn'
    if mut.startswith('rider_'):                          # a block_out whose res_conv rides in block2's accumulators
        return kind == 'block_out' and L.cin != L.cout
    if mut in ('drop_block', 'swap', 'unrounded_w'):
        return conv
    if mut == 'halo':
        return conv and kind != 'down'                    # (stride 2 over an even width never reads the right halo)
    if mut == 'gn_seam':
        return kind == 'block1' and L.cin == 192          # the (128 | 64) input: 6 channels per group, group 21 straddles the seam
    if mut == 'shift_img':
        return kind == 'block1'
    return name != 'final_conv'                           # trunc: every 16-bit store


MUTATIONS = {'rider_drop_block': (1, 0, 0, 0), 'rider_swap': (0, 1), 'drop_block': (1, 0, 1, 1), 'halo': True, 'swap': (0, 1), 'unrounded_w': True, 'gn_seam': 21, 'shift_img': True, 'trunc': True}


@pytest.mark.parametrize('fmt', FMTS)
def test_the_judge_rejects_single_faults_and_accepts_e32(net, fmt):
    """'device' = E64's own stored output with ONE fault: a (cout, 16-channel chunk, tap) block of products left out; the right halo of
    the last column read as its neighbour; two channels of a chunk swapped (each of these two also in the res_conv rider's products);
    weights unrounded; the GroupNorm scale of group g + 1 on
    group g across the (128 | 64) seam; image 0's noise shift on image 1; a truncating store.  Each is rejected at every operator it
    applies to; unmutated E32 passes at every operator.  (The truncating store sits exactly one spacing off: the bound alone lets it
    pass, the judge's tie rule is what rejects it.)"""
    cfg, sd = net
    x, nl = _inputs((2, 6, 16, 24), 2)
    e64, e32 = E.Emu(sd, cfg, fmt, torch.float64), E.Emu(sd, cfg, fmt, torch.float32)
    _, stored = e32.forward(x, nl)
    muts = {m: E.Emu(sd, cfg, fmt, torch.float64, {m: v}) for m, v in MUTATIONS.items()}
    pre64 = {}
    hit = {m: 0 for m in MUTATIONS}
    for op, p64, p32, s32, wide, _ in E.per_operator(e64, e32, stored, nl):
        of = E.out_format(op[0], fmt)
        ok = E.judge(s32, p64, p32, of, fmt, wide)
        assert ok['ok'] and ok['cap_ok'], (op[0], ok)
        for m, em in muts.items():
            if not _applies(m, op):
                continue
            with torch.no_grad():
                dev = em.run(op, stored, pre64, nl)[1]
            j = E.judge(dev, p64, p32, of, fmt, wide)
            print(f"{fmt} {op[0]:28s} {m:12s} rejected: |d| = {j['margin']:9.3g} x the bound, {j['unexplained']:6d} unexplained elements "
                  f"(farthest {j['tie_margin']:9.3g} x the grant from a boundary)")
            assert not j['ok'], (op[0], m, j)
            hit[m] += 1
        pre64[op[0]] = p64
    assert all(hit.values()) and hit['gn_seam'] >= 1, hit


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('shape', GPU_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cap_holds_for_every_operator_at_the_gpu_shapes(net, shape, fmt):
    """D = max|P32 - P64| <= ulp(rms(P64)), and rms(F) <= ulp(rms(P64)) for the widening of the undecided operand roundings, for every
    operator; inputs from a chained E32 forward; E32's stored output passes the judge"""
    cfg, sd = net
    x, nl = _inputs(shape, 7)
    e64, e32 = E.Emu(sd, cfg, fmt, torch.float64), E.Emu(sd, cfg, fmt, torch.float32)
    _, stored = e32.forward(x, nl)
    worst, wf, sharp = (0.0, ''), (0.0, 0.0, ''), (1.0, '')
    for op, p64, p32, s32, wide, _ in E.per_operator(e64, e32, stored, nl):
        j = E.judge(s32, p64, p32, E.out_format(op[0], fmt), fmt, wide)
        worst = max(worst, (j['delta_spacings'], op[0]))
        wf = max(wf, (j['widening_rms'], j['widening_max'], op[0]))
        if op[0] != 'final_conv':                                # (an fp32 store: its spacing is far below any spread)
            sharp = min(sharp, (j['sharp_share'], op[0]))
        assert j['cap_ok'], (op[0], j)
        assert j['ok'], (op[0], j)
    print(f'{fmt} {shape}: largest D = {worst[0]:.3g} spacings at rms ({worst[1]}); largest F: rms {wf[0]:.3g}, max {wf[1]:.3g} spacings at rms ({wf[2]}); '
          f'smallest share of elements whose grant stays below a quarter spacing: {sharp[0]:.3f} ({sharp[1]})')
