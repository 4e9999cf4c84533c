"""The UNet engine's bf16 and f16 modes judged against their own arithmetic, operator by operator (the other layerwise checks of these
modes compare a whole forward with the fp32 oracle at 3-4 % of a tensor's largest element).  After one debug forward every planned
operator -- downs.0, <p>.res_block.block1, the block output, <p> after CLAM + SLAM, downs.k, ups.k, final_conv -- is re-evaluated on
the CPU from the DEVICE'S OWN stored inputs (debug_tensor: the 16-bit values widened, the skip tensor included on the up path) by
tests/unet_16bit_emulation.py in fp64 (E64) and in fp32 (E32), and the device's stored output is judged per element:

    D = max |P32 - P64|                                                  (the two pre-rounding values; a CPU spread, no device number)
    S_e = 4 D + F_e        F_e: what the operand roundings that fp32 evaluation cannot decide move element e (Emu._stage_act; CPU only)
    |dev - rnd(P64)| <= ulp(max(|dev|, |P64|)) + S_e                      for EVERY element of EVERY operator
    dev may differ from rnd(P64) only where P64 lies within S_e of a rounding boundary    (unet_16bit_emulation.judge: the tie rule)

No error accumulates, so the bar is about one spacing of the storage format per element (bf16: 2^-8 of the element's own magnitude)
plus what fp32 evaluation moves a value, where the oracle comparisons allow 0.03-0.04 of the tensor's maximum.  D <= ulp(rms(P64)) and
rms(F) <= ulp(rms(P64)) are the conditions tests/test_unet_16bit_emulation_host.py checks at these shapes; both are printed here.
final_conv stores fp32: its bar is ulp_fp32 + S_e.  Every 16-bit tap holds format values.

GroupNorm.  The device's statistics are sums of the producer's fp32 values BEFORE their rounding, which no stored tensor shows, and they
are sharp enough to move operand roundings (unet_16bit_emulation.py, "GroupNorm statistics").  So the table the device applied
(fdsr_debug_gn_table: scale, shift per image and channel) is read back and fed to the operator like its tensors, and judged on its own
against the table of the emulation's statistics (the producer's P64): the producer's elements are known to S_e each, so a group mean to
U = mean of S_e over the group, a group's E[x^2] to 2 rms U, hence
    |scale_dev - scale| <= |scale| t,   t = (rms + |mean|) U / (var + 1e-5) + 8 * 2^-24
    |shift_dev - shift| <= |scale| U + |mean scale| t + 8 * 2^-24 (|beta| + |mean scale|).
Every case runs with `gn_consumer` = 0: a launch that forms scale / shift in its own prologue leaves no table (that form is tested in
test_gpu_gn_consumer.py and is not judged here).

Cases (each in bf16 and f16; options restored in `finally`): the kernels a small forward takes by default but for the consumer-side
GroupNorm; the k32 forms test_gpu_k32.py forces; the column-strip
forms on one strip, two strips, four segments (H = 40) and 16 unequal segments (H = 136); the one-workgroup strip form.  A forced
case also runs with the ONE option that selects its form turned off (everything else as forced) and fails unless an operator the
form covers computes other bits from bitwise equal inputs and table (the form was never taken).

Measured on an MI355X (EXPERIMENTS section 15 has the table per case): D <= 0.0076 and rms F <= 0.12 spacings at rms (bf16: 0.0005 and
0.031), at most 2.7 % of an operator's elements off rnd(P64), every GroupNorm table within 0.28 of its bound."""
import os

import pytest
import torch

import unet_16bit_emulation as E
from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_UNET, FASTDIFFSR_SCHEDULE_VAL
from fastdiffsr_amd.synth import synth_state_dict
from fastdiffsr_amd.schedule import schedule_buffers, sampling_scalars

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

DEFAULTS = dict(gn_consumer=1, k32=1275, k32_sb_min_wgs=1024, k32_stagger=0, th_min_wgs=256, splitk=1, strip=91, strip_min_wgs=512)
STRIP = dict(strip=127 - 4, splitk=0)    # every strip bit but the one-workgroup A/B form: 64 -> 64, (64|64) -> 64, riders, (128|64) -> 64 (bit 32), 128 couts
# Segments (fdsr_conv_strip.hip: strip_seg_rows halves the segment length, rounding up, while it is above 16 rows and strips x segments
# is below strip_min_wgs; the kernel then balances: segment s = rows [s H / segs, (s + 1) H / segs)).  A 40 x 64 map at strip_min_wgs = 3
# (the largest value conv_strip_ok admits there: ceil(40 / 16) = 3 workgroups): 40 -> 20 -> 10 rows, four segments -- of EQUAL length:
# halving 8 k rows rounds up only once the length is odd and above 16, first at H = 136 (136 -> 68 -> 34 -> 17 -> 9 at strip_min_wgs = 9:
# 16 segments of 8 and 9 rows), so unequal segments need that map.  The wide forms (concatenated input, rider) halve the threshold:
# whole strips at H = 40, eight segments of 17 rows at H = 136.
# A guard: (the ONE option that turns the form off -- everything else stays as forced, `splitk` included --, what the form covers).  An
# operator shows the form was taken if its stored inputs and GroupNorm table are bitwise the same in both forwards and its stored
# output is not: nothing but its own kernel changed.  covers(kind, cin, cout, level)
_BLOCK = ('block1', 'block_out')
_L0_64 = lambda kind, cin, cout, level: kind in _BLOCK and cout == 64 and level == 0
CASES = [
    # (not the shipped default: with the consumer-side GroupNorm off, module docstring)
    ('default-gn-finalize', {}, (2, 6, 32, 48), []),
    ('k32-small-workgroup', dict(k32=1275 | 512, k32_sb_min_wgs=1, splitk=0, k32_stagger=3), (2, 6, 32, 48), [(dict(k32=27), _L0_64)]),
    ('k32-largest-tile', dict(th_min_wgs=1), (2, 6, 32, 48), [(dict(th_min_wgs=256), lambda kind, cin, cout, level: kind in _BLOCK)]),
    ('strip-one', dict(STRIP, strip_min_wgs=1), (1, 6, 24, 64), [(dict(strip=0), _L0_64)]),
    ('strip-two', dict(STRIP, strip_min_wgs=1), (1, 6, 24, 128),
     [(dict(strip=0), _L0_64), (dict(strip=123 & ~64), lambda kind, cin, cout, level: kind in _BLOCK and cout == 128 and level == 1)]),
    ('strip-segments', dict(STRIP, strip_min_wgs=3), (1, 6, 40, 64), [(dict(strip=0), _L0_64)]),
    ('strip-unequal-segments', dict(STRIP, strip_min_wgs=9), (1, 6, 136, 64), [(dict(strip=0), _L0_64)]),
    # every bit: the (128|64) -> 64 launch (bit 32, off by default: spills) and the one-workgroup 64 -> 64 form (bit 4: the two-workgroup
    # kernel under another launch bound, the same sums in the same order, so no output can show it)
    ('strip-wide', dict(strip=127, splitk=0, strip_min_wgs=1), (1, 6, 24, 64),
     [(dict(strip=127 & ~32), lambda kind, cin, cout, level: kind == 'block1' and cin == 192 and cout == 64)]),
]


@pytest.fixture(scope='module')
def full():
    from fastdiffsr_amd.engine import Engine
    cfg = UNetConfig(**FASTDIFFSR_UNET)
    eng = Engine(cfg)
    sd = synth_state_dict(cfg, 0)
    eng.load_state_dict(sd)
    bufs, sp = schedule_buffers(FASTDIFFSR_SCHEDULE_VAL)
    eng.set_schedule(sampling_scalars(bufs, sp))
    eng.set_precision('f16x3')
    return cfg, eng, sd


@pytest.fixture(scope='module')
def emus(full):
    cfg, eng, sd = full
    return {fmt: (E.Emu(sd, cfg, fmt, torch.float64), E.Emu(sd, cfg, fmt, torch.float32)) for fmt in ('bf16', 'f16')}


def _taps(eng, ops, x, nl):
    """one debug forward: ({name: stored tensor}, {conv op: (scale, shift)})"""
    names = ['input'] + [op[0] for op in ops]
    out = eng.unet_forward(x.cuda(), nl.cuda())
    torch.cuda.synchronize()
    stored = {n: eng.debug_tensor(n).cpu() for n in names}
    tables = {c: tuple(t.cpu() for t in eng.debug_gn_table(c)) for c in filter(None, map(E.gn_conv_name, ops))}
    assert torch.equal(stored['input'][:, :x.shape[1]], x) and not stored['input'][:, x.shape[1]:].any()
    assert torch.equal(out.cpu(), stored['final_conv'])
    stored['input'] = x
    return stored, tables


def _table_check(e64, op, table, gn, grant):
    """the device's GroupNorm table `gn` against the statistics' one (module docstring); returns the worst ratio to the bound"""
    sc, sh, mean, var = table
    name, kind, L, ins = op
    srcs = ins if kind in ('block1', 'final') else ins[:1]
    B, C = sc.shape
    G = e64.G
    U = torch.cat([grant[n] for n in srcs], dim=1).reshape(B, G, -1).mean(-1)
    rms = (var + mean * mean).sqrt()
    t = ((rms + mean.abs()) * U / (var + 1e-5) + 8 * 2.0 ** -24).repeat_interleave(C // G, 1)
    U, mean = U.repeat_interleave(C // G, 1), mean.repeat_interleave(C // G, 1)
    beta = e64.sd[E.gn_key(op) + '.bias']
    r_sc = (gn[0].double() - sc).abs() / (sc.abs() * t).clamp(min=1e-300)
    r_sh = (gn[1].double() - sh).abs() / (sc.abs() * U + (mean * sc).abs() * t + 8 * 2.0 ** -24 * (beta.abs() + (mean * sc).abs()))
    return max(r_sc.max().item(), r_sh.max().item())


@pytest.mark.timeout(600)
@pytest.mark.parametrize('prec', ['bf16', 'f16'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_every_operator_against_the_modes_arithmetic(full, emus, case, prec):
    from fastdiffsr_amd import _lib
    cfg, eng, sd = full
    cid, options, shape, guards = case
    e64, e32 = emus[prec]
    ops = e64.operators()
    names = ['input'] + [op[0] for op in ops]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(*shape, generator=g)
    nl = torch.rand(shape[0], 1, generator=g) * 0.9 + 0.05
    try:
        _lib.debug_option('gn_consumer', 0)
        for k, v in options.items():
            _lib.debug_option(k, v)
        eng.set_precision(prec)
        eng.set_debug(True)
        stored, tables = _taps(eng, ops, x, nl)
        for n in names[1:-1]:                                    # every 16-bit tap holds format values
            assert torch.equal(stored[n], E.rnd(stored[n], prec)), n
        failures, grant = [], {}
        print(f'\n{cid} {prec} {shape}: worst |dev - rnd(P64)| in spacings | D, rms F in spacings at rms | share of elements off rnd(P64) | x the bound | GroupNorm table x its bound')
        for op, p64, p32, _, wide, stat_table in E.per_operator(e64, e32, stored, nl, tables):
            j = E.judge(stored[op[0]], p64, p32, E.out_format(op[0], prec), prec, wide)
            grant[op[0]] = torch.zeros_like(p64, dtype=torch.float64) + 4 * j['delta'] + (wide if wide is not None else 0.0)
            tab = _table_check(e64, op, stat_table, tables[E.gn_conv_name(op)], grant) if E.gn_conv_name(op) else 0.0
            print(f"  {op[0]:28s} {j['worst_spacings']:9.3g} {j['delta_spacings']:9.3g} {j['widening_rms']:9.3g} {j['share_diff']:10.3e} {j['margin']:9.3g} {tab:9.3g}"
                  + ('' if j['ok'] else f"   FAIL ({j['unexplained']} elements off farther than S from a boundary, worst {j['tie_margin']:.3g} x)"))
            if not j['ok'] or tab > 1 or not j['cap_ok']:            # (the caps, on the device's inputs and tables too: the bar must not widen silently)
                failures.append(op[0] + ('' if j['cap_ok'] else ' (cap)'))
        for off, covers in guards:                               # exercise guard: the forced form was taken (comment at CASES)
            for k, v in off.items():
                _lib.debug_option(k, v)
            plain, ptables = _taps(eng, ops, x, nl)
            for k in off:
                _lib.debug_option(k, options[k])
            shown = []
            for name, kind, L, ins in ops:
                level = (shape[3] // stored[name].shape[3]).bit_length() - 1
                conv = E.gn_conv_name((name, kind, L, ins))
                same_in = all(torch.equal(plain[i], stored[i]) for i in ins) and all(torch.equal(a, b) for a, b in zip(ptables.get(conv, ()), tables.get(conv, ())))
                if same_in and covers(kind, L.cin, L.cout, level) and not torch.equal(plain[name], stored[name]):
                    shown.append(name)
            moved = sum(not torch.equal(plain[n], stored[n]) for n in names[1:])
            print(f'  {off}: {moved} of {len(names) - 1} stored outputs differ; on bitwise equal inputs and table: {shown}')
            assert shown, f'{off}: no operator the form covers computed other bits on the same inputs: the form was never taken'
        assert not failures, failures
    finally:
        eng.set_debug(False)
        eng.set_precision('f16x3')
        for k, v in DEFAULTS.items():
            _lib.debug_option(k, v)
