"""The engine's three Philox streams against tests/philox_reference.py (numpy, written from the paper and include/fdsr.h,
held to the Random123 known-answer vectors by test_philox_reference_host.py): sampler noise element by element, the key
(seed, calls, plane, pixel), the extreme uniforms, the in-loop draws of a sibling and of a ragged shape, the dropout masks
bit for bit, and the training step's self-drawn target noise, also for a shard of a larger batch.

The bar of every value comparison is BAR = 4 x (max |fp32 numpy restatement - fp64 reference| of the same formula on 2^20
counters), a figure that comes from the reference alone (philox_reference.fp32_restatement_gap); the x4 is room for the device
libm's extra ulps in logf / sqrtf / sincospif.  Measured: restatement-vs-reference 1.777e-06, so BAR = 7.11e-06 absolute."""
import math

import numpy as np
import pytest
import torch

import philox_reference as P
from fastdiffsr_amd.arch import UNetConfig, FASTDIFFSR_SCHEDULE_VAL, build_layers
from fastdiffsr_amd.synth import synth_state_dict, synth_inputs

pytestmark = pytest.mark.gpu

SMALL = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=16, channel_mults=(1, 2, 2), res_blocks=1,
             dropout=0.0, image_size=32)
TRAIN = dict(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2, 4), attn_res=(16,),
             res_blocks=1, dropout=0.2, image_size=32)
GDP = dict(in_channel=6, out_channel=3, inner_channel=64, norm_groups=32, channel_mults=(1, 2, 2), attn_res=(2, 4), res_blocks=1,
           dropout=0.1, image_size=32, variant='gdp')

SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1, 0x0123456789ABCDEF)
PLANES = (0, 1, 19, 999, 1999)


def _engine(kw, weights_seed=3, schedule=FASTDIFFSR_SCHEDULE_VAL):
    from fastdiffsr_amd.engine import Engine
    from fastdiffsr_amd.schedule import schedule_buffers, sampling_scalars
    cfg = UNetConfig(**kw)
    e = Engine(cfg)
    e.load_state_dict(synth_state_dict(cfg, weights_seed))
    bufs, sp = schedule_buffers(schedule)
    e.set_schedule(sampling_scalars(bufs, sp))
    return e


@pytest.fixture(scope='module')
def eng():
    return _engine(SMALL)


@pytest.fixture(scope='module')
def bar():
    gap = P.fp32_restatement_gap()
    print(f'\nreference vs reference (fp32 numpy restatement against fp64, 3 x 2^20 normals): max |d| = {gap:.3e}; BAR = {4 * gap:.3e}')
    return 4 * gap


def _gap(dev, ref):
    """max |device - reference| over EVERY element; non-finite device values count as infinite."""
    d = np.abs(dev.double().cpu().numpy() - ref)
    assert d.shape == ref.shape
    return float(np.where(np.isfinite(d), d, np.inf).max())


@pytest.mark.timeout(300)
@pytest.mark.parametrize('shape', [(1, 64, 64), (3, 40, 56), (4, 256, 256)])
def test_sampler_noise_equals_the_reference(eng, bar, shape):
    """eng.randn(B,H,W,plane) at calls = 0 against randn_plane, every element, for 5 seeds x 5 planes (0, 1, 19 = the last of T = 20,
    999 and 1999 = the last of the siblings' T) per shape.  Measured on one MI355X: device-vs-reference max |d| = 5.013e-07,
    5.385e-07 and 7.619e-07 on the three shapes (75 planes in all), against 1.777e-06 reference-vs-reference and BAR = 7.106e-06."""
    B, H, W = shape
    worst = 0.0
    for seed in SEEDS:
        eng.set_seed(seed)
        for plane in PLANES:
            d = _gap(eng.randn(B, H, W, plane), P.randn_plane(seed, 0, plane, B, H, W))
            worst = max(worst, d)
            assert d <= bar, (hex(seed), plane, shape, d, bar)
    print(f'device vs reference {shape}: max |d| = {worst:.3e} (BAR {bar:.3e})')


@pytest.mark.timeout(300)
def test_key_is_seed_calls_plane_pixel(bar):
    """After set_seed(s) fdsr_randn reports calls = 0; every engine-drawn fdsr_sample advances the call counter by one before it
    draws (k samples: calls = k), eager and under graph replay (the counter lives on the device), and so does a training step that
    draws its own target.  Every plane is held against the reference AT THAT calls value, never against another engine call.
    The high seed word is part of the key.  (calls >> 32, which is xor-ed into key word 1, and i >> 32 are out of reach.)"""
    eng = _engine(TRAIN, 7)                                       # a configuration the training step runs too (Dropout off: eval mode)
    B, H, W = 2, 32, 32
    cond = synth_inputs(B, H, W, 20)[0].cuda()

    def check(seed, calls):
        for plane in (0, 1, 19):
            d = _gap(eng.randn(B, H, W, plane), P.randn_plane(seed, calls, plane, B, H, W))
            assert d <= bar, (hex(seed), calls, plane, d)

    seed = 0x00C0FFEE12345678
    eng.set_seed(seed)
    check(seed, 0)
    for k in (1, 2, 3):
        eng.sample(cond)
        check(seed, k)
    out = torch.empty(B, 3, H, W, device='cuda')
    eng.set_seed(seed)
    check(seed, 0)                                                # set_seed resets the counter
    for k in (1, 2, 3):
        eng.sample(cond, graph=True, out=out)                     # k = 1 captures and launches, 2 and 3 replay
        torch.cuda.synchronize()
        check(seed, k)
    eng.sample(cond, synth_inputs(B, H, W, 20)[1].cuda())         # explicit noise: no draw, no advance
    check(seed, 3)
    # a training step that draws its own target noise sits on the same counter
    g = torch.Generator().manual_seed(5)
    hr, sr = torch.rand(B, 3, H, W, generator=g).cuda(), torch.rand(B, 3, H, W, generator=g).cuda()
    gamma = (torch.rand(B, generator=g) * 0.5 + 0.4).cuda()
    eng.train_grads_pairs(hr, sr, gamma, None, 'l1', 1.0)
    check(seed, 4)
    eng.train_grads_pairs(hr, sr, gamma, eng.randn(B, H, W, 0), 'l1', 1.0)   # a target handed in: no advance
    check(seed, 4)
    # seeds that differ only in the high word
    lo_only, hi_a, hi_b = 5, (1 << 32) | 5, (2 << 32) | 5
    planes = {}
    for s in (lo_only, hi_a, hi_b):
        eng.set_seed(s)
        check(s, 0)
        planes[s] = eng.randn(B, H, W, 0)
    assert not torch.equal(planes[lo_only], planes[hi_a]) and not torch.equal(planes[hi_a], planes[hi_b])


@pytest.mark.timeout(300)
def test_extreme_uniforms(eng, bar):
    """The four committed tuples (philox_reference.EXTREME_TUPLES; the scan of 2^26 counters found one for each of the four
    kind x word combinations): a radius word with >> 8 == 0 (u = 2^-25, radius 5.887) and one with >> 8 == 0xFFFFFF (u = 1.0
    exactly, radius 0), in the channel pair 0/1 and in channel 2.  The device value there is finite and within BAR of the
    reference: up to 5.887 in magnitude in the first kind, exactly +-0 in the second.
    Measured: |d| = 1.9e-07 (pair, z = -3.652, -4.617) and 2.0e-07 (channel 2, z = 5.7295) at the two largest radii."""
    r_max = math.sqrt(-2.0 * math.log(2.0 ** -25))
    assert {(k, w) for k, _, _, _, w in P.EXTREME_TUPLES} == {('zero', 0), ('zero', 2), ('ones', 0), ('ones', 2)}
    for kind, seed, plane, i, word in P.EXTREME_TUPLES:
        eng.set_seed(seed)
        dev = eng.randn(4, 256, 256, plane)
        assert _gap(dev, P.randn_plane(seed, 0, plane, 4, 256, 256)) <= bar
        n, y, x = i // 65536, (i % 65536) // 256, i % 256
        got = dev[n, :, y, x].double().cpu().numpy()
        want = P.box_muller(P.noise_words(seed, 0, plane, np.array([i], np.uint64)))[0]
        chans = (0, 1) if word == 0 else (2,)
        assert np.isfinite(got).all()
        for c in chans:
            if kind == 'ones':
                assert got[c] == 0.0 and want[c] == 0.0, (kind, word, got)
            else:
                assert abs(got[c] - want[c]) <= bar and abs(got[c]) <= r_max + bar, (kind, word, got, want)
        if kind == 'zero':
            r = math.sqrt(sum(got[c] ** 2 for c in chans))
            if word == 0:
                assert abs(r - r_max) <= 2 * bar, (r, r_max)
            print(f'extreme {kind} word {word}: device {got[list(chans)]}, reference {want[list(chans)]}, '
                  f'max |d| = {np.abs(got - want)[list(chans)].max():.3e}')


@pytest.mark.timeout(600)
def test_in_loop_draws_equal_reported_planes_gdp_at_its_own_T():
    """GDP (the posterior takes the network output as x_0) at T = 1000: the engine-drawn run equals, bitwise, the explicit-noise run on
    the T + 1 planes fdsr_randn reports under that call's counter -- and those planes are the reference's (spot-checked here at the
    two ends; test_sampler_noise_equals_the_reference covers plane 999 in full)."""
    T = 1000
    eng = _engine(GDP, 5, dict(schedule='linear', n_timestep=T, linear_start=1e-4, linear_end=2e-2))
    B, H, W = 2, 32, 32
    cond = synth_inputs(B, H, W, 20)[0].cuda()
    eng.set_seed(424242)
    a = eng.sample(cond).clone()                                   # calls = 1
    planes = torch.stack([eng.randn(B, H, W, k) for k in range(T + 1)])
    gap = P.fp32_restatement_gap()
    for k in (0, 1, T - 1, T):
        assert _gap(planes[k], P.randn_plane(424242, 1, k, B, H, W)) <= 4 * gap
    b = eng.sample(cond, planes).clone()
    assert torch.equal(a, b)
    eng.set_seed(424242)
    c = eng.sample(cond, stepwise=True).clone()                    # the device-resident step state draws the same planes
    assert torch.equal(a, c)
    assert torch.isfinite(a).all()


@pytest.mark.timeout(300)
def test_in_loop_draws_equal_reported_planes_b3_40x56(eng, bar):
    """The same bitwise equality at B = 3, 40 x 56 (a grid that is no multiple of the 256-thread block)."""
    B, H, W = 3, 40, 56
    cond = synth_inputs(B, H, W, 20)[0].cuda()
    eng.set_seed(31337)
    a = eng.sample(cond).clone()
    planes = torch.stack([eng.randn(B, H, W, k) for k in range(20)])
    for k in (0, 19):
        assert _gap(planes[k], P.randn_plane(31337, 1, k, B, H, W)) <= bar
    assert torch.equal(a, eng.sample(cond, planes))
    assert not torch.equal(a, eng.sample(cond))


def _res_blocks(cfg):
    return [L.name for L in build_layers(cfg) if L.kind == 'res']


def _keep_bytes(e, block, p):
    """The keep bytes of `block` from the last training-mode forward, NHWC uint8, and their count; the engine reports
    keep / (1 - p) in NCHW."""
    m = e.dropout_mask(block)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    vals = torch.unique(m).cpu().numpy()
    assert all(v == 0.0 or abs(v - float(scale)) <= 1e-6 for v in vals.tolist()), vals
    keep = (m > 0).permute(0, 2, 3, 1).contiguous().cpu().numpy().astype(np.uint8)
    return keep, keep.size


@pytest.mark.timeout(300)
@pytest.mark.parametrize('p', [0.2, 0.5])
def test_dropout_masks_equal_the_reference(p):
    """Every block's mask of a training-mode forward equals dropout_keep(seed, step, slot, p, N*H*W*C), bit for bit, in NHWC order.
    The engine's rule (fdsr_engine.cpp): slot = the index of the residual block in network order (downs.*, mid.0, mid.1, ups.*:
    build order of the block2 convolutions), step = the number of training-mode forwards since the last fdsr_set_seed /
    fdsr_set_dropout_seed, the first being 1; fdsr_set_seed keys both generators, fdsr_set_dropout_seed only the masks.
    Masks of different blocks and of consecutive forwards differ in 2p(1-p) of their positions (5 sigma)."""
    import ctypes as C
    from fastdiffsr_amd import _lib
    e = _engine(dict(TRAIN, dropout=p))
    cfg = e.cfg
    blocks = _res_blocks(cfg)
    assert len(blocks) >= 6
    B, H, W = 4, 32, 32
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B, 6, H, W, generator=g).cuda()
    nl = (torch.rand(B, generator=g) * 0.5 + 0.4).cuda()
    e.set_training(True)

    def forward_masks(seed, step, first_image=0, xs=x, nls=nl):
        e.unet_forward(xs, nls)
        out = {}
        for slot, blk in enumerate(blocks):
            keep, n = _keep_bytes(e, blk, p)
            per_image = n // keep.shape[0]
            want = P.dropout_keep(seed, step, slot, p, n, first_elem=first_image * per_image)
            assert np.array_equal(keep.reshape(-1), want), (blk, slot, step, float((keep.reshape(-1) != want).mean()))
            out[blk] = keep
        return out

    seed = 0x0BADC0DE00000007
    e.set_seed(seed)
    plane_before = e.randn(2, 32, 32, 3).clone()
    m1 = forward_masks(seed, 1)
    m2 = forward_masks(seed, 2)
    m3 = forward_masks(seed, 3)
    e.set_seed(seed)                                              # the forward count starts again
    again = forward_masks(seed, 1)
    assert all(np.array_equal(again[b], m1[b]) for b in blocks)
    # independence the self-consistency tests cannot see: other block, other step
    expect = 2 * p * (1 - p)
    same_shape = {}
    for b in blocks:
        same_shape.setdefault(m1[b].shape, []).append(b)
    pairs = 0
    for shape, bs in same_shape.items():
        n = int(np.prod(shape))
        band = 5 * math.sqrt(expect * (1 - expect) / n)
        for b in bs:
            assert abs(m1[b].mean() - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), b
            for other in (m2[b], m3[b]):
                assert abs((m1[b] != other).mean() - expect) <= band, (b, 'steps')
        for i in range(len(bs)):
            for j in range(i + 1, len(bs)):
                assert abs((m1[bs[i]] != m1[bs[j]]).mean() - expect) <= band, (bs[i], bs[j])
                pairs += 1
    assert pairs >= 2                                             # blocks of equal shape exist in this network
    # fdsr_set_dropout_seed: another key for the masks, the forward count back to 0, the sampler's planes untouched
    dseed = 0x1122334455667788
    _lib.check(e.h, e.lib.fdsr_set_dropout_seed(e.h, C.c_uint64(dseed)))
    md = forward_masks(dseed, 1)
    assert not np.array_equal(md[blocks[0]], m1[blocks[0]])
    assert torch.equal(e.randn(2, 32, 32, 3), plane_before)
    # a shard of a larger batch ("drop_image_offset", the offset the data-parallel tests drive): images [2:4] of the B = 4 forward
    e.set_seed(seed)
    _lib.debug_option('drop_image_offset', 2)
    try:
        ms = forward_masks(seed, 1, first_image=2, xs=x[2:].contiguous(), nls=nl[2:].contiguous())
    finally:
        _lib.debug_option('drop_image_offset', 0)
    for b in blocks:
        assert np.array_equal(ms[b], m1[b][2:]), b


def _live_grads(e):
    return {k: e.get_grad(k).copy() for k, _, live in e.schema() if live}


@pytest.mark.timeout(300)
def test_self_drawn_training_noise(bar):
    """fdsr_train_grads_pairs with noise = NULL: the step advances the call counter and uses plane 0 at the new value, so it gives the
    loss and, bitwise, the gradients of the same step handed eng.randn(B,H,W,0) taken afterwards; with hr = sr = 0 and gamma = 0 the
    packed input's x_noisy channels ARE the drawn noise, which is held against the reference directly.

    Data-parallel ranks under one seed: a shard that holds images [lo, lo + n) of the global batch ("drop_image_offset" = lo, the
    offset its dropout masks already follow) draws pixels i = (lo + n') * H * W + pixel, i.e. the slice [lo : lo + n] of the
    full-batch plane; the shards' noise is NOT the same from rank to rank.  (Before this was plumbed, every rank drew images
    [0, n): two halves of a batch trained on identical noise.)  Without the offset a rank draws the first n images' noise."""
    from fastdiffsr_amd import _lib
    B, H, W = 4, 32, 32
    seed = 0x5EEDFACE0000BEEF
    e_full, e_a, e_b = (_engine(TRAIN, 7) for _ in range(3))
    for e in (e_full, e_a, e_b):
        e.set_training(True)
    g = torch.Generator().manual_seed(17)
    hr, sr = torch.rand(B, 3, H, W, generator=g).cuda() * 2 - 1, torch.rand(B, 3, H, W, generator=g).cuda() * 2 - 1
    gamma = (torch.rand(B, generator=g) * 0.5 + 0.4).cuda()
    scale = 1.0 / (B * 3 * H * W)
    zeros, gamma0 = torch.zeros_like(hr), torch.zeros_like(gamma)

    def step(e, lo, hi, noise, probe=False):
        """One step of images [lo, hi) as a shard at offset lo; probe: inputs that make x_noisy the noise itself."""
        _lib.debug_option('drop_image_offset', lo)
        try:
            if probe:
                e.train_grads_pairs(zeros[lo:hi].contiguous(), zeros[lo:hi].contiguous(), gamma0[lo:hi].contiguous(), noise, 'l1', scale)
                return e.debug_tensor('input')[:, 3:6].clone()
            loss = e.train_grads_pairs(hr[lo:hi].contiguous(), sr[lo:hi].contiguous(), gamma[lo:hi].contiguous(), noise, 'l1', scale)
            return loss, _live_grads(e)
        finally:
            _lib.debug_option('drop_image_offset', 0)

    # -- one engine, the whole batch --
    e_full.set_seed(seed)
    l_drawn, g_drawn = step(e_full, 0, B, None)                    # calls 0 -> 1, dropout forward 1
    full_plane = e_full.randn(B, H, W, 0)                          # plane 0 at calls = 1
    assert _gap(full_plane, P.randn_plane(seed, 1, 0, B, H, W)) <= bar
    e_full.set_seed(seed)                                          # same dropout masks again
    l_given, g_given = step(e_full, 0, B, full_plane)
    assert l_drawn == l_given
    for k in g_drawn:
        assert np.array_equal(g_drawn[k], g_given[k]), k
    e_full.set_seed(seed)
    seen = step(e_full, 0, B, None, probe=True)
    assert torch.equal(seen, full_plane)                           # -0 + 0 aside, which torch.equal treats as equal
    assert _gap(seen, P.randn_plane(seed, 1, 0, B, H, W)) <= bar

    # -- two engines under one seed, half a batch each --
    half = B // 2
    for e, lo in ((e_a, 0), (e_b, half)):
        e.set_seed(seed)
        seen = step(e, lo, lo + half, None, probe=True)
        assert torch.equal(seen, full_plane[lo:lo + half]), lo
        assert _gap(seen, P.randn_plane(seed, 1, 0, half, H, W, first_image=lo)) <= bar
        e.set_seed(seed)
        l_s, g_s = step(e, lo, lo + half, None)
        e.set_seed(seed)
        l_ref, g_ref = step(e, lo, lo + half, full_plane[lo:lo + half].contiguous())
        assert l_s == l_ref
        for k in g_s:
            assert np.array_equal(g_s[k], g_ref[k]), (lo, k)
    assert not torch.equal(full_plane[:half], full_plane[half:])
    # a rank that is told nothing about its position draws images [0, n)
    e_b.set_seed(seed)
    assert torch.equal(step(e_b, 0, half, None, probe=True), full_plane[:half])
    # fdsr_randn reports the unshifted plane whatever the offset is
    _lib.debug_option('drop_image_offset', half)
    try:
        assert torch.equal(e_b.randn(B, H, W, 0), full_plane)
    finally:
        _lib.debug_option('drop_image_offset', 0)
