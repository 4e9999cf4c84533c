"""The FID Inception of csrc/fdsr_fid.hip (metrics.FID) against the CPU restatement (fid_restatement.py: unfolded BN, unfused
input transform), on synthetic weights (synth.synth_inception_fid).

Bars: each module's output (module = k) and the pool3 features are held against the fp64 restatement within 4x the
restatement's own fp32-vs-fp64 spread at that tap, never looser than 1e-4 max|ref|; the measured values are printed.  The FID
bars are explained where they are asserted."""
import numpy as np
import pytest
import torch

import fid_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sd():
    from fastdiffsr_amd.synth import synth_inception_fid
    return synth_inception_fid(0)


@pytest.fixture(scope='module')
def fid(sd):
    from fastdiffsr_amd.metrics import FID
    return FID(sd)


@pytest.fixture(scope='module')
def ref256(sd):
    """the restatement at 256 x 256, B = 2, fp64 and fp32 (computed once for the module)"""
    u8 = R.seeded_images(1, 2, 256, 256)
    return u8, R.forward(sd, u8, torch.float64), R.forward(sd, u8, torch.float32)


def _dev(fid, u8, module=-1):
    return fid.features_u8(torch.from_numpy(np.ascontiguousarray(u8)).cuda(), module=module).cpu()


def _bound(r64, r32):
    spread = float((r32.double() - r64).abs().max())
    return min(4 * spread, 1e-4 * float(r64.abs().max())), spread


def test_resize_stage_matches_torch_interpolate(fid):
    """module = -2 (u8 / 255, bilinear 299, 2x - 1) against torch's CPU F.interpolate on the same fp32 u8 / 255.  Bitwise: the
    kernel evaluates the order of operations of torch's generic CPU bilinear kernel (source index, the two taps of each row, then
    the two rows; no contraction), which torch runs for a 3-channel NCHW input unless it is single-threaded.  A single-threaded
    torch takes its channels-last vector kernel, another order: there the bar is 2^-23 (one ulp of the interpolated value in
    [0.5, 1), doubled)."""
    bitwise = torch.get_num_threads() > 1
    for (h, w) in ((256, 256), (64, 48), (300, 200), (299, 299)):
        u8 = R.seeded_images(3, 2, h, w)
        ref = R.input_transform(u8, torch.float32).permute(0, 2, 3, 1).contiguous()
        got = _dev(fid, u8, module=-2)
        d = (got - ref).abs()
        same = float((got == ref).float().mean())
        print('resize %dx%d: max|d| = %.3g, bitwise-equal fraction %.6f' % (h, w, float(d.max()), same))
        assert float(d.max()) <= 2.0 ** -23
        if bitwise:
            assert torch.equal(got, ref)
        if (h, w) == (299, 299):
            # at 299 the resize is the identity: exactly 2 (u8 / 255) - 1
            x = torch.from_numpy(u8).float() / 255
            assert torch.equal(got, 2 * x - 1)


def test_every_module_and_pool3_against_fp64_restatement(fid, ref256):
    from fastdiffsr_amd.metrics import FID_MODULES
    u8, r64, r32 = ref256
    for k, (name, s, c) in enumerate(FID_MODULES):
        got = _dev(fid, u8, module=k)
        assert tuple(got.shape) == (2, s, s, c), (name, got.shape)
        ref = r64[k].permute(0, 2, 3, 1)
        bound, spread = _bound(ref, r32[k].permute(0, 2, 3, 1))
        d = float((got.double() - ref).abs().max())
        print('%-14s max|dev - f64| %.3g  f32-f64 spread %.3g  bound %.3g  max|ref| %.3g' % (name, d, spread, bound, float(ref.abs().max())))
        assert d <= bound, (name, d, bound)
    got = _dev(fid, u8)
    bound, spread = _bound(r64['pool3'], r32['pool3'])
    d = float((got.double() - r64['pool3']).abs().max())
    print('pool3          max|dev - f64| %.3g  f32-f64 spread %.3g  bound %.3g' % (d, spread, bound))
    assert got.shape == (2, 2048) and d <= bound


@pytest.mark.parametrize('hw', [(512, 512), (299, 299), (64, 48), (300, 200)])
def test_pool3_at_other_sizes(fid, sd, hw):
    u8 = R.seeded_images(7, 1, *hw)
    r64 = R.forward(sd, u8, torch.float64, taps=False)['pool3']
    r32 = R.forward(sd, u8, torch.float32, taps=False)['pool3']
    bound, spread = _bound(r64, r32)
    d = float((_dev(fid, u8).double() - r64).abs().max())
    print('pool3 %dx%d: max|dev - f64| %.3g, spread %.3g, bound %.3g' % (hw[0], hw[1], d, spread, bound))
    assert d <= bound


def test_bitwise_batch_position_and_reruns(fid):
    u8 = R.seeded_images(11, 7, 96, 80)
    alone = _dev(fid, u8[5:6])
    batch = _dev(fid, u8)
    assert torch.equal(alone[0], batch[5])
    assert torch.equal(batch, _dev(fid, u8))
    mid = _dev(fid, u8, module=10)
    assert torch.equal(mid[5:6], _dev(fid, u8[5:6], module=10))


def test_short_workspace_is_refused(fid):
    import ctypes as C
    from fastdiffsr_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device='cuda')
    out = torch.empty(2, 2048, device='cuda')
    ws = fid.workspace(2, 32, 32)
    need = fid._workspace_bytes(2, 32, 32)
    args = (C.c_void_p(x.data_ptr()), 2, 32, 32, -1, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()))
    assert lib.fdsr_fid_features_u8(fid._h, *args, C.c_size_t(need - 256), None) == -4      # FDSR_E_WORKSPACE
    assert lib.fdsr_fid_features_u8(fid._h, *args, C.c_size_t(need), None) == 0
    torch.cuda.synchronize()


# Two seeded sets of 48 images, features from the device and from the fp32 restatement (cached for the module).  With N = 48 <
# 2048 the covariances are singular and sqrtm works on a rank-47 product.  Measured on the restatement itself (fp32 vs fp64
# features of these very sets, synthetic seed 0): FID 0.45183, relative spread 9.2e-7, max feature spread 2.7e-6.  The
# device's fp32 features carry rounding of the same order, so relative 1e-3 leaves three orders of magnitude for sqrtm's
# conditioning at rank 47.
N_SET = 48


@pytest.fixture(scope='module')
def two_sets(sd):
    a, b = R.seeded_images(101, N_SET, 256, 256), R.seeded_images(202, N_SET, 256, 256)
    ra = torch.cat([R.forward(sd, a[i:i + 8], torch.float32, taps=False)['pool3'] for i in range(0, N_SET, 8)])
    rb = torch.cat([R.forward(sd, b[i:i + 8], torch.float32, taps=False)['pool3'] for i in range(0, N_SET, 8)])
    return a, b, ra, rb


def test_fid_of_two_sets_against_restatement(fid, two_sets):
    from fastdiffsr_amd.metrics import activation_statistics, frechet_distance
    a, b, ra, rb = two_sets
    da, db = _dev(fid, a), _dev(fid, b)
    f_dev = frechet_distance(*activation_statistics(da), *activation_statistics(db))
    f_ref = frechet_distance(*activation_statistics(ra), *activation_statistics(rb))
    print('FID device %.9g restatement %.9g rel %.3g' % (f_dev, f_ref, abs(f_dev - f_ref) / f_ref))
    assert f_ref > 0 and abs(f_dev - f_ref) <= 1e-3 * f_ref
    # FID of a set with itself: sqrtm(S S) of a singular S returns S only to its conditioning.  The floor is measured here on the
    # restatement's own fp32 features of set A (8.6e-7 when written); the device's may not exceed 4x that floor.
    s = activation_statistics(ra)
    floor = abs(frechet_distance(*s, *s))
    s = activation_statistics(da)
    f_self = frechet_distance(*s, *s)
    print('FID(A, A) device %.3g, restatement floor %.3g' % (f_self, floor))
    assert abs(f_self) <= 4 * max(floor, 1e-12)
