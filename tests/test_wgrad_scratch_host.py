"""The weight-gradient scratch bound covers every launch (host only: the library's slice plan, no GPU call).

`wgrad_scratch_floats` sizes the training workspace per layer geometry; the launchers choose their slice counts per launch
(precision, kernel form, debug options).  Both come from the same functions of fdsr_wgrad.hip; this sweep holds them against
each other and against the sizing formula the bound had before it was derived from the plan."""
import ctypes as C
import itertools

import pytest

KINDS = {'CONV3_S1': 0, 'CONV3_S2': 1, 'CONV3_UP': 2, 'CONV1': 3}            # enum ConvKind (fdsr_kernels.h)
BATCHES = (1, 2, 3, 5, 32)
MAPS = ((8, 8), (40, 56), (72, 48), (256, 256))
CHANNELS = ((8, 32), (32, 32), (64, 64), (96, 64), (128, 128), (256, 128))     # (Cin, Cout)
OPTIONS = {'wgrad_form': 0, 'wgrad_colsum': 1}                                # defaults, restored after the sweep


def _internal(lib, mangled, restype, argtypes):
    fn = getattr(lib, mangled)          # C++ functions of namespace fdsr (fdsr_train.h), exported with default visibility
    fn.restype, fn.argtypes = restype, argtypes
    return fn


def _earlier_bound(kind, N, H, W, Cin, Cout):
    """The hand-written bound this one replaces: no shape may get less room than it gave."""
    T, TH = (1 if kind == 3 else 9), (2 if kind == 1 else 4)
    ncb, nib = (Cout + 63) // 64, (Cin + 63) // 64
    blocks = ncb * nib
    ntiles = N * ((W + 15) // 16) * ((H + TH - 1) // TH)
    s = max(1, min((1024 + blocks - 1) // blocks, ntiles, 512))
    need = s * blocks * T * 4096
    if kind in (0, 2):
        k0 = max(1, 512 // (blocks * N))
        ns = N * (k0 + 1)
        if ns > 512:
            ns = N * k0
        ns = max(min(ns, 512), 512 // blocks)
        need = max(need, ns * blocks * T * 4096 + ns * ncb * 64)
    return need


def test_scratch_bound_covers_every_launch_and_is_no_smaller_than_before():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()
    bound = _internal(lib, '_ZN4fdsr20wgrad_scratch_floatsENS_8ConvKindEiiiii', C.c_size_t, [C.c_int] * 6)
    written = _internal(lib, '_ZN4fdsr19wgrad_launch_floatsENS_8ConvKindEiiiiibb', C.c_size_t, [C.c_int] * 6 + [C.c_bool] * 2)
    shapes = list(itertools.product(KINDS.values(), BATCHES, MAPS, CHANNELS))
    seen = set()
    try:
        for form, colsum in itertools.product((0, 1, 2), (1, 0)):
            _lib.debug_option('wgrad_form', form)
            _lib.debug_option('wgrad_colsum', colsum)
            for kind, N, (H, W), (Cin, Cout) in shapes:
                b = bound(kind, N, H, W, Cin, Cout)
                assert b >= _earlier_bound(kind, N, H, W, Cin, Cout), (kind, N, H, W, Cin, Cout)
                for gn_plain, f16x3 in itertools.product((False, True), (False, True)):
                    w = written(kind, N, H, W, Cin, Cout, gn_plain, f16x3)
                    assert 0 < w <= b, (kind, N, H, W, Cin, Cout, form, colsum, gn_plain, f16x3, w, b)
                    seen.add((form, colsum, gn_plain, f16x3, w))
    finally:
        for name, value in OPTIONS.items():
            _lib.debug_option(name, value)
    # the sweep reached the column-sum plan: at the defaults an f16x3 launch of a Swish layer carries its partials behind the slices
    T, ncb, nib = 9, 1, 1
    w = written(0, 2, 256, 256, 64, 64, False, True)       # 512 tiles per image: k = 256 slices per image fit
    slices, rem = divmod(w, ncb * nib * T * 4096 + ncb * 64)
    assert rem == 0 and slices % 2 == 0 and slices > 0, w          # image-aligned: a multiple of N = 2 slices, each with 64 partials
    assert written(0, 2, 256, 256, 64, 64, True, True) % (T * 4096) == 0   # a gn_plain layer: the 8-wave form without column sums


@pytest.mark.parametrize('kind', sorted(KINDS.values()))
def test_more_tiles_never_need_more_room_than_the_bound(kind):
    """The bound does not depend on the tile count beyond the 4-wave term: maps from one tile to many stay under it."""
    from fastdiffsr_amd import _lib
    lib = _lib.load()
    bound = _internal(lib, '_ZN4fdsr20wgrad_scratch_floatsENS_8ConvKindEiiiii', C.c_size_t, [C.c_int] * 6)
    written = _internal(lib, '_ZN4fdsr19wgrad_launch_floatsENS_8ConvKindEiiiiibb', C.c_size_t, [C.c_int] * 6 + [C.c_bool] * 2)
    for N, side in itertools.product((1, 4, 7), (1, 9, 16, 17, 33, 100)):
        for f16x3 in (False, True):
            assert written(kind, N, side, side + 3, 64, 128, False, f16x3) <= bound(kind, N, side, side + 3, 64, 128)
