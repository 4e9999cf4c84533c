"""The FID entry points of include/fdsr.h without a GPU: exported, wrong names / shapes refused (FDSR_E_KEY), a call with a
tensor missing refused (FDSR_E_STATE), empty sizes or a module outside [-2, 17] refused (FDSR_E_INVALID).  None of these reach the device: only
the BN tensors are loaded, so no layer is complete and nothing is folded or uploaded (FDSR_E_WORKSPACE needs all 470 tensors on
the device: tests/test_gpu_fid.py)."""
import ctypes as C

import numpy as np

FDSR_E_INVALID, FDSR_E_KEY, FDSR_E_STATE, FDSR_E_WORKSPACE = -1, -2, -3, -4
NAMES = ('fdsr_fid_create', 'fdsr_fid_load', 'fdsr_fid_workspace_bytes', 'fdsr_fid_features_u8', 'fdsr_fid_destroy')


def _lib():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load()


def _load(lib, h, name, shape):
    a = np.zeros(int(np.prod(shape)) or 1, dtype=np.float32)
    return lib.fdsr_fid_load(h, name.encode(), C.c_void_p(a.ctypes.data), (C.c_int64 * len(shape))(*shape), len(shape))


def test_symbols_exported():
    from fastdiffsr_amd import _lib as L
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SYMBOLS, n


def test_wrong_key_or_shape_is_refused():
    lib = _lib()
    h = C.c_void_p()
    assert lib.fdsr_fid_create(C.byref(h)) == 0 and h.value
    try:
        assert _load(lib, h, 'fc.weight', (1008, 2048)) == FDSR_E_KEY
        assert _load(lib, h, 'AuxLogits.conv0.conv.weight', (128, 768, 1, 1)) == FDSR_E_KEY
        assert _load(lib, h, 'Mixed_5b.branch1x1.bn.num_batches_tracked', ()) == FDSR_E_KEY
        assert _load(lib, h, 'Mixed_5b.branch1x1.conv.bias', (64,)) == FDSR_E_KEY
        assert _load(lib, h, 'Mixed_5b.branch1x1.bn.weight', (32,)) == FDSR_E_KEY
        assert _load(lib, h, 'Mixed_6b.branch7x7_2.conv.weight', (128, 128, 7, 1)) == FDSR_E_KEY
        assert b'Mixed_6b.branch7x7_2.conv.weight' in lib.fdsr_last_error(None)
        assert _load(lib, h, 'Conv2d_1a_3x3.bn.running_var', (32,)) == 0
    finally:
        lib.fdsr_fid_destroy(h)


def test_missing_tensor_sizes_and_workspace_are_refused():
    from fastdiffsr_amd.metrics import FID_TENSORS
    lib = _lib()
    h = C.c_void_p()
    assert lib.fdsr_fid_create(C.byref(h)) == 0
    fake = C.c_void_p(4096)          # never dereferenced: the checks come first
    try:
        big = C.c_size_t(1 << 40)
        assert lib.fdsr_fid_features_u8(h, fake, 2, 64, 64, -1, fake, fake, big, None) == FDSR_E_STATE
        for k, shape in FID_TENSORS.items():
            if '.bn.' in k:
                assert _load(lib, h, k, shape) == 0
        assert lib.fdsr_fid_features_u8(h, fake, 2, 64, 64, -1, fake, fake, big, None) == FDSR_E_STATE
        assert b'.conv.weight' in lib.fdsr_last_error(None)
        for b, hh, ww, m in ((0, 64, 64, -1), (2, 0, 64, -1), (2, 64, 0, -1), (2, 64, 64, 18), (2, 64, 64, -3)):
            assert lib.fdsr_fid_features_u8(h, fake, b, hh, ww, m, fake, fake, big, None) == FDSR_E_INVALID
        n = C.c_size_t()
        assert lib.fdsr_fid_workspace_bytes(h, 0, 8, 8, C.byref(n)) == FDSR_E_INVALID
        assert lib.fdsr_fid_workspace_bytes(h, 1, 0, 8, C.byref(n)) == FDSR_E_INVALID
        assert lib.fdsr_fid_workspace_bytes(h, 1, 1, 1, C.byref(n)) == 0 and n.value > 0
        m = C.c_size_t()
        assert lib.fdsr_fid_workspace_bytes(h, 4, 1, 1, C.byref(m)) == 0 and m.value > n.value
        # every size is resized to 299: the workspace does not depend on H, W
        assert lib.fdsr_fid_workspace_bytes(h, 4, 1024, 77, C.byref(n)) == 0 and n.value == m.value
    finally:
        lib.fdsr_fid_destroy(h)
