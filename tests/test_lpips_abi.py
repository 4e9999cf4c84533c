"""The LPIPS entry points of include/fdsr.h without a GPU: exported, wrong names / shapes refused (FDSR_E_KEY), a call without
the weights refused (FDSR_E_STATE), sizes below 32 refused (FDSR_E_INVALID).  None of these reach the device."""
import ctypes as C

import numpy as np

FDSR_E_INVALID, FDSR_E_KEY, FDSR_E_STATE = -1, -2, -3
NAMES = ('fdsr_lpips_create', 'fdsr_lpips_load', 'fdsr_lpips_workspace_bytes', 'fdsr_lpips_u8', 'fdsr_lpips_destroy')


def _lib():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    return _lib.load()


def _load(lib, h, name, shape):
    a = np.zeros(int(np.prod(shape)) or 1, dtype=np.float32)
    return lib.fdsr_lpips_load(h, name.encode(), C.c_void_p(a.ctypes.data), (C.c_int64 * len(shape))(*shape), len(shape))


def test_symbols_exported():
    from fastdiffsr_amd import _lib as L
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SYMBOLS, n


def test_wrong_key_or_shape_is_refused():
    lib = _lib()
    h = C.c_void_p()
    assert lib.fdsr_lpips_create(C.byref(h)) == 0 and h.value
    try:
        assert _load(lib, h, 'features.1.weight', (64, 3, 11, 11)) == FDSR_E_KEY
        assert _load(lib, h, 'classifier.1.weight', (4096, 9216)) == FDSR_E_KEY
        assert _load(lib, h, 'lin5.model.1.weight', (1, 64, 1, 1)) == FDSR_E_KEY
        assert _load(lib, h, 'features.0.weight', (64, 3, 5, 5)) == FDSR_E_KEY
        assert _load(lib, h, 'features.3.bias', (64,)) == FDSR_E_KEY
        assert _load(lib, h, 'lin1.model.1.weight', (1, 64, 1, 1)) == FDSR_E_KEY
        assert _load(lib, h, 'lin1.model.1.weight', (192,)) == FDSR_E_KEY
        assert b'lin1' in lib.fdsr_last_error(None)
    finally:
        lib.fdsr_lpips_destroy(h)


def test_call_without_weights_and_small_sizes_are_refused():
    lib = _lib()
    h = C.c_void_p()
    assert lib.fdsr_lpips_create(C.byref(h)) == 0
    fake = C.c_void_p(4096)          # never dereferenced: the checks come first
    try:
        args = (fake, fake, None, 2, 64, 64, fake, fake, C.c_size_t(1 << 40), None)
        assert lib.fdsr_lpips_u8(h, *args) == FDSR_E_STATE
        assert lib.fdsr_lpips_u8(h, fake, fake, fake, 2, 24, 64, fake, fake, C.c_size_t(1 << 40), None) == FDSR_E_INVALID
        assert lib.fdsr_lpips_u8(h, fake, fake, fake, 2, 64, 31, fake, fake, C.c_size_t(1 << 40), None) == FDSR_E_INVALID
        n = C.c_size_t()
        assert lib.fdsr_lpips_workspace_bytes(h, 4, 24, 24, C.byref(n)) == FDSR_E_INVALID
        assert lib.fdsr_lpips_workspace_bytes(h, 4, 32, 32, C.byref(n)) == 0 and n.value > 0
        m = C.c_size_t()
        assert lib.fdsr_lpips_workspace_bytes(h, 8, 32, 32, C.byref(m)) == 0 and m.value > n.value
    finally:
        lib.fdsr_lpips_destroy(h)
