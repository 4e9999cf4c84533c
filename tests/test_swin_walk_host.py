"""What the host side of SwinIR and HAT answers before any HIP call, to the byte and to the letter: the workspace sizes (a function
of the walk's buffer numbering and of every tensor it touches), the refusals of fdsr_<f>_create with their order (a configuration
wrong in two ways gets the message of the earlier check) and the reflect-pad refusal of the shape check.  The two families share
this code; the figures and texts below are what each of them answered when it still had a copy of its own.  No GPU."""
import ctypes as C

import pytest

import hat_restatement as HR
import swinir_restatement as SR

E_INVALID = -1
SWINIR_SHAPES = ((1, 8, 8), (1, 16, 24), (1, 12, 20), (3, 8, 8), (3, 12, 20))       # one window, 2 x 3 windows, padded to 16 x 24
HAT_SHAPES = ((1, 16, 16), (1, 32, 48), (1, 20, 36), (3, 16, 16), (3, 20, 36))      # one window, 2 x 3 windows, padded to 32 x 48

# (configuration, upscale, patch_norm) -> fdsr_<f>_workspace_bytes for each of the shapes above
SWINIR_BYTES = {
    ('SMALL', 2, True): (110336, 662016, 662016, 331008, 1986048),
    ('SMALL', 3, True): (192256, 1153536, 1153536, 576768, 3460608),
    ('SMALL', 4, True): (356096, 2136576, 2136576, 1068288, 6409728),
    ('SMALL', 8, True): (1339136, 8034816, 8034816, 4017408, 24104448),
    ('SMALL', 4, False): (356096, 2136576, 2136576, 1068288, 6409728),
    ('FULL', 2, True): (323328, 1939968, 1939968, 969984, 5819904),
    ('FULL', 3, True): (332544, 1995264, 1995264, 997632, 5985792),
    ('FULL', 4, True): (539392, 3236352, 3236352, 1618176, 9709056),
    ('FULL', 8, True): (1449728, 8698368, 8698368, 4349184, 26095104),
    ('FULL', 4, False): (539392, 3236352, 3236352, 1618176, 9709056),
}
HAT_BYTES = {
    ('SMALL', 2, True): (516096, 3094272, 3094272, 1547520, 9282304),
    ('SMALL', 3, True): (843776, 5060352, 5060352, 2530560, 15180544),
    ('SMALL', 4, True): (1499136, 8992512, 8992512, 4496640, 26977024),
    ('SMALL', 8, True): (5431296, 32585472, 32585472, 16293120, 97755904),
    ('FULL', 2, True): (1850112, 11095808, 11095808, 5549824, 33287168),
    ('FULL', 3, True): (1850112, 11095808, 11095808, 5549824, 33287168),
    ('FULL', 4, True): (2714368, 16281344, 16281344, 8142592, 48843776),
    ('FULL', 8, True): (6171392, 37023488, 37023488, 18513664, 111070208),
}


def module(family, name, upscale, patch_norm):
    if family == 'swinir':
        from fastdiffsr_amd.swinir import SwinIR
        return SwinIR(**dict(getattr(SR, name), upscale=upscale, patch_norm=patch_norm))
    from fastdiffsr_amd.hat import HAT
    return HAT(**dict(getattr(HR, name), upscale=upscale, patch_norm=patch_norm))


def workspace_bytes(family, m, b, h, w):
    """(code, bytes, fdsr_last_error) of fdsr_<family>_workspace_bytes on the module's handle"""
    from fastdiffsr_amd import _lib
    lib, n = _lib.load(), C.c_size_t(0)
    rc = getattr(lib, 'fdsr_%s_workspace_bytes' % family)(m._handle(), b, h, w, C.byref(n))
    return rc, n.value, (lib.fdsr_last_error(None) or b'').decode()


@pytest.mark.parametrize('family,key', [('swinir', k) for k in SWINIR_BYTES] + [('hat', k) for k in HAT_BYTES])
def test_workspace_bytes_are_the_recorded_ones(family, key):
    want, shapes = (SWINIR_BYTES[key], SWINIR_SHAPES) if family == 'swinir' else (HAT_BYTES[key], HAT_SHAPES)
    m = module(family, *key)
    got = tuple(workspace_bytes(family, m, *s) for s in shapes)
    print(family, key, tuple(g[1] for g in got))
    assert all(g[0] == 0 for g in got), got
    assert tuple(g[1] for g in got) == want


def create(family, **over):
    """fdsr_<family>_create of the small configuration with `over` written over it: (code, fdsr_last_error)"""
    from fastdiffsr_amd import _lib
    lib = _lib.load()
    if family == 'swinir':
        c = _lib.FdsrSwinirConfig()
        c.window_size, c.mlp_hidden = 8, 72
    else:
        c = _lib.FdsrHatConfig()
        c.window_size, c.mlp_hidden = 16, 144
        c.compress_ratio, c.squeeze_factor, c.conv_scale, c.overlap_win_size = 3, 12, 0.01, 24
    c.embed_dim, c.n_layers, c.upscale, c.patch_norm, c.img_range = 36, 2, 4, 1, 1.0
    c.depths[0] = c.depths[1] = 2
    c.num_heads[0] = c.num_heads[1] = 6
    for k, v in over.items():
        if k in ('depths', 'num_heads'):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    h = C.c_void_p()
    rc = getattr(lib, 'fdsr_%s_create' % family)(C.byref(c), C.byref(h))
    if rc == 0:
        getattr(lib, 'fdsr_%s_destroy' % family)(h)
    return rc, (lib.fdsr_last_error(None) or b'').decode()


# one configuration per check, in the order of the checks; `{f}` is fdsr_<family>_create, `{ws}` the family's window
SHARED_REFUSALS = (
    (dict(window_size=7), '{f}: window_size 7 is not supported ({ws} only)'),
    (dict(n_layers=0), '{f}: 0 layers (1..8)'),
    (dict(n_layers=9), '{f}: 9 layers (1..8)'),
    (dict(embed_dim=0), '{f}: embed_dim 0 (1..512), mlp hidden width {hid}'),
    (dict(embed_dim=516), '{f}: embed_dim 516 (1..512), mlp hidden width {hid}'),
    (dict(mlp_hidden=0), '{f}: embed_dim 36 (1..512), mlp hidden width 0'),
    (dict(depths=(2, 0)), '{f}: layer 1: depth 0, embed_dim 36 over 6 heads'),
    (dict(num_heads=(0,)), '{f}: layer 0: depth 2, embed_dim 36 over 0 heads'),
    (dict(num_heads=(6, 5)), '{f}: layer 1: depth 2, embed_dim 36 over 5 heads'),
    (dict(embed_dim=66, num_heads=(2, 2)), '{f}: layer 0: head_dim 33 is not supported (at most 32)'),
    (dict(embed_dim=66, num_heads=(6, 2)), '{f}: layer 1: head_dim 33 is not supported (at most 32)'),
    (dict(upscale=5), '{f}: upscale 5 is not supported (2, 3, 4, 8)'),
    (dict(upscale=1), '{f}: upscale 1 is not supported (2, 3, 4, 8)'),
    (dict(img_range=0.0), '{f}: img_range must be positive'),
    (dict(img_range=float('nan')), '{f}: img_range must be positive'),
    # wrong in two ways: the earlier check speaks
    (dict(window_size=7, n_layers=0), '{f}: window_size 7 is not supported ({ws} only)'),
    (dict(n_layers=9, embed_dim=516), '{f}: 9 layers (1..8)'),
    (dict(embed_dim=516, upscale=5), '{f}: embed_dim 516 (1..512), mlp hidden width {hid}'),
    (dict(num_heads=(6, 5), img_range=0.0), '{f}: layer 1: depth 2, embed_dim 36 over 5 heads'),
    (dict(depths=(0,), embed_dim=66, num_heads=(6, 2)), '{f}: layer 0: depth 0, embed_dim 66 over 6 heads'),
    (dict(upscale=5, img_range=0.0), '{f}: upscale 5 is not supported (2, 3, 4, 8)'),
)
HAT_REFUSALS = (
    (dict(overlap_win_size=20), '{f}: overlap window 20 is not supported (24 only: overlap_ratio 0.5)'),
    (dict(compress_ratio=0), '{f}: embed_dim 36 is not divisible by compress_ratio 0'),
    (dict(compress_ratio=5), '{f}: embed_dim 36 is not divisible by compress_ratio 5'),
    (dict(squeeze_factor=0), '{f}: squeeze_factor 0 leaves no channel of embed_dim 36'),
    (dict(squeeze_factor=37), '{f}: squeeze_factor 37 leaves no channel of embed_dim 36'),
    # wrong in two ways: the overlap window sits between the window and the layer count, compress_ratio and squeeze_factor
    # between embed_dim and the layers' heads
    (dict(window_size=8, overlap_win_size=20), '{f}: window_size 8 is not supported (16 only)'),
    (dict(overlap_win_size=20, n_layers=0), '{f}: overlap window 20 is not supported (24 only: overlap_ratio 0.5)'),
    (dict(embed_dim=516, compress_ratio=5), '{f}: embed_dim 516 (1..512), mlp hidden width 144'),
    (dict(compress_ratio=5, squeeze_factor=37), '{f}: embed_dim 36 is not divisible by compress_ratio 5'),
    (dict(squeeze_factor=37, num_heads=(5,)), '{f}: squeeze_factor 37 leaves no channel of embed_dim 36'),
    (dict(squeeze_factor=0, upscale=5), '{f}: squeeze_factor 0 leaves no channel of embed_dim 36'),
)


@pytest.mark.parametrize('family', ('swinir', 'hat'))
def test_create_refuses_with_the_message_of_the_first_failing_check(family):
    from fastdiffsr_amd import _lib
    lib = _lib.load()
    fill = dict(f='fdsr_%s_create' % family, ws={'swinir': 8, 'hat': 16}[family], hid={'swinir': 72, 'hat': 144}[family])
    assert create(family)[0] == 0
    for over, text in SHARED_REFUSALS + (HAT_REFUSALS if family == 'hat' else ()):
        rc, msg = create(family, **over)
        assert rc == E_INVALID and msg == text.format(**fill), (over, rc, msg)
    fn = getattr(lib, 'fdsr_%s_create' % family)
    h = C.c_void_p()
    assert fn(None, C.byref(h)) == E_INVALID and lib.fdsr_last_error(None).decode() == '%s: null argument' % fill['f']
    c = _lib.FdsrSwinirConfig() if family == 'swinir' else _lib.FdsrHatConfig()                 # all zero: wrong in every way
    assert fn(C.byref(c), None) == E_INVALID and lib.fdsr_last_error(None).decode() == '%s: null argument' % fill['f']


@pytest.mark.parametrize('family,shape,pad', [('swinir', (4, 8), (4, 0)), ('swinir', (8, 3), (0, 5)), ('swinir', (9, 4), (7, 4)),
                                              ('hat', (8, 16), (8, 0)), ('hat', (16, 8), (0, 8)), ('hat', (17, 8), (15, 8))])
def test_an_image_too_small_to_reflect_pad_is_refused(family, shape, pad):
    m = module(family, 'SMALL', 4, True)
    rc, _, msg = workspace_bytes(family, m, 1, *shape)
    assert rc == E_INVALID and msg == ('fdsr_%s_workspace_bytes: a %dx%d image cannot be reflect-padded by (%d, %d) to a multiple of the window'
                                       % ((family,) + shape + pad)), msg
    rc, _, msg = workspace_bytes(family, m, 0, 16, 16)
    assert rc == E_INVALID and msg == 'fdsr_%s_workspace_bytes: bad arguments (B 0, 16x16)' % family
