"""What the three comparator engines (SwinIR, HAT, TransENet) answer before any HIP call, and what their modules carry through
copy and pickle: the frames of fdsr_<f>_load / _forward / _debug_tensor / _workspace_bytes and the module scaffold are one
piece of code behind the three families, and these are its host-side promises.  No GPU: every call here returns at a check
that comes before the first device call, and the pointers handed over are never dereferenced."""
import copy
import ctypes as C
import pickle

import pytest
import torch

import hat_restatement as HR
import swinir_restatement as SR
import transenet_restatement as TR

E_INVALID, E_KEY, E_STATE = -1, -2, -3
FAMILIES = ('swinir', 'hat', 'transenet')
SHAPE = {'swinir': (1, 8, 8), 'hat': (1, 16, 16), 'transenet': (1, 32, 32)}


def make(family):
    if family == 'swinir':
        from fastdiffsr_amd.swinir import SwinIR
        return SwinIR(**dict(SR.SMALL, upscale=4))
    if family == 'hat':
        from fastdiffsr_amd.hat import HAT
        return HAT(**dict(HR.SMALL, upscale=4))
    from fastdiffsr_amd.transenet import TransENet
    return TransENet(**dict(TR.SMALL, scale=4, hr_patch_size=128))


class Engine:
    """The family's C functions on a fresh handle (no tensor loaded); every call returns (code, fdsr_last_error)."""

    def __init__(self, family):
        from fastdiffsr_amd import _lib
        self.family, self.lib, self.module = family, _lib.load(), make(family)
        self.graph = getattr(_lib, 'FDSR_%s_GRAPH' % family.upper())
        self.h = self.module._handle()
        # the first key of the schema that is a tensor of the engine (HAT's and SwinIR's schemas open with index buffers, which
        # are functions of the geometry and never loaded)
        self.first, p = self.module.named_reference_parameters()[0]
        self.first_shape = tuple(p.shape)
        self.host = (C.c_float * 64)()           # stands for x, out and the workspace: aligned or not, it is never reached

    def call(self, what, *args):
        rc = getattr(self.lib, 'fdsr_%s_%s' % (self.family, what))(self.h, *args)
        return rc, (self.lib.fdsr_last_error(None) or b'').decode()

    def load(self, name, data, shape):
        arr = (C.c_int64 * len(shape))(*shape)
        return self.call('load', name, data, arr, len(shape))

    def forward(self, x, out, ws, stream, flags):
        b, h, w = SHAPE[self.family]
        return self.call('forward', x, b, h, w, out, ws, C.sizeof(self.host), stream, flags)


@pytest.fixture(scope='module', params=FAMILIES)
def eng(request):
    return Engine(request.param)


def test_load_refuses_an_unknown_name(eng):
    rc, msg = eng.load(b'no.such.tensor', eng.host, (1,))
    assert rc == E_KEY and 'fdsr_%s_load' % eng.family in msg and 'no.such.tensor' in msg


def test_load_refuses_a_wrong_shape(eng):
    for d in range(len(eng.first_shape)):
        shape = list(eng.first_shape)
        shape[d] += 1
        rc, msg = eng.load(eng.first.encode(), eng.host, shape)
        assert rc == E_KEY and 'wrong shape' in msg and eng.first in msg
    rc, msg = eng.load(eng.first.encode(), eng.host, eng.first_shape[:-1])
    assert rc == E_KEY and 'wrong shape' in msg


def test_load_refuses_null_arguments(eng):
    assert eng.load(None, eng.host, eng.first_shape)[0] == E_INVALID
    assert eng.load(eng.first.encode(), None, eng.first_shape)[0] == E_INVALID
    assert eng.call('load', eng.first.encode(), eng.host, None, len(eng.first_shape))[0] == E_INVALID


def test_hat_names_one_upsampling_convolution_per_stage_it_has():
    e = Engine('hat')                            # x4: stages 0 and 2
    rc, msg = e.load(b'upsample.upsampling.4.bias', e.host, (256,))
    assert rc == E_KEY and 'upsample.upsampling.4.bias' in msg
    # .2 is .0 again: the name is known, so what is refused is the shape
    rc, msg = e.load(b'upsample.upsampling.2.bias', e.host, (255,))
    assert rc == E_KEY and 'wrong shape' in msg and 'upsample.upsampling.2.bias' in msg


def test_forward_checks_arguments_then_stream_then_tensors(eng):
    host, fake_stream = eng.host, C.c_void_p(64)
    rc, msg = eng.forward(host, host, host, None, 0)
    assert rc == E_STATE and 'is missing' in msg and "'%s'" % eng.first in msg and 'fdsr_%s_forward' % eng.family in msg
    rc, msg = eng.forward(host, host, host, fake_stream, eng.graph)
    assert rc == E_STATE and 'is missing' in msg
    assert eng.forward(host, None, host, None, 0)[0] == E_INVALID
    assert eng.forward(host, host, host, None, 2)[0] == E_INVALID
    assert eng.forward(host, host, host, None, eng.graph | 4)[0] == E_INVALID
    rc, msg = eng.forward(host, host, host, None, eng.graph)
    assert rc == E_INVALID and 'needs a created stream' in msg and 'FDSR_%s_GRAPH' % eng.family.upper() in msg
    # out and flags come before everything else: a null x with a null out is still 'bad arguments', not 'null argument'
    rc, msg = eng.forward(None, None, host, None, 0)
    assert rc == E_INVALID and 'bad arguments' in msg
    rc, msg = eng.forward(None, host, host, None, 0)
    assert rc == E_INVALID and 'null argument' in msg
    # the shape is checked before the tensors: a height of 3 is neither paddable to a window nor a multiple of the patch
    b, h, w = SHAPE[eng.family]
    rc, msg = eng.call('forward', host, b, 3, w, host, host, C.sizeof(host), None, 0)
    assert rc == E_INVALID and 'is missing' not in msg


def test_debug_tensor_and_workspace_bytes_refuse_null_arguments(eng):
    host, dims = eng.host, (C.c_int * 3)()
    b, h, w = SHAPE[eng.family]
    assert eng.call('debug_tensor', None, host, b, h, w, host, 64, dims, host, C.sizeof(host), None)[0] == E_INVALID
    assert eng.call('debug_tensor', b'x', host, b, h, w, None, 64, dims, host, C.sizeof(host), None)[0] == E_INVALID
    assert eng.call('debug_tensor', b'x', host, b, h, w, host, 64, None, host, C.sizeof(host), None)[0] == E_INVALID
    # its own null check, then prepare (here: the missing tensors), then the tap name
    rc, msg = eng.call('debug_tensor', b'no.such.tap', host, b, h, w, host, 64, dims, host, C.sizeof(host), None)
    assert rc == E_STATE and 'is missing' in msg and 'fdsr_%s_debug_tensor' % eng.family in msg
    rc, msg = eng.call('workspace_bytes', b, h, w, None)
    assert rc == E_INVALID and 'fdsr_%s_workspace_bytes' % eng.family in msg


@pytest.mark.parametrize('family', FAMILIES)
def test_copies_carry_the_tensors_and_create_an_engine_of_their_own(family):
    m = make(family)
    with torch.no_grad():
        for i, (_, p) in enumerate(m.named_reference_parameters()):
            p.fill_(0.25 + i)
    m._uploaded, m._ws, m._static = {'device': 'x'}, {'k': 1}, {'k': 2}      # as after a forward
    h = m._handle()
    assert h is not None and m._handle() is h
    sd = m.state_dict()
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._h is None and c._uploaded == {} and c._ws == {} and c._static == {}
        back = c.state_dict()
        assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
        assert all(back[k].data_ptr() != sd[k].data_ptr() for k in sd)
        assert c.cfg == m.cfg and list(c.schema) == list(m.schema)
        h2 = c._handle()
        assert h2 is not None and c._handle() is h2 and h2.value != h.value
    assert m._h is h and m._uploaded == {'device': 'x'}
