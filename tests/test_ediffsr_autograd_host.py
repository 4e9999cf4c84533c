"""What copy.deepcopy and pickle carry of a ConditionalNAFNet (no GPU: creating the engine object is host work).  ema_pytorch.EMA
deep-copies its model; a copy that shared the handle would have it destroyed twice."""
import copy
import pickle

import torch

SETTING = dict(width=16, enc_blk_nums=[1, 0], middle_blk_num=0, dec_blk_nums=[0, 1])


def _module():
    from fastdiffsr_amd.ediffsr import ConditionalNAFNet
    from fastdiffsr_amd.synth import synth_nafnet
    m = ConditionalNAFNet(**SETTING)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_nafnet(0, **SETTING).items()}, strict=True)
    m._handle()                                  # an engine object, as after a first forward
    m._uploaded = ('cuda:0', ())                 # and what goes with it
    m._ws['x'] = torch.zeros(4, dtype=torch.uint8)
    m._precision, m._sde_T = 'f16x3', 100
    return m


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_deep_copy_and_pickle_carry_no_handle():
    m = _module()
    assert m._h is not None
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._h is None and c._uploaded is None and c._ws == {}
        assert c.precision == 'f32' and not hasattr(c, '_sde_T') and not hasattr(c, '_graph_stream')
        assert _same(m, c)
        assert all(p.data_ptr() != q.data_ptr() for p, q in zip(m.parameters(), c.parameters()))
        assert c._handle().value != m._h.value          # an engine object of its own
        assert c.engine_schema() == m.engine_schema()
    assert m._h is not None and m._uploaded is not None and m._ws and m.precision == 'f16x3'   # the original keeps its own


def test_state_dict_round_trips_through_a_copy():
    m = _module()
    c = copy.deepcopy(m)
    with torch.no_grad():
        for p in c.parameters():
            p.mul_(0.5)
    assert not _same(m, c)
    back = copy.deepcopy(c)
    back.load_state_dict(m.state_dict(), strict=True)
    assert _same(m, back)
    assert all(not p.requires_grad for p in back.parameters())
    r = copy.deepcopy(m.requires_grad_(True))
    assert all(p.requires_grad for p in r.parameters())
