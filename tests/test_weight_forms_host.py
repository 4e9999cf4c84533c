"""The weight-form freshness record (csrc/fdsr_forms.h) against the rules it replaced (host only, no GPU call).

Before the record, six booleans on the engine said which device forms of the weights follow the master copy, and each entry
point applied its own rule to them.  `_Earlier` restates those rules.  Every state reachable from "all weights loaded" under
the engine's events and readers is walked breadth-first, the library's record beside the restatement: the packing passes with
their arguments, whether the captured graphs are dropped and the upsample form read must agree -- except where the earlier
rules let a reader see a form that lags the master copy; there the record must refresh, and the states are printed."""
import ctypes as C
from collections import deque

import pytest

F32, F16X3, BF16, F16 = 0, 1, 2, 3                                           # enum Precision
FWD32, WT32, FWD_H3, UP2_H3, B16, WT_H3, TEMB, SCHED = range(8)              # enum Family (fdsr_forms.h)
BEHIND, LAZY, HOST, DEVICE = range(4)                                        # enum Src
PASSES = ('DEVICE_SYNC', 'SYNC16', 'PACK_T', 'PACK_STEP_LAZY', 'PACK_STEP_FULL', 'PACK_ALL32', 'TEMB_TABLE', 'STEP_SCHED')
# the device passes as the calls they were: repack_from_master(forward_forms, all_f32_forms), and whether it ran lazily
REPACK = {'PACK_T': ('repack', 0, 0, 0), 'PACK_STEP_LAZY': ('repack', 1, 0, 1), 'PACK_STEP_FULL': ('repack', 1, 0, 0),
          'PACK_ALL32': ('repack', 1, 1, 0)}
UP2 = ('generic', 'host scale', 'device scale')


class Forms(C.Structure):
    _fields_ = [('st', C.c_uint8 * 8), ('lazy_skips', C.c_bool)]


class Plan(C.Structure):
    _fields_ = [('n', C.c_int), ('p', C.c_uint8 * 4), ('drop', C.c_bool)]


@pytest.fixture(scope='module')
def rec():
    from fastdiffsr_amd import _lib, build
    build.build(force=False, verbose=False)
    lib = _lib.load()

    def fn(mangled, restype, *argtypes):    # C++ functions of namespace fdsr_forms, exported with default visibility
        f = getattr(lib, mangled)
        f.restype, f.argtypes = restype, list(argtypes)
        return f
    R = C.POINTER(Forms)

    class Rec:
        on_load = fn('_ZN10fdsr_forms7on_loadERNS_5FormsE', Plan, R)
        on_schedule = fn('_ZN10fdsr_forms11on_scheduleERNS_5FormsE', Plan, R)
        on_step = fn('_ZN10fdsr_forms7on_stepERKNS_5FormsEi', Plan, R, C.c_int)
        on_precision = fn('_ZN10fdsr_forms12on_precisionERKNS_5FormsEii', Plan, R, C.c_int, C.c_int)
        on_sync = fn('_ZN10fdsr_forms7on_syncERKNS_5FormsE', Plan, R)
        need_forward = fn('_ZN10fdsr_forms12need_forwardERKNS_5FormsEib', Plan, R, C.c_int, C.c_bool)
        need_sample = fn('_ZN10fdsr_forms11need_sampleERKNS_5FormsEib', Plan, R, C.c_int, C.c_bool)
        need_train = fn('_ZN10fdsr_forms10need_trainERKNS_5FormsEi', Plan, R, C.c_int)
        up2_form = fn('_ZN10fdsr_forms8up2_formERKNS_5FormsEi', C.c_int, R, C.c_int)
        done = fn('_ZN10fdsr_forms4doneERNS_5FormsENS_4PassE', None, R, C.c_uint8)
    return Rec


def _fresh_forms():
    return Forms((C.c_uint8 * 8)(HOST, BEHIND, HOST, HOST, HOST, BEHIND, BEHIND, BEHIND), False)    # Forms{} of fdsr_forms.h


def _wform(prec):
    return F16X3 if prec == F16 else prec


class _Earlier:
    """The six flags and the sites that set and read them, as they stood (line numbers of the files before the record)."""
    FLAGS = ('wt_valid', 'h_forms_stale', 'up2_dev_fresh', 'f32_forms_stale', 'temb_table_valid', 'step_sched_valid')

    def __init__(self, flags=(False,) * 6):
        for k, v in zip(self.FLAGS, flags):
            setattr(self, k, v)

    def key(self):
        return tuple(getattr(self, k) for k in self.FLAGS)

    def repack(self, prec, forward_forms, all_f32, skips, out):      # fdsr_train.cpp:200-278
        lazy = prec == F16X3 and not all_f32
        out.append(('repack', int(forward_forms), int(all_f32), int(lazy)))
        if forward_forms:
            self.up2_dev_fresh = True
            self.h_forms_stale = True
        self.temb_table_valid = False
        self.f32_forms_stale = False if all_f32 else (self.f32_forms_stale or (lazy and skips))

    def sync(self, out):                                              # fdsr_train.cpp:761-777
        if not self.h_forms_stale:
            return
        out.append('SYNC16')
        self.h_forms_stale = False
        self.up2_dev_fresh = False

    def load(self):                                                   # fdsr_engine.cpp:932-937
        self.wt_valid = self.up2_dev_fresh = self.temb_table_valid = False
        return [], True

    def schedule(self):                                               # :955-959
        self.temb_table_valid = self.step_sched_valid = False
        return [], True

    def temb(self, out):                                              # ensure_temb_table
        if not self.temb_table_valid:
            out.append('TEMB_TABLE')
            self.temb_table_valid = True

    def forward(self, prec, training):                                # :982
        out = []
        if prec != F32 and self.h_forms_stale and not training:
            self.sync(out)
        return out, False

    def sample(self, prec, stepwise):                                 # :1002-1004, :1054-1056
        out = []
        if stepwise:
            if prec != F32 and self.h_forms_stale:
                self.sync(out)
            self.temb(out)
            if not self.step_sched_valid:                             # ensure_step_state
                out.append('STEP_SCHED')
                self.step_sched_valid = True
        else:
            self.temb(out)
            if prec != F32 and self.h_forms_stale:
                self.sync(out)
        return out, False

    def train(self, prec, skips):                                     # fdsr_train.cpp:387-393
        out = []
        if prec == F32 and self.f32_forms_stale:
            self.repack(prec, True, True, skips, out)
        if not self.wt_valid:
            self.repack(prec, prec == F16X3, False, skips, out)
            self.wt_valid = True
        return out, False

    def step(self, prec, skips):                                      # fdsr_train.cpp:683-689
        out = []
        self.repack(prec, True, False, skips, out)
        self.wt_valid = True
        self.h_forms_stale = True
        return out, True

    def precision(self, prec, mode, skips):                           # fdsr_engine.cpp:1248-1266
        out = []
        if mode == F32 and self.f32_forms_stale:
            out.append('DEVICE_SYNC')
            self.repack(prec, True, True, skips, out)
            out.append('DEVICE_SYNC')
        if mode != F32 and mode != prec and self.h_forms_stale:
            self.sync(out)
        return out, prec != mode

    def up2(self, prec):                                              # run_unet, :441-447
        up2_dev = _wform(prec) == F16X3 and self.up2_dev_fresh
        if not self.h_forms_stale or up2_dev:
            return 'device scale' if up2_dev else 'host scale'
        return 'generic'

    def reads_behind(self, prec, training):
        """A forward at `prec` reads 16-bit fragments that lag: the bf16 forms have no packer but the host's sync."""
        return prec == BF16 and self.h_forms_stale


def _run(rec, forms, plan):
    """What apply_plan() does with a plan: each pass in order, reported back through done()."""
    names = [PASSES[plan.p[i]] for i in range(plan.n)]
    for i in range(plan.n):
        rec.done(C.byref(forms), plan.p[i])
    return [REPACK.get(n, n) for n in names], bool(plan.drop)


def _events(prec, training, train_ready, has_sched):
    ev = [('load',), ('schedule',), ('forward',), ('sync',), ('training', not training)]
    ev += [('precision', m) for m in (F32, F16X3, BF16, F16)]
    if has_sched:
        ev += [('sample', False), ('sample', True)]
    if prec in (F32, F16X3):
        ev.append(('train',))
    if train_ready:
        ev.append(('step',))
    return ev


def _walk(rec, skips):
    """Breadth-first over (flags, record, precision, training flag, train_ready, schedule set).  Returns the number of states, the
    (state, event) pairs at which the earlier rules read a lagging family, and the reads of a family the record marks behind."""
    start = (_Earlier().key(), bytes(_fresh_forms().st), False, F32, False, False, False)
    seen, queue, holes, behind_reads = {start}, deque([start]), [], []
    while queue:
        state = queue.popleft()
        flags, st, lz, prec, training, train_ready, has_sched = state
        for ev in _events(prec, training, train_ready, has_sched):
            old, new = _Earlier(flags), Forms((C.c_uint8 * 8)(*st), lz)
            p2, tr2, ready2, sched2 = prec, training, train_ready, has_sched
            reads = None                                     # (precision, eval-mode forms needed) of the launch that follows
            if ev[0] == 'load':
                want, got = old.load(), _run(rec, new, rec.on_load(C.byref(new)))
            elif ev[0] == 'schedule':
                want, got, sched2 = old.schedule(), _run(rec, new, rec.on_schedule(C.byref(new))), True
            elif ev[0] == 'training':
                want = got = ([], False)
                tr2 = ev[1]
            elif ev[0] == 'sync':
                out = []
                old.sync(out)
                want, got = (out, False), _run(rec, new, rec.on_sync(C.byref(new)))
            elif ev[0] == 'precision':
                want, got = old.precision(prec, ev[1], skips), _run(rec, new, rec.on_precision(C.byref(new), prec, ev[1]))
                p2 = ev[1]
            elif ev[0] == 'step':
                want, got = old.step(prec, skips), _run(rec, new, rec.on_step(C.byref(new), prec))
            elif ev[0] == 'train':
                if not train_ready:
                    new.lazy_skips, ready2 = skips, True      # prepare_train_forms
                want, got = old.train(prec, skips), _run(rec, new, rec.need_train(C.byref(new), prec))
                reads = (prec, False)
                assert new.st[WT32] != BEHIND and new.st[WT_H3] != BEHIND, (state, ev)
            elif ev[0] == 'forward':
                want, got = old.forward(prec, training), _run(rec, new, rec.need_forward(C.byref(new), prec, training))
                reads = (prec, not training)
            else:
                want, got = old.sample(prec, ev[1]), _run(rec, new, rec.need_sample(C.byref(new), prec, ev[1]))
                reads = (prec, True)
                assert new.st[TEMB] != BEHIND and (not ev[1] or new.st[SCHED] != BEHIND), (state, ev)
            if reads and old.reads_behind(prec, training):
                # the one allowed difference: the record refreshes through the packer eval mode would use
                holes.append((state, ev))
                assert got == (want[0] + ['SYNC16'], want[1]), (state, ev, want, got)
                old.sync([])
            else:
                assert got == want, (state, ev, want, got)
            if reads:
                # no reader sees a family the record marks behind; eval-mode readers see the host's forms
                wf = _wform(reads[0])
                fams = {F32: [FWD32], F16X3: [FWD_H3], BF16: [B16]}[wf]
                if any(new.st[f] in (BEHIND, LAZY) for f in fams) or (reads[1] and wf == F16X3 and (new.st[FWD_H3], new.st[UP2_H3]) != (HOST, HOST)):
                    behind_reads.append((state, ev))
                if wf != F32:
                    up2 = UP2[rec.up2_form(C.byref(new), prec)]
                    assert up2 == old.up2(prec), (state, ev, up2, old.up2(prec))
                    if up2 != 'generic' and new.st[B16 if wf == BF16 else UP2_H3] == BEHIND:
                        behind_reads.append((state, ev))
            nxt = (old.key(), bytes(new.st), bool(new.lazy_skips), p2, tr2, ready2, sched2)
            if nxt not in seen:
                seen.add(nxt)
                queue.append(nxt)
    return len(seen), holes, behind_reads


@pytest.mark.parametrize('skips', [True, False], ids=['f16x3-capable', 'no-16-bit-conv'])
def test_record_agrees_with_the_earlier_rules_in_every_reachable_state(rec, skips):
    n, holes, behind_reads = _walk(rec, skips)
    assert 50 < n < 20000, n
    assert not behind_reads, behind_reads[:4]
    names = ('f32', 'f16x3', 'bf16', 'f16')
    print(f'{n} states; {len(holes)} (state, reader) pairs where the earlier rules read a lagging family:')
    for (flags, st, lz, prec, training, ready, sched), ev in holes:
        print(f'  prec={names[prec]} training={training} flags={dict(zip(_Earlier.FLAGS, flags))} reader={ev}')
    # all of them are the training-mode forward in bf16 after an optimiser step; an engine that can train reaches it
    assert all(s[3] == BF16 and s[4] and ev == ('forward',) for s, ev in holes), holes
    assert holes


def test_restating_the_precision_every_step_costs_no_host_repack(rec):
    """A training loop that calls set_precision('f16x3') before every step: no SYNC16, and after the first step nothing but the
    step's own lazy device pass."""
    f = _fresh_forms()
    passes = []
    for it in range(3):
        passes.append(_run(rec, f, rec.on_precision(C.byref(f), F16X3 if it else F32, F16X3))[0])
        if it == 0:
            f.lazy_skips = True
        passes.append(_run(rec, f, rec.need_train(C.byref(f), F16X3))[0])
        passes.append(_run(rec, f, rec.on_step(C.byref(f), F16X3))[0])
    lazy = REPACK['PACK_STEP_LAZY']
    assert passes == [[], [lazy], [lazy]] + [[], [], [lazy]] * 2, passes
