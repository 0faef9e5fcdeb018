"""The two-lane launch plans under every legal order of their lanes.

A train step is one plan of a few hundred launches on two lanes whose only cross-lane ordering is the Fork / Join markers that
hipdp/engine.py and hipdp/backward.py place by hand.  Neither tier of the suite sees a missing marker on its own: the emulator issues
every launch where it was recorded, the GPU only loses the race now and then.  tests/plan_order.py models the ordering the runners
implement and produces serial orders that are all legal under it; here every plan the project builds runs from identical state under
each of them, and everything a later step or the caller reads (parameters, BatchNorm statistics, gradients, ADAM moments, hyper
parameters, cost, output, inputs, counters) must come out bit-identical to the recorded order.

The first part tests the model itself on small synthetic plans with hand-written expected orderings."""
import contextlib
import hashlib

import numpy as np
import pytest

from hipdp import engine, heuristics, ops
from hipdp.ops import Fork, Join, Launch, Plan
from tests import plan_order as po
from tests.backends import BACKENDS, get_runtime


# ====================================================================================== the model on synthetic plans
def L(name, fn=None):
    """A "launch" that is a Python callable (on numpy arrays)."""
    def call(stream):
        if fn is not None:
            fn()
        return 0
    return Launch(call, (), (), name)


def closure(model):
    """All ordered pairs (before, after) of the model."""
    n = len(model)
    return set((a, b) for a in range(n) for b in range(n) if model.ordered(a, b))


def items(spec):
    """'m' main launch, 's' side launch, 'F' fork, 'J' join, 'C' a step that is not a launch (a collective)."""
    out = []
    for k, c in enumerate(spec):
        if c == 'F':
            out.append((Fork(), False))
        elif c == 'J':
            out.append((Join(), False))
        elif c == 'C':
            out.append((lambda stream: None, False))
        else:
            out.append((L('%s%d' % (c, k)), c == 's'))
    return out


def test_model_fork_without_join():
    m = po.build_model(items('mFsmsm'))                    # nodes: 0 m, 1 s, 2 m, 3 s, 4 m
    assert m.lane == [0, 1, 0, 1, 0]
    assert closure(m) == {(0, 1), (0, 2), (0, 3), (0, 4), (1, 3), (2, 4)}
    assert set(m.unordered_pairs()) == {(1, 2), (1, 4), (2, 3), (3, 4)}
    # (the second side launch is behind the ONLY fork: it does not wait for the main launch recorded after that fork)
    assert m.edges() == {(0, 1), (0, 2), (1, 3), (0, 3), (2, 4)}


def test_model_join_with_nothing_pending():
    m = po.build_model(items('mJmFsm'))                    # nodes: 0 m, 1 m, 2 s, 3 m
    assert closure(m) == {(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)}
    assert set(m.unordered_pairs()) == {(2, 3)}
    assert m.edges() == {(0, 1), (1, 2), (1, 3)}


def test_model_side_launch_behind_a_join_without_a_new_fork():
    m = po.build_model(items('mFsmJmsmJm'))                # nodes: 0 m, 1 s, 2 m, 3 m, 4 s, 5 m, 6 m
    assert m.lane == [0, 1, 0, 0, 1, 0, 0]
    want = {(0, b) for b in range(1, 7)} | {(1, 3), (1, 4), (1, 5), (1, 6), (2, 3), (2, 5), (2, 6), (3, 5), (3, 6), (4, 6), (5, 6)}
    assert closure(m) == want
    # the trap: side launch 4 was added after the join, but its lane last waited for main at the fork in front of launch 1
    assert set(m.unordered_pairs()) == {(1, 2), (2, 4), (3, 4), (4, 5)}


def test_model_two_plans_back_to_back():
    a, b = items('mFs'), items('JmsFsm')                   # nodes: 0 m, 1 s | 2 m, 3 s, 4 s, 5 m
    m = po.build_model([a, b])
    assert m.plan_of == [0, 0, 1, 1, 1, 1]
    want = {(0, x) for x in range(1, 6)} | {(1, 2), (1, 3), (1, 4), (1, 5), (2, 4), (2, 5), (3, 4)}
    assert closure(m) == want
    assert set(m.unordered_pairs()) == {(2, 3), (3, 5), (4, 5)}
    # the first plan alone leaves its side launch un-joined: only the second plan's opening join orders it
    alone = po.build_model(a + [x for x in b if not isinstance(x[0], Join)])
    assert not alone.ordered(1, 2) and m.ordered(1, 2)


def test_model_two_side_streams():
    spec = 'mFssmFsmFsJm'                                  # nodes: 0 m, 1 s, 2 s, 3 m, 4 s, 5 m, 6 s, 7 m
    m = po.build_model(items(spec), side_streams=2)
    assert m.lane == [0, 1, 1, 0, 2, 0, 1, 0]              # groups 0 and 2 on stream 0, group 1 on stream 1
    want = {(0, x) for x in range(1, 8)} | {(1, 2), (1, 6), (1, 7), (2, 6), (2, 7), (3, 4), (3, 5), (3, 6), (3, 7), (4, 7), (5, 6), (5, 7), (6, 7)}
    assert closure(m) == want
    assert set(m.unordered_pairs()) == {(1, 3), (1, 4), (1, 5), (2, 3), (2, 4), (2, 5), (4, 5), (4, 6)}
    one = po.build_model(items(spec), side_streams=1)     # one side stream: the three groups are a chain
    assert closure(one) == want | {(1, 4), (2, 4), (4, 6)}
    assert set(one.unordered_pairs()) == {(1, 3), (1, 5), (2, 3), (2, 5), (4, 5)}


def test_model_two_side_streams_over_two_plans():
    m = po.build_model([items('mFsFs'), items('FsmJm')], side_streams=2)        # nodes: 0 m, 1 s, 2 s | 3 s, 4 m, 5 m
    assert m.lane == [0, 1, 2, 1, 0, 0]                   # every plan counts its groups from zero
    # the runner folds stream 1 into stream 0 when a plan ends: launch 3 is behind launch 2 although they are on different streams
    want = {(0, x) for x in range(1, 6)} | {(1, 3), (1, 5), (2, 3), (2, 5), (3, 5), (4, 5)}
    assert closure(m) == want
    assert set(m.unordered_pairs()) == {(1, 2), (1, 4), (2, 4), (3, 4)}


def test_model_collective_is_a_barrier():
    m = po.build_model(items('mFsCsm'), side_streams=2)    # nodes: 0 m, 1 s, 2 C, 3 s, 4 m
    assert m.barrier == [False, False, True, False, False]
    assert closure(m) == {(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3), (0, 4), (1, 4), (2, 4)}
    assert set(m.unordered_pairs()) == {(3, 4)}


@pytest.mark.parametrize('S', [1, 2, 3])
def test_schedules_are_legal_and_oppose_every_unordered_pair(S):
    rng = np.random.RandomState(S)
    for trial in range(20):
        spec = 'm' + ''.join(rng.choice(list('mmmsssFFJ')) for _ in range(30))
        plans = [items(spec[:17]), items(spec[17:])]
        m = po.build_model(plans, side_streams=S)
        sch = po.schedules(m)
        assert list(sch) == po.schedule_names(S)
        for name, order in sch.items():
            assert po.is_topological(m, order), (spec, name)
        assert sch['recorded'] == list(range(len(m)))
        if S == 1:
            # one side lane: side_first and side_last alone run every unordered pair both ways round
            assert po.unopposed_pairs(m, [sch['side_first'], sch['side_last']]) == [], spec
        else:
            lanes = [po.lane_first(m, [l] + [k for k in range(S + 1) if k != l]) for l in range(S + 1)]
            assert po.unopposed_pairs(m, lanes) == [], spec
            if S == 2:
                four = [sch[k] for k in ('side_first', 'side_first_rev', 'side_last', 'side_last_rev')]
                assert po.unopposed_pairs(m, four) == [], spec
    assert not po.is_topological(m, list(reversed(range(len(m)))))


def synthetic_race(joined):
    """main: a = 1 | fork | side: b = 2 a | (join) | main: a = 5 | join | main: c = a + b.  Without the first join the side launch
    reads `a` while main overwrites it."""
    a, b, c = np.zeros(1), np.zeros(1), np.zeros(1)

    def set_a(v):
        def f():
            a[0] = v
        return f

    def set_b():
        b[0] = 2 * a[0]

    def set_c():
        c[0] = a[0] + b[0]
    plan = [(L('a=1', set_a(1)), False), (Fork(), False), (L('b=2a', set_b), True)] + ([(Join(), False)] if joined else []) + \
           [(L('a=5', set_a(5)), False), (Join(), False), (L('c=a+b', set_c), False)]
    return plan, c


def test_runner_shows_a_missing_join_and_nothing_else():
    for joined in (True, False):
        got = {}
        for name in po.schedule_names(1):
            plan, c = synthetic_race(joined)
            m = po.build_model(plan)
            po.run_serial(m, po.schedule(m, name), None)
            got[name] = float(c[0])
        if joined:
            assert set(got.values()) == {7.0}, got
        else:
            assert got['recorded'] == got['side_first'] == 7.0 and got['side_last'] == 15.0, got
    plan, _ = synthetic_race(True)
    m = po.build_model(plan)
    with pytest.raises(AssertionError):
        po.run_serial(m, [3, 0, 1, 2], None)               # not an order the plan allows
    assert len(po.build_model(po.without(plan, 3))) == len(m)
    with pytest.raises(AssertionError):
        po.without(plan, 0)                                 # only markers are dependencies


# ====================================================================================== the plans the project builds
@contextlib.contextmanager
def patched(obj, **values):
    """setattr for the duration of a build (the compiled engines are cached across tests, so pytest's monkeypatch, which is undone
    per test, only serves the test that happens to build)."""
    old = dict((k, getattr(obj, k)) for k in values)
    try:
        for k, v in values.items():
            setattr(obj, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


class Memory(object):
    """Every device buffer allocated while an engine and its plans were built, with the bytes they held before the first run.
    Restoring ALL of it between schedules -- not only the parameters, moments and counters -- matters: an intermediate tensor that
    still holds the previous run's value would hand a launch that runs too early exactly the value it was meant to wait for."""

    def __init__(self, rt):
        self.rt, self.bufs, self.saved = rt, [], None

    def __enter__(self):
        orig = self.rt.alloc

        def alloc(*a, **k):
            b = orig(*a, **k)
            self.bufs.append(b)
            return b
        self.rt.alloc = alloc
        return self

    def __exit__(self, *exc):
        del self.rt.alloc

    def _raw(self, b):
        return self.rt._arr(b) if self.rt.is_emulator else self.rt._tensor(b)

    def snapshot(self):
        self.rt.synchronize()
        self.saved = [self._raw(b).copy() if self.rt.is_emulator else self._raw(b).clone() for b in self.bufs]

    def restore(self):
        self.rt.synchronize()
        for b, s in zip(self.bufs, self.saved):
            if self.rt.is_emulator:
                self._raw(b)[:] = s
            else:
                self._raw(b).copy_(s)
        self.rt.synchronize()


class Case(object):
    """One compiled configuration: the engine, the plans of its sequence (run back to back), the buffers that are live-out and a
    cache of the live-out state per (side streams, schedule)."""

    def __init__(self, rt, mem, eng, plans, extra=()):
        self.rt, self.mem, self.eng, self.plans = rt, mem, eng, plans
        st = eng.store
        self.live = dict(w=st.w, nt=st.nt, g=st.g, m=st.m, v=st.v, hyper=eng.hyper, cost=eng.cost, out=eng.out.buf, y_in=eng.y_in)
        for k, t in enumerate(eng.x_ins):
            self.live['x_in%d' % k] = t.buf
        if eng.step_ctr is not None:
            self.live['dropout_counter'] = eng.step_ctr
        for name, buf in extra:
            self.live[name] = buf
        self.models, self.results = {}, {}
        mem.snapshot()

    def model(self, S, plans=None):
        if plans is not None:
            return po.build_model(plans, side_streams=S)
        if S not in self.models:
            self.models[S] = po.build_model(self.plans, side_streams=S)
        return self.models[S]

    def state(self):
        """name -> (digest of the bytes, all values finite) of every live-out buffer (digests: a worker keeps ~100 of these states)."""
        self.rt.synchronize()
        out = {}
        for k, b in self.live.items():
            a = b.get()
            out[k] = (hashlib.sha1(a.tobytes()).hexdigest(), bool(np.isfinite(a).all()) if a.dtype.kind == 'f' else True)
        return out

    def run(self, model, order):
        self.mem.restore()
        po.run_serial(model, order, self.rt.stream)
        return self.state()

    def result(self, S, name):
        if name == 'recorded':
            S = 1                                            # the recorded order does not depend on the model
        if (S, name) not in self.results:
            m = self.model(S)
            order = tuple(po.schedule(m, name))
            if order not in self.results:                    # (two schedules may come out as the same order)
                self.results[order] = self.run(m, order)
            self.results[(S, name)] = self.results[order]
        return self.results[(S, name)]


def differing(a, b):
    """Names of the live-out buffers whose bytes differ."""
    assert sorted(a) == sorted(b)
    return sorted(k for k in a if a[k] != b[k])


B, SIZE = 2, 32
WD = 1e-3
FC1_SMALL = dict(EARLY_BUCKET_MIN=1 << 18)                  # the 32x32 net's FC1 (1 M weights) counts as "the big one"


def resnet(type_=0):
    from net.resnet import ResNet, ResNetParams
    nJ, nD = (1, 30) if type_ == 0 else (14, 3)
    return ResNet(np.random.RandomState(23455), cfgParams=ResNetParams(type=type_, nChan=1, wIn=SIZE, hIn=SIZE, batchSize=B, numJoints=nJ,
                                                                       nDims=nD))


def feed(eng, seed=5):
    from oracle import nets
    r = np.random.RandomState(seed)
    N = eng.N
    shapes = [(t.shape[1], t.shape[2]) for t in eng.x_ins]
    x = nets.synthetic_crops(r, N, shapes[0][0], shapes[0][1], np.float32)
    eng.set_input(x if len(shapes) == 1 else nets.scalenet_inputs(x))
    eng.y_in.set(r.normal(0, 0.3, (N, eng.out_dim)).astype(np.float32))
    eng.set_lr(1e-3)


def augmentation(rt, eng, out_x, out_y, nsl=2):
    """The device augmentation plans of bench.py: one fused launch per data slice that draws from a device-resident counter and
    writes a minibatch into out_x / out_y.  Returns (plans, [(name, buffer)] of the draw counter and its ticket word)."""
    from hipdp.augmenter import camera_tuple
    from tools import synth
    J = 14
    di, imgs, coms, cubes, Ms, gts, pca_mean, pca_comp = synth.crop_db(nsl * B, SIZE, J, seed=23455)
    f32 = lambda a: rt.upload(np.ascontiguousarray(a, np.float32))       # noqa: E731
    db = dict(img=f32(imgs), com=f32(coms), cube=f32(cubes), M=f32(Ms.reshape(nsl * B, 9)), gt=f32(gts))
    pm, pc = f32(pca_mean), f32(pca_comp)
    table = rt.upload(np.array([1, 2, 0], np.int32))
    aug = ops.AugmentState(rt, B, seed=1234, sample0=0, global_batch=B)
    plans = []
    for sl in range(nsl):
        o = sl * B
        p = Plan('augment')
        for op in aug.ops(db['img'].view(o * SIZE * SIZE, (B, SIZE, SIZE)), db['com'].view(o * 3, (B, 3)), db['cube'].view(o * 3, (B, 3)),
                          db['M'].view(o * 9, (B, 9)), db['gt'].view(o * J * 3, (B, J, 3)), J, SIZE, camera_tuple(di), out_x, out_y,
                          mode_table=table, n_modes=3, pca_mean=pm, pca_comp=pc, E=30):
            p.add(op)
        plans.append(p)
    return plans, [('augment_counter', aug.counter), ('augment_ticket', aug.ticket)]


def build_default(rt, bf16=False, steps=2, type_=0, wd=WD):
    eng = engine.CompiledNet(resnet(type_), train=True, runtime=rt, loss=dict(kind='embedding'), weight_decay=wd, bf16=bf16)
    feed(eng)
    return eng, [eng.step_plan()] * steps, ()


def build_pipelined(rt, mode):
    """mode: before | prefetch | prefetch_early (a prefix: 'prefetch_stem_side' is 'prefetch' under another patch)."""
    mode = 'prefetch' if mode == 'prefetch_stem_side' else mode
    eng = engine.CompiledNet(resnet(), train=True, runtime=rt, loss=dict(kind='embedding'), weight_decay=WD)
    x_out = eng.x_in.buf.reshape(B, SIZE, SIZE)
    feed(eng)
    if mode == 'before':
        aug, extra = augmentation(rt, eng, x_out, eng.y_in)
        return eng, [eng.step_plan(before=aug[0]), eng.step_plan(before=aug[1])], extra
    if mode == 'prefetch':
        aug, extra = augmentation(rt, eng, x_out, eng.y_in)
        aug[0].run(rt)                                       # the minibatch of the first step
        return eng, [eng.step_plan(prefetch=aug[1]), eng.step_plan(prefetch=aug[0])], extra
    # the cascade's wiring: the next minibatch is produced into staging buffers BESIDE the forward pass (early=) and only copied into
    # x_in / y_in under the ADAM update (prefetch=)
    x_stage, y_stage = rt.alloc((B, SIZE, SIZE), zero=False), rt.alloc((B, 30), zero=False)
    aug, extra = augmentation(rt, eng, x_stage, y_stage)
    copy = Plan('stage_to_input')
    n = SIZE * SIZE
    copy.add(ops.copy2d(rt, x_stage.reshape(B * n), n, x_out.reshape(B * n), n, B, n, name='load_crops'))
    copy.add(ops.copy2d(rt, y_stage.reshape(B * 30), 30, eng.y_in.reshape(B * 30), 30, B, 30, name='load_labels'))
    aug[0].run(rt)
    copy.run(rt)
    return eng, [eng.step_plan(prefetch=copy, early=aug[1]), eng.step_plan(prefetch=copy, early=aug[0])], \
        extra + [('x_stage', x_stage), ('y_stage', y_stage)]


def build_poseregnet(rt):
    from net.poseregnet import PoseRegNet, PoseRegNetParams
    net = PoseRegNet(np.random.RandomState(23455), cfgParams=PoseRegNetParams(type=0, wIn=128, hIn=128, batchSize=B, numJoints=1, nDims=30))
    eng = engine.CompiledNet(net, train=True, runtime=rt, loss=dict(kind='embedding'))
    feed(eng)
    return eng, [eng.step_plan()], ()


def build_scalenet(rt):
    from hipdp import runtime as R
    from net.scalenet import ScaleNet, ScaleNetParams
    R.set_default_runtime(rt)
    net = ScaleNet(np.random.RandomState(23455), cfgParams=ScaleNetParams(type=1, batchSize=B, numJoints=1, nDims=3, shared_conv=True))
    eng = engine.CompiledNet(net, train=True, runtime=rt, loss=dict(kind='embedding'))
    feed(eng)
    return eng, [eng.step_plan()], ()


def stem_wgrad_on_the_side():
    knob = heuristics.knob
    return patched(heuristics, knob=lambda name, default: '1' if name == 'DPP_STEM_WGRAD_SIDE' else knob(name, default))


# name -> (patches of hipdp.heuristics while the engine and its plans are built, builder)
CONFIGS = {
    'default_f32': (lambda: patched(heuristics), lambda rt: build_default(rt)),
    'default_bf16': (lambda: patched(heuristics, FC1_MIN_K=512), lambda rt: build_default(rt, bf16=True)),
    'before': (lambda: patched(heuristics), lambda rt: build_pipelined(rt, 'before')),
    'prefetch': (lambda: patched(heuristics), lambda rt: build_pipelined(rt, 'prefetch')),
    'prefetch_early': (lambda: patched(heuristics), lambda rt: build_pipelined(rt, 'prefetch_early')),
    # the prefetch writes x_in, the stem's filter gradient reads it: both on the gradient branch here
    'prefetch_stem_side': (stem_wgrad_on_the_side, lambda rt: build_pipelined(rt, 'prefetch_stem_side')),
    'early_adam': (lambda: patched(heuristics, EARLY_ADAM=True, **FC1_SMALL), lambda rt: build_default(rt)),
    'tail_reduce': (lambda: patched(heuristics, TAIL_REDUCE=True), lambda rt: build_default(rt, steps=1)),
    'early_reduce': (lambda: patched(heuristics, EARLY_REDUCE_BYTES=1 << 14), lambda rt: build_default(rt, steps=1)),
    'stem_wgrad_side': (stem_wgrad_on_the_side, lambda rt: build_default(rt, steps=1)),
    'fc1_defer': (lambda: patched(heuristics, FC1_WGRAD_DEFER=4, FC1_MIN_K=512, FC1_STREAM='1', **FC1_SMALL), lambda rt: build_default(rt, steps=1)),
    'type3_dropout': (lambda: patched(heuristics), lambda rt: build_default(rt, type_=3, wd=0.0)),
    'poseregnet': (lambda: patched(heuristics), build_poseregnet),
    'scalenet_shared': (lambda: patched(heuristics), build_scalenet),
}
# configurations that hipdp.engine refuses to build for more than one side stream (their gradient-branch launches read what an
# EARLIER group of the branch wrote, and groups on different streams are not ordered): see test_two_side_streams_refuse_...
ONE_SIDE_STREAM_ONLY = ('early_adam', 'tail_reduce', 'early_reduce')

_cases = {}


def get_case(backend, config):
    key = (backend, config)
    if key not in _cases:
        rt = get_runtime(backend)
        patch, build = CONFIGS[config]
        with Memory(rt) as mem, patch():
            eng, plans, extra = build(rt)
            for p in plans:
                assert isinstance(p, Plan)
        _cases[key] = Case(rt, mem, eng, plans, extra)
    return _cases[key]


SEEDS = {1: (0, 1), 2: (0,)}                                 # random orders per number of side streams
CASES = [(c, S, name) for c in CONFIGS for S in (1, 2) for name in po.schedule_names(S, SEEDS[S])[1:]
         if not (S == 2 and c in ONE_SIDE_STREAM_ONLY) and not (S == 1 and c == 'prefetch_stem_side')]  # (S = 1: each knob alone)


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('config,S,sched', CASES, ids=['%s-S%d-%s' % c for c in CASES])
def test_live_out_state_does_not_depend_on_the_order_of_the_lanes(backend, config, S, sched):
    case = get_case(backend, config)
    want = case.result(1, 'recorded')
    assert all(want[k][1] for k in ('w', 'nt', 'g', 'm', 'v', 'cost', 'out')), "the recorded order itself went wrong"
    m = case.model(S)
    order = po.schedule(m, sched)
    if sched == 'side_last' or (S > 1 and sched.startswith('side_')):
        # the schedule really moves launches.  (Not asserted for side_first on ONE side stream: the engine records every side launch
        # directly behind its fork, so there the recorded order already IS the side-first order -- and side_last is its opposite.)
        assert order != po.recorded(m)
    got = case.result(S, sched)
    bad = differing(want, got)
    if bad:
        pos = dict((i, k) for k, i in enumerate(order))
        flipped = [(m.names([a])[0], m.names([b])[0]) for a, b in m.unordered_pairs() if pos[a] > pos[b]]
        pytest.fail("%s differ from the recorded order under %s (S = %d); %d unordered pairs run the other way round, e.g. %r"
                    % (bad, sched, S, len(flipped), flipped[:12]))


def test_configurations_contain_what_they_are_named_after():
    """(emulator only: this is about the plans, not about a backend)"""
    def names(c, side=None):
        return [getattr(o, 'name', '') for p in get_case('emu', c).plans[:1] for o, s in p.ops if side is None or s == side]
    assert sum(n.startswith('conv1x1') for n in names('default_f32', True)) == 3          # projection shortcuts beside the chain
    assert 'axpy_multi' in names('default_f32', False) and 'sumsq_multi' in names('default_f32', False)       # weight decay
    assert get_case('emu', 'default_bf16').eng.store16
    assert names('before')[0] == 'augment' and names('before', True).count('augment') == 0
    p = get_case('emu', 'prefetch').plans[0].ops
    assert isinstance(p[0][0], Join) and names('prefetch', True)[-1] == 'augment' and names('prefetch', False)[-1] == 'adam'
    pe = names('prefetch_early', True)
    assert pe[0] == 'augment' and pe[-2:] == ['load_crops', 'load_labels'] and not any(n.startswith('conv1x1') for n in pe)
    assert 'adam_fc1' in names('early_adam', True) and names('early_adam', False).count('adam') == 2
    assert 'reduce_multi_side' in names('tail_reduce', True) and names('early_reduce', True).count('reduce_multi_early') >= 3
    for c in ('stem_wgrad_side', 'prefetch_stem_side'):
        assert 'stem_wgrad' in names(c, True) and 'stem_wgrad' in names('default_f32', False)
    eng = get_case('emu', 'fc1_defer').eng
    side = [o for o, s in eng.bwd.ops if s and isinstance(o, Launch)]
    assert eng._fc1_wgrad_op is not None and side.index(eng._fc1_wgrad_op) >= 4, "FC1's filter gradient was not moved down the branch"
    assert 'bernoulli_mask' in names('type3_dropout', False) and 'dropout_counter' in get_case('emu', 'type3_dropout').live
    assert any(n.startswith('convpool_wgrad') for n in names('poseregnet', True))
    assert get_case('emu', 'scalenet_shared').eng.__dict__.get('_shared_grad_adds') and 'axpy' in names('scalenet_shared', False)


# ------------------------------------------------------------------------------------------ sensitivity
def step_parts(eng, plan):
    """Index ranges of the forward and the backward part of a default step plan."""
    ops_ = [o for o, _ in plan.ops]
    f0, f1 = ops_.index(eng.fwd.ops[0][0]), ops_.index(eng.fwd.ops[-1][0])
    b0, b1 = ops_.index(eng.bwd.ops[0][0]), ops_.index(eng.bwd.ops[-1][0])
    return (f0, f1), (b0, b1)


@pytest.mark.parametrize('backend', BACKENDS)
def test_default_step_really_has_unordered_launches_and_the_schedules_oppose_them(backend):
    case = get_case(backend, 'default_f32')
    eng = case.eng
    assert [sum(isinstance(o, Launch) for o, _ in p.ops) for p in case.plans] == [len(case.plans[0])] * 2
    for S in (1, 2):
        m = case.model(S)
        sch = po.schedules(m)
        for name, order in sch.items():
            assert po.is_topological(m, order)
        assert sch['side_last'] != sch['recorded'] and sch['side_first'] != sch['side_last']
        moved = sum(a != b for a, b in zip(sch['side_last'], sch['recorded']))
        assert moved > len(m) // 2, moved                    # most of the step runs at another position
        if S == 1:
            # every side launch of the default step is recorded directly behind its fork: the recorded order is the side-first one
            # (so `recorded` and `side_last` are the two opposite extremes); with two side streams side_first moves launches too
            assert sch['side_first'] == sch['recorded']
        else:
            assert sch['side_first'] != sch['recorded'] and sch['side_first_rev'] != sch['side_first']
        free = m.unordered_pairs()
        fwd = set(id(o) for o in eng.fwd.launches())
        bwd = set(id(o) for o in eng.bwd.launches())
        cross = [(a, b) for a, b in free if (m.lane[a] == 0) != (m.lane[b] == 0)]
        assert any(id(m.nodes[a]) in fwd and id(m.nodes[b]) in fwd for a, b in cross)       # projection shortcuts beside the chain
        assert any(id(m.nodes[a]) in bwd and id(m.nodes[b]) in bwd for a, b in cross)       # filter gradients beside the data gradients
        if S == 1:
            assert po.unopposed_pairs(m, [sch['side_first'], sch['side_last']]) == []
        else:
            assert any(m.lane[a] != m.lane[b] and m.lane[a] and m.lane[b] for a, b in free)     # two side streams: side / side pairs too
            assert po.unopposed_pairs(m, [sch[k] for k in ('side_first', 'side_first_rev', 'side_last', 'side_last_rev')]) == []


def mutations(eng, plan):
    """Copies of a default step plan with ONE dependency removed."""
    ops_ = [o for o, _ in plan.ops]
    final = [i for i, o in enumerate(ops_) if getattr(o, 'name', '') == 'reduce_multi'][-1]
    join = max(i for i in range(final) if isinstance(ops_[i], Join))
    assert all(not isinstance(o, (Launch, Fork)) for o in ops_[join + 1:final])
    first_side = [i for i, (o, side) in enumerate(plan.ops) if side and any(o is b for b, _ in eng.bwd.ops)][0]
    fork = max(i for i in range(first_side) if isinstance(ops_[i], Fork))
    return {'join_before_final_reduce': po.without(plan, join), 'fork_before_first_wgrad': po.without(plan, fork)}


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('mutation', ['join_before_final_reduce', 'fork_before_first_wgrad'])
def test_a_removed_dependency_shows_in_some_schedule(backend, mutation):
    """The schedule set has teeth: with the join in front of the final reduce_multi removed (the reduction may then run before the
    filter gradients it sums), or the fork in front of the first filter-gradient group (which may then run before the data it
    reads exists), at least one schedule leaves other parameters than the recorded order does."""
    case = get_case(backend, 'default_f32')
    plan = case.plans[0]
    broken = mutations(case.eng, plan)[mutation]
    assert len(broken) == len(plan.ops) - 1
    whole, m = case.model(1, [plan]), case.model(1, [broken])              # (one step is enough here)
    # the same launches in the same recorded order -- the recorded order cannot show the fault -- but fewer edges
    assert len(m) == len(whole) and all(a is b for a, b in zip(m.nodes, whole.nodes))
    assert closure_size(m) < closure_size(whole)
    want = case.run(whole, po.recorded(whole))
    shown = []
    for name in ('side_last', 'side_first'):
        order = po.schedule(m, name)
        if order != po.recorded(m) and differing(want, case.run(m, order)):
            shown.append(name)
            break
    assert shown, "no schedule shows the missing dependency"


def closure_size(model):
    return sum(bin(a).count('1') for a in model.anc)


# ------------------------------------------------------------------------------------------ two side streams: refused combinations
@pytest.mark.parametrize('config', ONE_SIDE_STREAM_ONLY)
def test_two_side_streams_refuse_the_knobs_whose_groups_depend_on_each_other(config):
    """DPP_SIDE_STREAMS > 1 deals the groups of the gradient branch to streams that are not ordered against each other.  The early FC1
    update reads the gradient an earlier group wrote, reduce_multi_side / reduce_multi_early sum the partials of earlier groups: the
    engine refuses to build those plans for more than one side stream instead of letting them race."""
    rt = get_runtime('emu')
    patch, build = CONFIGS[config]
    with patch(), patched(ops, SIDE_STREAMS=2):
        with pytest.raises(NotImplementedError, match='DPP_SIDE_STREAMS'):
            eng, plans, _ = build(rt)
    # why: in the plan built for one side stream, the two-stream model leaves producer and consumer unordered
    case = get_case('emu', config)
    m = case.model(2)
    names = m.names()
    consumer = {'early_adam': 'adam_fc1', 'tail_reduce': 'reduce_multi_side', 'early_reduce': 'reduce_multi_early'}[config]
    c = names.index(consumer)
    producers = [i for i in range(c) if m.lane[i] and m.lane[i] != m.lane[c] and not m.ordered(i, c)
                 and (names[i].startswith('fc_wgrad') if config == 'early_adam' else 'wgrad' in names[i])]
    assert producers, "no unordered producer in front of %s" % consumer
    assert all(case.model(1).ordered(i, c) for i in producers)


# ------------------------------------------------------------------------------------------ the real two-stream runner
@pytest.mark.gpu
@pytest.mark.parametrize('config', ['default_f32', 'prefetch', 'prefetch_early'])
def test_native_two_stream_runner_equals_the_recorded_serial_order(config):
    """Two steps through dpp_plan_run on the two HIP streams (events for fork / join) against the same launches issued serially in
    recorded order: the event plumbing of the native runner implements at least the ordering of the model."""
    case = get_case('hip', config)
    rt = case.rt
    assert rt.has_side_stream and ops.LAUNCH_MODE == 'native'
    want = case.result(1, 'recorded')
    case.mem.restore()
    for p in case.plans:
        p.run(rt)
    got = case.state()                                       # (synchronises the device: the last prefetch is left un-joined)
    assert differing(want, got) == []
