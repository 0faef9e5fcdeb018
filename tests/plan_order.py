"""TEST INFRASTRUCTURE ONLY: the happens-before model of a two-lane launch plan, serial schedules of it and a one-stream runner.

A train step is one `hipdp.ops.Plan`: a list of `(op, side)` items whose only cross-lane ordering is the `Fork` / `Join` markers the
engine places by hand.  This module models the ordering that `Plan.run` (python mode) and `dpp_plan_run` (csrc/plan.hip) give those
items, and turns it into serial orders of the launches that are all LEGAL under that ordering.  Running the same launches in every
such order, one after the other on one stream, makes a missing fork or join deterministic: a launch that reads what another one
writes without an edge between them sees the other value in one of the orders.

The model (`build_model`), for a sequence of plans run back to back:

  * main launches are a chain;
  * side launches are a chain when side_streams == 1;
  * with side_streams == S > 1 every `Fork` opens group g, whose launches go to stream g % S (a launch recorded before the plan's
    first fork goes to stream 0); every stream is a chain, the streams are not ordered among themselves;
  * a fork makes the stream of its group wait for every main launch recorded before it: a side launch comes after every main launch
    in front of the most recent fork (none if no fork has been recorded on its stream's behalf yet);
  * a join makes main wait for every side launch recorded before it, on every stream;
  * a step that is not a `Launch` (a collective) is a full barrier: after everything before it, before everything behind it;
  * the lanes carry over from one plan to the next: what a plan leaves un-joined (the prefetch of the next minibatch) is only ordered
    by the join that the next plan opens with.  With S > 1 `dpp_plan_run` counts its groups from zero in every call and folds the
    extra streams into stream 0 before it returns; the model does the same at every plan boundary.

Schedules (`schedules`): every one is a topological order of that DAG.  `lane_first(model, lanes)` places the launches of the first
lane of `lanes` as early as their edges allow (each preceded by nothing but its own unplaced ancestors), then those of the second
lane, and so on.  For two launches x, y that the model leaves unordered, a schedule that puts x's lane first runs x before y, one
that puts y's lane first runs y before x (`unopposed_pairs` checks exactly that):

  * `side_first`  = side streams, then main: every side launch as early as possible;
  * `side_last`   = main, then the side streams: every side launch as late as the next join (or the end of the sequence) allows;
  * `side_first_rev` / `side_last_rev` (S > 1 only): the same with the side streams in reverse order;
  * `seeded(k)`: a random topological order.
"""
import random

import numpy as np

from hipdp.ops import Fork, Join, Launch

MAIN = 0            # lane numbers: 0 = main, 1 + s = side stream s


class Model(object):
    """nodes[i] = the i-th launch (or barrier step) in recorded order; lane[i]; preds[i] = set of direct predecessors (all < i);
    plan_of[i] = index of the plan it came from; `anc[i]` = bit set of all ancestors."""

    def __init__(self, side_streams):
        self.side_streams = side_streams
        self.nodes, self.lane, self.preds, self.plan_of, self.barrier = [], [], [], [], []
        self.anc = []

    def __len__(self):
        return len(self.nodes)

    def _add(self, op, lane, preds, plan, barrier=False):
        i = len(self.nodes)
        ps = set(p for p in preds if p is not None)
        assert all(p < i for p in ps)
        self.nodes.append(op)
        self.lane.append(lane)
        self.preds.append(ps)
        self.plan_of.append(plan)
        self.barrier.append(barrier)
        a = 0
        for p in ps:
            a |= self.anc[p] | (1 << p)
        self.anc.append(a)
        return i

    def edges(self):
        """The direct edges as a set of (before, after) pairs."""
        return set((p, i) for i, ps in enumerate(self.preds) for p in ps)

    def ordered(self, a, b):
        """True if the model orders a before b."""
        return bool((self.anc[b] >> a) & 1)

    def reach(self):
        """R[a, b] = a is an ancestor of b, as a boolean matrix."""
        n = len(self)
        R = np.zeros((n, n), bool)
        for b in range(n):
            a, bits = 0, self.anc[b]
            while bits:
                low = bits & -bits
                a = low.bit_length() - 1
                R[a, b] = True
                bits ^= low
        return R

    def unordered_pairs(self):
        """All (a, b), a < b, that the model leaves unordered."""
        R = self.reach()
        free = np.triu(~(R | R.T), 1)
        return [(int(a), int(b)) for a, b in zip(*np.nonzero(free))]

    def names(self, order=None):
        return [getattr(self.nodes[i], 'name', '?') for i in (range(len(self)) if order is None else order)]


def _items(plan):
    return list(plan.ops) if hasattr(plan, 'ops') else list(plan)


def build_model(plans, side_streams=1):
    """plans: one plan or a list of plans run back to back; a plan is a `hipdp.ops.Plan` or a plain list of (op, side) items."""
    if hasattr(plans, 'ops') or (plans and isinstance(plans[0], tuple)):
        plans = [plans]
    S = int(side_streams)
    assert S >= 1
    m = Model(S)
    last_main = None                         # tail of the main chain
    tails = [set() for _ in range(S)]        # per side stream: what its next launch comes after on that stream
    waited = [None] * S                      # per side stream: the main launch its latest fork made it wait for
    joined = set()                           # side launches main has to wait for (the joins since the last main launch)
    for pi, plan in enumerate(plans):
        cur, groups = 0, 0                   # dpp_plan_run counts its groups from zero in every call
        for op, side in _items(plan):
            if isinstance(op, Fork):
                if S > 1:
                    cur = groups % S
                    groups += 1
                waited[cur] = last_main
            elif isinstance(op, Join):
                for t in tails:
                    joined |= t
            elif isinstance(op, Launch) and side:
                tails[cur] = {m._add(op, 1 + cur, sorted(tails[cur]) + [waited[cur]], pi)}
            elif isinstance(op, Launch):
                last_main = m._add(op, MAIN, [last_main] + sorted(joined), pi)
                joined = set()
            else:
                # a collective: issued from the host between two native segments, behind both lanes and in front of both
                allp = [last_main] + sorted(joined) + [x for t in tails for x in t]
                i = m._add(op, MAIN, allp, pi, barrier=True)
                last_main, tails, waited, joined = i, [{i} for _ in range(S)], [i] * S, set()
                cur, groups = 0, 0
        for s in range(1, S):                # ... and folds the extra streams into stream 0 before it returns
            tails[0] |= tails[s]
    return m


# ------------------------------------------------------------------------------------------ schedules
def is_topological(model, order):
    pos = {i: k for k, i in enumerate(order)}
    return len(pos) == len(model) == len(order) and all(pos[p] < pos[i] for i in range(len(model)) for p in model.preds[i])


def recorded(model):
    return list(range(len(model)))


def lane_first(model, lanes):
    """The launches of lanes[0] as early as their edges allow, then those of lanes[1], ...: a launch is preceded by nothing but its own
    unplaced ancestors (in recorded order, which is a topological one).  Barriers belong to the main lane."""
    placed, order = 0, []
    for lane in lanes:
        for i in range(len(model)):
            if model.lane[i] != lane or (placed >> i) & 1:
                continue
            need = (model.anc[i] | (1 << i)) & ~placed
            placed |= need
            while need:
                low = need & -need
                order.append(low.bit_length() - 1)
                need ^= low
    assert len(order) == len(model), "lanes %r do not cover the model" % (lanes,)
    return order


def side_first(model, reverse=False):
    sides = list(range(1, 1 + model.side_streams))
    return lane_first(model, (sides[::-1] if reverse else sides) + [MAIN])


def side_last(model, reverse=False):
    sides = list(range(1, 1 + model.side_streams))
    return lane_first(model, [MAIN] + (sides[::-1] if reverse else sides))


def seeded(model, k):
    """A random topological order: every next launch drawn uniformly from the ones whose predecessors have all run."""
    rng = random.Random(k)
    n = len(model)
    left = [len(ps) for ps in model.preds]
    succ = [[] for _ in range(n)]
    for i, ps in enumerate(model.preds):
        for p in ps:
            succ[p].append(i)
    ready = [i for i in range(n) if left[i] == 0]
    order = []
    while ready:
        i = ready.pop(rng.randrange(len(ready)))
        order.append(i)
        for s in succ[i]:
            left[s] -= 1
            if left[s] == 0:
                ready.append(s)
    assert len(order) == n
    return order


def schedule_names(side_streams, seeds=(0, 1)):
    """The names of the schedule set of a model with that many side streams ('recorded' first)."""
    names = ['recorded', 'side_first', 'side_last']
    if side_streams > 1:
        names += ['side_first_rev', 'side_last_rev']
    return names + ['seeded%d' % k for k in seeds]


def schedule(model, name):
    if name == 'recorded':
        return recorded(model)
    if name in ('side_first', 'side_first_rev'):
        return side_first(model, reverse=name.endswith('_rev'))
    if name in ('side_last', 'side_last_rev'):
        return side_last(model, reverse=name.endswith('_rev'))
    if name.startswith('seeded'):
        return seeded(model, int(name[len('seeded'):]))
    raise KeyError(name)


def schedules(model, seeds=(0, 1)):
    return dict((name, schedule(model, name)) for name in schedule_names(model.side_streams, seeds))


def unopposed_pairs(model, orders):
    """The unordered pairs (a, b) of the model that every order in `orders` runs the same way round: what the schedule set cannot see."""
    R = model.reach()
    free = np.triu(~(R | R.T), 1)
    fwd = np.zeros_like(free)
    bwd = np.zeros_like(free)
    for order in orders:
        pos = np.empty(len(model), np.int64)
        pos[np.asarray(order)] = np.arange(len(order))
        before = pos[:, None] < pos[None, :]
        fwd |= before
        bwd |= ~before
    return [(int(a), int(b)) for a, b in zip(*np.nonzero(free & ~(fwd & bwd)))]


# ------------------------------------------------------------------------------------------ runner
def run_serial(model, order, stream):
    """Issue the launches of `order` one after the other on ONE stream (None: the emulator).  No NativePlan, no second stream."""
    assert is_topological(model, order), "not a legal order of the plan"
    for i in order:
        model.nodes[i](stream)


def without(plan, index):
    """A copy of the plan's item list with item `index` (a Fork or Join marker) removed: a plan with one dependency missing."""
    items = _items(plan)
    assert isinstance(items[index][0], (Fork, Join))
    return items[:index] + items[index + 1:]
