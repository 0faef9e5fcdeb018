"""TEST INFRASTRUCTURE ONLY: fingerprints of the realtime tracking plans, pinned in tests/golden/track_plans.json.

A plan is a list of prepared launches, each a C symbol and an argument tuple: what the device does in a tick is decided by exactly
that.  `fingerprints(rt, backend)` builds the plans of HandTracker, MultiTracker (one camera for all sources and unlike sources; both
input slots; with and without a sensor; with and without groups), FrameDetector (one hand and two hands of a source) and the
refinement stage as HandDetector.track builds it, and reduces every launch to

    [launch name, C symbol name, normalised arguments]              (refine_stage: + the `side` flag of the (op, side) pair)

The symbol is found by identity against the runtime's library over lib.SIGNATURES.  In the arguments every pointer is replaced by a
label: '<buffer>+<byte offset>' where it falls inside one of the owning object's named buffers (a tracker's frames, raw frames,
partials, records, cubes, result block, index arrays, source table, rig arrays, the nets' input and output buffers; 'det.<buffer>' for
what a detector owns itself), else 'ext#k', numbered by first appearance in the plan.  Floats are written with repr, a ctypes
argument (a net's descriptor struct) as its type name.  Only plan().launches(), Launch.fn / .args / .name and buffer attributes are
used, so the module runs on any commit that has these classes: the golden file was written at the commit BEFORE the Python ops were
folded to one per launch, and tests/test_track_plans.py requires the working tree to build the same launches.

The two backends build different nets (tests.test_multitrack._nets: a small PoseRegNet on the emulator, the ResNet on the GPU), so
the nets' own launches differ and the file has one section per backend.

    python -m tests.track_plan_fingerprint --write [--backend emu|hip]        rewrite that backend's section of the golden file
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'deep-prior-pp_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'track_plans.json')
SENSOR = dict(dtype='uint16', median=True, mirror=True)
TRACKS = [(0, False), (0, True), (1, False)]
CUBE = (250., 250., 250.)


def _regions(owner, prefix=''):
    """(label, first byte, one past the last byte) of the named buffers of a tracker or a detector, in matching order."""
    found = []

    def add(label, buf):
        if isinstance(buf, (list, tuple)):
            for k, b in enumerate(buf):
                add('%s[%d]' % (label, k), b)
        elif buf is not None:
            found.append((prefix + label, buf.ptr, buf.ptr + buf.nbytes))
    for label, attr in (('frames', 'frames'), ('raw', 'raw'), ('inputs2', '_inputs2'), ('partial', 'partial'), ('rec', 'rec'),
                        ('cube', 'cube'), ('res', 'res'), ('com', 'com'), ('src', 'src'), ('gate', 'gate'), ('tflags', 'tflags'),
                        ('gate2', '_gate2')):
        add(label, getattr(owner, attr, None))
    table, rig = getattr(owner, 'table', None), getattr(owner, 'rig', None)
    if table is not None:
        add('table.dev', table.dev)
    if rig is not None:
        for k in ('extr', 'members', 'offsets'):
            add('rig.' + k, getattr(rig, k))
    for name in ('ceng', 'peng'):
        eng = getattr(owner, name, None)
        if eng is not None:
            add(name + '.x_ins', [t.buf for t in eng.x_ins])
            add(name + '.out', eng.out.buf)
    return found


def _symbol(rt, fn):
    from hipdp import lib
    for name in lib.SIGNATURES:
        if getattr(rt.lib, name) is fn:
            return name
    raise KeyError("launch calls a function that is no symbol of lib.SIGNATURES: %r" % (fn,))


def reduce_launches(rt, launches, regions, sides=None):
    ext, out = {}, []

    def norm(v):
        if isinstance(v, bool) or v is None or isinstance(v, str):
            return v
        if isinstance(v, int):
            for label, lo, hi in regions:
                if lo <= v < hi:
                    return '%s+%d' % (label, v - lo)
            if v >= 1 << 32:                                           # a pointer into nobody's named buffer
                return 'ext#%d' % ext.setdefault(v, len(ext))
            return v
        if isinstance(v, float):
            return repr(v)
        return type(v).__name__
    for i, l in enumerate(launches):
        row = [l.name, _symbol(rt, l.fn), [norm(v) for v in l.args]]
        if sides is not None:
            row.append(bool(sides[i]))
        out.append(row)
    return out


def fingerprints(rt, backend):
    """{case: reduced launches} of every pinned plan on runtime `rt`."""
    import numpy as np

    from data.importers import ICVLImporter, MSRA15Importer
    from hipdp import ops, tracker
    from hipdp import runtime as R
    from hipdp.augmenter import camera_tuple
    from hipdp.multitrack import MultiTracker
    from hipdp.tracker import HandTracker
    from tests.test_multitrack import _nets
    R.set_default_runtime(rt)
    icvl, msra = ICVLImporter('../data/ICVL/'), MSRA15Importer('../data/MSRA15/')
    H, W = 120, 160
    out = {}
    (snet1, _, _), (pnet1, _, _) = _nets(rt, backend, 1)
    (snet3, _, _), (pnet3, _, _) = _nets(rt, backend, len(TRACKS))

    for sens in (None, SENSOR):
        tr = HandTracker(rt, icvl, pnet1, snet1, H, W, CUBE, sensor=sens)
        for flags in (0, ops.POSE_HAND_RIGHT | ops.POSE_INV_X):
            tr.set_hand(bool(flags & ops.POSE_HAND_RIGHT))
            tr.set_inv(bool(flags & ops.POSE_INV_X), False)
            for slot in (0, 1):
                out['hand/sensor=%d/flags=%d/slot=%d' % (sens is not None, flags, slot)] = \
                    reduce_launches(rt, tr.plan(slot).launches(), _regions(tr))

    for kind in ('homogeneous', 'heterogeneous'):
        if kind == 'homogeneous':
            args = (icvl, pnet3, snet3, H, W, CUBE, TRACKS)
        else:
            args = ([icvl, msra], pnet3, snet3, [H, 96], [W, 128], CUBE, TRACKS)
        for sens in (None, SENSOR):
            for grouped in (False, True):
                kw = dict(sensor=sens)
                if grouped:
                    eye = (np.eye(3), np.zeros(3))
                    kw.update(extrinsics=[eye, eye], groups=[[0, 2]], max_dev=50., handover=True)
                mt = MultiTracker(rt, *args, **kw)
                plans = [mt.plan(0).launches(), mt.plan(1).launches()]            # slot 1 makes the second input set: label it in both
                for slot in (0, 1):
                    out['multi/%s/sensor=%d/groups=%d/slot=%d' % (kind, sens is not None, grouped, slot)] = \
                        reduce_launches(rt, plans[slot], _regions(mt))
                if not grouped:
                    for what, det in (('detector', mt.detector(0)), ('source_detector', mt.source_detector(0)[0])):
                        out['%s/%s/sensor=%d' % (what, kind, sens is not None)] = \
                            reduce_launches(rt, det.plan(False).launches(), _regions(mt) + _regions(det, 'det.'))

    # the refinement stage as HandDetector.track builds it: a state block of its own, the frame's partials, tracks=None
    ceng = tracker._engine_b1(snet1, rt, 'refineNet')
    fr = rt.alloc((1, H, W), np.float32)
    st = rt.alloc(16, np.float32)
    com_in, com_out, com3d, status = st.view(0, (1, 3)), st.view(3, (1, 3)), st.view(6, (1, 3)), st.view(9, (1,), np.int32)
    cube, partial = rt.alloc((1, 3), np.float32), ops.frame_range_workspace(rt, 1)
    rec = rt.alloc(rt.lib.dpp_crop_record_bytes(), np.uint8)
    stage = tracker.refine_stage(rt, fr, H, W, partial, rec, com_in, cube, ceng, camera_tuple(icvl), 241.42, 241.42, 128, com_out, com3d, rec,
                                 status)
    regions = [(label, b.ptr, b.ptr + b.nbytes) for label, b in (('frame', fr), ('state', st), ('cube', cube), ('partial', partial),
                                                                 ('rec', rec), ('ceng.out', ceng.out.buf))]
    regions += [('ceng.x_ins[%d]' % k, t.buf.ptr, t.buf.ptr + t.buf.nbytes) for k, t in enumerate(ceng.x_ins)]
    pairs = [(op, side) for op, side in stage if isinstance(op, ops.Launch)]
    out['refine_stage'] = reduce_launches(rt, [op for op, _ in pairs], regions, sides=[side for _, side in pairs])
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--write', action='store_true', help="rewrite the backend's section of tests/golden/track_plans.json")
    ap.add_argument('--backend', default='emu', choices=['emu', 'hip'])
    ap.add_argument('--out', default=GOLDEN)
    a = ap.parse_args(argv)
    from tests.backends import get_runtime
    got = fingerprints(get_runtime(a.backend), a.backend)
    if not a.write:
        want = load_golden()[a.backend]
        bad = sorted(k for k in set(want) | set(got) if want.get(k) != json.loads(json.dumps(got.get(k))))
        print("%d plans, %d differ from the golden file%s" % (len(got), len(bad), ''.join('\n  ' + k for k in bad)))
        return 1 if bad else 0
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[a.backend] = got
    with open(a.out, 'w') as f:                                        # one line per plan: a changed launch shows as one changed line
        f.write('{\n' + ',\n'.join('"%s": {\n%s\n}' % (b, ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':')))
                                                                      for k, v in sorted(doc[b].items()))) for b in sorted(doc)) + '\n}\n')
    print("wrote %d plans of backend %s to %s" % (len(got), a.backend, a.out))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
