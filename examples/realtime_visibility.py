#!/usr/bin/env python3
"""
examples/test_realtimepipeline.py with every joint classified by what the frame SHOWS around it, on the device: one launch behind
pose_finish counts, in the frame's pixels within RADIUS of each joint, those within MARGIN mm of the joint's depth and those nearer
(this project's own semantics: hipdp/multitrack.py, VISIBILITY; RealtimeHandposePipeline(visibility=...), csrc/visibility.hip).  A
single camera cannot average an occluded joint away, but a consumer can grey it out or hold it.

    --visibility RADIUS MARGIN MIN_SUPPORT   pixels, mm, pixels: none has been chosen for a dataset, and none is invented

Without --visibility this IS examples/test_realtimepipeline.py: there is no second main here, as in examples/realtime_smooth.py.  The
option is taken off the command line, everything else (--seed, --hand, the checkpoints, ...) goes to that example's own main(), which
runs with a pipeline class that carries the parameters.  (The option lives here and not in that example because its file name,
test_*.py, puts it among the test files, which a change that adds a feature leaves as they are.)  After that example's own output the
share of the recorded sequence's joints per class is printed: visible, occluded, unsupported (guessed onto background or into a hole),
off-frame.  With untrained nets the shares only show that the launch ran.

    python examples/realtime_visibility.py --dataset icvl --data ../data/ICVL/ --visibility 2 40 6
"""
import argparse
import importlib.util
import os

import numpy

_spec = importlib.util.spec_from_file_location('realtime_driver_base', os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  'test_realtimepipeline.py'))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)                           # a private copy of the example: sets sys.path; one name is replaced below
Pipeline = base.RealtimeHandposePipeline

CLASSES = (('visible', 1), ('occluded', 2), ('unsupported', 4), ('off-frame', 8))          # ops.VIS_*


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument('--visibility', nargs=3, type=float, default=None, metavar=('RADIUS', 'MARGIN', 'MIN_SUPPORT'))
    args, rest = ap.parse_known_args(argv)
    if args.visibility is None:
        return base.main(rest)
    visibility = dict(radius=int(args.visibility[0]), margin=args.visibility[1], min_support=int(args.visibility[2]))
    made = []

    def pipeline(*a, **k):                               # the example's pipeline, with the classifier's parameters
        made.append(Pipeline(*a, visibility=visibility, **k))
        return made[-1]
    base.RealtimeHandposePipeline = pipeline
    try:
        poses, err = base.main(rest)
    finally:
        base.RealtimeHandposePipeline = Pipeline
    classes = made[-1].vis_classes
    shares = dict((name, float((classes == v).mean()) if classes.size else float('nan')) for name, v in CLASSES)
    print("visibility: " + ', '.join("{} {:.3f}".format(name, shares[name]) for name, _ in CLASSES))
    return poses, err, shares, classes


if __name__ == '__main__':
    main()
