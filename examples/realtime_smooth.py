#!/usr/bin/env python3
"""
examples/test_realtimepipeline.py with the joints smoothed ON THE DEVICE: the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012; this
project's own semantics: hipdp/multitrack.py, SMOOTHING) runs over the regressed joints as the LAST launch of the per-frame plan
(RealtimeHandposePipeline(smooth=...), csrc/smooth.hip).

    --smooth RATE MINCUTOFF BETA   frames per second, Hz, Hz per mm/s: no tuned default exists, and none is invented
    --hold N                       frames a lost hand keeps its last filtered pose (max_hold; default 0)

Without --smooth this IS examples/test_realtimepipeline.py: there is no second main here, as in examples/realtime_sensor.py.  The two
options are taken off the command line, everything else (--seed, --hand, the checkpoints, ...) goes to that example's own main(), which
runs with a pipeline class that carries the filter's parameters.  (The options live here and not in that example because its file
name, test_*.py, puts it among the test files, which a change that adds a feature leaves as they are.)  After that example's own output two sanity figures are printed,
not bars: the mean frame-to-frame displacement of the raw and of the filtered joints over the recorded sequence, and the mean
raw-to-filtered distance.  With untrained nets they only show that the filter ran.

    python examples/realtime_smooth.py --dataset icvl --data ../data/ICVL/ --smooth 30 1.0 0.007 --hold 2
"""
import argparse
import importlib.util
import os

_spec = importlib.util.spec_from_file_location('realtime_driver_base', os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  'test_realtimepipeline.py'))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)                           # a private copy of the example: sets sys.path; one name is replaced below
Pipeline = base.RealtimeHandposePipeline

from util.realtimehandposepipeline import smoothing_figures  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument('--smooth', nargs=3, type=float, default=None, metavar=('RATE', 'MINCUTOFF', 'BETA'))
    ap.add_argument('--hold', type=int, default=0, metavar='N')
    args, rest = ap.parse_known_args(argv)
    if args.smooth is None:
        return base.main(rest)
    smooth = dict(rate=args.smooth[0], mincutoff=args.smooth[1], beta=args.smooth[2], max_hold=args.hold)
    made = []

    def pipeline(*a, **k):                               # the example's pipeline, with the filter's parameters
        made.append(Pipeline(*a, smooth=smooth, **k))
        return made[-1]
    base.RealtimeHandposePipeline = pipeline
    try:
        poses, err = base.main(rest)
    finally:
        base.RealtimeHandposePipeline = Pipeline
    fig = smoothing_figures(poses, made[-1].poses_f)
    print("smoothing (sanity figures): mean frame-to-frame displacement {raw_step:.3f} mm raw, {filtered_step:.3f} mm filtered; "
          "mean raw-to-filtered distance {distance:.3f} mm".format(**fig))
    return poses, err, fig, made[-1].poses_f


if __name__ == '__main__':
    main()
