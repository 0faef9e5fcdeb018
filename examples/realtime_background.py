#!/usr/bin/env python3
"""
examples/test_realtimepipeline.py in a room that is not empty: a learned per-pixel background is removed from every frame ON THE
DEVICE, as the first step of the frame's plan (RealtimeHandposePipeline(background=...), csrc/background.hip; this project's own
semantics: hipdp/tracker.py, BACKGROUND), so that the detector's nearest object is the hand and not the desk edge.

    --background MARGIN REL           mm and a share of the depth: a pixel is kept where it is nearer than the learned background by
                                      more than MARGIN + REL * depth.  No default exists for a sensor, and none is invented
    --learn N                         frames the model is learned from (default 5)
    --clutter X0:Y0:X1:Y1:DEPTH       a static rectangle (columns X0 .. X1 - 1, rows Y0 .. Y1 - 1) at DEPTH mm pasted into every frame

Without --background this IS examples/test_realtimepipeline.py: there is no second main here, as in examples/realtime_smooth.py.  The
options are taken off the command line, everything else goes to that example's own main(), which runs with a pipeline class that
carries the option and a device class that pastes the clutter.  A recorded sequence has no frames of the empty room, so the model is
learned from the first N frames with the hand taken out: every depth inside the cube's depth range around the first frame's annotated
centre is set to 0 (not defined), the clutter stays.  After learning, the example prints where whole-frame detection (seed_detect's
acquire) lands in the first frame with and without the model -- sanity figures, not accuracy claims -- and then plays the sequence.

    python examples/realtime_background.py --dataset icvl --data ../data/ICVL/ --background 30 0.01 --learn 8 --clutter 250:20:310:100:300
"""
import argparse
import importlib.util
import os

_spec = importlib.util.spec_from_file_location('realtime_driver_base', os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  'test_realtimepipeline.py'))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)                           # a private copy of the example: sets sys.path; its names are replaced below
numpy = base.numpy
FileDevice, Pipeline = base.FileDevice, base.RealtimeHandposePipeline


def parse_clutter(text):
    """'X0:Y0:X1:Y1:DEPTH' -> (x0, y0, x1, y1, depth) or None."""
    if text is None:
        return None
    try:
        x0, y0, x1, y1, d = text.split(':')
        c = (int(x0), int(y0), int(x1), int(y1), float(d))
    except ValueError:
        raise SystemExit("--clutter takes X0:Y0:X1:Y1:DEPTH, not %r" % (text,))
    if not (0 <= c[0] < c[2] and 0 <= c[1] < c[3] and c[4] > 0.):
        raise SystemExit("--clutter needs X0 < X1, Y0 < Y1 and a depth > 0: %r" % (text,))
    return c


def paste(frame, clutter):
    """The static rectangle into a frame (clipped to it)."""
    if clutter is not None:
        x0, y0, x1, y1, d = clutter
        frame[y0:y1, x0:x1] = d
    return frame


class ClutterDevice(FileDevice):
    """A FileDevice in a room with a static object: the rectangle is pasted into every frame; with `hand` = (z, cube_z) the hand is
    taken out first (every depth within cube_z / 2 of z becomes 0): the empty room the model is learned from."""

    def __init__(self, filenames, di, clutter=None, hand=None):
        super(ClutterDevice, self).__init__(filenames, di)
        self.clutter, self.hand = clutter, hand

    def getDepth(self):
        ret, frame = super(ClutterDevice, self).getDepth()
        frame = numpy.array(frame, numpy.float32)
        if self.hand is not None:
            z, cz = self.hand
            frame[numpy.abs(frame - z) <= cz / 2.] = 0.
        return ret, paste(frame, self.clutter)


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument('--background', nargs=2, type=float, default=None, metavar=('MARGIN', 'REL'))
    ap.add_argument('--learn', type=int, default=5, metavar='N')
    ap.add_argument('--clutter', default=None, metavar='X0:Y0:X1:Y1:DEPTH')
    args, rest = ap.parse_known_args(argv)
    if args.background is None:
        if args.clutter is not None:
            raise SystemExit("--clutter needs --background")
        return base.main(rest)
    clutter = parse_clutter(args.clutter)
    background = dict(margin=args.background[0], rel=args.background[1])
    made, figures = [], {}

    def pipeline(*a, **k):                               # the example's pipeline, with the option
        made.append(Pipeline(*a, background=background, **k))
        return made[-1]

    def device(filenames, di):                           # learn the empty room, look where detection lands, then the example's device
        rtp = made[-1]
        if rtp.init_com is None:
            raise SystemExit("--background takes the hand out of the learning frames around the annotated centre: it needs --seed gt")
        n = min(max(1, args.learn), len(filenames))
        hand = (float(rtp.init_com[2]), float(rtp.sync['config']['cube'][2]))
        rtp.learnBackground(ClutterDevice(filenames[:n], di, clutter, hand=hand), frames=n)
        first = paste(numpy.array(di.loadDepthMap(filenames[0]), numpy.float32), clutter)
        t = rtp.tracker(*first.shape)
        with_model = t.acquire(first)
        model = t.background_model()
        t.clear_background()
        without = t.acquire(first)
        t.set_background_model(model)
        figures.update(with_model=with_model, without=without, known=float(numpy.isfinite(model['cut']).mean()))
        return ClutterDevice(filenames, di, clutter)
    base.RealtimeHandposePipeline, base.FileDevice = pipeline, device
    try:
        poses, err = base.main(rest)
    finally:
        base.RealtimeHandposePipeline, base.FileDevice = Pipeline, FileDevice

    def where(a):
        return "(%.1f, %.1f, %.1f mm)" % tuple(a['com']) if a['found'] else "nothing"
    print("background (sanity figures): model known at {:.1%} of the pixels; detection in the first frame lands at {} with the model, "
          "at {} without it".format(figures['known'], where(figures['with_model']), where(figures['without'])))
    return poses, err, figures


if __name__ == '__main__':
    main()
