#!/usr/bin/env python3
"""
examples/test_realtimepipeline.py in a room that is not empty: a learned per-pixel background is removed from every frame ON THE
DEVICE, as the first step of the frame's plan (RealtimeHandposePipeline(background=...), csrc/background.hip; this project's own
semantics: hipdp/tracker.py, BACKGROUND), so that the detector's nearest object is the hand and not the desk edge.

    --background MARGIN REL           mm and a share of the depth: a pixel is kept where it is nearer than the learned background by
                                      more than MARGIN + REL * depth.  No default exists for a sensor, and none is invented
    --learn N                         frames the model is learned from (default 5)
    --clutter X0:Y0:X1:Y1:DEPTH[:START]   a static rectangle (columns X0 .. X1 - 1, rows Y0 .. Y1 - 1) at DEPTH mm pasted into every
                                      frame; with START only into the frames from tick START of the played sequence on, and not
                                      into the learning frames: an object put down after the model was learned
    --adapt PERSIST GUARD             keep the model current while tracking (hipdp/tracker.py, ADAPTATION): a depth that stays for
                                      PERSIST adapting ticks becomes the background; the tracked hand's crop window, dilated by GUARD
                                      pixels, is kept out.  No default exists for a sensor, and none is invented
    --adapt-every N                   adapt in every N-th tick (default 1)

Without --background this IS examples/test_realtimepipeline.py: there is no second main here, as in examples/realtime_smooth.py.  The
options are taken off the command line, everything else goes to that example's own main(), which runs with a pipeline class that
carries the option and a device class that pastes the clutter.  A recorded sequence has no frames of the empty room, so the model is
learned from the first N frames with the hand taken out: every depth inside the cube's depth range around the first frame's annotated
centre is set to 0 (not defined), the clutter stays.  After learning, the example prints where whole-frame detection (seed_detect's
acquire) lands in the first frame with and without the model -- sanity figures, not accuracy claims -- and then plays the sequence.
With a late rectangle it also looks, before every tick, where a detector of its own lands on the frame with the cut map as it stands
(the tracker is not disturbed), and prints the tick from which that is the hand again: with --adapt PERSIST adapting ticks after START,
without it never.  A sanity figure as well, not a threshold.

    python examples/realtime_background.py --dataset icvl --data ../data/ICVL/ --background 30 0.01 --learn 8 --clutter 250:20:310:100:300
    python examples/realtime_background.py --dataset icvl --data ../data/ICVL/ --background 30 0.01 --clutter 250:20:310:100:300:10 --adapt 5 4
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


def parse_clutter(text, with_start=False):
    """'X0:Y0:X1:Y1:DEPTH' -> (x0, y0, x1, y1, depth) or None; with_start: 'X0:Y0:X1:Y1:DEPTH[:START]' -> (that, START or None)."""
    if text is None:
        return (None, None) if with_start else None
    try:
        parts = text.split(':')
        start = int(parts.pop()) if with_start and len(parts) == 6 else None
        x0, y0, x1, y1, d = parts
        c = (int(x0), int(y0), int(x1), int(y1), float(d))
    except ValueError:
        raise SystemExit("--clutter takes X0:Y0:X1:Y1:DEPTH%s, not %r" % ("[:START]" if with_start else "", text))
    if not (0 <= c[0] < c[2] and 0 <= c[1] < c[3] and c[4] > 0.) or (start is not None and start < 0):
        raise SystemExit("--clutter needs X0 < X1, Y0 < Y1, a depth > 0 and a start tick >= 0: %r" % (text,))
    return (c, start) if with_start else c


def parse_adapt(ap_args):
    """--adapt PERSIST GUARD [--adapt-every N] -> background's adapt dict or None (the values are checked by the tracker's options)."""
    if ap_args.adapt is None:
        if ap_args.adapt_every is not None:
            raise SystemExit("--adapt-every needs --adapt PERSIST GUARD")
        return None
    return dict(persist=ap_args.adapt[0], guard=ap_args.adapt[1], every=1 if ap_args.adapt_every is None else ap_args.adapt_every)


def on_clutter(com, clutter):
    """A detected centre sits on the rectangle: inside its outline, or at its depth."""
    x0, y0, x1, y1, d = clutter
    return (x0 <= com[0] < x1 and y0 <= com[1] < y1) or abs(float(com[2]) - d) < 25.


def paste(frame, clutter):
    """The static rectangle into a frame (clipped to it)."""
    if clutter is not None:
        x0, y0, x1, y1, d = clutter
        frame[y0:y1, x0:x1] = d
    return frame


class ClutterDevice(FileDevice):
    """A FileDevice in a room with a static object: the rectangle is pasted into every frame; with `hand` = (z, cube_z) the hand is
    taken out first (every depth within cube_z / 2 of z becomes 0): the empty room the model is learned from."""

    def __init__(self, filenames, di, clutter=None, hand=None, first=0, probe=None):
        super(ClutterDevice, self).__init__(filenames, di)
        self.clutter, self.hand, self.first, self.probe = clutter, hand, first, probe
        self.ticks, self.landed = 0, []                   # per delivered frame: where `probe` (frame -> centre or None) landed

    def getDepth(self):
        ret, frame = super(ClutterDevice, self).getDepth()
        frame = numpy.array(frame, numpy.float32)
        if self.hand is not None:
            z, cz = self.hand
            frame[numpy.abs(frame - z) <= cz / 2.] = 0.
        if ret and self.ticks >= self.first:
            frame = paste(frame, self.clutter)
        if ret and self.probe is not None:
            self.landed.append(self.probe(frame))
        self.ticks += 1
        return ret, frame


def main(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument('--background', nargs=2, type=float, default=None, metavar=('MARGIN', 'REL'))
    ap.add_argument('--learn', type=int, default=5, metavar='N')
    ap.add_argument('--clutter', default=None, metavar='X0:Y0:X1:Y1:DEPTH[:START]')
    ap.add_argument('--adapt', nargs=2, type=int, default=None, metavar=('PERSIST', 'GUARD'))
    ap.add_argument('--adapt-every', type=int, default=None, metavar='N')
    args, rest = ap.parse_known_args(argv)
    if args.background is None:
        if args.clutter is not None or args.adapt is not None or args.adapt_every is not None:
            raise SystemExit("--clutter and --adapt need --background")
        return base.main(rest)
    clutter, start = parse_clutter(args.clutter, with_start=True)
    background = dict(margin=args.background[0], rel=args.background[1])
    adapt = parse_adapt(args)
    if adapt is not None:
        background['adapt'] = adapt
    late = clutter is not None and start is not None    # the rectangle appears in the played sequence, not in the learning frames
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
        rtp.learnBackground(ClutterDevice(filenames[:n], di, None if late else clutter, hand=hand), frames=n)
        first = paste(numpy.array(di.loadDepthMap(filenames[0]), numpy.float32), None if late and start > 0 else clutter)
        t = rtp.tracker(*first.shape)
        with_model = t.acquire(first)
        model = t.background_model()
        t.clear_background()
        without = t.acquire(first)
        t.set_background_model(model)
        figures.update(with_model=with_model, without=without, known=float(numpy.isfinite(model['cut']).mean()))
        if not late:
            return ClutterDevice(filenames, di, clutter)
        from hipdp.detect import FrameDetector           # a detector of its own on a view of the tracker's cut map: it does not adapt
        det = FrameDetector(t.rt, t.H, t.W, t.fx, t.fy, 1, background=t.background, cut=t.bg.view(t.bg.cut, 0))

        def probe(frame):
            coms, _, found = det.run(frame[None], t.cube_host[None])[:3]
            return coms[0] if found[0] else None
        figures['device'] = ClutterDevice(filenames, di, clutter, first=start, probe=probe)
        return figures['device']
    base.RealtimeHandposePipeline, base.FileDevice = pipeline, device
    try:
        poses, err = base.main(rest)
    finally:
        base.RealtimeHandposePipeline, base.FileDevice = Pipeline, FileDevice

    def where(a):
        return "(%.1f, %.1f, %.1f mm)" % tuple(a['com']) if a['found'] else "nothing"
    print("background (sanity figures): model known at {:.1%} of the pixels; detection in the first frame lands at {} with the model, "
          "at {} without it".format(figures['known'], where(figures['with_model']), where(figures['without'])))
    if late:                                             # the first tick from which every detection is the hand again
        landed = figures.pop('device').landed
        hand = [c is not None and not on_clutter(c, clutter) for c in landed]
        again = next((k for k in range(start, len(hand)) if all(hand[k:])), None)
        figures.update(landed=landed, hand_again=again)
        print("background (sanity figure): the rectangle appears in tick {}; detection lands on the hand again from tick {}".format(
            start, "%d on" % again if again is not None else "-- never in this sequence --"))
    return poses, err, figures


if __name__ == '__main__':
    main()
