"""
HandDetector -- the augmentation slice of /root/reference/src/util/handdetector.py (comToBounds / comToTransform
:204-258, moveCoM / rotateHand / scaleHand / recropHand :678-803, sampleRandomPoses :805-909) and its crop helpers
(bilinearResize :132-202, getInverseCrop / resizeCrop / applyCrop3D :298-380).

The crop warps run on the MI355X through the crop kernels (csrc/crop.hip); this class keeps the
reference's per-crop method signatures for callers and computes only the tiny 3x3 crop geometry on the host.
cropArea3D (handdetector.py:382-490, docom=False: the call the importers make for every frame) runs on the device too;
`crop_frames` is its batched form fused with Dataset.imgStackDepthOnly.  recropHand, resizeCrop, bilinearResize,
getInverseCrop and applyCrop3D are device-backed as well, with batched forms `recrop_crops`, `resize_crops` and
`inverse_crops` (one launch per batch each).  CoM refinement by a ScaleNet (refineCoM, handdetector.py:634-676) goes
through the net's computeOutput.  track (handdetector.py:504-544, doHandSize=False) runs on the device with the kernels of the
realtime tracker (hipdp/tracker.py), refineCoMIterative has a batched device form (`refine_com_iterative`).  Whole-frame detection
and hand-size estimation as the reference has them (detect, estimateHandsize: cv2 contour analysis) are not built; what they are for
-- the nearest sufficiently large connected object, and the bounding box of the largest object in the hand's depth range -- is, by
8-connected component labelling on the device (csrc/components.hip, hipdp/detect.py): `label_components`, `find_hands`,
HandDetector.detectComponents and estimateHandsizeComponents.

resizeMethod is honoured where the reference reads it: RESIZE_CV2_NN (the default) is cv2's nearest-neighbour resize,
RESIZE_BILINEAR the reference's own ND-aware bilinearResize.  RESIZE_CV2_LINEAR (cv2 INTER_LINEAR) is not built: the new
methods raise NotImplementedError for it, and cropArea3D still crops with nearest neighbour under it (a known gap).
"""
import numpy

from data.transformations import rotatePoints2D      # noqa: F401  (part of the module surface the reference exposes)


class HandDetector(object):
    RESIZE_BILINEAR = 0
    RESIZE_CV2_NN = 1
    RESIZE_CV2_LINEAR = 2

    def __init__(self, dpt, fx, fy, importer=None, refineNet=None):
        self.dpt = dpt
        self.maxDepth = min(1500, dpt.max())
        self.minDepth = max(10, dpt.min())
        self.dpt[self.dpt > self.maxDepth] = 0.
        self.dpt[self.dpt < self.minDepth] = 0.
        self.fx, self.fy = fx, fy
        self.refineNet = refineNet
        self.importer = importer
        self.resizeMethod = self.RESIZE_CV2_NN

    @staticmethod
    def detectionModeToString(com, refineNet):
        """Tag of the cache files (handdetector.py:72-89)."""
        if com is False and refineNet is False:
            return 'gt'
        if com is True and refineNet is False:
            return 'com'
        if com is True and refineNet is True:
            return 'comref'
        raise NotImplementedError("com {}, refineNet {}".format(com, refineNet))

    def checkImage(self, tol):
        """Is there some content in the image (handdetector.py:110-120)."""
        return not (numpy.std(self.dpt) < tol)

    # ---- crop geometry (host, a handful of flops) -----------------------------------------------------------
    def comToBounds(self, com, size):
        """Project the metric cube around the CoM back to pixel bounds (handdetector.py:204-226)."""
        if numpy.isclose(com[2], 0.):
            print("Warning: CoM ill-defined!")
            xstart = self.dpt.shape[0] // 4
            xend = xstart + self.dpt.shape[0] // 2
            ystart = self.dpt.shape[1] // 4
            yend = ystart + self.dpt.shape[1] // 2
            return xstart, xend, ystart, yend, self.minDepth, self.maxDepth
        c0, c1, c2 = float(com[0]), float(com[1]), float(com[2])
        zstart, zend = c2 - size[2] / 2., c2 + size[2] / 2.
        xstart = int(numpy.floor((c0 * c2 / self.fx - size[0] / 2.) / c2 * self.fx + 0.5))
        xend = int(numpy.floor((c0 * c2 / self.fx + size[0] / 2.) / c2 * self.fx + 0.5))
        ystart = int(numpy.floor((c1 * c2 / self.fy - size[1] / 2.) / c2 * self.fy + 0.5))
        yend = int(numpy.floor((c1 * c2 / self.fy + size[1] / 2.) / c2 * self.fy + 0.5))
        return xstart, xend, ystart, yend, zstart, zend

    def comToTransform(self, com, size, dsize=(128, 128)):
        """Affine crop transform off . scale . trans (handdetector.py:228-258); the reference's Python-2 integer
        divisions are kept as floor divisions."""
        xstart, xend, ystart, yend, _, _ = self.comToBounds(com, size)
        wb, hb = (xend - xstart), (yend - ystart)
        if wb > hb:
            s = dsize[0] / float(wb)
            sz = (dsize[0], hb * dsize[0] // wb)
        else:
            s = dsize[1] / float(hb)
            sz = (wb * dsize[1] // hb, dsize[1])
        xs = int(numpy.floor(dsize[0] / 2. - sz[1] / 2.))
        ys = int(numpy.floor(dsize[1] / 2. - sz[0] / 2.))
        return numpy.array([[s, 0., s * float(-xstart) + xs], [0., s, s * float(-ystart) + ys], [0., 0., 1.]])

    # ---- single-crop warps on the device ----------------------------------------------------------------------
    def _run(self, dpt_norm, cube, com, joints3D, M, mode, off=(0., 0., 0.), rot=0., sc=1.):
        from hipdp import ops
        from hipdp.augmenter import MODE_CODE, camera_tuple
        from hipdp.runtime import default_runtime
        rt = default_runtime()
        J = joints3D.shape[0]
        dsz = dpt_norm.shape[0]
        f32 = lambda a: rt.upload(numpy.ascontiguousarray(a, numpy.float32))       # noqa: E731
        com3d = self.importer.jointImgTo3D(com)
        rec = rt.alloc(rt.lib.dpp_augment_record_bytes(), numpy.uint8)
        out_y, out_x = rt.alloc((1, J * 3)), rt.alloc((1, dsz, dsz))
        img = f32(dpt_norm[None])
        ops.augment_prepare(rt, img, f32(com3d[None]), f32(numpy.asarray(cube)[None]), f32(numpy.asarray(M).reshape(1, 9)),
                            f32(joints3D.reshape(1, J, 3)), 1, J, dsz, camera_tuple(self.importer), rec, out_y,
                            mode=rt.upload(numpy.array([MODE_CODE[mode]], numpy.int32)), off=rt.upload(numpy.asarray(off, numpy.float64)),
                            rot=rt.upload(numpy.array([rot], numpy.float64)), sc=rt.upload(numpy.array([sc], numpy.float64)))(rt.stream)
        ops.augment_warp(rt, img, rec, 1, dsz, out_x)(rt.stream)
        rt.synchronize()
        return out_x.get()[0], out_y.get().reshape(J, 3)

    def _normalise(self, dpt, cube, com):
        d = numpy.asarray(dpt, numpy.float32).copy()
        d[d == 0] = com[2] + cube[2] / 2.
        return (d - com[2]) / (cube[2] / 2.)

    def moveCoM(self, dpt, cube, com, off, joints3D, M, pad_value=0):
        """Simulate a different CoM on an already cropped image (handdetector.py:678-710).  dpt is in mm like in the
        reference; returns (new_dpt [normalised to the NEW CoM, far plane filled], new_joints3D, new_com, Mnew)."""
        if numpy.allclose(off, 0.):
            return dpt, joints3D, com, M
        new_com = self.importer.joint3DToImg(self.importer.jointImgTo3D(com) + off)
        img, lab = self._run(self._normalise(dpt, cube, com), cube, com, numpy.asarray(joints3D, numpy.float32), M, 'com', off=off)
        Mnew = self.comToTransform(new_com, cube, dpt.shape) if not (numpy.allclose(com[2], 0.) or numpy.allclose(new_com[2], 0.)) else M
        return img, lab * (cube[2] / 2.), new_com, Mnew

    def rotateHand(self, dpt, cube, com, rot, joints3D, pad_value=0):
        """In-plane rotation about the crop centre (handdetector.py:712-747)."""
        if numpy.allclose(rot, 0.):
            return dpt, joints3D, rot
        M = self.comToTransform(com, cube, dpt.shape)
        img, lab = self._run(self._normalise(dpt, cube, com), cube, com, numpy.asarray(joints3D, numpy.float32), M, 'rot', rot=rot)
        return img, lab * (cube[2] / 2.), numpy.mod(rot, 360)

    def scaleHand(self, dpt, cube, com, sc, joints3D, M, pad_value=0):
        """Re-crop with a scaled metric cube (handdetector.py:750-780)."""
        if numpy.allclose(sc, 1.):
            return dpt, joints3D, cube, M
        new_cube = [s * sc for s in cube]
        img, _ = self._run(self._normalise(dpt, cube, com), cube, com, numpy.asarray(joints3D, numpy.float32), M, 'sc', sc=sc)
        Mnew = self.comToTransform(com, new_cube, dpt.shape) if not numpy.allclose(com[2], 0.) else M
        return img, joints3D, new_cube, Mnew

    # ---- pose-space sampling for the PCA prior (one-off set-up, host) ------------------------------------------------
    @staticmethod
    def sampleRandomPoses(importer, rng, base_poses, base_com, base_cube, num_poses, aug_modes, retall=False, rot3D=False,
                          sigma_com=None, sigma_sc=None, rot_range=None):
        """Random pose augmentation in label space only, used once to fit the 30-D PCA prior
        (handdetector.py:805-909; main_nyu_posereg_embedding.py:86-88).  Same draws from `rng`, in the same order."""
        sigma_com = 5. if sigma_com is None else sigma_com
        sigma_sc = 0.02 if sigma_sc is None else sigma_sc
        rot_range = 180. if rot_range is None else rot_range
        simple = ('none', 'rot', 'sc', 'com')
        combo = ('rot+com', 'com+rot')
        combo_sc = ('rot+com+sc', 'rot+sc+com')
        assert all(m in simple + combo + combo_sc + ('sc+rot+com', 'sc+com+rot', 'com+sc+rot', 'com+rot+sc') for m in aug_modes)
        n = int(num_poses)
        new_poses = numpy.zeros((n, base_poses.shape[1], base_poses.shape[2]), dtype=base_poses.dtype)
        new_com = numpy.zeros((n, 3), dtype=base_poses.dtype)
        new_cube = numpy.zeros((n, 3), dtype=base_poses.dtype)
        modes = rng.randint(0, len(aug_modes), n)
        ridxs = rng.randint(0, base_poses.shape[0], n)
        off = rng.randn(n, 3) * sigma_com
        sc = numpy.fabs(rng.randn(n) * sigma_sc + 1.)
        rot = rng.uniform(-rot_range, rot_range, size=(n, 3))
        if aug_modes == ['none']:
            out = base_poses / (base_cube[:, 2] / 2.)[:, None, None]
            return (out, base_com, base_cube) if retall else out
        # The reference loops over the n (= 1e6 in the scripts) samples in Python; the same arithmetic, in the same operation
        # order and precision (float64 products rounded to the arrays' float32 where the reference rounds), is done here per
        # augmentation mode on whole index sets.
        f32 = numpy.float32
        fx, fy, ux, uy, flip = float(importer.fx), float(importer.fy), float(importer.ux), float(importer.uy), bool(importer.flip_y)

        def to_img(p):                      # joints3DToImg on (..., 3), DepthImporter.joint3DToImg
            p = numpy.asarray(p, numpy.float64)
            z = p[..., 2]
            ok = z != 0.
            zz = numpy.where(ok, z, 1.)
            u = numpy.where(ok, p[..., 0] / zz * fx + ux, ux)
            v = numpy.where(ok, (uy - p[..., 1] / zz * fy) if flip else (p[..., 1] / zz * fy + uy), uy)
            return numpy.stack([u, v, numpy.where(ok, z, 0.)], axis=-1).astype(f32)

        def to_3d(q):                       # jointsImgTo3D on (..., 3)
            q = numpy.asarray(q, numpy.float64)
            x = (q[..., 0] - ux) * q[..., 2] / fx
            y = ((uy - q[..., 1]) if flip else (q[..., 1] - uy)) * q[..., 2] / fy
            return numpy.stack([x, y, q[..., 2]], axis=-1).astype(f32)

        def rot_2d(pts, center, angle):     # rotatePoints2D about per-sample centres, transformations.py:71-88
            alpha = (angle * numpy.pi / 180.)[:, None]
            pp0 = (pts[..., 0] - center[:, None, 0]).astype(f32)
            pp1 = (pts[..., 1] - center[:, None, 1]).astype(f32)
            r0 = (pp0.astype(numpy.float64) * numpy.cos(alpha) - pp1.astype(numpy.float64) * numpy.sin(alpha)).astype(f32)
            r1 = (pp0.astype(numpy.float64) * numpy.sin(alpha) + pp1.astype(numpy.float64) * numpy.cos(alpha)).astype(f32)
            out = pts.copy()
            out[..., 0] = r0 + center[:, None, 0]
            out[..., 1] = r1 + center[:, None, 1]
            return out

        def rot_3d(pts, center, angles):    # rotatePoints3D about per-sample centres with per-sample angles, transformations.py:105-155
            from data.transformations import euler_rxyz_matrix
            a = numpy.asarray(angles, numpy.float64) * numpy.pi / 180.
            R = euler_rxyz_matrix(a[:, 0], a[:, 1], a[:, 2])
            rel = (pts - center[:, None]).astype(numpy.float64)             # the offset is formed in the points' precision
            return (numpy.einsum('nab,njb->nja', R, rel) + center[:, None].astype(numpy.float64)).astype(pts.dtype)

        dt = base_poses.dtype
        mode_of = numpy.asarray([aug_modes[m] for m in range(len(aug_modes))])
        mname = mode_of[modes]
        cube_all, com_all, pose_all = base_cube[ridxs], base_com[ridxs], base_poses[ridxs]
        for mode in sorted(set(mname.tolist())):
            I = numpy.nonzero(mname == mode)[0]
            cube, com3D, pose = cube_all[I], com_all[I], pose_all[I]
            if mode == 'com':
                nc = (com3D + off[I]).astype(dt)
                new_com[I], new_cube[I] = nc, cube
                new_poses[I] = (pose + com3D[:, None] - nc[:, None]) / (new_cube[I][:, 2] / 2.)[:, None, None]
            elif mode == 'rot':
                new_com[I], new_cube[I] = com3D, cube
                nc = new_com[I]
                if rot3D:
                    new_poses[I] = (rot_3d(pose + nc[:, None], nc, rot[I]) - nc[:, None]) / (new_cube[I][:, 2] / 2.)[:, None, None]
                    continue
                joint_2D = to_img(pose + nc[:, None])
                data_2D = rot_2d(joint_2D, to_img(com3D), rot[I, 0])
                new_poses[I] = (to_3d(data_2D) - nc[:, None]) / (new_cube[I][:, 2] / 2.)[:, None, None]
            elif mode == 'sc':
                new_com[I] = com3D
                new_cube[I] = cube * sc[I].astype(f32)[:, None]          # float32 array x float64 scalar stays float32 in the reference's NumPy
                new_poses[I] = pose / (new_cube[I][:, 2] / 2.)[:, None, None]
            elif mode == 'none':
                new_com[I], new_cube[I] = com3D, cube
                new_poses[I] = pose / (new_cube[I][:, 2] / 2.)[:, None, None]
            elif mode in combo or mode in combo_sc:
                nc = (com3D + off[I]).astype(dt)
                new_com[I], new_cube[I] = nc, cube
                p = pose + com3D[:, None] - new_com[I][:, None]
                if mode in combo_sc:
                    p = p * sc[I].astype(f32)[:, None, None]
                if rot3D:                    # handdetector.py:891, 903: about the NEW centre, re-centred on it
                    nc = new_com[I]
                    new_poses[I] = (rot_3d(p + nc[:, None], nc, rot[I]) - nc[:, None]) / (new_cube[I][:, 2] / 2.)[:, None, None]
                    continue
                joint_2D = to_img(p + com3D[:, None])
                data_2D = rot_2d(joint_2D, to_img(new_com[I]), rot[I, 0])
                new_poses[I] = (to_3d(data_2D) - com3D[:, None]) / (new_cube[I][:, 2] / 2.)[:, None, None]
            else:
                raise NotImplementedError()
        return (new_poses, new_com, new_cube, rot) if retall else new_poses

    # ---- initial crop on the device ---------------------------------------------------------------------------------------
    def getNDValue(self):
        """Value of 'not defined' depth (handdetector.py:122-130): the most frequent out-of-range value -- 0 after the
        constructor zeroed everything outside [minDepth, maxDepth]."""
        lo, hi = self.dpt[self.dpt < self.minDepth], self.dpt[self.dpt > self.maxDepth]
        vals = lo if lo.shape[0] > hi.shape[0] else hi
        if vals.shape[0] == 0:
            return 0.
        u, c = numpy.unique(vals, return_counts=True)
        return u[numpy.argmax(c)]

    def cropArea3D(self, com=None, size=(250, 250, 250), dsize=(128, 128), docom=False):
        """Crop the metric cube `size` (mm) around `com` (image coordinates, z in mm) and resize it to `dsize`
        (handdetector.py:382-490).  Returns (crop in mm, crop transform M, com) like the reference."""
        if len(size) != 3 or len(dsize) != 2:
            raise ValueError("Size must be 3D and dsize 2D bounding box")
        if com is None:
            com = self.calculateCoM(self.dpt)            # handdetector.py:401-402: centre of mass of the whole (range-limited) frame
        if dsize[0] != dsize[1]:
            raise NotImplementedError("square destination sizes only")
        frame = numpy.asarray(self.dpt, numpy.float32)[None]
        cube = numpy.asarray(size, numpy.float32)[None]
        nd = self.getNDValue()
        # RESIZE_BILINEAR switches every resize of the crop (the final one and the refinement net's input) to bilinearResize;
        # RESIZE_CV2_LINEAR is not built and still gives the nearest-neighbour crop (see the module docstring)
        rm = HandDetector.RESIZE_BILINEAR if self.resizeMethod == HandDetector.RESIZE_BILINEAR else HandDetector.RESIZE_CV2_NN
        crops, Ms, coms = crop_frames(frame, numpy.asarray(com, numpy.float32)[None], cube, self.fx, self.fy, dsize[0], normalize=False,
                                      nd_value=nd, docom=docom, return_com=True, resize_method=rm)
        if docom and self.refineNet is not None and self.importer is not None:
            # handdetector.py:429-440: a ScaleNet regresses the offset of the true CoM from the crop; crop again around it.  The net
            # looks at resizeCrop(cropped, dsize): the window resized to dsize AS IT IS (:430), not the aspect-preserving paste
            # (at the net's own input size: the reference passes dsize, which has to be that size there)
            dims = self.refineNet.cfgParams.inputDim
            rs = int((dims[0] if isinstance(dims[0], (list, tuple)) else dims)[2])
            rz, _ = crop_frames(frame, coms[0][None], cube, self.fx, self.fy, rs, normalize=False, nd_value=nd, stretch=True, resize_method=rm)
            newCom3D = self.refineCoM(rz[0], size, coms[0]) + self.importer.jointImgTo3D(coms[0])
            com2 = numpy.asarray(self.importer.joint3DToImg(newCom3D), numpy.float64)
            if numpy.allclose(com2, 0.):
                com2[2] = crops[0][crops[0].shape[0] // 2, crops[0].shape[1] // 2]
            crops, Ms, coms = crop_frames(frame, com2.astype(numpy.float32)[None], cube, self.fx, self.fy, dsize[0], normalize=False,
                                          nd_value=nd, return_com=True, resize_method=rm)
        return crops[0], Ms[0].astype(numpy.float64), (coms[0].astype(numpy.float64) if docom else com)

    def refineCoM(self, cropped, size, com):
        """Offset (mm) of the hand centre predicted by the refinement net from a crop around `com` (handdetector.py:634-676):
        normalise and clamp the crop to the cube, feed it with its 1/2 and 1/4 centre crops."""
        imgD = numpy.asarray(cropped, 'float32').copy()
        imgD[imgD == 0] = com[2] + (size[2] / 2.)
        imgD[imgD >= com[2] + (size[2] / 2.)] = com[2] + (size[2] / 2.)
        imgD[imgD <= com[2] - (size[2] / 2.)] = com[2] - (size[2] / 2.)
        imgD -= com[2]
        imgD /= (size[2] / 2.)
        test_data = numpy.zeros((1, 1, cropped.shape[0], cropped.shape[1]), dtype='float32')
        test_data[0, 0] = imgD
        inputs = [test_data]
        for k in (2, 4):
            dsize = (int(test_data.shape[2] // k), int(test_data.shape[3] // k))
            xstart = int(test_data.shape[2] / 2 - dsize[0] / 2)
            ystart = int(test_data.shape[3] / 2 - dsize[1] / 2)
            inputs.append(numpy.ascontiguousarray(test_data[:, :, ystart:ystart + dsize[1], xstart:xstart + dsize[0]]))
        if self.refineNet.cfgParams.numInputs == 1:
            jts = self.refineNet.computeOutput(test_data)
        elif self.refineNet.cfgParams.numInputs == 3:
            jts = self.refineNet.computeOutput(inputs)
        else:
            raise NotImplementedError("Number of inputs is {}".format(self.refineNet.cfgParams.numInputs))
        return jts[0] * (size[2] / 2.)

    def calculateCoM(self, dpt):
        """Centre of mass (mean column, mean row, mean depth) of the pixels inside [minDepth, maxDepth]
        (handdetector.py:91-108); host NumPy -- the per-crop version used by cropArea3D(docom=True) runs on the device."""
        dc = numpy.asarray(dpt).copy()
        dc[dc < self.minDepth] = 0
        dc[dc > self.maxDepth] = 0
        ys, xs = numpy.nonzero(dc > 0)
        num = numpy.count_nonzero(dc)
        if num == 0:
            return numpy.array((0, 0, 0), float)
        return numpy.array((xs.mean() * num, ys.mean() * num, dc.sum()), float) / num

    def getCrop(self, dpt, xstart, xend, ystart, yend, zstart, zend, thresh_z=True, background=0):
        """Window of the frame, zero-padded where it leaves the frame, z-thresholded (handdetector.py:260-296)."""
        if len(dpt.shape) != 2:
            raise NotImplementedError()
        H, W = dpt.shape
        cropped = dpt[max(ystart, 0):min(yend, H), max(xstart, 0):min(xend, W)].copy()
        cropped = numpy.pad(cropped, ((abs(ystart) - max(ystart, 0), abs(yend) - min(yend, H)),
                                      (abs(xstart) - max(xstart, 0), abs(xend) - min(xend, W))), mode='constant', constant_values=background)
        if thresh_z is True:
            msk1 = numpy.logical_and(cropped < zstart, cropped != 0)
            msk2 = numpy.logical_and(cropped > zend, cropped != 0)
            cropped[msk1] = zstart
            cropped[msk2] = 0.
        return cropped

    def refineCoMIterative(self, com, num_iter, size=(250, 250, 250)):
        """Re-centre the cube on the centre of mass of its own content, num_iter times (handdetector.py:540-558)."""
        for _ in range(num_iter):
            xstart, xend, ystart, yend, zstart, zend = self.comToBounds(com, size)
            cropped = self.getCrop(self.dpt, xstart, xend, ystart, yend, zstart, zend)
            com = self.calculateCoM(cropped)
            if numpy.allclose(com, 0.):
                com[2] = cropped[cropped.shape[0] // 2, cropped.shape[1] // 2]
            com[0] += max(xstart, 0)
            com[1] += max(ystart, 0)
        return com

    # ---- crop helpers on the device (handdetector.py:132-202, 298-380, 782-803) ---------------------------------------------
    def _resize_mode(self, what):
        if self.resizeMethod == self.RESIZE_CV2_NN:
            return self.RESIZE_CV2_NN
        if self.resizeMethod == self.RESIZE_BILINEAR:
            return self.RESIZE_BILINEAR
        if self.resizeMethod == self.RESIZE_CV2_LINEAR:
            raise NotImplementedError("%s: RESIZE_CV2_LINEAR (cv2 INTER_LINEAR: fixed-point coordinates, float coefficient tables, 2x downscale "
                                      "as INTER_AREA) is not built -- it cannot be pinned without OpenCV; use RESIZE_CV2_NN or RESIZE_BILINEAR" % what)
        raise NotImplementedError("Unknown resize method!")

    @staticmethod
    def bilinearResize(src, dsize, ndValue):
        """Bilinear resize that spares out undefined depth (handdetector.py:132-202), on the device: src (h, w) -> float32
        (dsize[1], dsize[0]).  A tap equal to ndValue drops out and the remaining weights are renormalised; more than two such
        taps give ndValue.  The arithmetic is the reference's on NumPy 1 (float64 weights and sum, one rounding to float32).
        A source narrower or shorter than 2 pixels raises UserWarning("Shape mismatch") like the reference."""
        src = numpy.asarray(src)
        if src.ndim != 2:
            raise NotImplementedError("2-D depth maps only")
        return resize_crops(src[None], dsize, HandDetector.RESIZE_BILINEAR, ndValue)[0]

    def resizeCrop(self, crop, sz):
        """Resize a crop to sz = (w, h) with self.resizeMethod (handdetector.py:336-351): cv2 INTER_NEAREST or bilinearResize with
        getNDValue().  Computed in float32 (depth in mm); returned in crop's dtype under nearest neighbour, float32 under bilinear."""
        mode = self._resize_mode('resizeCrop')
        crop = numpy.asarray(crop)
        if crop.ndim != 2:
            raise NotImplementedError("2-D depth maps only")
        nd = self.getNDValue() if mode == self.RESIZE_BILINEAR else 0.
        rz = resize_crops(crop[None], sz, mode, nd)[0]
        return rz if mode == self.RESIZE_BILINEAR else rz.astype(crop.dtype, copy=False)

    def recropHand(self, crop, M, Mnew, target_size, background_value=0., nv_val=0., thresh_z=True, com=None, size=(250, 250, 250)):
        """Warp a crop in mm by dot(M, Mnew) to target_size = (w, h) (handdetector.py:782-803): cv2.warpPerspective INTER_NEAREST,
        border background_value, pixels close to nv_val -> background_value, then (thresh_z) the cube's z range around com.
        RESIZE_BILINEAR raises NotImplementedError like the reference."""
        if self.resizeMethod == self.RESIZE_BILINEAR:
            raise NotImplementedError
        self._resize_mode('recropHand')
        if thresh_z is True:
            assert com is not None
            _, _, _, _, zstart, zend = self.comToBounds(com, size)
            zr = numpy.array([[zstart, zend]], numpy.float64)
        else:
            zr = None
        crop = numpy.asarray(crop)
        out = _recrop(crop[None], numpy.asarray(M, numpy.float64)[None], numpy.asarray(Mnew, numpy.float64)[None], target_size,
                      background_value, nv_val, zr)
        return out[0]

    def getInverseCrop(self, crop, sz, xstart, xend, ystart, yend, zstart, zend, thresh_z=True, background=0):
        """Paste a crop back into a frame of shape sz (handdetector.py:298-334): the crop resized (self.resizeMethod) to the window
        (xend - xstart, yend - ystart) on a canvas of `background`, then (thresh_z) the z-threshold over the whole frame.  A window
        entirely outside the frame or of zero size gives the bare canvas.  float32."""
        mode = self._resize_mode('getInverseCrop')
        crop = numpy.asarray(crop)
        if crop.ndim != 2 or len(sz) != 2:
            raise NotImplementedError("2-D depth maps only")
        nd = self.getNDValue() if mode == self.RESIZE_BILINEAR else 0.
        bounds = numpy.array([[xstart, xend, ystart, yend, zstart, zend]], numpy.float64)
        return inverse_crops(crop[None], sz, bounds, thresh_z=thresh_z, background=background, method=mode, nd_value=nd)[0]

    def applyCrop3D(self, dpt, com, size, dsize, thresh_z=True, background=None):
        """cropArea3D's crop applied to an arbitrary image `dpt` (handdetector.py:353-380): the window of the metric cube around com
        (no detector range test), z-thresholded when thresh_z, resized with self.resizeMethod and pasted centred into dsize.
        background is both getCrop's pad value outside the frame and the fill outside the paste; background=None fills with
        getNDValue() and pads with what numpy.pad(..., constant_values=None) gives on a float32 array, NaN on current NumPy.
        float32 (dsize square)."""
        mode = self._resize_mode('applyCrop3D')
        if len(size) != 3 or len(dsize) != 2:
            raise ValueError("Size must be 3D and dsize 2D bounding box")
        if dsize[0] != dsize[1]:
            raise NotImplementedError("square destination sizes only")
        if numpy.isclose(com[2], 0.):
            raise NotImplementedError("applyCrop3D around an ill-defined CoM (com[2] == 0) is not built")
        dpt = numpy.asarray(dpt, numpy.float32)
        if dpt.ndim != 2:
            raise NotImplementedError("2-D depth maps only")
        if background is None:
            pad = float(numpy.pad(numpy.zeros((1, 1), numpy.float32), ((1, 0), (0, 0)), mode='constant', constant_values=None)[0, 0])
            fill = self.getNDValue()
        else:
            pad = fill = background
        nd = self.getNDValue()
        flags = _CROP_NO_RANGE | (0 if thresh_z is True else _CROP_NO_THRESH)
        crops, _ = crop_frames(dpt[None], numpy.asarray(com, numpy.float32)[None], numpy.asarray(size, numpy.float32)[None], self.fx, self.fy,
                               dsize[0], normalize=False, nd_value=nd, resize_method=mode, _flags=flags, _fill=fill, _pad=pad)
        return crops[0]

    def detect(self, *args, **kwargs):
        """Not built: the reference finds the hand by contour analysis of depth slabs (cv2.findContours / contourArea / moments,
        handdetector.py:569-632), which cannot be pinned without OpenCV.  Seed a track with a known centre instead (track, or
        util.realtimehandposepipeline's init_com / whole-frame centre of mass)."""
        raise NotImplementedError("hand detection (cv2.findContours slab analysis, handdetector.py:569-632) is not built: it cannot be pinned "
                                  "without OpenCV; seed the track with a known centre (RealtimeHandposePipeline(init_com=...) or reset(com))")

    _COMPONENT_DEVIATIONS = """Deviations from the reference, which walks cv2.findContours' contour list:
          1. a component's pixel count stands in for cv2.contourArea (the > 200 threshold, and "largest");
          2. among the components of the winning slab the raster-first one (smallest y * W + x) wins, not cv2's contour order;
          3. a depth exactly on a slab boundary belongs to the nearer slab only (the reference keeps it in both)."""

    def detectComponents(self, size=(250, 250, 250), doHandSize=True, max_hands=1, max_extent=None):
        """Detect the hand as the closest object to the camera, by connected components on the device: the depth range in 20 slabs,
        nearest first; the first slab with an 8-connected component of more than 200 px; the centre of mass of the +-100 px window
        around that component's centroid inside the slab; refineCoMIterative(com, 5, size); with doHandSize the cube from the bounding
        box of the largest component of the depth range com_z -+ size_z / 2 (estimateHandsizeComponents).  Returns (com, size) with
        detect's convention (handdetector.py:569-632): no hand gives ((0, 0, 0), size).

        max_hands=K > 1 returns up to K hands of the frame (find_hands): (coms (K, 3) float64, size), an empty slot being (0, 0, 0);
        max_extent (mm) keeps components wider or higher than that out.  Hand size is a one-hand procedure: with K > 1 doHandSize
        must not be True (ValueError).
        """
        if int(max_hands) > 1:
            if doHandSize is True:
                raise ValueError("hand size is measured for one hand per frame: doHandSize needs max_hands=1")
            coms, _, found = find_hands(numpy.asarray(self.dpt, numpy.float32)[None], numpy.asarray(size, numpy.float32)[None], self.fx,
                                        self.fy, max_hands=max_hands, max_extent=max_extent)
            return numpy.where(found[0][:, None], coms[0], 0).astype(numpy.float64), size
        coms, cubes, found = find_hands(numpy.asarray(self.dpt, numpy.float32)[None], numpy.asarray(size, numpy.float32)[None], self.fx,
                                        self.fy, do_hand_size=doHandSize is True, max_extent=max_extent)
        if not found[0]:
            return numpy.array((0, 0, 0), numpy.float64), size
        if doHandSize is True:
            return coms[0].astype(numpy.float64), tuple(float(c) for c in cubes[0])
        return coms[0].astype(numpy.float64), size
    detectComponents.__doc__ += "\n        " + _COMPONENT_DEVIATIONS

    def estimateHandsizeComponents(self, com, cube=(250, 250, 250), tol=0.):
        """estimateHandsize (handdetector.py:911-937) without a contour argument: the bounding box is that of the largest 8-connected
        component of the pixels with com_z - cube_z / 2 <= d <= com_z + cube_z / 2 (detect's part_ref, :616-624), measured on the
        device.  Returns the metric cube (x, y, z); an empty depth range returns `cube` unchanged.
        """
        from hipdp import ops
        from hipdp.runtime import default_runtime
        rt = default_runtime()
        frame = numpy.ascontiguousarray(self.dpt, numpy.float32)
        H, W = frame.shape
        det = _detector(rt, H, W, self.fx, self.fy, 1)
        det.frames.set(frame[None])
        det.com.set(numpy.asarray(com, numpy.float32).reshape(1, 3))
        det.cube.set(numpy.asarray(cube, numpy.float32).reshape(1, 3))
        cubes, status = det.hand_size(tol=tol)
        if status[0] & ops.DETECT_NO_SIZE:
            return tuple(cube)
        return tuple(float(c) for c in cubes[0])
    estimateHandsizeComponents.__doc__ += "\n        " + _COMPONENT_DEVIATIONS

    def track(self, com, size=(250, 250, 250), dsize=(128, 128), doHandSize=True):
        """Follow the hand from the previous frame's centre `com` (handdetector.py:504-544): the window of the cube around com,
        resized to dsize as it is, goes through the refinement net; returns (new centre in image coordinates, size).  One frame
        through the kernels of hipdp.tracker (frame_range, crop_prepare_ranged, crop_warp, the net's plan, track_refine).
        dsize must be the refinement net's input size, as in the reference.  doHandSize=True (hand-size estimation from
        cv2.findContours, :527-542) is not built.  A centre whose depth is close to 0 cannot be tracked from (comToBounds'
        ill-defined branch is not built either): ValueError."""
        if self.refineNet is None or self.importer is None:
            raise RuntimeError("Need refineNet for this")
        if doHandSize is True:
            raise NotImplementedError("track(doHandSize=True): hand-size estimation needs cv2.findContours (handdetector.py:527-542), which is "
                                      "not built; pass doHandSize=False")
        if numpy.isclose(com[2], 0.):
            raise ValueError("track from an ill-defined CoM (com[2] == 0) is not built")
        if dsize[0] != dsize[1]:
            raise NotImplementedError("square destination sizes only")
        from hipdp import ops, tracker
        from hipdp.augmenter import camera_tuple
        from hipdp.runtime import default_runtime
        rt = default_runtime()
        ceng = tracker._engine_b1(self.refineNet, rt, 'refineNet')
        if int(ceng.x_ins[0].shape[1]) != int(dsize[0]):
            raise ValueError("dsize %r is not the refinement net's input size %d" % (tuple(dsize), ceng.x_ins[0].shape[1]))
        frame = numpy.ascontiguousarray(self.dpt, numpy.float32)
        H, W = frame.shape
        fr = rt.upload(frame[None])
        st = rt.alloc(16, numpy.float32)                     # centre in, centre out, com3D, status
        com_in, com_out, com3d, status = st.view(0, (1, 3)), st.view(3, (1, 3)), st.view(6, (1, 3)), st.view(9, (1,), numpy.int32)
        host = numpy.zeros(16, numpy.float32)
        host[0:3] = numpy.asarray(com, numpy.float32)
        st.set(host)
        cube = rt.upload(numpy.asarray(size, numpy.float32).reshape(1, 3))
        partial = ops.frame_range_workspace(rt, 1)
        rec = rt.alloc(rt.lib.dpp_crop_record_bytes(), numpy.uint8)
        ops.frame_range(rt, fr, 1, H, W, partial)(rt.stream)
        plan = ops.Plan('track1')
        for op, side in tracker.refine_stage(rt, fr, H, W, partial, rec, com_in, cube, ceng, camera_tuple(self.importer), self.fx, self.fy,
                                             int(dsize[0]), com_out, com3d, rec, status):
            plan.add(op, side)
        plan.run(rt)
        rt.synchronize()
        return st.get()[3:6].copy(), size


_CROP_NORMALIZE, _CROP_BILINEAR, _CROP_NO_RANGE, _CROP_NO_THRESH = 1, 2, 4, 8     # hipdp.ops.CROP_* (dpp_crop_warp_ex flags)


def _bounds(com, size, fx, fy):
    """comToBounds (handdetector.py:204-226) without the ill-defined branch, in the device's arithmetic (com as float32)."""
    c0, c1, c2 = float(numpy.float32(com[0])), float(numpy.float32(com[1])), float(numpy.float32(com[2]))
    s0, s1 = float(numpy.float32(size[0])), float(numpy.float32(size[1]))
    return (int(numpy.floor((c0 * c2 / fx - s0 / 2.) / c2 * fx + 0.5)), int(numpy.floor((c0 * c2 / fx + s0 / 2.) / c2 * fx + 0.5)),
            int(numpy.floor((c1 * c2 / fy - s1 / 2.) / c2 * fy + 0.5)), int(numpy.floor((c1 * c2 / fy + s1 / 2.) / c2 * fy + 0.5)))


def _check_bilinear(sw, sh, dw, dh):
    """bilinearResize raises UserWarning("Shape mismatch") when a tap leaves the source (handdetector.py:160-162); its last row
    and column reach furthest."""
    x = int((dw - 1) * (float(sw - 1) / dw)) if dw > 0 else 0
    y = int((dh - 1) * (float(sh - 1) / dh)) if dh > 0 else 0
    if sw < 2 or sh < 2 or x + 1 >= sw or y + 1 >= sh:
        raise UserWarning("Shape mismatch")


def _method(method):
    if method == HandDetector.RESIZE_CV2_NN:
        return False
    if method == HandDetector.RESIZE_BILINEAR:
        return True
    if method == HandDetector.RESIZE_CV2_LINEAR:
        raise NotImplementedError("RESIZE_CV2_LINEAR (cv2 INTER_LINEAR) is not built: it cannot be pinned without OpenCV")
    raise NotImplementedError("Unknown resize method!")


def crop_frames(frames, coms, cubes, fx, fy, dsize=128, normalize=True, nd_value=0., runtime=None, docom=False, return_com=False,
                stretch=False, resize_method=HandDetector.RESIZE_CV2_NN, _flags=0, _fill=None, _pad=0.):
    """Batched cropArea3D (+ Dataset.imgStackDepthOnly when normalize): frames (B, H, W) raw depth in mm, coms (B, 3) crop
    centres in image coordinates, cubes (B, 3) in mm -> (crops (B, dsize, dsize) float32, M (B, 3, 3) float32[, coms]).
    Two kernel launches for the whole batch (csrc/crop.hip: crop_prepare / crop_warp); docom=True re-centres every crop
    on the centre of mass of its first window (two more launches), as handdetector.py:413-427 does; stretch=True resizes the
    window to dsize x dsize as it is (resizeCrop(cropped, dsize), the refinement net's input, :430).  resize_method
    RESIZE_BILINEAR resizes the window with bilinearResize (ND value nd_value) instead of nearest neighbour; a window
    narrower or shorter than 2 pixels then raises UserWarning("Shape mismatch")."""
    from hipdp import ops
    from hipdp.runtime import default_runtime
    bilinear = _method(resize_method)
    rt = runtime or default_runtime()
    frames = numpy.ascontiguousarray(frames, numpy.float32)
    B, H, W = frames.shape
    fr = rt.upload(frames)
    co = rt.upload(numpy.ascontiguousarray(coms, numpy.float32).reshape(B, 3))
    cu = rt.upload(numpy.ascontiguousarray(cubes, numpy.float32).reshape(B, 3))
    rec = rt.alloc(B * rt.lib.dpp_crop_record_bytes(), numpy.uint8)
    out, M = rt.alloc((B, dsize, dsize), zero=False), rt.alloc((B, 9), zero=False)
    ops.crop_prepare(rt, fr, B, H, W, co, cu, fx, fy, dsize, rec, M, stretch=stretch)(rt.stream)
    if docom:
        co2 = rt.alloc((B, 3), zero=False)
        ops.crop_com(rt, fr, rec, B, H, W, co2)(rt.stream)
        ops.crop_prepare(rt, fr, B, H, W, co2, cu, fx, fy, dsize, rec, M, stretch=stretch)(rt.stream)
        co = co2
    if bilinear:
        cube_h = numpy.ascontiguousarray(cubes, numpy.float32).reshape(B, 3)
        com_h = co.get() if docom else numpy.ascontiguousarray(coms, numpy.float32).reshape(B, 3)
        for i in range(B):
            xs, xe, ys, ye = _bounds(com_h[i], cube_h[i], abs(fx), abs(fy))
            wb, hb = xe - xs, ye - ys
            if stretch:
                dw, dh = dsize, dsize
            elif wb > hb:
                dw, dh = dsize, (hb * dsize) // wb
            else:
                dw, dh = (wb * dsize) // hb if hb else 0, dsize
            _check_bilinear(wb, hb, dw, dh)
    if bilinear or _flags or _fill is not None or _pad != 0.:
        flags = _flags | (_CROP_NORMALIZE if normalize else 0) | (_CROP_BILINEAR if bilinear else 0)
        ops.crop_warp_ex(rt, fr, rec, B, H, W, dsize, out, flags=flags, nd_value=nd_value, fill_value=_fill, pad_value=_pad)(rt.stream)
    else:
        ops.crop_warp(rt, fr, rec, B, H, W, dsize, out, normalize=normalize, nd_value=nd_value)(rt.stream)
    rt.synchronize()
    if return_com:
        return out.get(), M.get().reshape(B, 3, 3), co.get()
    return out.get(), M.get().reshape(B, 3, 3)


def resize_crops(crops, sz, method=HandDetector.RESIZE_CV2_NN, nd_value=0., runtime=None):
    """Batched resizeCrop: crops (B, h, w) -> float32 (B, sz[1], sz[0]) (sz in cv2's (w, h) order), cv2 INTER_NEAREST
    (RESIZE_CV2_NN) or bilinearResize with nd_value (RESIZE_BILINEAR).  One launch."""
    from hipdp import ops
    from hipdp.runtime import default_runtime
    bilinear = _method(method)
    crops = numpy.ascontiguousarray(crops, numpy.float32)
    if crops.ndim != 3:
        raise ValueError("crops must be (B, h, w)")
    B, sh, sw = crops.shape
    dw, dh = int(sz[0]), int(sz[1])
    if dw < 1 or dh < 1:
        raise ValueError("empty destination size %r" % (tuple(sz),))
    if bilinear:
        _check_bilinear(sw, sh, dw, dh)
    rt = runtime or default_runtime()
    src = rt.upload(crops)
    out = rt.alloc((B, dh, dw), zero=False)
    ops.resize_crops(rt, src, B, sh, sw, dh, dw, out, bilinear=bilinear, nd_value=nd_value)(rt.stream)
    rt.synchronize()
    return out.get()


def _recrop(crops, M, Mnew, target_size, background_value, nv_val, zrange, runtime=None):
    from hipdp import ops
    from hipdp.runtime import default_runtime
    crops = numpy.ascontiguousarray(crops, numpy.float32)
    if crops.ndim != 3:
        raise ValueError("crops must be (B, h, w)")
    B, h, w = crops.shape
    tw, th = int(target_size[0]), int(target_size[1])
    if tw < 1 or th < 1:
        raise ValueError("empty target size %r" % (tuple(target_size),))
    rt = runtime or default_runtime()
    src = rt.upload(crops)
    m = rt.upload(numpy.ascontiguousarray(M, numpy.float64).reshape(B, 9))
    mn = rt.upload(numpy.ascontiguousarray(Mnew, numpy.float64).reshape(B, 9))
    zr = None if zrange is None else rt.upload(numpy.ascontiguousarray(zrange, numpy.float64).reshape(B, 2).astype(numpy.float32))
    out = rt.alloc((B, th, tw), zero=False)
    ops.recrop(rt, src, B, h, w, m, mn, th, tw, out, background=background_value, nv_val=nv_val, zrange=zr)(rt.stream)
    rt.synchronize()
    return out.get()


def recrop_crops(crops, M, Mnew, target_size, coms, sizes, fx, fy, background_value=0., nv_val=0., thresh_z=True, min_depth=None,
                 max_depth=None, runtime=None):
    """Batched recropHand (RESIZE_CV2_NN): crops (B, h, w) in mm, M / Mnew (B, 3, 3), target_size (w, h), coms (B, 3) and sizes
    (B, 3) for the z range (comToBounds) -> float32 (B, h', w').  A crop whose com[2] is close to 0 takes comToBounds' ill-defined
    branch, whose z range is the detector's [min_depth, max_depth] (then required).  One launch."""
    crops = numpy.asarray(crops)
    B = crops.shape[0]
    zr = None
    if thresh_z is True:
        coms = numpy.asarray(coms).reshape(B, 3)
        sizes = numpy.asarray(sizes).reshape(B, 3)
        zr = numpy.empty((B, 2), numpy.float64)
        for i in range(B):
            if numpy.isclose(coms[i][2], 0.):
                if min_depth is None or max_depth is None:
                    raise ValueError("crop %d: ill-defined CoM (z == 0) needs min_depth / max_depth" % i)
                zr[i] = (min_depth, max_depth)
            else:
                zr[i] = (float(coms[i][2]) - sizes[i][2] / 2., float(coms[i][2]) + sizes[i][2] / 2.)
    return _recrop(crops, numpy.asarray(M, numpy.float64).reshape(B, 3, 3), numpy.asarray(Mnew, numpy.float64).reshape(B, 3, 3), target_size,
                   background_value, nv_val, zr, runtime)


def inverse_crops(crops, frame_shape, bounds, thresh_z=True, background=0., method=HandDetector.RESIZE_CV2_NN, nd_value=0., runtime=None):
    """Batched getInverseCrop: crops (B, h, w) pasted into frames of frame_shape (H, W) at bounds (B, 6) = (xstart, xend, ystart,
    yend, zstart, zend) per crop (comToBounds' order) -> float32 (B, H, W).  method: RESIZE_CV2_NN or RESIZE_BILINEAR (ND value
    nd_value).  One launch."""
    from hipdp import ops
    from hipdp.runtime import default_runtime
    bilinear = _method(method)
    crops = numpy.ascontiguousarray(crops, numpy.float32)
    if crops.ndim != 3:
        raise ValueError("crops must be (B, h, w)")
    B, ch, cw = crops.shape
    H, W = int(frame_shape[0]), int(frame_shape[1])
    bounds = numpy.asarray(bounds, numpy.float64).reshape(B, 6)
    box = numpy.ascontiguousarray(bounds[:, :4]).astype(numpy.int64)
    if not numpy.array_equal(box, bounds[:, :4]) or numpy.abs(box).max(initial=0) >= 2 ** 30:
        raise ValueError("window bounds must be integers")
    for xs, xe, ys, ye in box:
        early = (xe < 0 and xs < 0) or (ye < 0 and ys < 0) or (xe > W and xs > W) or (ye > H and ys > H) or xe == xs or ye == ys
        if early:
            continue
        if xe < xs or ye < ys:
            raise ValueError("window of negative size: (%d, %d, %d, %d)" % (xs, xe, ys, ye))
        if bilinear:
            _check_bilinear(cw, ch, xe - xs, ye - ys)
    rt = runtime or default_runtime()
    src = rt.upload(crops)
    bd = rt.upload(box.astype(numpy.int32))
    zr = rt.upload(numpy.ascontiguousarray(bounds[:, 4:]).astype(numpy.float32)) if thresh_z is True else None
    out = rt.alloc((B, H, W), zero=False)
    ops.inverse_crop(rt, src, B, ch, cw, bd, H, W, out, bilinear=bilinear, nd_value=nd_value, background=background, zrange=zr)(rt.stream)
    rt.synchronize()
    return out.get()


_DEVICE_CACHE = {}                 # (kind, id(runtime), shape, ...) -> FrameDetector / ComponentWorkspace: allocated once per shape
_DEVICE_CACHE_MAX = 4


def _cached(key, make):
    """The device workspaces of the batched detection calls are large (40 bytes per pixel of statistics): one per shape is kept and
    used again, the oldest of more than a few dropped."""
    if key not in _DEVICE_CACHE:
        while len(_DEVICE_CACHE) >= _DEVICE_CACHE_MAX:
            _DEVICE_CACHE.pop(next(iter(_DEVICE_CACHE)))
        _DEVICE_CACHE[key] = (make(), key[1])
    return _DEVICE_CACHE[key][0]


def label_components(keys, runtime=None, return_stats=False):
    """8-connected component labelling on the device: keys (B, H, W) uint8, 255 = background -> labels (B, H, W) int32, the smallest
    linear index y * W + x of the pixel's component of equal key, -1 for background.  With return_stats also a dict of arrays, one
    entry per component ordered by (frame, root): frame, root, key, count, xmin, xmax, ymin, ymax, sum_x, sum_y (integers, exact)."""
    from hipdp import ops
    from hipdp.runtime import default_runtime
    rt = runtime or default_runtime()
    keys = numpy.ascontiguousarray(keys, numpy.uint8)
    if keys.ndim != 3:
        raise ValueError("keys must be (B, H, W)")
    B, H, W = keys.shape
    ws = _cached(('labels', rt, B, H, W, bool(return_stats)), lambda: ops.ComponentWorkspace(rt, B, H, W, stats=return_stats))
    ws.keys.set(keys)
    ops.label_components(rt, ws, stats=return_stats)(rt.stream)
    rt.synchronize()
    labels = ws.labels.get().reshape(B, H, W)
    if not return_stats:
        return labels
    rec = ws.stats.get().view(ops.COMPONENT_STAT).reshape(B, H * W)
    fb, root = numpy.nonzero(labels.reshape(B, H * W) == numpy.arange(H * W, dtype=numpy.int32)[None])
    r = rec[fb, root]
    stats = dict(frame=fb.astype(numpy.int32), root=root.astype(numpy.int32), key=keys.reshape(B, H * W)[fb, root], count=r['count'].copy(),
                 xmin=~r['ixmin'], xmax=r['xmax'].copy(), ymin=~r['iymin'], ymax=r['ymax'].copy(),
                 sum_x=r['sum_x'].astype(numpy.int64), sum_y=r['sum_y'].astype(numpy.int64))
    return labels, stats


def _detector(rt, H, W, fx, fy, B, hands=1, max_extent=None):
    from hipdp import detect
    ext = float(max_extent) if max_extent else 0.0
    return _cached(('detector', rt, B, H, W, abs(float(fx)), abs(float(fy)), int(hands), ext),
                   lambda: detect.FrameDetector(rt, H, W, fx, fy, B, hands=hands, max_extent=max_extent))


def find_hands(frames, cubes, fx, fy, do_hand_size=False, runtime=None, return_seed=False, chunk=8, max_hands=1, max_extent=None):
    """Batched HandDetector.detectComponents: frames (B, H, W) raw depth in mm, cubes (B, 3) -> (coms (B, 3) float32 in image
    coordinates, cubes (B, 3) float32, found (B,) bool).  One device plan per chunk of frames (hipdp.detect.FrameDetector, kept
    per frame shape and used again by later calls): depth
    range, slab keys, labelling, seed, refineCoMIterative(5) and, with do_hand_size, the hand's cube; a frame without a hand gets
    com (0, 0, 0) and its input cube.  return_seed adds the centres before the refinement.

    max_hands=K > 1 finds up to K hands per frame in the same plan (one launch more): coms (B, K, 3), cubes (B, K, 3) (the frame's
    cube in every slot), found (B, K), seeds likewise; slot k is the k-th accepted component in (slab, raster) order, empty slots are
    all zero.  The candidates are the components of more than 200 px; one whose centroid lies in the +-100 px seed window of an
    accepted one is suppressed (a hand across a slab boundary is two components), and with max_extent (mm) one wider or higher than
    that at its slab's far bound is no candidate at all (a wall is no hand).  Both rules are this project's, not the reference's.
    max_hands=1 returns today's shapes.  Hand size is a one-hand procedure: do_hand_size with max_hands > 1 raises ValueError."""
    from hipdp.runtime import default_runtime
    rt = runtime or default_runtime()
    frames = numpy.ascontiguousarray(frames, numpy.float32)
    if frames.ndim != 3:
        raise ValueError("frames must be (B, H, W)")
    B, H, W = frames.shape
    cubes = numpy.ascontiguousarray(cubes, numpy.float32).reshape(B, 3)
    K = int(max_hands)
    if do_hand_size and K > 1:
        raise ValueError("hand size is measured for one hand per frame: do_hand_size needs max_hands=1")
    if K == 1 and not max_extent:
        coms, sizes, found, seeds = (numpy.zeros((B, 3), numpy.float32), cubes.copy(), numpy.zeros(B, bool), numpy.zeros((B, 3), numpy.float32))
        for i0 in range(0, B, chunk):
            n = min(chunk, B - i0)
            det = _detector(rt, H, W, fx, fy, n)
            coms[i0:i0 + n], sizes[i0:i0 + n], found[i0:i0 + n], seeds[i0:i0 + n], _ = det.run(frames[i0:i0 + n], cubes[i0:i0 + n], do_hand_size)
        return (coms, sizes, found, seeds) if return_seed else (coms, sizes, found)
    coms, sizes, found, seeds = (numpy.zeros((B, K, 3), numpy.float32), numpy.zeros((B, K, 3), numpy.float32), numpy.zeros((B, K), bool),
                                 numpy.zeros((B, K, 3), numpy.float32))
    for i0 in range(0, B, chunk):
        n = min(chunk, B - i0)
        det = _detector(rt, H, W, fx, fy, n, K, max_extent)
        coms[i0:i0 + n], sizes[i0:i0 + n], found[i0:i0 + n], seeds[i0:i0 + n] = det.run(frames[i0:i0 + n], cubes[i0:i0 + n], do_hand_size)[:4]
    if K == 1:                                       # one hand under the extent filter: today's shapes
        coms, sizes, found, seeds = coms[:, 0], sizes[:, 0], found[:, 0], seeds[:, 0]
    return (coms, sizes, found, seeds) if return_seed else (coms, sizes, found)


def refine_com_iterative(frames, coms, cubes, fx, fy, num_iter, runtime=None, return_status=False):
    """Batched HandDetector.refineCoMIterative (handdetector.py:546-567) on the device: frames (B, H, W) raw depth in mm (the
    detector's range [max(10, min), min(1500, max)] is applied per frame as the constructor does), coms (B, 3), cubes (B, 3) ->
    float32 (B, 3).  Two launches for the whole batch: the depth ranges, then one workgroup per frame runs all num_iter iterations
    with a float64 centre (window sums in float64, where the host method sums depth in the frame's dtype).  A frame whose centre's
    depth becomes close to 0 (comToBounds' ill-defined branch) is finished by the host method."""
    from hipdp import ops
    from hipdp.runtime import default_runtime
    rt = runtime or default_runtime()
    frames = numpy.ascontiguousarray(frames, numpy.float32)
    B, H, W = frames.shape
    fr = rt.upload(frames)
    co = rt.upload(numpy.ascontiguousarray(coms, numpy.float32).reshape(B, 3))
    cu = rt.upload(numpy.ascontiguousarray(cubes, numpy.float32).reshape(B, 3))
    partial = ops.frame_range_workspace(rt, B)
    out, status = rt.alloc((B, 3), zero=False), rt.alloc((B,), numpy.int32)
    ops.frame_range(rt, fr, B, H, W, partial)(rt.stream)
    ops.refine_com_iterative(rt, fr, partial, B, H, W, co, cu, abs(fx), abs(fy), int(num_iter), out, status)(rt.stream)
    rt.synchronize()
    res, st = out.get(), status.get()
    for i in numpy.nonzero(st)[0]:
        hd = HandDetector(frames[i].copy(), abs(fx), abs(fy))
        res[i] = hd.refineCoMIterative(numpy.asarray(coms[i], numpy.float64), int(num_iter), tuple(float(c) for c in numpy.asarray(cubes[i])))
    return (res, st) if return_status else res
