// crop_rec.h -- the crop record that crop.hip's prepare launches write and its warp launches read, one per frame or track
// (dpp_crop_record_bytes()).  crop.hip owns every field; background.hip reads the window of a track's final crop (xstart, ystart, cw,
// ch as track_refine left them: the empty window, cw = ch = 0, for a lost or gated track) to keep the tracked hand out of the
// background model.
#pragma once

namespace {

struct CropRec {
    int xstart, ystart, cw, ch;    // crop window in the frame (may leave the frame: zero padding)
    int szw, szh, xs, ys;          // resized size and paste offset inside the dsz x dsz output
    double ifx, ify;               // resizeNN: source index = min(floor(x * ifx), cw - 1)
    float min_depth, max_depth;    // detector range: outside -> 0
    float zstart, zend;
    float far_v, norm_off, norm_div;
};

}  // namespace
