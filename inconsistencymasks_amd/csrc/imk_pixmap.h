// The flip / quarter-turn pixel map of augment_image_and_mask (functions.py:2795-2818): cv2.flip(., 0) if flip_v, cv2.flip(., 1) if
// flip_h, then cv2.rotate by rot (0 none, 1 = 90 CW, 2 = 180, 3 = 90 CCW).  ONE definition, shared by augment_kernel (imk_aug.hip:
// image and mask) and the teacher-label kernels (imk_student.hip: the label lands where the image's pixel lands).
#pragma once
#include "imk_common.h"

// output pixel (yo, xo) -> the source pixel it shows.  Quarter turns only with H == W (the hosts refuse the others).
__device__ __forceinline__ void imk_aug_src(int flip_v, int flip_h, int rot, int H, int W, int yo, int xo, int &ys, int &xs) {
    switch (rot) {                                              // undo the rotation
        case 1: ys = H - 1 - xo; xs = yo; break;                // ROTATE_90_CLOCKWISE
        case 2: ys = H - 1 - yo; xs = W - 1 - xo; break;        // ROTATE_180
        case 3: ys = xo; xs = W - 1 - yo; break;                // ROTATE_90_COUNTERCLOCKWISE
        default: ys = yo; xs = xo;
    }
    if (flip_h) xs = W - 1 - xs;
    if (flip_v) ys = H - 1 - ys;
}
