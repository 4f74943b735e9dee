"""NumPy model of cv2.remap(src, map16SC2, map16UC1, INTER_LINEAR) on 8-bit images with BORDER_CONSTANT 0: the second
half of cv2.undistort (stereo_camera.py:430-431), what k_remap_fixed_bilinear implements.

Independent of the kernel and of the oracle's remap loop; only the weight table comes from the oracle
(``oracle.bilinear_itab()``: 32 x 32 phase entries of 4 int16 weights summing to 32768).  Per destination pixel
(OpenCV's remapBilinear): the cell corner (sx, sy) from the int16 map, the phase entry ``mapa & 1023`` (cv2 masks the
fractional map to INTER_TAB_SIZE^2 - 1), the four taps (sx, sy), (sx+1, sy), (sx, sy+1), (sx+1, sy+1) -- each one the
source pixel when it lies inside the image, 0 otherwise -- accumulated in int32 and rounded by (sum + 2^14) >> 15,
saturated to 0..255."""
import numpy as np


def remap_fixed_bilinear(src, mapxy, mapa, itab):
    """src (h, w) or (h, w, cn) uint8; mapxy (dh, dw, 2) int16; mapa (dh, dw) uint16 (or its int16 view); itab
    (1024, 4) int16.  -> (dh, dw[, cn]) uint8."""
    src = np.asarray(src, np.uint8)
    img = src if src.ndim == 3 else src[..., None]
    out = remap_fixed_bilinear_batch(img[None], mapxy, mapa, itab)[0]
    return out if src.ndim == 3 else out[..., 0]


def remap_fixed_bilinear_batch(imgs, mapxy, mapa, itab):
    """The same for a batch (n, h, w, cn) through one pair of maps -> (n, dh, dw, cn) uint8."""
    imgs = np.asarray(imgs, np.uint8)
    sh, sw = imgs.shape[1:3]
    sx = np.asarray(mapxy[..., 0], np.int64)
    sy = np.asarray(mapxy[..., 1], np.int64)
    a = np.asarray(mapa).view(np.uint16).astype(np.int64) & 1023
    w = np.asarray(itab, np.int32)[a]  # (dh, dw, 4)
    acc = np.zeros((imgs.shape[0],) + sx.shape + (imgs.shape[3],), np.int32)  # (at most 255 * 32768: no overflow)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
        wk = np.where(inside, w[..., k], 0)[None, ..., None]  # a tap outside the image reads the border value 0
        acc += imgs[:, np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)] * wk
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
