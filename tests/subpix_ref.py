"""cv2.cornerSubPix, cv2.getRectSubPix and cv2.cvtColor(COLOR_BGR2GRAY) on uint8, restated in NumPy from recollection
(UNPINNED, cv2 is not installed here) with float32 and float64 exactly where
include/calibrating_amd.h says.  The GPU kernels (csrc/subpix.hip) must match ``order="wave"`` bit for bit.

Switches.  ``order``: "cv2" adds the window's pixels one after the other, as cv2's loop does; "wave" adds them as the
kernel does -- pixel k belongs to lane k % 64, a lane adds its pixels in rising k, an xor butterfly (1, 2, ... 32) joins the
lanes.  ``bilinear`` (U31): "four_tap" forms a patch sample as ((a11 p00 + a12 p01) + a21 p10) + a22 p11, the kernel's
form; "running" is cv2's one-channel loop as recalled, which carries a product from column to column and can differ in
the last float32 bit.  ``bits`` (U32): 15 = OpenCV 4.x's gray weights, 14 = older releases'.
"""
import numpy as np

F = np.float32
SINGULAR, LEFT_IMAGE, REVERTED, BAD_START = 1, 2, 4, 8
GRAY_WEIGHTS = {15: (3735, 19235, 9798), 14: (1868, 9617, 4899)}  # B, G, R
DBL_EPSILON = np.finfo(np.float64).eps
LANE = np.arange(64)


def gray(img, code="bgr", bits=15):
    """(..., 3) uint8 -> (...) uint8: (c0 BY + c1 GY + c2 RY + half) >> bits with code "bgr"; "rgb" swaps BY and RY."""
    by, gy, ry = GRAY_WEIGHTS[bits]
    k = (by, gy, ry) if code == "bgr" else (ry, gy, by)
    c = np.asarray(img).astype(np.int64)
    return ((c[..., 0] * k[0] + c[..., 1] * k[1] + c[..., 2] * k[2] + (1 << (bits - 1))) >> bits).astype(np.uint8)


def exp32(v):
    """expf, correctly rounded: the float64 exponential rounded to float32"""
    return F(np.exp(np.float64(v)))


def mask(win, zero_zone=(-1, -1)):
    ww, wh = win
    m = np.zeros((2 * wh + 1, 2 * ww + 1), F)
    for i in range(2 * wh + 1):
        y = F(i - wh) / F(wh)
        vy = exp32(-(y * y))
        for j in range(2 * ww + 1):
            x = F(j - ww) / F(ww)
            m[i, j] = F(vy * exp32(-(x * x)))
    zx, zy = zero_zone
    if zx >= 0 and zy >= 0 and zx * 2 + 1 < ww * 2 + 1 and zy * 2 + 1 < wh * 2 + 1:
        for i in range(wh - zy, wh + zy + 1):
            for j in range(ww - zx, ww + zx + 1):
                m[i, j] = 0
    return m


def criteria(c):
    """(max_iters, eps squared) of (count, eps) -- None = not carried -- or cv2's (type, count, eps)"""
    if len(c) == 3:
        c = (c[1] if c[0] & 1 else None, c[2] if c[0] & 2 else None)
    count, eps = c
    max_iters = 100 if count is None else min(max(int(count), 1), 100)
    eps = 0.0 if eps is None else max(float(eps), 0.0)
    return max_iters, eps * eps


def rect_sub_pix(img, cx, cy, pw, ph, bilinear="four_tap"):
    """getRectSubPix(img, (pw, ph), (cx, cy)) -> (ph, pw) float32; the centre is float32; replicate border"""
    h, w = img.shape
    x = F(cx) - F(pw - 1) * F(0.5)
    y = F(cy) - F(ph - 1) * F(0.5)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = int(fx), int(fy)
    a, b = F(x - fx), F(y - fy)
    x0, x1 = np.clip(ix + np.arange(pw), 0, w - 1), np.clip(ix + 1 + np.arange(pw), 0, w - 1)
    y0, y1 = np.clip(iy + np.arange(ph), 0, h - 1), np.clip(iy + 1 + np.arange(ph), 0, h - 1)
    one = F(1)
    if bilinear == "four_tap":
        a11, a12, a21, a22 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
        p00, p01 = img[y0][:, x0].astype(F), img[y0][:, x1].astype(F)
        p10, p11 = img[y1][:, x0].astype(F), img[y1][:, x1].astype(F)
        return ((a11 * p00 + a12 * p01) + a21 * p10) + a22 * p11
    assert bilinear == "running"
    a = max(a, F(0.0001))
    a12, a22, b1, b2 = a * (one - b), a * b, one - b, b
    s = (one - a) / a
    out = np.empty((ph, pw), F)
    for i in range(ph):
        r0, r1 = img[y0[i]].astype(F), img[y1[i]].astype(F)
        prev = (one - a) * (b1 * r0[x0[0]] + b2 * r1[x0[0]])
        for j in range(pw):
            t = a12 * r0[x1[j]] + a22 * r1[x1[j]]
            out[i, j] = prev + t
            prev = F(t * s)
    return out


def _sum(v, order):
    if order == "cv2":
        return np.add.accumulate(np.concatenate([[0.0], v]))[-1]
    assert order == "wave"
    part = np.zeros(64)  # a lane's sum in rising k, from +0; a lane beyond the window in the last round adds nothing
    for r in range(-(-len(v) // 64)):
        n = min(64, len(v) - 64 * r)
        part[:n] = part[:n] + v[64 * r:64 * r + n]
    for m in (1, 2, 4, 8, 16, 32):
        part = part + part[LANE ^ m]
    return part[0]


def refine(img, start, win, m, max_iters, eps, order="cv2", bilinear="four_tap"):
    """One corner -> (x, y float32, iterations, status)"""
    h, w = img.shape
    ww, wh = win
    cT = (F(start[0]), F(start[1]))
    if not (np.isfinite(cT[0]) and np.isfinite(cT[1]) and 0 <= cT[0] < w and 0 <= cT[1] < h):
        return start[0], start[1], 0, BAD_START
    cI = cT
    m64 = m.astype(np.float64).reshape(-1)
    py, px = np.mgrid[-wh:wh + 1, -ww:ww + 1]
    px, py = px.reshape(-1).astype(np.float64), py.reshape(-1).astype(np.float64)
    it = count = status = 0
    with np.errstate(all="ignore"):
        while True:
            count += 1
            p = rect_sub_pix(img, cI[0], cI[1], 2 * ww + 3, 2 * wh + 3, bilinear).astype(np.float64)
            tgx = (p[1:-1, 2:] - p[1:-1, :-2]).reshape(-1)
            tgy = (p[2:, 1:-1] - p[:-2, 1:-1]).reshape(-1)
            gxx, gxy, gyy = tgx * tgx * m64, tgx * tgy * m64, tgy * tgy * m64
            a, b, c = _sum(gxx, order), _sum(gxy, order), _sum(gyy, order)
            bb1, bb2 = _sum(gxx * px + gxy * py, order), _sum(gxy * px + gyy * py, order)
            det = a * c - b * b
            if not abs(det) > DBL_EPSILON * DBL_EPSILON:
                status |= SINGULAR
                break
            scale = 1.0 / det
            nx = F(np.float64(cI[0]) + c * scale * bb1 - b * scale * bb2)
            ny = F(np.float64(cI[1]) - b * scale * bb1 + a * scale * bb2)
            dx, dy = np.float64(F(nx - cI[0])), np.float64(F(ny - cI[1]))
            err = dx * dx + dy * dy
            cI = (nx, ny)
            if not (0 <= cI[0] < w and 0 <= cI[1] < h):
                status |= LEFT_IMAGE
                break
            it += 1
            if not (it < max_iters and err > eps):
                break
        if not (abs(F(cI[0] - cT[0])) <= ww and abs(F(cI[1] - cT[1])) <= wh):
            cI = cT
            status |= REVERTED
    return cI[0], cI[1], count, status


def corner_sub_pix(images, corners, win=(4, 4), zero_zone=(-1, -1), crit=(30, 0.01), frame_of=None, order="cv2",
                   bilinear="four_tap"):
    """``corners`` (n, 2) float32 / float64 on gray ``images`` (h, w) or (f, h, w) with ``frame_of`` (n,) -> (corners in
    the same type, iterations, status)"""
    images = np.asarray(images)
    if images.ndim == 2:
        images = images[None]
    corners = np.asarray(corners)
    frame_of = np.zeros(len(corners), int) if frame_of is None else frame_of
    m = mask(win, zero_zone)
    max_iters, eps = criteria(crit)
    out = corners.copy()
    its, sts = np.zeros(len(corners), np.int32), np.zeros(len(corners), np.int32)
    for q, (c, f) in enumerate(zip(corners, frame_of)):
        out[q, 0], out[q, 1], its[q], sts[q] = refine(images[f], c, win, m, max_iters, eps, order, bilinear)
    return out, its, sts
