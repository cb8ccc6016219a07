"""Plain Python restatement of the OpenCV 4.x drawing functions the reference's `_draw_tracking` calls
(marker_detection.py:398-427), from imgproc/src/drawing.cpp, for 3-channel uint8 images, LINE_8 and shift 0:

    circle(img, c, r, color, -1)          -> Circle(fill=1)
    line(img, p0, p1, color, t > 1)       -> ThickLine: FillConvexPoly (XY_SHIFT = 16, outline by Line2 after clipLine)
                                             + two radius-(t/2) filled Circle caps
    arrowedLine(img, p0, p1, color, t, tipLength)

Every function paints sequentially into `img` (NumPy [H,W,3], BGR), exactly as cv2 would; C++ integer semantics are kept
(division truncates toward zero, cvRound rounds half to even).  This is the truth the device overlay (`vbs_draw_tracking`)
is tested against.  No cv2 is available to check this file itself: it is a restatement, unverified against OpenCV.
"""
import math

import numpy as np

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT
DBL_EPSILON = 2.220446049250313e-16


def _cdiv(a, b):
    """C integer division (toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def cv_round(v):
    return int(np.rint(v))


def _hline(img, y, x1, x2, color):
    h, w = img.shape[:2]
    if y < 0 or y >= h:
        return
    x1, x2 = max(x1, 0), min(x2, w - 1)
    if x1 <= x2:
        img[y, x1:x2 + 1] = color


def _put(img, x, y, color):
    h, w = img.shape[:2]
    if 0 <= x < w and 0 <= y < h:
        img[y, x] = color


def _circle_filled(img, cx, cy, radius, color):
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        _hline(img, cy - dy, cx - dx, cx + dx, color)
        _hline(img, cy + dy, cx - dx, cx + dx, color)
        _hline(img, cy - dx, cx - dy, cx + dy, color)
        _hline(img, cy + dx, cx - dy, cx + dy, color)
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2


def _clip_line(w, h, x1, y1, x2, y2):
    right, bottom = w - 1, h - 1
    if w <= 0 or h <= 0:
        return None
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (x1, y1, x2, y2) if (c1 | c2) == 0 else None


def _line2(img, x1, y1, x2, y2, color):
    h, w = img.shape[:2]
    clipped = _clip_line(w << XY_SHIFT, h << XY_SHIFT, x1, y1, x2, y2)
    if clipped is None:
        return
    x1, y1, x2, y2 = clipped
    dx, dy = x2 - x1, y2 - y1
    ax, ay = abs(dx), abs(dy)
    if ax > ay:
        if dx < 0:
            dy = -dy
            x1, x2, y1, y2 = x2, x1, y2, y1
        y_step = _cdiv(dy * XY_ONE, ax | 1)
        ecount = (x2 - x1) >> XY_SHIFT
    else:
        if dy < 0:
            dx = -dx
            x1, x2, y1, y2 = x2, x1, y2, y1
        x_step = _cdiv(dx * XY_ONE, ay | 1)
        ecount = (y2 - y1) >> XY_SHIFT
    x1 += XY_ONE >> 1
    y1 += XY_ONE >> 1
    _put(img, (x2 + (XY_ONE >> 1)) >> XY_SHIFT, (y2 + (XY_ONE >> 1)) >> XY_SHIFT, color)
    if ax > ay:
        x1 >>= XY_SHIFT
        while ecount >= 0:
            _put(img, x1, y1 >> XY_SHIFT, color)
            x1 += 1
            y1 += y_step
            ecount -= 1
    else:
        y1 >>= XY_SHIFT
        while ecount >= 0:
            _put(img, x1 >> XY_SHIFT, y1, color)
            x1 += x_step
            y1 += 1
            ecount -= 1


def _fill_convex_poly(img, v, color):
    """FillConvexPoly(img, v, npts, color, LINE_8, shift=XY_SHIFT); v = [(x, y)] in XY_SHIFT fixed point."""
    h, w = img.shape[:2]
    npts = len(v)
    delta = XY_ONE >> 1
    xmin = xmax = v[0][0]
    ymin = ymax = v[0][1]
    imin = 0
    p0 = v[npts - 1]
    for i, p in enumerate(v):
        if p[1] < ymin:
            ymin, imin = p[1], i
        ymax, xmax, xmin = max(ymax, p[1]), max(xmax, p[0]), min(xmin, p[0])
        _line2(img, p0[0], p0[1], p[0], p[1], color)
        p0 = p
    xmin, xmax = (xmin + delta) >> XY_SHIFT, (xmax + delta) >> XY_SHIFT
    ymin, ymax = (ymin + delta) >> XY_SHIFT, (ymax + delta) >> XY_SHIFT
    if npts < 3 or xmax < 0 or ymax < 0 or xmin >= w or ymin >= h:
        return
    ymax = min(ymax, h - 1)
    edge = [{"idx": imin, "di": 1, "x": -XY_ONE, "dx": 0, "ye": ymin}, {"idx": imin, "di": npts - 1, "x": -XY_ONE, "dx": 0, "ye": ymin}]
    y = ymin
    edges = npts
    while True:
        for e in edge:
            if y >= e["ye"]:
                idx0, di = e["idx"], e["di"]
                idx = idx0 + di
                if idx >= npts:
                    idx -= npts
                while True:
                    go = edges > 0
                    edges -= 1
                    if not go:
                        break
                    ty = (v[idx][1] + delta) >> XY_SHIFT
                    if ty > y:
                        xs, xe = v[idx0][0], v[idx][0]
                        e["ye"] = ty
                        e["dx"] = _cdiv((xe - xs) * 2 + (ty - y), 2 * (ty - y))
                        e["x"] = xs
                        e["idx"] = idx
                        break
                    idx0 = idx
                    idx += di
                    if idx >= npts:
                        idx -= npts
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if edge[0]["x"] > edge[1]["x"] else (0, 1)
            xx1 = (edge[left]["x"] + delta) >> XY_SHIFT
            xx2 = (edge[right]["x"] + delta) >> XY_SHIFT
            if xx2 >= 0 and xx1 < w:
                _hline(img, y, xx1, xx2, color)
        edge[0]["x"] += edge[0]["dx"]
        edge[1]["x"] += edge[1]["dx"]
        y += 1
        if y > ymax:
            break


def circle(img, center, radius, color, thickness=-1):
    """cv2.circle with thickness -1 (FILLED), LINE_8, shift 0."""
    if thickness >= 0:
        raise NotImplementedError("only filled circles are restated")
    _circle_filled(img, int(center[0]), int(center[1]), int(radius), color)


def line(img, pt1, pt2, color, thickness=1):
    """cv2.line with thickness >= 2, LINE_8, shift 0 (ThickLine)."""
    if thickness < 2:
        raise NotImplementedError("only the thick-line path (thickness >= 2) is restated")
    p0x, p0y = int(pt1[0]) << XY_SHIFT, int(pt1[1]) << XY_SHIFT
    p1x, p1y = int(pt2[0]) << XY_SHIFT, int(pt2[1]) << XY_SHIFT
    dx = (p0x - p1x) / XY_ONE
    dy = (p1y - p0y) / XY_ONE
    r = dx * dx + dy * dy
    odd = thickness & 1
    t = thickness << (XY_SHIFT - 1)
    if abs(r) > DBL_EPSILON:
        r = (t + odd * XY_ONE * 0.5) / math.sqrt(r)
        dpx, dpy = cv_round(dy * r), cv_round(dx * r)
        _fill_convex_poly(img, [(p0x + dpx, p0y + dpy), (p0x - dpx, p0y - dpy), (p1x - dpx, p1y - dpy), (p1x + dpx, p1y + dpy)],
                          color)
    rad = (t + (XY_ONE >> 1)) >> XY_SHIFT
    for px, py in ((p0x, p0y), (p1x, p1y)):
        _circle_filled(img, (px + (XY_ONE >> 1)) >> XY_SHIFT, (py + (XY_ONE >> 1)) >> XY_SHIFT, rad, color)


def arrowed_line(img, pt1, pt2, color, thickness=1, tip_length=0.1):
    """cv2.arrowedLine (LINE_8, shift 0)."""
    x1, y1 = int(pt1[0]), int(pt1[1])
    x2, y2 = int(pt2[0]), int(pt2[1])
    tip = math.sqrt(float(x1 - x2) * (x1 - x2) + float(y1 - y2) * (y1 - y2)) * tip_length
    line(img, (x1, y1), (x2, y2), color, thickness)
    ang = math.atan2(float(y1) - y2, float(x1) - x2)
    for s in (1, -1):
        p = (cv_round(x2 + tip * math.cos(ang + s * math.pi / 4)), cv_round(y2 + tip * math.sin(ang + s * math.pi / 4)))
        line(img, p, (x2, y2), color, thickness)


def bresenham(p0, p1):
    """The one-pixel 8-connected line between two integer points (pixels as a set of (x, y))."""
    (x0, y0), (x1, y1) = p0, p1
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err, pts = dx + dy, set()
    while True:
        pts.add((x0, y0))
        if (x0, y0) == (x1, y1):
            return pts
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def draw_tracking(frame, ox, oy, cx, cy, major, minor, angle):
    """The reference's `_draw_tracking(frame, ref, curr)` (marker_detection.py:398-427) on one marker."""
    circle(frame, (int(cx), int(cy)), 4, (0, 0, 255), -1)
    arrowed_line(frame, (int(ox), int(oy)), (int(cx), int(cy)), (0, 0, 255), 2, tip_length=0.25)
    angle_rad = np.deg2rad(angle)
    maj_len, min_len = major / 2, minor / 2
    maj_p1 = (int(cx - maj_len * np.cos(angle_rad)), int(cy - maj_len * np.sin(angle_rad)))
    maj_p2 = (int(cx + maj_len * np.cos(angle_rad)), int(cy + maj_len * np.sin(angle_rad)))
    line(frame, maj_p1, maj_p2, (0, 255, 255), 2)
    min_p1 = (int(cx - min_len * np.cos(angle_rad + np.pi / 2)), int(cy - min_len * np.sin(angle_rad + np.pi / 2)))
    min_p2 = (int(cx + min_len * np.cos(angle_rad + np.pi / 2)), int(cy + min_len * np.sin(angle_rad + np.pi / 2)))
    line(frame, min_p1, min_p2, (255, 0, 0), 2)


def draw_frame(frame, rows):
    """Every row of one frame, in order: rows = iterable of (Ox, Oy, Cx, Cy, major, minor, angle) - the CSV's rows of that
    frame, which are in reference-dict (slot) order.  Returns a painted copy."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    for ox, oy, cx, cy, major, minor, angle in rows:
        draw_tracking(out, ox, oy, cx, cy, major, minor, angle)
    return out
