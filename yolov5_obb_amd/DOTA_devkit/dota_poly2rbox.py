"""Quad <-> rotated box conversions of the reference's DOTA_devkit/dota_poly2rbox.py, host numpy: the single-box functions
with the reference's signatures, return types and arithmetic (float32 corners and edge lengths, `arctan2` in double of the
float32 differences, `norm_angle` with numpy's `%`), and array forms (`poly2rbox`, `poly2rbox_v2`, `poly2rbox_v3`:
(n, 8) -> (n, 5)) that give the same bits row by row.  `convert2rbox` (file walking) is not part of this package.

These stay on the host on purpose: `norm_angle` wraps at -pi/4 and 3pi/4, a 45-degree quad with integer corners has
`arctan2` exactly equal to `-np.pi / 4`, and an `atan2` that is one ulp off flips the result by pi.
"""
import math

import numpy as np


def cal_line_length(point1, point2):
    """:8-9."""
    return math.sqrt(math.pow(point1[0] - point2[0], 2) + math.pow(point1[1] - point2[1], 2))


def get_best_begin_point_single(coordinate):
    """:11-33.  The rotation of the four corners that is closest (sum of corner distances) to the horizontal box's
    [top-left, top-right, bottom-right, bottom-left]; the first of equal ones."""
    x1, y1, x2, y2, x3, y3, x4, y4 = coordinate
    pts = [[x1, y1], [x2, y2], [x3, y3], [x4, y4]]
    xmin, ymin, xmax, ymax = min(x1, x2, x3, x4), min(y1, y2, y3, y4), max(x1, x2, x3, x4), max(y1, y2, y3, y4)
    dst = [[xmin, ymin], [xmax, ymin], [xmax, ymax], [xmin, ymax]]
    force, flag = 100000000.0, 0
    for i in range(4):
        rot = pts[i:] + pts[:i]
        f = cal_line_length(rot[0], dst[0]) + cal_line_length(rot[1], dst[1]) + cal_line_length(rot[2], dst[2]) \
            + cal_line_length(rot[3], dst[3])
        if f < force:
            force, flag = f, i
    return np.array(pts[flag:] + pts[:flag]).reshape(8)


def norm_angle(angle, range=[-np.pi / 4, np.pi]):
    """:79-80."""
    return (angle - range[0]) % range[1] + range[0]


def _single_parts(poly):
    """float32 corners, the two float32 edge lengths (pt1-pt2, pt2-pt3) of :41-51."""
    poly = np.array(poly[:8], dtype=np.float32)
    pt1, pt2, pt3, pt4 = (poly[0], poly[1]), (poly[2], poly[3]), (poly[4], poly[5]), (poly[6], poly[7])
    edge1 = np.sqrt((pt1[0] - pt2[0]) * (pt1[0] - pt2[0]) + (pt1[1] - pt2[1]) * (pt1[1] - pt2[1]))
    edge2 = np.sqrt((pt2[0] - pt3[0]) * (pt2[0] - pt3[0]) + (pt2[1] - pt3[1]) * (pt2[1] - pt3[1]))
    return pt1, pt2, pt3, pt4, edge1, edge2


def _long_edge(pt1, pt2, pt4, edge1, edge2):
    """(width, height, angle of the longer edge) of :53-66; zeros when neither comparison holds (a NaN edge)."""
    if edge1 > edge2:
        return edge1, edge2, np.arctan2(float(pt2[1] - pt1[1]), float(pt2[0] - pt1[0]))
    if edge2 >= edge1:
        return edge2, edge1, np.arctan2(float(pt4[1] - pt1[1]), float(pt4[0] - pt1[0]))
    return 0, 0, 0


def poly2rbox_single(poly):
    """:35-77.  [x0 y0 .. x3 y3] -> np.array([x_ctr, y_ctr, w, h, angle]), the angle wrapped once into [-pi/4, 3pi/4]."""
    pt1, pt2, pt3, pt4, edge1, edge2 = _single_parts(poly)
    width, height, angle = _long_edge(pt1, pt2, pt4, edge1, edge2)
    if angle > np.pi * 3 / 4:
        angle -= np.pi
    if angle < -np.pi / 4:
        angle += np.pi
    x_ctr = float(pt1[0] + pt3[0]) / 2
    y_ctr = float(pt1[1] + pt3[1]) / 2
    return np.array([x_ctr, y_ctr, width, height, angle])


def poly2rbox_single_v2(poly):
    """:83-125.  The same with norm_angle; a tuple of five floats."""
    pt1, pt2, pt3, pt4, edge1, edge2 = _single_parts(poly)
    width, height, angle = _long_edge(pt1, pt2, pt4, edge1, edge2)
    angle = norm_angle(angle)
    x_ctr = float(pt1[0] + pt3[0]) / 2
    y_ctr = float(pt1[1] + pt3[1]) / 2
    return float(x_ctr), float(y_ctr), float(width), float(height), float(angle)


def poly2rbox_single_v3(poly):
    """:128-190.  v2, except that a near-square box (edge ratio < 1.15) takes the edge whose normalised angle is smaller in
    magnitude (the first edge when equal)."""
    pt1, pt2, pt3, pt4, edge1, edge2 = _single_parts(poly)
    max_edge = max(edge1, edge2)
    min_edge = min(edge1, edge2)
    ratio = max_edge / min_edge
    if ratio < 1.15:
        width, height = max_edge, min_edge
        angle1_norm = norm_angle(np.arctan2(float(pt2[1] - pt1[1]), float(pt2[0] - pt1[0])))
        angle2_norm = norm_angle(np.arctan2(float(pt4[1] - pt1[1]), float(pt4[0] - pt1[0])))
        final_angle = angle2_norm if abs(angle1_norm) > abs(angle2_norm) else angle1_norm
    else:
        width, height, final_angle = _long_edge(pt1, pt2, pt4, edge1, edge2)
        final_angle = norm_angle(final_angle)
    x_ctr = float(pt1[0] + pt3[0]) / 2
    y_ctr = float(pt1[1] + pt3[1]) / 2
    return float(x_ctr), float(y_ctr), float(width), float(height), float(final_angle)


def rbox2poly_single(rrect):
    """:193-209.  [x_ctr, y_ctr, w, h, angle] -> the float32 corners, rotated to the best begin point."""
    cx, cy, w, h, theta = rrect[:5]
    half_w, half_h = w / 2, h / 2
    # the corners around the origin, top-left first, as the columns of a 2 x 4 matrix; one matrix product turns them (the
    # reference's `R.dot(rect)`: the sums are the product's, not written out), then the centre is added in double
    corners = np.array([[-half_w, half_w, half_w, -half_w], [-half_h, -half_h, half_h, half_h]])
    c, s = np.cos(theta), np.sin(theta)
    turned = np.array([[c, -s], [s, c]]).dot(corners)
    xy = np.stack((turned[0] + cx, turned[1] + cy), 1)               # (4, 2): x0 y0 / x1 y1 / ..
    return get_best_begin_point_single(xy.reshape(8).astype(np.float32))


# ---- array forms: the same operations on columns, in the same number formats and order ------------------------------
# `ratio < 1.15` compares a float32 scalar with a Python float: in float32 under NumPy 2's promotion, in double before it.
_RATIO_BOUND = np.float32(1.15) if isinstance(np.float32(1) + 1.15, np.float32) else np.float64(1.15)


def _array_parts(polys):
    p = np.asarray(polys)[:, :8].astype(np.float32)
    x1, y1, x2, y2, x3, y3, x4, y4 = (p[:, k] for k in range(8))
    with np.errstate(all='ignore'):
        edge1 = np.sqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2))
        edge2 = np.sqrt((x2 - x3) * (x2 - x3) + (y2 - y3) * (y2 - y3))
        angle1 = np.arctan2((y2 - y1).astype(np.float64), (x2 - x1).astype(np.float64))
        angle2 = np.arctan2((y4 - y1).astype(np.float64), (x4 - x1).astype(np.float64))
        x_ctr = (x1 + x3).astype(np.float64) / 2
        y_ctr = (y1 + y3).astype(np.float64) / 2
    return edge1, edge2, angle1, angle2, x_ctr, y_ctr


def _array_long_edge(edge1, edge2, angle1, angle2):
    first = edge1 > edge2
    second = ~first & (edge2 >= edge1)
    zero = np.zeros(len(edge1))
    width = np.where(first, edge1, np.where(second, edge2, zero)).astype(np.float64)
    height = np.where(first, edge2, np.where(second, edge1, zero)).astype(np.float64)
    angle = np.where(first, angle1, np.where(second, angle2, zero))
    return width, height, angle


def poly2rbox(polys):
    """poly2rbox_single of every row: (n, >= 8) -> (n, 5) float64."""
    edge1, edge2, angle1, angle2, x_ctr, y_ctr = _array_parts(polys)
    width, height, angle = _array_long_edge(edge1, edge2, angle1, angle2)
    angle = np.where(angle > np.pi * 3 / 4, angle - np.pi, angle)
    angle = np.where(angle < -np.pi / 4, angle + np.pi, angle)
    return np.stack((x_ctr, y_ctr, width, height, angle), 1)


def poly2rbox_v2(polys):
    """poly2rbox_single_v2 of every row: (n, >= 8) -> (n, 5) float64."""
    edge1, edge2, angle1, angle2, x_ctr, y_ctr = _array_parts(polys)
    width, height, angle = _array_long_edge(edge1, edge2, angle1, angle2)
    return np.stack((x_ctr, y_ctr, width, height, norm_angle(angle)), 1)


def poly2rbox_v3(polys):
    """poly2rbox_single_v3 of every row: (n, >= 8) -> (n, 5) float64."""
    edge1, edge2, angle1, angle2, x_ctr, y_ctr = _array_parts(polys)
    max_edge = np.where(edge2 > edge1, edge2, edge1)                 # Python's max(edge1, edge2) / min(edge1, edge2)
    min_edge = np.where(edge2 < edge1, edge2, edge1)
    with np.errstate(all='ignore'):
        near_square = (max_edge / min_edge).astype(_RATIO_BOUND.dtype) < _RATIO_BOUND
    width, height, angle = _array_long_edge(edge1, edge2, angle1, angle2)
    angle1_norm, angle2_norm = norm_angle(angle1), norm_angle(angle2)
    square_angle = np.where(np.abs(angle1_norm) > np.abs(angle2_norm), angle2_norm, angle1_norm)
    width = np.where(near_square, max_edge.astype(np.float64), width)
    height = np.where(near_square, min_edge.astype(np.float64), height)
    return np.stack((x_ctr, y_ctr, width, height, np.where(near_square, square_angle, norm_angle(angle))), 1)
