"""Writes tests/golden/point/point_kat.npz: known answers of the point-set
restatement (tests/_point_ref.py) for one small batch -- four graphs of 5, 12, 1
and 20 points on a half-unit lattice in [0, 2)^3 (equal distances, repeated points
and points on the boundary abound) and queries for three of them -- fps at two ratios and from
given starts, radius at two caps, radius_graph with and without loops, and the
edge-feature matrix of the radius edges.  The file lives in its own directory
(see make_golden_spline.py).  Regenerate with

    python tests/golden/make_golden_point.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _point_ref as R  # noqa: E402

SIZES = (5, 12, 1, 20)
Y_SIZES = (3, 0, 1, 6)
RADIUS = 0.75


def inputs():
    rng = np.random.default_rng(41)
    n, m = sum(SIZES), sum(Y_SIZES)
    pos = (rng.integers(0, 4, (n, 3)) * 0.5).astype(np.float32)
    pos[8], pos[30], pos[33] = pos[6], pos[25], pos[25]       # repeated points in the graphs of 12 and 20
    y = (rng.integers(0, 4, (m, 3)) * 0.5).astype(np.float32)
    feat = rng.standard_normal((n, 4)).astype(np.float32)
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    batch_y = np.repeat(np.arange(len(Y_SIZES)), Y_SIZES).astype(np.int64)
    start = np.asarray([4, 7, 0, 19], dtype=np.int64)
    return pos, y, feat, batch, batch_y, start


def answers(pos, y, feat, batch, batch_y, start):
    out = {}
    for name, ratio in (("half", 0.5), ("all", 1.0)):
        out["fps_%s" % name] = R.fps(pos, batch, ratio)
        out["fps_%s_start" % name] = R.fps(pos, batch, ratio, start)
    for cap in (2, 32):
        out["radius_cap%d" % cap] = R.radius(pos, y, RADIUS, batch, batch_y, cap)
    out["radius_graph"] = R.radius_graph(pos, RADIUS, batch, False, 3)
    out["radius_graph_loop_t2s"] = R.radius_graph(pos, RADIUS, batch, True, 3, "target_to_source")
    row, col = out["radius_cap32"]
    out["edge_features"] = R.edge_features(feat, pos, y, col, row)
    out["edge_features_pos_only"] = R.edge_features(None, pos, y, col, row)
    return out


def main():
    names = ("pos", "y", "feat", "batch", "batch_y", "start")
    ins = inputs()
    out = dict(zip(names, ins))
    out.update(answers(*ins))
    os.makedirs(os.path.join(HERE, "point"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "point", "point_kat.npz"), **out)


if __name__ == "__main__":
    main()
