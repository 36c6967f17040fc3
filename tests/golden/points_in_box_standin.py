"""Stand-in for nuscenes.utils.geometry_utils.points_in_box, which models/base_model.py:278 calls and which is not installed
here (nuScenes-devkit is absent).  Written from the function's documented behaviour: a point is inside the box when its
projections onto the three edges that leave corner 0 of `box.corners(wlh_factor)` -- towards corner 4 (length), corner 1
(width) and corner 3 (height) -- all lie between 0 and the squared length of the edge, both bounds INCLUDED.

Parity with the devkit's own implementation is unpinned at that boundary: nothing here can check which way the devkit rounds
a point that sits on a face (the README says the same of `pointnet2_ops`).  The fixture generator therefore asserts that no
row it feeds this function lies within 1e-3 m of a face.  Used by tests/golden/make_golden_motion_tracking.py only."""
import numpy as np


def points_in_box(box, points, wlh_factor=1.0):
    """box: an object with .corners(wlh_factor) -> (3,8); points (3,N) -> (N,) bool"""
    corners = box.corners(wlh_factor=wlh_factor)
    p0 = corners[:, 0]
    edges = [corners[:, 4] - p0, corners[:, 1] - p0, corners[:, 3] - p0]
    v = points - p0.reshape(3, 1)
    mask = np.ones(points.shape[1], bool)
    for e in edges:
        proj = e @ v
        mask &= (0 <= proj) & (proj <= e @ e)
    return mask
