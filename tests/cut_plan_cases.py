"""What the CPU tests of the cuts' host hooks share (tests/test_primary_leaf_list_plan.py, tests/test_primary_cut_node_plan.py): the Cornell
box scaled as the GPU tests scale it, with rs_build_bvh's tables; its cameras; the rays of a block in double precision; the traversal order."""
import numpy as np
import pytest

from restir_amd import capi
from tests import geometric_cases as gc
from tests.common import get_scene

SIZE = (96, 54)


@pytest.fixture(scope="module")
def box():
    sd = get_scene("cornell")
    gc._affine(sd, scale=(0.45,) * 3)
    boxes, nodes = capi.build_bvh(sd.vertices)
    return sd, boxes, nodes


def camera(sd, **args):
    from restir_amd.ctypes_structs import make_camera
    return capi.camera_update(make_camera(SIZE[0], SIZE[1], **dict(sd.camera_args, **args)))


def directions(cam, x0, y0, w=8, h=8):
    """Camera::sample's unnormalised directions (rs_cuts.h cut_corner_dir) for every pixel of the w x h block at (x0, y0) at jitters 0, 0.5,
    1 and a few odd ones."""
    W, H = SIZE
    right, up, view = (np.array([getattr(cam, n)[i] for i in range(3)], np.float64) for n in ("right", "up", "view"))
    tan_y = float(np.tan(np.float32(np.radians(cam.fov[1])))); aspect = float(np.float32(W) / np.float32(H)); focal = float(cam.focalDist)
    out = []
    for y in range(y0, y0 + h):
        for x in range(x0, x0 + w):
            for jx, jy in ((0, 0), (1, 1), (0, 1), (1, 0), (0.5, 0.5), (0.25, 0.875), (0.9375, 0.125)):
                X = (1.0 - (x + jx) / W * 2.0) * aspect * tan_y * focal
                Y = (1.0 - (y + jy) / H * 2.0) * tan_y * focal
                out.append(right * X + up * Y + view * focal)
    return np.array(out)


def order_of(d):
    """DevScene::getMTBVHId of -d."""
    v = -d
    a = np.abs(v)
    if a[0] > a[1]:
        if a[0] > a[2]:
            return 0 if v[0] > 0 else 1
        return 4 if v[2] > 0 else 5
    if a[1] > a[2]:
        return 2 if v[1] > 0 else 3
    return 4 if v[2] > 0 else 5
