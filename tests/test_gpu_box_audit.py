"""Every triangle of the device's tree through the box-overlap kernels (tests/test_box_audit.py has the rule and runs the host twin on the
small trees): on dragon50k, built at levels 0 and 2 and refitted, the box p +- eps around each of the four aimed positions of each triangle
lists that triangle, through the persistent and the one-box-per-thread kernel, with no exception."""
import numpy as np
import pytest

import box_cases as bc
import crossing_cases as cc
from refit_cases import wave

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("accel", [0, 2])
def test_every_triangle_of_dragon50k_is_listed_by_the_box_around_it(rt, gpu_ctx, accel):
    tris = cc.geometry(rt, "dragon50k")
    gpu_ctx.set_triangles(tris); gpu_ctx.build_bvh(accel)
    for what, now in (("built", tris), ("wave", wave(tris, 0.02, 3))):
        if what == "wave":
            gpu_ctx.update_triangles(now)
        boxes, tri = bc.aimed_boxes(rt, now)
        counts = gpu_ctx.box_count(boxes, stats=True)
        assert gpu_ctx.stats()["stack_drops"] == 0 and np.all(counts >= 1)
        for simple in (False, True):
            res = gpu_ctx.box_search(boxes, simple=simple)
            bc.assert_audited(res, tri, "dragon50k accel %d %s simple %d" % (accel, what, simple))
            assert np.array_equal(np.diff(res[0].astype(np.int64)), counts)
