"""Every triangle of every tree through the box-overlap query on the host twin (pt_box_search_bvh4): the box
p +- eps around each of the four aimed positions of each triangle (box_cases.aimed_boxes) lists that triangle, with no exception.  The
sampled tests of tests/test_box_host.py see a triangle only where a sampled box happens to meet it; here no triangle of no tree is left out.
The trees are those of tests/test_point_audit.py -- the small soups at accel 0, 1 and 2, built and refitted after `wave` and `deform` --
and the f16 grid; tests/test_gpu_box_audit.py runs dragon50k through the kernels."""
import numpy as np
import pytest

import box_cases as bc
import treeaudit as ta
from test_point_audit import ACCELS, SCENES, scene, states

SMALL = [n for n in SCENES if n.startswith("soup") and int(n[4:]) < 1000] + ["f16_grid"]


@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", SMALL)
def test_every_triangle_is_listed_by_the_box_around_it(rt, orc, name, accel):
    host = ta.HostContext(rt, orc)
    tris = scene(rt, name)
    for what, now in states(name, tris):
        if what == "built":
            host.set_triangles(tris); host.build_bvh(accel)
        else:
            host.update_triangles(now)
        boxes, tri = bc.aimed_boxes(rt, now)
        res = rt.box_search_bvh4(now, host.read_bvh4(), boxes, stats=True)
        assert res[3]["stack_drops"] == 0
        bc.assert_audited(res, tri, "%s accel %d %s" % (name, accel, what))
        assert np.all(np.diff(res[0].astype(np.int64)) >= 1)
