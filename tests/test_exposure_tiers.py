"""The second exposure tier on the CPU: the definition of tests/exposeref.py at the gate 0.2999 against the oracle --
shadow-ray origins built as the megakernel builds them for hits at |n . d| >= 0.3008f, traced by the oracle's any-hit traversal --, the
monotonicity of the tiers, and the host twin at both gates inside the reference's band.  The scenes are those of tests/exposure_cases.py and
a bumpy plate (tests/exposure_tier_cases.py) on which the tiers differ by a quarter of the triangles."""
import importlib

import numpy as np
import pytest

import exposeref
import exposure_cases as xc
import exposure_tier_cases as tc
import orc as orc_mod


@pytest.fixture(scope="module")
def orc():
    return orc_mod.load()


def flags(name, k, **kw):
    t = tc.scene(name)
    s_max, d_max = xc.bounds(t)
    return tc.flags(t, k, s_max, d_max, key=name, **kw)


def occluded_rays(orc, name, flagged, k, per_tri, seed=5):
    """(shadow rays started on flagged triangles by hits that pass tier k's f32 gate, those of them the oracle finds occluded)"""
    t = tc.scene(name)
    flat = np.ascontiguousarray(t.reshape(-1))
    _, bvh4 = orc.build_bvh4(flat)
    n32 = exposeref.records(t)[3]
    L = exposeref.light32()
    started = occluded = 0
    for o, d in xc.aimed_rays(t, np.nonzero(flagged)[0], per_tri, seed):
        hit, tt, _, tri = orc.trace_ray(flat, bvh4, o, d)
        if not hit or not flagged[tri]:
            continue
        with tc.tier(k):
            so = xc.shadow_origin(o, d, tt, n32[tri])
        if so is None:
            continue
        started += 1
        occluded += bool(orc.trace_ray(flat, bvh4, so, L, anyhit=True)[0])
    return started, occluded


@pytest.mark.parametrize("name", tc.NAMES)
def test_no_shadow_ray_from_a_triangle_of_the_second_tier_is_occluded(orc, name):
    """0 occluded is the condition.  A run (triangles / flagged by tier 1 / by tier 2): torus 1,920 / 762 / 813, bumpy_plate 2,592 / 1,739 /
    2,427; on the other scenes the tiers flag the same triangles."""
    f = flags(name, 2)
    started, occluded = occluded_rays(orc, name, f, 2, per_tri=4 if name == "bumpy_plate" else 12)
    print(name, "triangles", len(f), "tier 1", int(flags(name, 1).sum()), "tier 2", int(f.sum()), "shadow rays", started, "occluded", occluded)
    assert occluded == 0
    if f.any():
        assert started > 0


def test_the_tiers_are_nested_and_the_second_is_not_the_first():
    for name in tc.NAMES:
        f1, f2 = flags(name, 1), flags(name, 2)
        assert not (f1 & ~f2).any(), name
    f1, f2 = flags("bumpy_plate", 1), flags("bumpy_plate", 2)
    print("bumpy_plate: tier 1", int(f1.sum()), "tier 2", int(f2.sum()))
    assert (f2 & ~f1).sum() >= 500           # a run: 1,739 and 2,427 of 2,592 -- 688 more


def test_the_check_can_fail_at_the_second_gate(orc):
    """As tests/test_exposure_reference.py::test_the_check_can_fail: with the margins negated the floor triangles under the lip are flagged,
    and shadow rays from them are occluded."""
    good = flags("vfold_lip", 2)
    bad = flags("vfold_lip", 2, rho_scale=-1.0)
    assert (bad & ~good).any()
    started, occluded = occluded_rays(orc, "vfold_lip", bad & ~good, 2, per_tri=400, seed=9)
    print("negated margins: extra flagged", int((bad & ~good).sum()), "shadow rays", started, "occluded", occluded)
    assert occluded > 0


@pytest.mark.parametrize("k", (1, 2))
@pytest.mark.parametrize("name", tc.NAMES)
def test_host_twin_lies_in_the_band_at_both_gates(name, k):
    rt = importlib.import_module("raytracer-public_amd")
    t = tc.scene(name)
    s_max, d_max = xc.bounds(t)
    twin = rt.exposure_flags_host(t, s_max, d_max, gate=tc.GATES[k][0])
    inner, outer = tc.band(t, k, s_max, d_max, key=name)
    print(name, "tier", k, "inner", int(inner.sum()), "twin", int(twin.sum()), "outer", int(outer.sum()))
    assert not (inner & ~twin).any() and not (twin & ~outer).any()
    assert (inner != outer).sum() <= 2


def test_host_twin_without_a_gate_is_the_first_tier_and_the_tiers_are_nested():
    rt = importlib.import_module("raytracer-public_amd")
    assert rt.EXPOSE_GATES == (tc.GATES[1][0], tc.GATES[2][0])
    for name in ("soup", "bumpy_plate"):
        t = tc.scene(name)
        s_max, d_max = xc.bounds(t)
        one, two = (rt.exposure_flags_host(t, s_max, d_max, gate=g) for g in rt.EXPOSE_GATES)
        assert np.array_equal(one, rt.exposure_flags_host(t, s_max, d_max))
        assert not (one & ~two).any() and two.sum() > one.sum()
    with pytest.raises(rt.PtError):
        rt.exposure_flags_host(tc.scene("soup"), 4.0, 1.0, gate=0.0)
