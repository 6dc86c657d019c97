"""tests/session_model.py without a device: the generator is deterministic, the committed seeds meet every coverage condition that the
records decide, the model replays each session end to end from the twins and the oracle alone, and two scripted sessions give the words
that are spelled out here by hand."""
import time

import numpy as np
import pytest

import session_model as sm
from refit_cases import wave
from scenes import random_soup

REPLAY_CAP_S = 60.0         # wall time of one model-only replay (measured: 3.3 to 4.5 s; the twins and the oracle are single-threaded)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_the_generator_is_deterministic():
    for seed in sm.SEEDS:
        a, b = sm.generate(seed, sm.LENGTH), sm.generate(seed, sm.LENGTH)
        assert a == b and len(a) == sm.LENGTH
    assert sm.generate(sm.SEEDS[0]) != sm.generate(sm.SEEDS[1])
    lines = [sm.line(i, op) for i, op in enumerate(sm.generate(sm.SEEDS[0]))]
    assert len(set(lines)) == len(lines) and all("\n" not in s for s in lines)         # one line per operation


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_the_seeds_meet_the_coverage_conditions(seed):
    ops = sm.generate(seed, sm.LENGTH)
    cov = sm.coverage(ops)
    sm.check_coverage(cov, device=False)
    # the vocabulary: every scene kind, the empty scene and the single triangle, counts that go down and up
    kinds = {op["scene"][0] for op in ops if op["op"] == "set_triangles"}
    assert kinds == {"proc", "soup", "deck", "comb", "one", "empty"}
    counts = [sm.scene_count(op["scene"]) for op in ops if op["op"] == "set_triangles"]
    steps = np.sign(np.diff(counts))
    assert (steps < 0).sum() >= len(sm.FAMILIES) and (steps > 0).sum() >= 3
    queries = [op for op in ops if op["op"] == "query"]
    assert {q["family"] for q in queries} == set(sm.FAMILIES)
    assert {1, 63, 64, 65} <= {q["n"] for q in queries} and max(q["n"] for q in queries) == 5000
    for key in ("torch", "simple", "stats"):
        assert {q[key] for q in queries} == {False, True}
    assert {op["which"] for op in ops if op["op"] == "refuse"} == set(sm.REFUSALS)
    assert {op["mid"] for op in ops if op["op"] == "accum_run"} == {"none", "query", "update"}
    assert {op["torch"] for op in ops if op["op"] == "update"} == {False, True}
    assert {op["accel"] for op in ops if op["op"] == "build_bvh"} == {0, 1, 2}
    assert {op["mode"] for op in ops if op["op"] == "render"} == {0, 1, 2}
    assert any(op["stats"] for op in ops if op["op"] == "render") and any(op["simple"] for op in ops if op["op"] == "render")
    for i, op in enumerate(ops[:-1]):                                                   # a refused call is followed by an observation
        if op["op"] == "refuse":
            assert ops[i + 1]["op"] in sm.OBSERVATIONS


def test_coverage_conditions_can_fail():
    ops = sm.generate(sm.SEEDS[0], sm.LENGTH)
    with pytest.raises(AssertionError):
        sm.check_coverage(sm.coverage([op for op in ops if op["op"] != "flush"]), device=False)
    with pytest.raises(AssertionError):
        sm.check_coverage(sm.coverage([op for op in ops if op["op"] != "read_bvh2"]), device=False)
    with pytest.raises(AssertionError):
        sm.check_coverage(sm.coverage([op for op in ops if not (op["op"] == "query" and op["n"] == 5000)]), device=False)
    with pytest.raises(AssertionError):
        sm.check_coverage(sm.coverage([op for op in ops if not (op["op"] == "large" and op["cam"] == "far")]), device=False)
    with pytest.raises(AssertionError):                                                 # no flush ever meets pending frames
        sm.check_coverage(sm.coverage([op for op in ops if not (op["op"] == "batch_run" and op["event"] == "flush")]), device=False)
    with pytest.raises(AssertionError):                                                 # the stale tail is read on the host route only
        sm.check_coverage(sm.coverage([dict(op, torch=True) if op["op"] == "query" else op for op in ops]), device=False)
    with pytest.raises(AssertionError):                                                 # every refusal twice
        seen = set()
        once = [op for op in ops if not (op["op"] == "refuse" and op["which"] == "build_accel_7" and (op["which"] in seen or seen.add(op["which"])))]
        sm.check_coverage(sm.coverage(once), device=False)


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_the_model_replays_the_session_alone(rt, orc, seed):
    t0 = time.time()
    cov = sm.run(seed, device=False, rt=rt, orc=orc)
    dt = time.time() - t0
    print("session %d: model-only replay of %d operations in %.1f s" % (seed, cov["operations"], dt))
    assert cov["operations"] == sm.LENGTH and dt < REPLAY_CAP_S


def play(rt, orc, ops):
    s = sm.Session(rt, orc, 0, ops, False)
    for op in ops:
        s.play(op)
    return s.model


def test_scripted_build_update_and_back_is_the_built_tree(rt, orc):
    scene = ("soup", 900, 4)
    tris = random_soup(900, 4)
    built2 = rt.build_bvh2_ploc(tris)
    built4 = rt.collapse_bvh2_to_bvh4_accel(built2, 900, rt.PT_ACCEL_PLOC)[0]
    head = [dict(op="set_triangles", scene=scene), dict(op="build_bvh", accel=2)]
    m = play(rt, orc, head)
    assert same_bits(m.tris, tris) and np.array_equal(m.bvh2, built2) and np.array_equal(m.bvh4, built4)
    moved = wave(tris, 0.05, 3)
    m = play(rt, orc, head + [dict(op="update", how=("wave", 0.05, 3), torch=False)])
    assert same_bits(m.tris, moved) and np.array_equal(m.bvh4, rt.refit_bvh4(moved, built4)) and np.array_equal(m.bvh2, rt.refit_bvh2(moved, built2))
    assert not np.array_equal(m.bvh4, built4) and m.bvh4[0] == built4[0]
    m = play(rt, orc, head + [dict(op="update", how=("wave", 0.05, 3), torch=False), dict(op="update", how=("wave", 0.02, 1), torch=True),
                              dict(op="update", how=("back",), torch=False), dict(op="read_bvh4"), dict(op="read_bvh2")])
    assert same_bits(m.tris, tris) and np.array_equal(m.bvh4, built4) and np.array_equal(m.bvh2, built2)


def test_scripted_level_2_then_the_level_0_words_is_level_0(rt, orc):
    scene = ("soup", 700, 9)
    tris = random_soup(700, 9)
    level0_2, level0_4 = orc.build_bvh4(tris)
    assert np.array_equal(level0_4, rt.collapse_lbvh2_to_bvh4(level0_2, 700)[0])
    ops = [dict(op="set_triangles", scene=scene), dict(op="build_bvh", accel=2), dict(op="set_bvh4", words="level0")]
    m = play(rt, orc, ops)
    assert np.array_equal(m.bvh4, level0_4)
    assert np.array_equal(m.bvh2, rt.build_bvh2_ploc(tris))                  # set_bvh4 leaves the context's BVH2 alone: still level 2's
    direct = play(rt, orc, [dict(op="set_triangles", scene=scene), dict(op="build_bvh", accel=0)])
    assert np.array_equal(direct.bvh4, level0_4) and np.array_equal(direct.bvh2, level0_2)
    # and what the model then expects of a frame and of a query is what level 0 gives
    cam = sm.CAMS[1]
    p = orc.make_params(64, 40, 700, cam[0], cam[1], mode=2, spp=2, max_bounces=3, seed=5, frame=1)
    assert same_bits(m.frame(64, 40, cam, 2, spp=2, max_bounces=3, seed=5, frame=1)[0], orc.render(p, tris, level0_4)[0])
    q = dict(op="query", family="closest_points", n=65, qseed=3, torch=False, simple=False, stats=True)
    rec = sm.query_input(rt, tris, q)
    want, counters, _ = sm.expected(m, q, rec)
    twin = rt.closest_points_bvh4(tris, level0_4, rec, stats=True)
    assert all(same_bits(a, b) for a, b in zip(want, twin[:4])) and counters == twin[4]
    other = rt.closest_points_bvh4(tris, rt.collapse_bvh2_to_bvh4_accel(rt.build_bvh2_ploc(tris), 700, 2)[0], rec, stats=True)
    assert counters != other[4]                                              # (the level-2 tree is walked differently: the check above can tell)
