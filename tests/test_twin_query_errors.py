"""What the host twins of the batched queries refuse, and with which words (include/mi355pt.h; csrc/pt_api_queries.cpp).  One table over
all nine *_bvh4 entry points, after test_gpu_query_errors.py: the checks of each in the order the library makes them, with the exact
PtStatus and pt_last_error(NULL) text.  Every check is tried alone, and every pair of checks together (the earlier one wins).  Then what
each twin accepts at its edges: no tree with brute force, an empty batch without records, no entries with capacity 0; and a tree that is
shorter than its node count is PT_ERR_BAD_BVH.  No GPU: a 20-triangle deck, its level-0 host tree and one input record."""
import ctypes as C

import numpy as np
import pytest

import crossing_cases as cc
import hitlist_cases as hlc

PT_OK, PT_ERR_INVALID_ARG, PT_ERR_BAD_BVH = 0, 1, 5         # include/mi355pt.h PtStatus
BIG = 1 << 32
NULL, BY4 = None, 4                                         # a pointer override: NULL, or the buffer's address plus so many bytes
CAP = 32                                                    # entries: more than the deck's 20 triangles
CON_OK = dict(samples=3, seed=1, index_base=0, flags=0)
NULLS = lambda *names: [{k: NULL} for k in names]           # "null pointer": every pointer of the twin in turn


def con(**kw):
    return {"con": dict(CON_OK, **kw)}


def item_checks(noun):
    return [("unknown flags", [{"flags": 8}]),
            ("null pointer", NULLS("tris", "rec", "out", "bvh4")),
            ("more than 2^32 - 1 %s" % noun, [{"n": BIG}])]


def list_checks(noun, unknown=8):
    return [("unknown flags", [{"flags": unknown}]),
            ("null pointer", NULLS("tris", "rec", "off", "ent", "bvh4")),
            ("offsets must be 8-byte aligned", [{"off": BY4}]),
            ("more than 2^32 - 1 %s" % noun, [{"n": BIG}])]


ITEM = ("tris", "num_tris", "bvh4", "words", "rec", "n", "flags", "out", "stats")
LIST = ("tris", "num_tris", "bvh4", "words", "rec", "n", "flags", "off", "ent", "cap", "stats")
# entry point -> (signature, checks in the library's order, the brute-force flag or None)
# a signature names each argument: a buffer (tris, bvh4, rec = the input record, out, off, ent), the parameter block or a scalar
TWINS = {
    "pt_closest_points_bvh4": (ITEM, item_checks("points"), "PT_CLOSEST_BRUTE_FORCE"),
    "pt_sweep_spheres_bvh4": (ITEM, item_checks("sweeps"), "PT_SWEEP_BRUTE_FORCE"),
    "pt_count_hits_bvh4": (ITEM, item_checks("rays"), "PT_COUNT_BRUTE_FORCE"),
    "pt_contains_bvh4": (("tris", "num_tris", "bvh4", "words", "rec", "n", "con", "out", "stats"),
                         [("null params", [{"con": None}]),
                          ("unknown flags", [con(flags=4)]),
                          ("more than 2^32 - 1 points", [{"n": BIG}]),
                          ("samples must be odd and in 1..255", [con(samples=s) for s in (0, 2, 4, 256, 257)]),
                          ("more than 2^32 - 1 sample rays (n * samples)", [{"n": 1 << 31, "con": dict(CON_OK, samples=3)},
                                                                           {"n": BIG // 3 + 1, "con": dict(CON_OK, samples=3), "rec": NULL, "out": NULL}]),
                          ("null pointer", NULLS("tris", "rec", "out", "bvh4"))], None),
    "pt_radius_search_bvh4": (LIST, list_checks("points"), "PT_RADIUS_BRUTE_FORCE"),
    "pt_box_search_bvh4": (LIST, list_checks("boxes"), "PT_BOX_BRUTE_FORCE"),
    "pt_tri_search_bvh4": (LIST, list_checks("triangles"), "PT_TRI_BRUTE_FORCE"),
    "pt_list_hits_bvh4": (LIST, list_checks("rays", 16), "PT_HITS_BRUTE_FORCE"),
    "pt_nearest_k_bvh4": (("tris", "num_tris", "bvh4", "words", "rec", "n", "k", "flags", "out", "stats"),
                          [("unknown flags", [{"flags": 8}]),
                           ("k must be 1 .. PT_NEAREST_MAX_K", [{"k": 0}, {"k": 65}]),
                           ("null pointer", NULLS("tris", "rec", "out", "bvh4")),
                           ("more than 2^32 - 1 points", [{"n": BIG}])], "PT_NEAREST_BRUTE_FORCE"),
}


class Rig:
    """the deck, its tree and one buffer per kind"""

    def __init__(self, rt, orc):
        self.rt = rt
        tris, _ = hlc.deck(10, 7)                                         # 20 triangles; the ray below crosses all ten quads
        b4 = np.ascontiguousarray(cc.host_trees(rt, orc, tris, 0)[1], np.uint32)
        # one record that reads as a PtRay, a radius-0 PtSweep, a PtPoint with no limit, a PtBox that is not walked (lo > hi) and a PtTri
        rec = rt._aligned_zeros((1, 12), np.float32)
        rec[0, :8] = np.float32([0.1, 0.2, 3.0, np.inf, 0.0, 0.0, -1.0, 0.0])
        self.buf = {"tris": np.ascontiguousarray(tris, np.float32), "bvh4": b4, "rec": rec,
                    "out": rt._aligned_zeros((64, 4), np.uint32),         # a row of k = 64 records
                    "off": np.zeros(3, np.uint64), "ent": rt._aligned_zeros((CAP, 4), np.uint32)}
        self.valid = dict(num_tris=tris.size // 9, words=b4.size, n=1, flags=0, k=2, cap=CAP, con=CON_OK)

    def call(self, entry, over):
        """one call with the valid arguments but for `over`; returns (status, pt_last_error(NULL) text)"""
        rt = self.rt
        v = dict(self.valid, **over)
        keep, args = [], []
        for a in TWINS[entry][0]:
            if a in self.buf:
                shift = v.get(a, 0)
                args.append(C.c_void_p(None if shift is None else self.buf[a].ctypes.data + shift))
            elif a == "con":
                if v[a] is None:
                    args.append(None)
                    continue
                s = rt.PtContainParams()
                for f, x in v[a].items():
                    setattr(s, f, x)
                keep.append(s); args.append(C.byref(s))
            elif a == "stats":
                args.append(None)
            else:
                args.append((C.c_uint64 if a in ("words", "n", "cap") else C.c_uint32)(v[a]))
        status = getattr(rt.lib, entry)(*args)
        return status, (rt.lib.pt_last_error(None) or b"").decode()


@pytest.fixture(scope="module")
def rig(rt, orc):
    return Rig(rt, orc)


def merged(a, b):
    """both overrides at once, or None when they set the same argument"""
    return None if set(a) & set(b) else dict(a, **b)


@pytest.mark.parametrize("entry", list(TWINS))
def test_refusals_in_order_and_in_words(rig, entry):
    sig, checks, brute = TWINS[entry]
    say = lambda text: "%s: %s" % (entry, text)
    assert rig.call(entry, {})[0] == PT_OK
    # every check alone
    for text, variants in checks:
        for over in variants:
            assert rig.call(entry, over) == (PT_ERR_INVALID_ARG, say(text)), over
    # every two checks together: the earlier one wins
    for i, (text, variants) in enumerate(checks):
        for _, later in checks[i + 1:]:
            for over in variants:
                for other in later:
                    both = merged(over, other)
                    if both is not None:
                        assert rig.call(entry, both) == (PT_ERR_INVALID_ARG, say(text)), both
    # no tree, and no words of one: only with brute force
    assert rig.call(entry, {"bvh4": NULL, "words": 0}) == (PT_ERR_INVALID_ARG, say("null pointer"))
    if brute is not None:
        assert rig.call(entry, {"bvh4": NULL, "words": 0, "flags": getattr(rig.rt, brute)})[0] == PT_OK
    # a tree shorter than its node count
    assert rig.call(entry, {"words": rig.valid["words"] - 3})[0] == PT_ERR_BAD_BVH
    # an empty batch needs no records
    empty = {"n": 0, "rec": NULL}
    if "out" in sig:
        empty["out"] = NULL
    assert rig.call(entry, empty)[0] == PT_OK
    if "ent" in sig:                             # offsets alone: no entries with capacity 0
        assert rig.call(entry, {"ent": NULL, "cap": 0})[0] == PT_OK
    assert rig.call(entry, {})[0] == PT_OK
