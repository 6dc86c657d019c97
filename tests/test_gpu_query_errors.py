"""What the batched queries refuse, and with which words (include/mi355pt.h; csrc/pt_api_queries.cpp).  One table over every context entry
point of the query front end, device and host forms: the checks of each in the order the library makes them, with the exact PtStatus and
pt_last_error text.  Every check is tried alone on a context with a scene, with triangles only and with nothing (an argument error comes
before PT_ERR_NO_SCENE), and every pair of checks together (the earlier one wins).  Nothing that is refused launches anything; one valid
n = 1 call per entry point at the end shows that the context is still usable."""
import ctypes as C
import math

import numpy as np
import pytest

import hitlist_cases as hlc

pytestmark = pytest.mark.gpu

PT_OK, PT_ERR_INVALID_ARG, PT_ERR_NO_SCENE = 0, 1, 4        # include/mi355pt.h PtStatus
RECORDS = 64                                                # one 64-record buffer per kind
BIG = 1 << 32
NO_SCENE = "scene not set (triangles + BVH)"
NULL, BY4, BY8, BY2 = None, 4, 8, 2                         # a pointer override: NULL, or the buffer's address plus so many bytes

# the sixteen-byte pairs every query shares
P16 = lambda *names: [{k: v} for k in names for v in (NULL, BY8, BY4)]
OCC_OK = dict(samples=4, seed=1, index_base=0, bias=1e-4, flags=0)
CON_OK = dict(samples=3, seed=1, index_base=0, flags=0)
CAM_OK = dict(width=8, height=8, focal=1.0, aspect=1.0)     # 64 rays: the buffer exactly


def occ(**kw):
    return {"occ": dict(OCC_OK, **kw)}


def con(**kw):
    return {"con": dict(CON_OK, **kw)}


def cam(**kw):
    return {"cam": dict(CAM_OK, **kw)}


def list_checks(noun, entries):
    return [("unknown flags", [{"flags": 16}]),
            ("more than 2^32 - 1 %s" % noun, [{"n": BIG}]),
            ("%s must be non-null and 16-byte aligned" % noun, P16("rec")),
            ("offsets must be non-null and 8-byte aligned", [{"off": NULL}, {"off": BY4}]),
            ("%s must be 16-byte aligned, and non-null unless capacity is 0" % entries,
             [{"ent": NULL}, {"ent": BY8}, {"ent": BY4}, {"ent": BY8, "cap": 0}])]


def contain_checks():
    return [("null params", [{"con": None}]),
            ("unknown flags", [con(flags=4)]),
            ("more than 2^32 - 1 points", [{"n": BIG}]),
            ("samples must be odd and in 1..255", [con(samples=0), con(samples=2), con(samples=257)]),
            ("more than 2^32 - 1 sample rays (n * samples)", [{"n": 1 << 31, "con": dict(CON_OK, samples=3)}]),
            ("points and results must be non-null and 16-byte aligned", P16("rec", "out"))]


def occlusion_checks():
    return [("null params", [{"occ": None}]),
            ("unknown flags", [occ(flags=4)]),
            ("more than 2^32 - 1 surfels", [{"n": BIG}]),
            ("samples must be 1..65536", [occ(samples=0), occ(samples=65537)]),
            ("more than 2^32 - 1 sample rays (n * samples)", [{"n": 65536, "occ": dict(OCC_OK, samples=65536)}]),
            ("bias must be >= 0", [occ(bias=-1.0), occ(bias=math.nan)]),
            ("surfels and results must be non-null and 16-byte aligned", P16("rec", "out"))]


# family -> (signature, checks in the library's order, what a valid call answers without a scene: (status, text), None = PT_OK)
# a signature names each argument after the context: a buffer kind (rec = the input records, out, off, ent) or a scalar
FAMILIES = {
    "pt_trace_rays": (("rec", "n", "flags", "out"),
                      [("unknown flags", [{"flags": 8}]),
                       ("more than 2^32 - 1 rays", [{"n": BIG}]),
                       ("rays and hits must be non-null and 16-byte aligned", P16("rec", "out"))], NO_SCENE),
    "pt_closest_points": (("rec", "n", "flags", "out"),
                          [("unknown flags", [{"flags": 8}]),
                           ("more than 2^32 - 1 points", [{"n": BIG}]),
                           ("points and results must be non-null and 16-byte aligned", P16("rec", "out"))], NO_SCENE),
    "pt_occlusion": (("rec", "n", "occ", "out"), occlusion_checks(), NO_SCENE),
    "pt_hit_surfels": (("rec", "ent", "n", "rmax", "out"),
                       [("more than 2^32 - 1 rays", [{"n": BIG}]),
                        ("rays, hits and surfels must be non-null and 16-byte aligned", P16("rec", "ent", "out"))], "no triangles set"),
    "pt_count_hits": (("rec", "n", "flags", "out"),
                      [("unknown flags", [{"flags": 8}]),
                       ("more than 2^32 - 1 rays", [{"n": BIG}]),
                       ("rays must be non-null and 16-byte aligned, counts non-null and 4-byte aligned",
                        P16("rec") + [{"out": NULL}, {"out": BY2}])], NO_SCENE),
    "pt_contains": (("rec", "n", "con", "out"), contain_checks(), NO_SCENE),
    "pt_signed_distance": (("rec", "n", "con", "out"), contain_checks(), NO_SCENE),
    "pt_radius_count": (("rec", "n", "flags", "out"),
                        [("unknown flags", [{"flags": 8}]),
                         ("more than 2^32 - 1 points", [{"n": BIG}]),
                         ("points must be non-null and 16-byte aligned", P16("rec")),
                         ("counts must be non-null and 4-byte aligned", [{"out": NULL}, {"out": BY2}])], NO_SCENE),
    "pt_radius_search": (("rec", "n", "flags", "off", "ent", "cap"), list_checks("points", "entries"), NO_SCENE),
    "pt_list_hits": (("rec", "n", "flags", "off", "ent", "cap"), list_checks("rays", "hits"), NO_SCENE),
    "pt_nearest_k": (("rec", "n", "k", "flags", "out"),
                     [("unknown flags", [{"flags": 8}]),
                      ("k must be 1 .. PT_NEAREST_MAX_K", [{"k": 0}, {"k": 65}]),
                      ("more than 2^32 - 1 points", [{"n": BIG}]),
                      ("points and results must be non-null and 16-byte aligned", P16("rec", "out"))], NO_SCENE),
    "pt_sweep_spheres": (("rec", "n", "flags", "out"),
                         [("unknown flags", [{"flags": 8}]),
                          ("more than 2^32 - 1 sweeps", [{"n": BIG}]),
                          ("sweeps and hits must be non-null and 16-byte aligned", P16("rec", "out"))], NO_SCENE),
    "pt_box_count": (("rec", "n", "flags", "out"),
                     [("unknown flags", [{"flags": 8}]),
                      ("more than 2^32 - 1 boxes", [{"n": BIG}]),
                      ("boxes must be non-null and 16-byte aligned", P16("rec")),
                      ("counts must be non-null and 4-byte aligned", [{"out": NULL}, {"out": BY2}])], NO_SCENE),
    "pt_box_search": (("rec", "n", "flags", "off", "ent", "cap"), list_checks("boxes", "entries"), NO_SCENE),
    "pt_tri_count": (("rec", "n", "flags", "out"),
                     [("unknown flags", [{"flags": 8}]),
                      ("more than 2^32 - 1 triangles", [{"n": BIG}]),
                      ("triangles must be non-null and 16-byte aligned", P16("rec")),
                      ("counts must be non-null and 4-byte aligned", [{"out": NULL}, {"out": BY2}])], NO_SCENE),
    "pt_tri_search": (("rec", "n", "flags", "off", "ent", "cap"), list_checks("triangles", "entries"), NO_SCENE),
}
# the entry points without a host form of the same shape: device only, and needing no scene
DEVICE_ONLY = {
    "pt_occlusion_rays": (("rec", "n", "occ", "out"), occlusion_checks(), None),
    "pt_camera_rays": (("cam", "out"),
                       [("null params", [{"cam": None}]),
                        ("rays must be non-null and 16-byte aligned", P16("out")),
                        ("bad resolution", [cam(width=0), cam(height=0), cam(width=32769), cam(height=32769)])], None),
}
ENTRY_POINTS = [(name + form, name, form == "_host") for name in FAMILIES for form in ("", "_host")] + [(name, name, False) for name in DEVICE_ONLY]
VALID = dict(n=1, flags=0, k=2, cap=RECORDS, rmax=math.inf, occ=OCC_OK, con=CON_OK, cam=CAM_OK)


class Rig:
    """three contexts (a scene, triangles only, nothing) and one 64-record buffer per kind, on the device and on the host"""

    def __init__(self, rt):
        self.rt, self.hip = rt, C.CDLL("libamdhip64.so")
        tris, _ = hlc.deck(10, 7)                                     # 20 triangles; the ray below crosses all ten quads
        self.full, self.tris_only, self.empty = rt.Context(0), rt.Context(0), rt.Context(0)
        self.full.set_triangles(tris); self.full.build_bvh()
        self.tris_only.set_triangles(tris)
        # one record that reads as a PtRay, a PtSurfel and (its first half) a PtPoint: from (0.1, 0.2, 3) down -z, no limit
        rec = rt._aligned_zeros((RECORDS, 8), np.float32)
        rec[:] = np.float32([0.1, 0.2, 3.0, np.inf, 0.0, 0.0, -1.0, 0.0])
        self.host = {"rec": rec}
        self.dev = {}
        for kind in ("rec", "out", "off", "ent"):                     # ent doubles as the hits of pt_hit_surfels: all zero = triangle 0 at t = 0
            self.host.setdefault(kind, rt._aligned_zeros((RECORDS, 8), np.float32))
            ptr = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(ptr), C.c_size_t(RECORDS * 32)) == 0
            assert self.hip.hipMemcpy(ptr, C.c_void_p(self.host[kind].ctypes.data), C.c_size_t(RECORDS * 32), C.c_int(1)) == 0
            self.dev[kind] = ptr.value

    def close(self):
        for c in (self.full, self.tris_only, self.empty):
            c.close()
        for p in self.dev.values():
            self.hip.hipFree(C.c_void_p(p))

    def call(self, ctx, entry, family, host, over):
        """one call with the valid arguments but for `over`; returns (status, pt_last_error text)"""
        rt = self.rt
        sig = (FAMILIES.get(family) or DEVICE_ONLY[family])[0]
        v = dict(VALID, **over)
        keep, args = [], []
        for a in sig:
            if a in ("rec", "out", "off", "ent"):
                base = self.host[a].ctypes.data if host else self.dev[a]
                shift = v.get(a, 0)
                args.append(C.c_void_p(None if shift is None else base + shift))
            elif a in ("occ", "con", "cam"):
                if v[a] is None:
                    args.append(None)
                    continue
                s = {"occ": rt.PtOcclusionParams, "con": rt.PtContainParams, "cam": rt.PtRenderParams}[a]()
                for f, x in v[a].items():
                    setattr(s, f, x)
                keep.append(s); args.append(C.byref(s))
            elif a == "rmax":
                args.append(C.c_float(v[a]))
            else:
                args.append((C.c_uint64 if a in ("n", "cap") else C.c_uint32)(v[a]))
        h = ctx.h if ctx is not None else None
        status = getattr(rt.lib, entry)(h, *args)
        return status, (rt.lib.pt_last_error(h) or b"").decode()


@pytest.fixture(scope="module")
def rig(rt):
    r = Rig(rt)
    yield r
    r.close()


def merged(a, b):
    """both overrides at once, or None when they set the same argument"""
    return None if set(a) & set(b) else dict(a, **b)


@pytest.mark.parametrize("entry,family,host", ENTRY_POINTS, ids=[e[0] for e in ENTRY_POINTS])
def test_refusals_in_order_and_in_words(rig, entry, family, host):
    _, checks, unset = FAMILIES.get(family) or DEVICE_ONLY[family]
    say = lambda text: "%s: %s" % (entry, text)
    assert rig.call(None, entry, family, host, {}) == (PT_ERR_INVALID_ARG, "null context")
    # every check alone: the same refusal whatever the context holds
    for text, variants in checks:
        for over in variants:
            for ctx in (rig.full, rig.tris_only, rig.empty):
                assert rig.call(ctx, entry, family, host, over) == (PT_ERR_INVALID_ARG, say(text)), (over, ctx is rig.full)
    # every two checks together: the earlier one wins
    for i, (text, variants) in enumerate(checks):
        for _, later in checks[i + 1:]:
            for over in variants:
                both = merged(over, later[0])
                if both is not None:
                    assert rig.call(rig.full, entry, family, host, both) == (PT_ERR_INVALID_ARG, say(text)), both
    # valid arguments, no scene
    if unset is not None:
        assert rig.call(rig.empty, entry, family, host, {}) == (PT_ERR_NO_SCENE, say(unset))
        if unset == NO_SCENE:                    # triangles without a tree are no scene either
            assert rig.call(rig.tris_only, entry, family, host, {}) == (PT_ERR_NO_SCENE, say(unset))
    # and the context still works: one valid call -- on the barest context the entry point accepts
    ctx = rig.empty if unset is None else rig.tris_only if unset != NO_SCENE else rig.full
    assert rig.call(ctx, entry, family, host, {})[0] == PT_OK
    ctx.synchronize()
    if entry == "pt_trace_rays_host":            # the nearest of the ten quads lies at z = 2
        assert rig.host["out"].view(np.float32)[0, 0] == np.float32(1.0) and rig.host["out"].view(np.uint32)[0, 1] < 20
