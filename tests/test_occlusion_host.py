"""The sample rays of the ambient-occlusion query (pt_occlusion_rays_host) against the oracle's primitives --
orc_rnd -> orc_cosine_dir -> p + n * bias restated in numpy float32 -- bit for bit and ray for ray; the untraced records, the wrap of
index_base + i, the argument errors and the record layouts.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
S = 64
BIAS = np.float32(1e-4)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def make_surfels(seed=5):
    """>= 200 surfels: random unit normals, the six axis normals, normals whose z sits on either side of the basis' sign branch (+-0, tiny,
    -1 exactly) with |n.x| from 0 to nearly 1 on both sides, and a mix of r_max."""
    rng = np.random.default_rng(seed)
    normals = [unit(rng.normal(size=(200, 3)))]
    normals.append(np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]))
    branch = []
    for nx in (0.0, 1e-7, 1e-3, 0.3, 0.6, 0.99, 0.9999999):
        for sx in (1.0, -1.0):
            for nz in (0.0, -0.0, 1e-30, -1e-30, 1e-4, -1e-4, 0.5, -0.5):
                ny = np.sqrt(max(0.0, 1.0 - nx * nx - nz * nz))
                branch.append([sx * nx, ny, nz])
    normals.append(np.float32(branch))                    # (as given: the library does not normalise, and neither does this test)
    n = np.concatenate(normals).astype(np.float32)
    p = rng.uniform(-2, 2, n.shape).astype(np.float32)
    r = rng.choice(np.float32([np.inf, 0.25, 3.0, 1e-3]), len(n)).astype(np.float32)
    sf = np.zeros((len(n), 8), np.float32)
    sf[:, 0:3], sf[:, 3], sf[:, 4:7] = p, r, n
    return sf


def oracle_rays(orc, sf, samples, seed, index_base, bias):
    """Every ray of every surfel from the oracle's exported primitives; no ray is left out."""
    n = len(sf)
    out = np.zeros((n * samples, 8), np.float32)
    o = (sf[:, 0:3] + sf[:, 4:7] * np.float32(bias)).astype(np.float32)
    assert o.dtype == np.float32
    d = (C.c_float * 3)()
    for i in range(n):
        nrm = np.ascontiguousarray(sf[i, 4:7])
        pixel = (index_base + i) & 0xFFFFFFFF
        for s in range(samples):
            u1 = orc.lib.orc_rnd(seed, pixel, s, 0, 2)
            u2 = orc.lib.orc_rnd(seed, pixel, s, 0, 3)
            orc.lib.orc_cosine_dir(nrm.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(u1), C.c_float(u2), d)
            k = i * samples + s
            out[k, 0:3] = o[i]; out[k, 3] = sf[i, 3]; out[k, 4:7] = d[:]
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("seed,index_base", [(0, 12345), (0xC0FFEE, 0xFFFFFF00)])
def test_rays_equal_the_oracles_primitives(rt, orc, seed, index_base):
    sf = make_surfels()
    assert len(sf) >= 200
    got = rt.occlusion_rays_host(sf, S, seed=seed, bias=BIAS, index_base=index_base)      # the second base wraps past 2^32 inside the batch
    want = oracle_rays(orc, sf, S, seed, index_base, BIAS)
    assert got.shape == want.shape == (len(sf) * S, 8)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:2]], want[bad[:2]])


def test_two_seeds_give_different_rays(rt):
    sf = make_surfels()
    a, b = rt.occlusion_rays_host(sf, S, seed=1), rt.occlusion_rays_host(sf, S, seed=2)
    assert same_bits(a[:, 0:4], b[:, 0:4]) and not same_bits(a[:, 4:7], b[:, 4:7])


def test_index_base_splits_a_batch_and_wraps(rt):
    sf = make_surfels()
    for base in (0, 77, 0xFFFFFFFF - 50):                 # the last one wraps mod 2^32 in the middle of the batch
        whole = rt.occlusion_rays_host(sf, 16, seed=9, index_base=base)
        k = 101
        first = rt.occlusion_rays_host(sf[:k], 16, seed=9, index_base=base)
        second = rt.occlusion_rays_host(sf[k:], 16, seed=9, index_base=(base + k) & 0xFFFFFFFF)
        assert same_bits(whole, np.concatenate([first, second]))
    assert not same_bits(rt.occlusion_rays_host(sf, 16, seed=9, index_base=0)[:, 4:7], rt.occlusion_rays_host(sf, 16, seed=9, index_base=1)[:, 4:7])


def test_untraced_surfels_give_t_max_0_records(rt):
    base = np.float32([0.5, -0.25, 1.0, np.inf, 0.0, 0.6, 0.8, 0.0])
    sf = np.tile(base, (10, 1))
    sf[0, 0] = np.nan; sf[1, 2] = np.nan; sf[2, 4] = np.nan; sf[3, 6] = np.nan; sf[4, 3] = np.nan      # a NaN in p, n or r_max
    sf[5, 3] = 0.0; sf[6, 3] = -0.0; sf[7, 3] = -1.0; sf[8, 3] = -np.inf                                # r_max <= 0
    rays = rt.occlusion_rays_host(sf, 5, seed=3).reshape(10, 5, 8)
    for i in range(9):
        for s in range(5):
            want = sf[i].copy(); want[3] = 0.0; want[7] = 0.0
            assert same_bits(rays[i, s], want), (i, s, rays[i, s])
    assert np.all(np.isposinf(rays[9, :, 3])) and not same_bits(rays[9, 0, 4:7], rays[9, 1, 4:7])       # the traced one
    # +inf coordinates are no NaN: the surfel is traced (whatever its rays turn out to be)
    sf2 = np.tile(base, (1, 1)); sf2[0, 0] = np.inf
    assert np.all(np.isposinf(rt.occlusion_rays_host(sf2, 3)[:, 3]))


def test_directions_stay_in_the_hemisphere(rt):
    sf = make_surfels()
    nrm = sf[:, 4:7].astype(np.float64)
    unitish = np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-6
    assert unitish.sum() >= 200
    rays = rt.occlusion_rays_host(sf, S, seed=4).reshape(len(sf), S, 8)
    d, n = rays[unitish][:, :, 4:7], sf[unitish][:, None, 4:7]
    dot = (d[..., 0] * n[..., 0] + d[..., 1] * n[..., 1]) + d[..., 2] * n[..., 2]
    assert dot.dtype == np.float32
    assert dot.min() >= -1e-6, dot.min()
    assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0) < 1e-5)
    assert 0.6 < dot.mean() < 0.72                         # E[cos] of a cosine lobe is 2/3


def test_normals_are_used_as_given(rt, orc):
    """A zero normal and an infinite one hold no NaN: the surfels are traced, and their rays are whatever the pinned arithmetic gives (the
    infinite normal gives NaN directions, which pt_trace_rays does not traverse: such samples count as unoccluded)."""
    sf = np.float32([[0, 0, 0, np.inf, 0, 0, 0, 0], [1, 2, 3, 0.5, np.inf, 0, 0, 0]])
    rays = rt.occlusion_rays_host(sf, 4, seed=2, index_base=3)
    assert same_bits(rays, oracle_rays(orc, sf, 4, 2, 3, 1e-4))
    assert np.all(np.isposinf(rays[:4, 3])) and np.all(rays[4:, 3] == 0.5)
    assert np.all(rays[:4, 0:3] == 0) and not np.isnan(rays[:4]).any()
    assert np.isnan(rays[4:, 4:7]).any(axis=1).all()


def raw(rt, sf, n, params, rays):
    return rt.lib.pt_occlusion_rays_host(sf.ctypes.data_as(C.POINTER(rt.PtSurfel)) if sf is not None else None, C.c_uint64(n),
                                         C.byref(params) if params is not None else None,
                                         rays.ctypes.data_as(C.POINTER(rt.PtRay)) if rays is not None else None)


def test_argument_errors(rt):
    sf = make_surfels()[:4]
    rays = np.zeros((4 * 70000, 8), np.float32)

    def params(samples=4, bias=1e-4, flags=0):
        p = rt.PtOcclusionParams(); p.samples, p.seed, p.index_base, p.bias, p.flags = samples, 1, 0, bias, flags
        return p
    INVALID = 1
    assert raw(rt, sf, 4, params(), rays) == 0
    assert raw(rt, sf, 4, params(samples=0), rays) == INVALID
    assert raw(rt, sf, 4, params(samples=65537), rays) == INVALID
    assert raw(rt, sf, 4, params(samples=65536), rays) == 0                               # the largest allowed
    assert raw(rt, sf, 65536, params(samples=65536), rays) == INVALID                      # n * samples = 2^32 (refused before any access)
    assert raw(rt, sf, (1 << 32) - 1, params(samples=2), rays) == INVALID
    assert raw(rt, sf, 1 << 32, params(samples=1), rays) == INVALID                        # n > UINT32_MAX
    assert raw(rt, sf, 4, params(bias=float("nan")), rays) == INVALID
    assert raw(rt, sf, 4, params(bias=-1e-6), rays) == INVALID
    assert raw(rt, sf, 4, params(bias=0.0), rays) == 0
    assert raw(rt, sf, 4, params(flags=4), rays) == INVALID                                # unknown flag
    assert raw(rt, sf, 4, params(flags=3), rays) == 0                                      # the known ones change nothing
    assert raw(rt, sf, 4, None, rays) == INVALID
    assert raw(rt, None, 4, params(), rays) == INVALID and raw(rt, sf, 4, params(), None) == INVALID
    assert raw(rt, None, 0, params(), None) == 0                                           # n = 0: nothing to do
    assert b"pt_occlusion_rays_host" in rt.lib.pt_last_error(None)
    with pytest.raises(rt.PtError):
        rt.occlusion_rays_host(sf, 0)


def test_python_records_match_the_header(rt):
    assert C.sizeof(rt.PtSurfel) == 32 and C.sizeof(rt.PtOcclusion) == 16 and C.sizeof(rt.PtOcclusionParams) == 20
    assert rt.PtSurfel.r_max.offset == 12 and rt.PtSurfel.n.offset == 16 and rt.PtSurfel.reserved.offset == 28
    assert rt.PtOcclusion.unoccluded.offset == 4 and rt.PtOcclusion.samples.offset == 8 and rt.PtOcclusion.reserved.offset == 12
    assert [f[0] for f in rt.PtOcclusionParams._fields_] == ["samples", "seed", "index_base", "bias", "flags"]
    assert rt.PtOcclusionParams.bias.offset == 12 and rt.PtOcclusionParams.flags.offset == 16
    assert (rt.PT_OCCLUSION_STATS, rt.PT_OCCLUSION_SIMPLE_KERNEL) == (1, 2)


def test_header_records(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    if not (os.path.isabs(cc) and os.path.exists(cc)):
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stddef.h>\n#include "mi355pt.h"\n'
        "_Static_assert(sizeof(PtSurfel) == 32 && sizeof(PtSurfel) == sizeof(PtRay), \"PtSurfel\");\n"
        "_Static_assert(offsetof(PtSurfel, r_max) == offsetof(PtRay, t_max) && offsetof(PtSurfel, n) == offsetof(PtRay, dir) && offsetof(PtSurfel, reserved) == 28, \"PtSurfel fields\");\n"
        "_Static_assert(sizeof(PtOcclusion) == 16, \"PtOcclusion\");\n"
        "_Static_assert(offsetof(PtOcclusion, unoccluded) == 4 && offsetof(PtOcclusion, samples) == 8 && offsetof(PtOcclusion, reserved) == 12, \"PtOcclusion fields\");\n"
        "_Static_assert(sizeof(PtOcclusionParams) == 20 && offsetof(PtOcclusionParams, bias) == 12 && offsetof(PtOcclusionParams, flags) == 16, \"PtOcclusionParams\");\n"
        "_Static_assert(PT_OCCLUSION_STATS == 1 && PT_OCCLUSION_SIMPLE_KERNEL == 2, \"flags\");\n")
    subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True, capture_output=True, timeout=120)
