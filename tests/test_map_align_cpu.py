"""CPU tests of the alignment against the voxel map: the numpy restatement (tests/map_align_reference.py) against a plain loop and a
brute-force nearest neighbour, its convergence and decision margins on the inputs the GPU tests use, and the agreement of the header,
the ctypes binding and the C++ adapter."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import map_align_reference as A
import voxel_map_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 6          # the perturbed guess of the GPU tests (1 cm, 3 mrad): chosen so that every stop / continue decision has a margin > 3


@pytest.fixture(scope="module")
def world(oracle_mod, small_pair):
    """The GPU tests' inputs: the first synthetic frame's convention-2 cloud (the checker's, bit-equal to the device's), the pose the
    maps are built at, the perturbed guess."""
    cloud = oracle_mod.sphere_cloud(small_pair[0][1], 2)
    P = R.general_pose()
    return dict(cloud=cloud, P=P, guess=A.perturbed(P, 0.01, 0.003, SEED), maps={leaf: R.Map([(cloud, None, P)], leaf) for leaf in (0.05, 0.2)})


def test_numpy_cloud_is_the_device_cloud_to_a_few_ulp(oracle_mod, small_pair):
    a, b = oracle_mod.sphere_cloud(small_pair[0][1], 2), A.sphere_cloud_np(small_pair[0][1])
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) < 2e-6


@pytest.mark.parametrize("leaf", [0.05, 0.2])
def test_the_27_cells_hold_the_nearest_centroid(world, leaf):
    """max_dist = 0.8 leaf: the match of every passing point equals the brute-force nearest centroid over the whole map."""
    tgt = world["maps"][leaf]
    max_dist = np.float32(0.8 * leaf)
    for pose in (world["P"], world["guess"]):
        ev = A.Evaluation(tgt, world["cloud"], pose, leaf, R.DEFAULT_BOX, max_dist)
        w, idx, _ = R.passing(world["cloud"], pose, R.DEFAULT_BOX)
        assert len(w) > 15000
        md2 = max_dist * max_dist
        checked = 0
        for lo in range(0, len(w), 400):
            e = w[lo:lo + 400, None, :] - tgt.xyz[None, :, :]
            d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            near = d2.min(axis=1)
            got = ev.d2[idx[lo:lo + 400]]
            within = near <= md2
            # inside the radius the 27 cells give the same distance; outside it the point has no kept match
            assert np.array_equal(got[within], near[within])
            assert np.array_equal(ev.key3[idx[lo:lo + 400], 0] != A.NO_KEY, within)
            unique = within & ((d2 == near[:, None]).sum(axis=1) == 1)
            assert np.array_equal(ev.key3[idx[lo:lo + 400]][unique], tgt.key[d2.argmin(axis=1)[unique]])
            checked += len(near)
        assert checked == len(w) and ev.n > 0.9 * len(w)


@pytest.mark.parametrize("leaf", [0.05, 0.2])
def test_restatement_converges_with_clear_decisions(world, leaf):
    al = A.Alignment(world["maps"][leaf], world["cloud"], world["guess"], leaf, R.DEFAULT_BOX, leaf)
    print("leaf", leaf, "iterations", al.iterations, "margins", al.margins, "error", A.pose_error(world["guess"], world["P"]), "->", A.pose_error(al.pose, world["P"]))
    assert al.status == A.OK and al.converged == 1 and 1 <= al.iterations < 10
    assert min(al.margins) >= 2.0
    r0, t0 = A.pose_error(world["guess"], world["P"])
    r1, t1 = A.pose_error(al.pose, world["P"])
    assert r1 <= 0.5 * r0 and t1 <= 0.5 * t0
    assert al.n_matched == al.final.n > 15000 and al.fitness < (0.5 * leaf) ** 2


def loop_evaluation(target, xyz, pose, leaf, box, max_dist, min_count):
    """Steps 2-4 point by point with numpy float32 scalars and a dict: (key3 or None, d2) per passing point."""
    f = np.float32
    cells = {tuple(k): (int(c), S) for k, c, S in zip(target.key.tolist(), target.count, target.S)}
    w, idx, _ = R.passing(xyz, pose, box)
    i = R.voxel_index(w, leaf)
    out = []
    for p, ip in zip(w, i.tolist()):
        best, best_key = f(np.inf), None
        for dx, dy, dz in A.CELLS:
            key = (ip[0] + dx, ip[1] + dy, ip[2] + dz)
            if key not in cells or cells[key][0] < min_count:
                continue
            n, S = cells[key]
            c = [f(float(s) / (n * 1048576.0)) for s in S.tolist()]
            e = [f(p[k] - c[k]) for k in range(3)]
            d2 = f(f(f(e[0] * e[0]) + f(e[1] * e[1])) + f(e[2] * e[2]))
            if d2 < best:
                best, best_key = d2, key
        out.append((best_key if best_key is not None and best <= f(max_dist) * f(max_dist) else None, best))
    return idx, out


@pytest.mark.parametrize("min_count", [1, 2])
def test_restatement_equals_the_point_by_point_loop(world, min_count):
    sel = np.linspace(0, len(world["cloud"]) - 1, 700).astype(np.int64)
    xyz = world["cloud"][sel]
    tgt = world["maps"][0.2]
    ev = A.Evaluation(tgt, xyz, world["guess"], 0.2, R.DEFAULT_BOX, 0.15, min_count)
    idx, loop = loop_evaluation(tgt, xyz, world["guess"], 0.2, R.DEFAULT_BOX, 0.15, min_count)
    assert len(idx) > 300
    for j, (key, d2) in zip(idx, loop):
        assert ev.d2[j] == d2 or (math.isinf(d2) and math.isinf(ev.d2[j]))
        assert ev.key3[j].tolist() == (list(key) if key is not None else [A.NO_KEY] * 3)
    assert ev.n == sum(1 for key, _ in loop if key is not None)


def test_header_binding_and_adapter_agree():
    from rgbd360_amd import _lib, build
    L = C.CDLL(build.build())
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip_diag.h")).read(), flags=re.S)
    for name in ("rgbd360_map_default_align_params", "rgbd360_map_align_sphere", "rgbd360_map_align_cloud"):
        assert re.search(r"\b%s\s*\(" % name, main) and hasattr(L, name) and name in _lib.SYMBOLS
    for name in ("rgbd360_map_align_eval", "rgbd360_map_time_align"):
        assert re.search(r"\b%s\s*\(" % name, diag) and name not in main and hasattr(L, name) and name in _lib.SYMBOLS

    def fields(text, struct):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[.*", "", part).split()[-1] for part in decl.split(",")]
        return names

    for text, struct, cls, size in ((main, "rgbd360_map_align_params", _lib.MapAlignParams, 24), (main, "rgbd360_map_align_result", _lib.MapAlignResult, 224),
                                    (diag, "rgbd360_map_align_trace", _lib.MapAlignTrace, 40)):
        assert fields(text, struct) == [n for n, _ in cls._fields_], struct
        assert C.sizeof(cls) == size, struct
    L.rgbd360_map_default_align_params.argtypes = [C.c_void_p, C.POINTER(_lib.MapAlignParams)]
    L.rgbd360_map_default_align_params.restype = None
    p = _lib.MapAlignParams()
    L.rgbd360_map_default_align_params(None, C.byref(p))
    assert (p.max_iters, p.min_count, p.min_matches) == (10, 1, 6) and p.eps == np.float32(1e-6) and p.max_dist == np.float32(0.05)
    hpp = open(os.path.join(ROOT, "include", "rgbd360", "GlobalMap.hpp")).read()
    for name in ("alignSphere", "alignCloud", "rgbd360_map_align_sphere", "rgbd360_map_align_cloud", "rgbd360_map_default_align_params"):
        assert name in hpp, name
    py = open(os.path.join(ROOT, "rgbd360_amd", "voxel_map.py")).read()
    assert "def align_sphere" in py and "def align_cloud" in py
