"""What every rgbd360_map_* entry that takes a frame or a cloud answers to a bad or an empty input, through the C ABI: the return code,
and that a refused call leaves its outputs and the map alone.  One table for all of them -- insert, remove, move, align, align_plane
for a sphere image and for a cloud, and the two evaluation entries of the diagnostics header -- recorded from the library as it stood
before its host code got one description of an input (csrc/voxel_map.h, MapInput): the table is that library's behaviour.

Where the entries differ from the plain table, as they always did:
  * an evaluation entry takes depth == NULL as "the cloud xyz / n": a null depth with n = 0 is an empty input (0), not an error;
    rgbd360_map_align_eval with a null pose is the trace query (0, nothing evaluated), rgbd360_map_align_plane_eval refuses it;
  * the align entries refuse a null guess even for an empty input; an empty input with a guess is RGBD360_NO_VALID_PIXELS;
  * what an evaluation entry leaves in sums / counters when it refuses a CLOUD is not asserted (the header does not say).
The map is leaf 0.05 with 1024 slots and holds one voxel; no call here gets as far as a launch over more than one point."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_VALID_PIXELS = 2
SENTINEL = 0x5A
SPHERE, CLOUD = "sphere", "cloud"
FAMILIES = ("insert", "remove", "move", "align", "align_plane", "eval", "plane_eval")
EDITS = ("insert", "remove", "move")


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fresh(t):
    o = t()
    C.memset(C.byref(o), SENTINEL, C.sizeof(o))
    return o


def untouched(o):
    return bytes(o) == bytes([SENTINEL]) * C.sizeof(o)


def outputs(family):
    from rgbd360_amd import _lib
    return {"insert": (_lib.MapStats,), "remove": (_lib.MapEditStats,), "move": (_lib.MapEditStats, _lib.MapStats),
            "align": (C.c_float * 16, _lib.MapAlignResult), "align_plane": (C.c_float * 16, _lib.MapAlignPlaneResult),
            "eval": (C.c_double * 17, C.c_longlong * 3), "plane_eval": (C.c_double * 30, C.c_longlong * 5)}[family]


def call(L, H, family, kind, a, pose, pose_new, outs):
    """One entry.  a: (rgb, rgb_step, depth, depth_step, depth_type, rows, cols, convention) or (xyz, rgb3, n); host input."""
    o = [C.byref(x) if isinstance(x, C.Structure) else x for x in outs]
    if family in EDITS:
        f = getattr(L, "rgbd360_map_%s_%s" % (family, kind))
        return f(H, *a, pose, pose_new, 0, *o) if family == "move" else f(H, *a, pose, 0, *o)
    geom = a[2:] if kind == SPHERE else (a[0], a[2])
    if family in ("align", "align_plane"):
        return getattr(L, "rgbd360_map_%s_%s" % (family, kind))(H, *geom, pose, 0, None, *o)
    both = geom + (None, 0) if kind == SPHERE else (None, 0, 0, 0, 0, 0) + geom
    if family == "eval":
        return L.rgbd360_map_align_eval(H, *both, pose, 0, None, *o, None, None, 0, None, None)
    return L.rgbd360_map_align_plane_eval(H, *both, pose, 0, None, *o, None, None, None, None)


@pytest.fixture(scope="module")
def reg(hip_lib):
    from rgbd360_amd.register import RegisterPhotoICP
    r = RegisterPhotoICP(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def gmap(reg):
    from rgbd360_amd.voxel_map import VoxelMap
    with VoxelMap(reg, 0.05, 1024) as m:
        m.set_box(None, None)
        m.insert_cloud(np.array([[0.31, 0.32, 0.33]], np.float32), None, np.eye(4))
        assert len(m) == 1
        yield m
        assert len(m) == 1      # nothing below changed it


ROWS, COLS = 4, 5
DEPTH = np.ones((ROWS, COLS), np.float32)
RGB = np.full((ROWS, COLS, 3), 7, np.uint8)
ONE = np.ones(4, np.float32)         # "pointers to a 1-element buffer"
XYZ = np.array([[0.31, 0.32, 0.33]] * 5, np.float32)
POSE = np.ascontiguousarray(np.eye(4, dtype=np.float32).reshape(16))
POSE_B = POSE.copy()


def image(rgb=RGB, rgb_step=COLS * 3, depth=DEPTH, depth_step=COLS * 4, depth_type=1, rows=ROWS, cols=COLS, convention=2):
    return (vp(rgb), rgb_step, vp(depth), depth_step, depth_type, rows, cols, convention)


# (case, input, pose, new pose of a move, expected return code; None: see expected())
SPHERE_CASES = [
    ("null depth", image(depth=None), POSE, POSE_B, -1),
    ("null pose", image(), None, POSE_B, -1),
    ("convention 3", image(convention=3), POSE, POSE_B, -1),
    ("depth_type 2", image(depth_type=2), POSE, POSE_B, -1),
    ("rows -1", image(rows=-1), POSE, POSE_B, -1),
    ("2^30 pixels", image(rgb=ONE, rgb_step=32768 * 3, depth=ONE, depth_step=32768 * 4, rows=32768, cols=32768), POSE, POSE_B, -1),
    ("depth_step one byte short", image(depth_step=COLS * 4 - 1), POSE, POSE_B, -1),
    ("rgb_step one byte short", image(rgb_step=COLS * 3 - 1), POSE, POSE_B, -1),
    ("0 x 5", image(rows=0), POSE, POSE_B, 0),
    ("5 x 0", image(rows=5, cols=0, depth_step=0, rgb_step=0), POSE, POSE_B, 0),
    ("null new pose", image(), POSE, None, -1),
]
CLOUD_CASES = [
    ("n -1", (vp(XYZ), None, -1), POSE, POSE_B, -1),
    ("n 2^40", (vp(XYZ), None, 1 << 40), POSE, POSE_B, -1),
    ("null xyz", (None, None, 5), POSE, POSE_B, -1),
    ("null pose", (vp(XYZ), None, 5), None, POSE_B, -1),
    ("n 0, null xyz, null pose", (None, None, 0), None, None, 0),
    ("n 0, null xyz", (None, None, 0), POSE, POSE_B, 0),
    ("null new pose", (vp(XYZ), None, 1), POSE, None, -1),
]


def expected(family, kind, name, pose, want):
    """The return code of `family` for the row, None where the row does not apply to it."""
    if name == "null new pose":
        return want if family == "move" else None
    if name == "rgb_step one byte short" and family not in EDITS:
        return None      # (these entries take no colour)
    if family in EDITS:
        return want
    if family in ("align", "align_plane"):
        return -1 if pose is None else NO_VALID_PIXELS if want == 0 else want
    if name == "null depth":
        return 0         # the cloud form of an evaluation entry, with no points
    if pose is None:
        return 0 if family == "eval" else -1
    return want


ROWS_OF_THE_TABLE = [(family, kind, case) for family in FAMILIES for kind, cases in ((SPHERE, SPHERE_CASES), (CLOUD, CLOUD_CASES)) for case in cases
                     if expected(family, kind, case[0], case[2], case[4]) is not None]


@pytest.mark.parametrize("family,kind,case", ROWS_OF_THE_TABLE, ids=["%s_%s-%s" % (f, k, c[0]) for f, k, c in ROWS_OF_THE_TABLE])
def test_the_entry_answers_as_the_table_says(hip_lib, gmap, family, kind, case):
    name, a, pose, pose_new, want = case
    want = expected(family, kind, name, pose, want)
    H = gmap._handle()
    outs = [fresh(t) for t in outputs(family)]
    rc = call(hip_lib, H, family, kind, a, vp(pose), vp(pose_new), outs)
    print("%s_%s, %s: returned %d, expected %d" % (family, kind, name, rc, want))
    assert rc == want
    assert hip_lib.rgbd360_map_size(H) == 1
    if rc < 0:
        assert hip_lib.rgbd360_map_last_error(H) != b""
        if not (family in ("eval", "plane_eval") and kind == CLOUD):
            assert all(untouched(o) for o in outs)
    elif family in EDITS:        # an empty input: the statistics zeroed, n_voxels the map's size
        for st in outs:
            values = {n: getattr(st, n) for n, _ in st._fields_}
            assert values.pop("n_voxels") == 1 and not any(values.values()), values
    elif family in ("align", "align_plane"):      # pose_out = guess, the result zeroed but for its status
        pose_out, res = outs
        assert bytes(pose_out) == pose.tobytes()
        zero = type(res)()
        zero.status = NO_VALID_PIXELS
        assert bytes(res) == bytes(zero)
    elif pose is None:           # the trace query of rgbd360_map_align_eval: nothing evaluated
        assert all(untouched(o) for o in outs)
    else:
        assert all(bytes(o) == bytes(C.sizeof(o)) for o in outs)
