"""The resident frame store without a device: the ABI is declared, exported and bound; the Python mirror validates its arguments on
the host; nothing degrades to a CPU path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STORE_SYMBOLS = ["rgbd360_store_align", "rgbd360_store_create", "rgbd360_store_destroy", "rgbd360_store_entry_bytes",
                 "rgbd360_store_last_error", "rgbd360_store_occupied", "rgbd360_store_put"]


@pytest.fixture(scope="module")
def built_lib():
    from rgbd360_amd import build
    return C.CDLL(build.build())          # hipcc cross-compiles for gfx950 without a GPU


def test_store_symbols_are_declared_exported_and_bound(built_lib):
    from rgbd360_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbd360_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbd360_store_[a-z0-9_]+)\s*\(", txt)))
    assert declared == STORE_SYMBOLS
    for s in STORE_SYMBOLS:
        assert hasattr(built_lib, s), s
        assert s in _lib.SYMBOLS
    L = _lib.load()
    assert L.rgbd360_store_entry_bytes.restype is C.c_size_t and L.rgbd360_store_last_error.restype is C.c_char_p
    assert len(L.rgbd360_store_align.argtypes) == 10 and len(L.rgbd360_store_put.argtypes) == 9


def test_store_kernels_are_in_the_gfx950_code_object(built_lib):
    """The pass, the per-slot start pose and the set-up into entries are device code of the library, for gfx950."""
    from rgbd360_amd import build
    strings = subprocess.run(["strings", "-n", "8", build.LIB], capture_output=True, text=True, check=True).stdout
    for name in ("k_eval_p", "k_level_init_p", "k_frame_level_e"):
        assert name in strings, name
    assert "gfx950" in strings


def test_null_handles_are_rejected_on_the_host(built_lib):
    from rgbd360_amd import _lib
    L = _lib.load()
    h = C.c_void_p()
    assert L.rgbd360_store_create(None, 4, 128, 256, C.byref(h)) == -1 and not h.value
    assert L.rgbd360_store_create(None, 4, 128, 256, None) == -1
    assert L.rgbd360_store_put(None, 0, None, None, 0, None, 0, 0, 0) == -1
    assert L.rgbd360_store_align(None, 0, None, None, None, 0, 0, 1, None, None) == -1
    assert L.rgbd360_store_occupied(None, 0) == -1
    assert L.rgbd360_store_entry_bytes(None) == 0
    assert L.rgbd360_store_last_error(None)
    L.rgbd360_store_destroy(None)


def test_frame_store_argument_validation(built_lib):
    """Shape / dtype / index checks of the mirror raise before anything touches a device."""
    from rgbd360_amd.register import RegisterPhotoICP, Rgbd360Error
    from rgbd360_amd.store import FrameStore
    reg = RegisterPhotoICP()
    for bad in ((0, 128, 256), (-1, 128, 256), (4, 1, 256), (4, 128, 4)):
        with pytest.raises(Rgbd360Error):
            FrameStore(reg, *bad)
    st = FrameStore(reg, 4, 32, 64)
    rgb, d = np.zeros((32, 64, 3), np.uint8), np.zeros((32, 64), np.uint16)
    bad_puts = [
        ([0, 1], [(rgb, d)]),                                        # one entry per frame
        ([4], [(rgb, d)]), ([-1], [(rgb, d)]),                       # outside the store
        ([1, 1], [(rgb, d), (rgb, d)]),                              # twice
        ([0.5], [(rgb, d)]),                                         # not an integer
        ([0], [(rgb.astype(np.float32), d)]),                        # colour dtype
        ([0], [(rgb[:, :, :2], d)]), ([0], [(rgb[:16], d[:16])]),    # colour shape, size
        ([0], [(rgb, d.astype(np.int32))]),                          # depth dtype
        ([0], [(rgb, d[:, :32])]),                                   # depth shape
        ([0, 1], [(rgb, d), (rgb, d.astype(np.float32))]),           # mixed depth types
    ]
    for entries, frames in bad_puts:
        with pytest.raises(Rgbd360Error):
            st.put(entries, frames)
    with pytest.raises(Rgbd360Error):
        st.put_dev([0], [1, 2], [3], 0)
    with pytest.raises(Rgbd360Error):
        st.put_dev([0], [1], [3], 2)
    with pytest.raises(Rgbd360Error):
        st.put_dev([9], [1], [3], 0)
    bad_aligns = [
        dict(pairs=[(0, 4)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, 1, 2)]), dict(pairs=[(0.0, 1.0)]),
        dict(pairs=[(0, 1)], method=3), dict(pairs=[(0, 1)], n_inflight=0), dict(pairs=[(0, 1)], n_inflight=65),
        dict(pairs=[(0, 1)], guesses=np.zeros((2, 4, 4))), dict(pairs=[(0, 1), (1, 0)], guesses=np.eye(4)),
    ]
    for kw in bad_aligns:
        with pytest.raises(Rgbd360Error):
            st.align(**kw)
    st.put([], [])                                                   # nothing to do: no device needed
    st.close()
    with pytest.raises(Rgbd360Error):
        st.put([0], [(rgb, d)])                                      # closed


def test_store_fails_loudly_without_a_gpu(built_lib):
    """No CPU fallback: without a HIP device the store cannot be created, exactly as rgbd360_create cannot."""
    from rgbd360_amd import _lib
    from rgbd360_amd.register import RegisterPhotoICP, Rgbd360Error
    from rgbd360_amd.store import FrameStore
    if _lib.load().rgbd360_device_count() > 0:
        pytest.skip("a GPU is visible here")
    reg = RegisterPhotoICP()
    st = FrameStore(reg, 2, 32, 64)
    with pytest.raises(Rgbd360Error):
        st.open()
    with pytest.raises(Rgbd360Error):
        st.put([0], [(np.zeros((32, 64, 3), np.uint8), np.zeros((32, 64), np.uint16))])
    with pytest.raises(Rgbd360Error):
        st.align([(0, 1)])


def test_keyframe_example_compiles_against_the_headers(tmp_path):
    from rgbd360_amd import build
    lib = build.build()
    exe = os.path.join(str(tmp_path), "keyframe_odometry")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "keyframe_odometry.cpp"), "-L" + os.path.dirname(lib), "-lrgbd360_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-pthread", "-o", exe])
    assert subprocess.call([exe]) == 2                                           # usage
    assert subprocess.call([exe, str(tmp_path / "missing"), "2", "8", "8"]) == 3     # its own I/O check: it linked and started
