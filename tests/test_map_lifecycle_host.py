"""The key-frame store's new entry points without a device: exported, declared for C, and safe to call with nothing."""
import ctypes as C
import os

from simpleslam_amd.pcr import ABI_SYMBOLS, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pcr_map_set_poses", "pcr_map_keyframe", "pcr_map_read_keyframe", "pcr_map_downsample_keyframes", "pcr_map_update_all", "pcr_map_view"]


def test_new_entry_points_are_exported_and_declared():
    lib = load_library()
    header = open(os.path.join(ROOT, "include", "pcr_hip.h")).read()
    for name in NEW:
        assert name in ABI_SYMBOLS and hasattr(lib, name)
        assert f" {name}(" in header


def test_a_null_map_is_an_error_and_never_a_crash():
    lib = load_library()
    n, s = C.c_size_t(5), C.c_size_t(5)
    pose = (C.c_double * 16)()
    assert lib.pcr_map_set_poses(None, 0, 0, None) != 0
    assert lib.pcr_map_read_keyframe(None, 0, None, 0, C.byref(n), pose) != 0
    assert lib.pcr_map_downsample_keyframes(None, 0, 0.4, C.byref(n)) != 0
    assert lib.pcr_map_update_all(None, 0.4, C.byref(n)) != 0
    assert lib.pcr_map_keyframe(None, 0, C.byref(n), C.byref(s), pose) is None and (n.value, s.value) == (0, 0)
    assert lib.pcr_map_view(None) is None
    assert b"NULL" in lib.pcr_map_last_error(None)


def test_map_check_is_built():
    assert os.path.exists(os.path.join(ROOT, "simpleslam_amd", "lib", "map_check")), "map_check not built (run __graft_entry__.build())"
