"""pcr_sc_add_keyframes without a device: the C ABI declares it, the built library exports it, both mirrors offer addKeyFrames, and the slab
size the GPU test names is the kernel's."""
import inspect
import os
import re
import subprocess

from simpleslam_amd import ScanContext
from simpleslam_amd.pcr import ABI_SYMBOLS, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_header_declares_it():
    h = _read("include", "pcr_hip.h")
    assert re.search(r"\bint\s+pcr_sc_add_keyframes\s*\(\s*pcr_sc\s*\*\s*sc\s*,\s*const\s+pcr_map\s*\*\s*m\s*,\s*size_t\s+first\s*,\s*size_t\s+count\s*,"
                     r"\s*double\s+grid_size\s*,\s*size_t\s*\*\s*n_added\s*\)\s*;", h)
    assert h.index("typedef struct pcr_map pcr_map;") < h.index("pcr_sc_add_keyframes(pcr_sc*")      # the map's type is known where it is declared


def test_the_library_exports_it():
    assert "pcr_sc_add_keyframes" in ABI_SYMBOLS
    lib = load_library()
    assert hasattr(lib, "pcr_sc_add_keyframes")
    assert len(lib.pcr_sc_add_keyframes.argtypes) == 6


def test_the_python_mirror():
    sig = inspect.signature(ScanContext.addKeyFrames)
    assert list(sig.parameters) == ["self", "submap", "first", "count", "grid_size"]
    assert (sig.parameters["first"].default, sig.parameters["count"].default, sig.parameters["grid_size"].default) == (0, None, 0.0)


CPP = r'''
#include "PCR/HipRegister.hpp"
size_t (context::ScanContext::*with_leaf)(const PCR::SubMap&, size_t, size_t, double) = &context::ScanContext::addKeyFrames;
size_t all_of(context::ScanContext& sc, const PCR::SubMap& m) { return sc.addKeyFrames(m, 0, m.keyframes()); }      // grid_size defaults to 0
'''


def test_the_cpp_mirror_compiles(tmp_path):
    hpp = _read("simpleslam_amd", "host", "PCR", "HipRegister.hpp")
    assert re.search(r"addKeyFrames\(const (PCR::)?SubMap&\s*\w+,\s*size_t first,\s*size_t count,\s*double grid_size = 0\)", hpp)
    (tmp_path / "use.cpp").write_text(CPP)
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "simpleslam_amd", "host"), str(tmp_path / "use.cpp")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_the_gpu_test_names_the_kernels_slab():
    import test_sc_add_keyframes_gpu as g
    m = re.search(r"constexpr unsigned int kScSlab = (\d+);", _read("simpleslam_amd", "csrc", "scancontext.hip"))
    assert m and int(m.group(1)) == g.K_SLAB
